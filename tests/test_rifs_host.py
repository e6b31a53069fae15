"""Host pieces of the per-replicate RIFs of the variance, the Gini and quantile ranges: the
restatement over counts against tests/rif_stat_ref.py on the expanded resample, the shape limits and every argument
error of ob_rifs_pass and of the builder's entry points before any device work. No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rifs_ref as F  # noqa: E402
import rifq_ref as R  # noqa: E402

IQR = ("iqr", {"upper": 0.9, "lower": 0.1})


def _code(N, fn):
    with pytest.raises(N.OaxacaError) as e:
        fn()
    return e.value.code, str(e.value)


def test_restatement_equals_rif_stat_ref_on_expanded_resamples(O):
    """rifs_ref.restatement_error asserts the counts form against rif_stat_ref's variance, gini and iqr on
    np.repeat(y_sorted, c) within max(8 E, 1e-12) over every GPU test input; E stays below the floor, so that bound
    is the floor, and the figures written into rifs_ref are the measured ones."""
    E = F.restatement_error(O)
    print({k: {q: f"{v:.3e}" for q, v in e.items()} for k, e in E.items()})
    for name, e in E.items():
        for key, val in e.items():
            assert 8 * val < F.FLOOR, (name, key, val)
            assert val <= 2 * F.E_MEASURED[name][key] + 1e-18, (name, key, val)


def test_tie_term_only_moves_the_scalar(O):
    """z is the same at a row and at the end of its tie run, so E enters R alone; it is 0 on distinct values."""
    y, x = R.panel(257, 2, decimals=1)
    assert F.tie_runs(y) and not F.tie_runs(R.panel(257, 2)[0])
    assert F.tie_runs(np.full(5, 3.25)) == [(0, 5)]
    c = R.stream_counts(O, 257, 1)[0]
    r = F.restate(y, c, (("gini", {}),), x)
    nu, gy = F.expanded(y, c, "gini", {}, x)
    assert abs(r["nu"][0] - nu) <= 1e-13 and F.mixed_err(r["gy"][0], gy) <= 1e-13
    no_e = F.gini_counts(y, c.astype(float), F._design(257, x, np.float64), 257.0, [])
    assert abs(no_e[0] - nu) > 1e-6  # without E the statistic is wrong on ties


def test_row_len_and_shape(ob, N):
    for k, nb in ((1, 0), (3, 0), (9, 2), (32, 0)):
        assert ob.rifs_row_len(k, nb) == 6 + 2 * (k + nb) + 5 * k + 2
    assert ob.rifs_row_len(0) == 0
    assert N.OB_RIFS_MAX_STATS == 8
    ob.rifs_check_shape(32, ["variance", "gini", IQR], 33, 33)
    ob.rifs_check_shape(1, ["gini"], 2, 2)
    ob.rifs_check_shape(3, ["variance"] * 8, 100, 100)
    four = [("iqr", {"upper": u, "lower": l}) for u, l in ((0.9, 0.1), (0.8, 0.2), (0.7, 0.3), (0.6, 0.4))]
    ob.rifs_check_shape(3, four, 100, 100)  # 8 distinct quantiles
    ob.rifs_check_shape(3, four + [("iqr", {"upper": 0.9, "lower": 0.4})], 100, 100)  # still 8
    assert _code(N, lambda: ob.rifs_check_shape(33, ["variance"], 100, 100))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.rifs_check_shape(3, ["variance"] * 9, 100, 100))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.rifs_check_shape(3, four + [("iqr", {"upper": 0.55, "lower": 0.4})], 100, 100))[0] == \
        N.OB_E_UNSUPPORTED  # a ninth quantile
    assert _code(N, lambda: ob.rifs_check_shape(3, ["gini"], 2 ** 31, 100))[0] == N.OB_E_UNSUPPORTED
    for u, l in ((0.1, 0.9), (0.5, 0.5), (1.0, 0.1), (0.9, 0.0), (float("nan"), 0.1)):
        assert _code(N, lambda: ob.rifs_check_shape(3, [("iqr", {"upper": u, "lower": l})], 100, 100))[0] == \
            N.OB_E_INVALID, (u, l)
    assert _code(N, lambda: ob.rifs_check_shape(3, [(7, 0.0, 0.0)], 100, 100))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.rifs_check_shape(3, [(N.OB_RIF_QUANTILE, 0.5, 0.0)], 100, 100))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.rifs_check_shape(3, [], 100, 100))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.rifs_check_shape(0, ["gini"], 100, 100))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.rifs_check_shape(3, ["gini"], -1, 100))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.rifs_check_shape(3, ["gini"], 3, 100))[0] == N.OB_E_INSUFFICIENT
    assert _code(N, lambda: ob.rifs_check_shape(3, ["gini"], 100, 3))[0] == N.OB_E_INSUFFICIENT
    assert _code(N, lambda: ob.rifs_check_shape(1, ["gini"], 1, 100))[0] == N.OB_E_INSUFFICIENT
    assert N.lib().ob_rifs_last_timing(None) == N.OB_E_INVALID
    assert set(ob.rifs_last_timing()) == {f + "_ms" for f in ("moment", "scan", "gini", "tie", "finish", "gram",
                                                              "solve", "rifq")}


def test_new_names_are_exported(N):
    for name in ("ob_rifs_row_len", "ob_rifs_check_shape", "ob_rifs_pass", "ob_rifs_last_timing",
                 "ob_builder_prepare_statistics_refit", "ob_builder_decompose_statistics_refit",
                 "ob_prepared_rifs_info"):
        assert name in N.EXPORTED and hasattr(N.lib(), name), name


def test_pass_argument_errors_come_before_any_device_work(ob, N):
    """Every refusal of ob_rifs_pass is made before the context is read: the codes are the same without a GPU."""
    y, x = R.panel(10, 2)
    assert np.all(y > 0)
    ones = np.ones((1, 10), dtype=int)
    every = ["variance", "gini", IQR]
    assert _code(N, lambda: ob.rifs_pass(y, every, ones, x=np.ones((10, 32))))[0] == N.OB_E_UNSUPPORTED  # K = 33
    assert _code(N, lambda: ob.rifs_pass(y, ["variance"] * 9, ones))[0] == N.OB_E_UNSUPPORTED
    five = [("iqr", {"upper": 0.5 + 0.05 * i, "lower": 0.5 - 0.05 * i}) for i in range(1, 6)]
    assert _code(N, lambda: ob.rifs_pass(y, five, ones))[0] == N.OB_E_UNSUPPORTED  # 10 quantiles
    big = np.zeros((16385, 10), dtype=np.uint8)
    assert _code(N, lambda: ob.rifs_pass(y, every, big))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.rifs_pass(y, [("iqr", {"upper": 0.1, "lower": 0.9})], ones))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.rifs_pass(y, [(9, 0.0, 0.0)], ones))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.rifs_pass(y, [], ones))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.rifs_pass(y[:1], every))[0] == N.OB_E_INSUFFICIENT
    assert _code(N, lambda: ob.rifs_pass(y[::-1], every))[0] == N.OB_E_INVALID  # not ascending
    bad = y.copy()
    bad[3] = np.nan
    assert _code(N, lambda: ob.rifs_pass(bad, every))[0] == N.OB_E_INVALID
    xb = x.copy()
    xb[2, 1] = np.inf
    assert _code(N, lambda: ob.rifs_pass(y, every, ones, x=xb))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.rifs_pass(y, every, 2 * ones))[0] == N.OB_E_INVALID  # counts sum to 2 n
    assert _code(N, lambda: ob.rifs_pass(y, every, np.vstack([ones, ones])[:, :10] * [[1], [0]]))[0] == N.OB_E_INVALID
    neg = np.concatenate([[-0.5], y[1:]])
    assert _code(N, lambda: ob.rifs_pass(neg, ["gini"]))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.rifs_pass(np.zeros(10), ["variance", "gini"]))[0] == N.OB_E_INVALID  # no positive y
    # the variance and a range take a negative y: only the missing context stops these
    for stats in (["variance", IQR], every):
        code, msg = _code(N, lambda: N.check(_null_ctx_pass(N, neg if "gini" not in stats else y, stats)))
        assert code == N.OB_E_INVALID and "ctx" in msg, (stats, msg)
    with pytest.raises(ValueError):
        ob.rifs_pass(y, every, np.full((1, 10), 256))
    with pytest.raises(ValueError):
        ob.rifs_pass(y, every, ones[:, :9])
    with pytest.raises(ValueError):
        ob.rifs_pass(y, every, ones, x=x[:9])


def _null_ctx_pass(N, y, stats):
    """ob_rifs_pass with good arguments and a NULL context."""
    import ctypes as C
    from importlib import import_module

    eng = import_module(N.__name__.rsplit(".", 1)[0] + ".engine")
    specs, parsed = eng._rif_specs(stats)
    y = np.ascontiguousarray(y, dtype=np.float64)
    nu, gy = np.empty(len(parsed)), np.empty((len(parsed), 2))
    dp = C.POINTER(C.c_double)
    return N.lib().ob_rifs_pass(None, y.ctypes.data_as(dp), len(y), None, 1, specs, len(parsed), None, len(y), 0,
                                nu.ctypes.data_as(dp), gy.ctypes.data_as(dp), None, None)


def _frame(n=80):
    rng = np.random.default_rng(4)
    return {"y": np.exp(rng.normal(2.5, 0.5, n)).tolist(), "g": np.where(np.arange(n) % 2 == 0, "A", "B").tolist(),
            "w": rng.uniform(0.5, 2.0, n).tolist(), "s": (rng.random(n) < 0.7).astype(float).tolist(),
            "x1": rng.normal(size=n).tolist(), "x2": rng.normal(size=n).tolist(),
            "c": [f"l{v}" for v in rng.integers(0, 3, n)], "cl": rng.integers(0, 9, n).tolist()}


def _builder(ob, f=None):
    return ob.OaxacaBuilder(f or _frame(), "y", "g", "B").predictors(["x1", "x2"]).bootstrap_reps(8).seed(3)


def test_builder_refusals_without_a_gpu(ob, N):
    """Every refusal of the refit's entry points comes before the context is read."""
    for call in (lambda b: b.prepare_statistics_refit(["gini"]),
                 lambda b: b.decompose_statistics(["variance", IQR], refit=True),
                 lambda b: b.decompose_statistic("iqr", refit=True, upper=0.75, lower=0.25)):
        assert _code(N, lambda: call(_builder(ob).weights("w")))[0] == N.OB_E_UNSUPPORTED
        assert _code(N, lambda: call(_builder(ob).categorical_predictors(["c"]).normalize(["c"])))[0] == N.OB_E_UNSUPPORTED
        assert _code(N, lambda: call(_builder(ob).heckman_selection("s", ["x1"])))[0] == N.OB_E_UNSUPPORTED
        assert _code(N, lambda: call(_builder(ob).cluster("cl")))[0] == N.OB_E_UNSUPPORTED
    b = _builder(ob)
    assert _code(N, lambda: b.prepare_statistics_refit(["variance"] * 9))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: b.prepare_statistics_refit([("iqr", {"upper": 0.2, "lower": 0.4})]))[0] == N.OB_E_INVALID
    assert _code(N, lambda: b.prepare_statistics_refit(["skewness"]))[0] == N.OB_E_INVALID
    for col, val in (("x1", None), ("y", None), ("x2", float("inf")), ("y", float("nan"))):
        f = _frame()
        f[col][5] = val
        assert _code(N, lambda: _builder(ob, f).prepare_statistics_refit(["variance"]))[0] == N.OB_E_INVALID, (col, val)
    f = _frame()
    f["y"][7] = -1.0
    assert _code(N, lambda: _builder(ob, f).prepare_statistics_refit(["variance", "gini"]))[0] == N.OB_E_INVALID
    f = _frame(8)  # 4 rows a group, K = 5 with the categorical
    assert _code(N, lambda: _builder(ob, f).categorical_predictors(["c"]).prepare_statistics_refit(["gini"]))[0] == \
        N.OB_E_INSUFFICIENT
    lib = N.lib()
    assert lib.ob_prepared_rifs_info(None, None) == N.OB_E_INVALID
    assert lib.ob_builder_prepare_statistics_refit(None, None, 0, 0, None, None, 0, None) == N.OB_E_INVALID
    assert lib.ob_builder_decompose_statistics_refit(None, None, 0, 0, None, None, 0, None) == N.OB_E_INVALID


def test_refit_false_calls_the_same_entry_point(ob, N, monkeypatch):
    """Without refit the call path is unchanged: the same C entry point with the same arguments, and the refit's
    entry points are never reached."""
    lib = N.lib()
    calls = []

    def recorder(name):
        def fn(*args):
            calls.append((name, args))
            return N.OB_E_INVALID
        return fn

    monkeypatch.setattr(N, "context", lambda device=None: None)
    for name in ("ob_builder_decompose_statistics", "ob_builder_prepare_statistics_refit",
                 "ob_builder_decompose_statistics_refit"):
        monkeypatch.setattr(lib, name, recorder(name), raising=False)
    b = _builder(ob)
    for call in (lambda: b.decompose_statistic("gini"), lambda: b.decompose_statistic("gini", refit=False),
                 lambda: b.decompose_statistics(["variance", IQR]),
                 lambda: b.decompose_statistics(["variance", IQR], refit=False)):
        with pytest.raises(N.OaxacaError):
            call()
    assert [c[0] for c in calls] == ["ob_builder_decompose_statistics"] * 4
    assert calls[0][1][6] == calls[1][1][6] == 1 and calls[2][1][6] == calls[3][1][6] == 2
    assert all(len(c[1]) == 8 for c in calls)
    plain = ob.OaxacaBlinder(_frame(), "y", "g", "B", ["x1"], bootstrap_reps=4)
    with pytest.raises(N.OaxacaError):
        plain.fit_statistic("gini")
    assert calls[-1][0] == "ob_builder_decompose_statistics"
    with pytest.raises(N.OaxacaError):
        plain.fit_statistic("gini", refit=True)
    assert calls[-1][0] == "ob_builder_prepare_statistics_refit"
