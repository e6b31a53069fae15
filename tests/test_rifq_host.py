"""Host pieces of the per-replicate quantile RIF: the restatement over counts against the oracle's
rif on the expanded resample, the Gram-patch identities, the shape limits and every argument error of
ob_rifq_pass before any device work. No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rifq_ref as R  # noqa: E402


def _code(N, fn):
    with pytest.raises(N.OaxacaError) as e:
        fn()
    return e.value.code, str(e.value)


def _expanded_quantile(ye, tau):
    h = (np.float64(len(ye)) - 1.0) * np.float64(tau)
    hf, hc = np.floor(h), np.ceil(h)
    return ye[int(hf)] if hf == hc else ye[int(hf)] + (h - hf) * (ye[int(hc)] - ye[int(hf)])


def test_restatement_equals_oracle_rif_on_expanded_resample(O):
    for name, y, x, cs, taus in R.cases(O):
        for c in cs:
            r = R.restate(y, c, taus, x)
            R.check_steps(r)
            ye = np.repeat(y, c)
            for t, tau in enumerate(taus):
                assert r["q"][t] == _expanded_quantile(ye, tau), (name, tau)  # bitwise
                want = O.rif(ye, tau)
                got = np.repeat(R.rif_values(y, r, t), c)
                assert np.all(np.abs(got - want) <= 1e-13 * np.maximum(np.abs(want), 1.0)), (name, tau)
                assert r["n_le"][t] == int((ye <= r["q"][t]).sum())


def test_unit_counts_reproduce_rif_of_the_sample(O):
    for n in R.SIZES:
        y, _ = R.panel(n, 0)
        r = R.restate(y, np.ones(n, dtype=int), R.TAUS)
        for t, tau in enumerate(R.TAUS):
            want = O.rif(y, tau)
            assert np.all(np.abs(R.rif_values(y, r, t) - want) <= 1e-13 * np.maximum(np.abs(want), 1.0))


def test_gram_patch_identities(O):
    for name, y, x, cs, taus in R.cases(O):
        v = np.hstack([np.ones((len(y), 1)), x])
        for c in cs:
            r = R.restate(y, c, taus, x)
            for t in range(len(taus)):
                rif = R.rif_values(y, r, t)
                want = np.concatenate([(c[:, None] * v * rif[:, None]).sum(0), [(c * rif * rif).sum()]])
                scale = np.abs(want).max()
                # a sum of n terms against its closed form: n eps relative to the largest pair
                assert np.all(np.abs(r["gy"][t] - want) <= 4 * len(y) * np.finfo(float).eps * scale), (name, t)


def test_row_prefix_is_monotone_in_tau(O):
    for _, y, x, cs, taus in R.cases(O):
        for c in cs:
            r = R.restate(y, c, taus)
            assert all(a <= b for a, b in zip(r["p"], r["p"][1:]))
            assert all(a <= b for a, b in zip(r["q"], r["q"][1:]))


def test_restatement_error_is_far_below_the_floor(O):
    E = R.restatement_error(O)
    print({k: f"{v:.3e}" for k, v in E.items()})
    assert all(8 * v < R.FLOOR for v in E.values())  # so the GPU tests' bound is the 1e-12 floor


def test_row_len_and_shape(ob, N):
    for k, nb in ((1, 0), (3, 0), (9, 2), (32, 0)):
        assert ob.rifq_row_len(k, nb) == 6 + 2 * (k + nb) + 5 * k + 6
    assert ob.rifq_row_len(0) == 0
    assert (N.OB_RIFQ_MAX_K, N.OB_RIFQ_MAX_TAUS) == (32, 8)
    ob.rifq_check_shape(32, [0.1, 0.5, 0.9], 33, 33)
    ob.rifq_check_shape(1, [0.5], 2, 2)
    ob.rifq_check_shape(3, np.linspace(0.1, 0.9, 8), 100, 100)
    assert _code(N, lambda: ob.rifq_check_shape(33, [0.5], 100, 100))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.rifq_check_shape(3, np.linspace(0.1, 0.9, 9), 100, 100))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.rifq_check_shape(3, [0.5], 2 ** 31, 100))[0] == N.OB_E_UNSUPPORTED
    for bad in ([0.0], [1.0], [-0.1], [float("nan")], [0.5, 0.5], [0.9, 0.1], []):
        assert _code(N, lambda: ob.rifq_check_shape(3, bad, 100, 100))[0] == N.OB_E_INVALID, bad
    assert _code(N, lambda: ob.rifq_check_shape(0, [0.5], 100, 100))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.rifq_check_shape(3, [0.5], -1, 100))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.rifq_check_shape(3, [0.5], 3, 100))[0] == N.OB_E_INSUFFICIENT
    assert _code(N, lambda: ob.rifq_check_shape(3, [0.5], 100, 3))[0] == N.OB_E_INSUFFICIENT
    assert _code(N, lambda: ob.rifq_check_shape(1, [0.5], 1, 100))[0] == N.OB_E_INSUFFICIENT
    assert N.lib().ob_rifq_last_timing(None) == N.OB_E_INVALID


def test_pass_argument_errors_come_before_any_device_work(ob, N):
    """Every refusal of ob_rifq_pass is made before the context is read: the codes are the same without a GPU."""
    y, x = R.panel(10, 2)
    ones = np.ones((1, 10), dtype=int)
    assert _code(N, lambda: ob.rifq_pass(y, [0.5, 0.4], ones))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.rifq_pass(y, [1.5], ones))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.rifq_pass(y, np.linspace(0.1, 0.9, 9), ones))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.rifq_pass(y, [0.5], ones, x=np.ones((10, 32))))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.rifq_pass(y[:1], [0.5]))[0] == N.OB_E_INSUFFICIENT
    assert _code(N, lambda: ob.rifq_pass(y[::-1], [0.5]))[0] == N.OB_E_INVALID  # not ascending
    bad = y.copy()
    bad[3] = np.nan
    assert _code(N, lambda: ob.rifq_pass(bad, [0.5]))[0] == N.OB_E_INVALID
    xb = x.copy()
    xb[2, 1] = np.inf
    assert _code(N, lambda: ob.rifq_pass(y, [0.5], ones, x=xb))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.rifq_pass(y, [0.5], 2 * ones))[0] == N.OB_E_INVALID  # counts sum to 2 n
    with pytest.raises(ValueError):
        ob.rifq_pass(y, [0.5], np.full((1, 10), 256))
    with pytest.raises(ValueError):
        ob.rifq_pass(y, [0.5], ones[:, :9])
    with pytest.raises(ValueError):
        ob.rifq_pass(y, [0.5], ones, x=x[:9])


def _frame(n=80):
    rng = np.random.default_rng(4)
    return {"y": rng.normal(2.5, 0.5, n).tolist(), "g": np.where(np.arange(n) % 2 == 0, "A", "B").tolist(),
            "w": rng.uniform(0.5, 2.0, n).tolist(), "s": (rng.random(n) < 0.7).astype(float).tolist(),
            "x1": rng.normal(size=n).tolist(), "x2": rng.normal(size=n).tolist(),
            "c": [f"l{v}" for v in rng.integers(0, 3, n)], "cl": rng.integers(0, 9, n).tolist()}


def _builder(ob, f=None):
    return ob.OaxacaBuilder(f or _frame(), "y", "g", "B").predictors(["x1", "x2"]).bootstrap_reps(8).seed(3)


def test_builder_refusals_without_a_gpu(ob, N):
    """Every refusal of the refit's entry points comes before the context is read."""
    for call in (lambda b: b.prepare_quantiles_refit([0.5]), lambda b: b.decompose_quantiles([0.1, 0.9], refit=True),
                 lambda b: b.decompose_quantile(0.5, refit=True)):
        assert _code(N, lambda: call(_builder(ob).weights("w")))[0] == N.OB_E_UNSUPPORTED
        assert _code(N, lambda: call(_builder(ob).categorical_predictors(["c"]).normalize(["c"])))[0] == N.OB_E_UNSUPPORTED
        assert _code(N, lambda: call(_builder(ob).heckman_selection("s", ["x1"])))[0] == N.OB_E_UNSUPPORTED
        assert _code(N, lambda: call(_builder(ob).cluster("cl")))[0] == N.OB_E_UNSUPPORTED
    b = _builder(ob)
    assert _code(N, lambda: b.prepare_quantiles_refit(np.linspace(0.1, 0.9, 9)))[0] == N.OB_E_UNSUPPORTED
    for bad in ([0.0], [1.2], [0.5, 0.5], [0.9, 0.1]):
        assert _code(N, lambda: b.prepare_quantiles_refit(bad))[0] == N.OB_E_INVALID, bad
    for col, val in (("x1", None), ("y", None), ("x2", float("inf")), ("y", float("nan"))):
        f = _frame()
        f[col][5] = val
        assert _code(N, lambda: _builder(ob, f).prepare_quantiles_refit([0.5]))[0] == N.OB_E_INVALID, (col, val)
    f = _frame(8)  # 4 rows a group, K = 5 with the categorical
    assert _code(N, lambda: _builder(ob, f).categorical_predictors(["c"]).prepare_quantiles_refit([0.5]))[0] in (
        N.OB_E_INSUFFICIENT,)
    lib = N.lib()
    assert lib.ob_prepared_rifq_info(None, None) == N.OB_E_INVALID
    assert lib.ob_prepared_finish_tau(None, 0, None, None, 0, None) == N.OB_E_INVALID
    assert lib.ob_builder_prepare_quantiles_refit(None, None, 0, 0, None, None, 0, None) == N.OB_E_INVALID


def test_refit_false_calls_the_same_entry_point(ob, N, monkeypatch):
    """Without refit the call path is unchanged: the same C entry point with the same arguments, and the refit's
    entry point is never reached."""
    lib = N.lib()
    calls = []

    def recorder(name):
        def fn(*args):
            calls.append((name, args))
            return N.OB_E_INVALID
        return fn

    monkeypatch.setattr(N, "context", lambda device=None: None)
    for name in ("ob_builder_decompose_quantile", "ob_builder_decompose_quantiles",
                 "ob_builder_prepare_quantiles_refit", "ob_builder_decompose_quantiles_refit"):
        monkeypatch.setattr(lib, name, recorder(name), raising=False)
    b = _builder(ob)
    for call in (lambda: b.decompose_quantile(0.25), lambda: b.decompose_quantile(0.25, refit=False),
                 lambda: b.decompose_quantiles([0.1, 0.9]), lambda: b.decompose_quantiles([0.1, 0.9], refit=False)):
        with pytest.raises(N.OaxacaError):
            call()
    assert [c[0] for c in calls] == ["ob_builder_decompose_quantile"] * 2 + ["ob_builder_decompose_quantiles"] * 2
    assert calls[0][1][5] == calls[1][1][5] == 0.25 and len(calls[0][1]) == len(calls[1][1]) == 7
    assert calls[2][1][6] == calls[3][1][6] == 2 and len(calls[2][1]) == len(calls[3][1]) == 8
    plain = ob.OaxacaBlinder(_frame(), "y", "g", "B", ["x1"], bootstrap_reps=4)
    with pytest.raises(N.OaxacaError):
        plain.fit_quantile(0.5)
    assert calls[-1][0] == "ob_builder_decompose_quantile"
