"""The weighted RIF pass without a GPU: the argument errors of ob_rif_stat_weighted and of the
reweighted statistic's entry points (they come back with a NULL context, which is the proof that the checks precede
device work), statistic 3 still refused by ob_rif_stat, the Python parsing, and two properties of the numpy
restatement tests/wrif_ref.py: at w = 1 it is tests/rif_stat_ref.py, and integer weights are repeated rows."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rif_stat_ref as U  # noqa: E402
import wrif_ref as W  # noqa: E402

_D = C.POINTER(C.c_double)


def _spec(N, stat, p0=0.0, p1=0.0):
    return N.ob_rif_spec(stat, p0, p1)


def _rc(N, y, w, spec, n=None):
    y = np.ascontiguousarray(y, dtype=np.float64)
    w = np.ascontiguousarray(w, dtype=np.float64)
    out, val = np.zeros(max(len(y), 1)), C.c_double()
    rc = N.lib().ob_rif_stat_weighted(None, y.ctypes.data_as(_D), w.ctypes.data_as(_D), len(y) if n is None else n,
                                      C.byref(spec), out.ctypes.data_as(_D), C.byref(val))
    return rc, N.lib().ob_last_error().decode()


def test_array_errors_need_no_device(N):
    good, one = np.array([1.0, 2.0, 4.0]), np.ones(3)
    var, gini = _spec(N, N.OB_RIF_VARIANCE), _spec(N, N.OB_RIF_GINI)
    cases = [
        (good, one, _spec(N, 4), None, N.OB_E_INVALID, "unknown RIF statistic"),
        (good, one, _spec(N, -1), None, N.OB_E_INVALID, "unknown RIF statistic"),
        (good, one, _spec(N, N.OB_RIF_QUANTILE, 0.0), None, N.OB_E_INVALID, "0 < tau < 1"),
        (good, one, _spec(N, N.OB_RIF_QUANTILE, 1.0), None, N.OB_E_INVALID, "0 < tau < 1"),
        (good, one, _spec(N, N.OB_RIF_QUANTILE, np.nan), None, N.OB_E_INVALID, "0 < tau < 1"),
        (good, one, _spec(N, N.OB_RIF_IQR, 0.1, 0.9), None, N.OB_E_INVALID, "0 < lower < upper < 1"),
        (good[:1], one[:1], var, None, N.OB_E_INSUFFICIENT, "at least 2 rows"),
        (good[:0], one[:0], gini, None, N.OB_E_INSUFFICIENT, "at least 2 rows"),
        (good, one, var, 2 ** 28 + 1, N.OB_E_UNSUPPORTED, "at most 2^28 rows"),  # refused before a row is read
        (np.array([1.0, np.nan, 2.0]), one, var, None, N.OB_E_INVALID, "outcome row 1 is not finite"),
        (good, np.array([1.0, np.inf, 1.0]), var, None, N.OB_E_INVALID, "weight row 1 is not finite"),
        (good, np.array([1.0, np.nan, 1.0]), var, None, N.OB_E_INVALID, "weight row 1 is not finite"),
        (good, np.array([1.0, 1.0, -1e-300]), var, None, N.OB_E_INVALID, "weight row 2 is negative"),
        (good, np.zeros(3), var, None, N.OB_E_INVALID, "positive sum"),
        (np.array([1.0, -0.5, 2.0]), one, gini, None, N.OB_E_INVALID, "negative"),
        (np.array([0.0, 0.0, 2.0]), np.array([1.0, 1.0, 0.0]), gini, None, N.OB_E_INVALID, "mean outcome must be positive"),
        # the Gini's checks look at the rows with w > 0 only: a negative y of weight 0 is legal
        (np.array([1.0, -0.5, 2.0]), np.array([1.0, 0.0, 1.0]), gini, None, N.OB_E_INVALID, "null pointer"),
        (good, one, _spec(N, N.OB_RIF_QUANTILE, 0.5), None, N.OB_E_INVALID, "null pointer"),  # only the context is missing
        (good, one, _spec(N, N.OB_RIF_IQR, 0.9, 0.1), None, N.OB_E_INVALID, "null pointer"),
    ]
    for y, w, spec, n, code, text in cases:
        rc, msg = _rc(N, y, w, spec, n)
        assert rc == code and text in msg, (rc, msg, text)


def test_the_unweighted_entry_points_still_refuse_the_quantile(ob, N):
    y = np.array([1.0, 2.0, 4.0])
    out, val = np.zeros(3), C.c_double()
    spec = _spec(N, N.OB_RIF_QUANTILE, 0.5)
    rc = N.lib().ob_rif_stat(None, y.ctypes.data_as(_D), 3, C.byref(spec), out.ctypes.data_as(_D), C.byref(val))
    assert rc == N.OB_E_INVALID and "unknown RIF statistic" in N.lib().ob_last_error().decode()
    with pytest.raises(N.OaxacaError) as e:
        ob.parse_rif_statistic("quantile", tau=0.5)
    assert e.value.code == N.OB_E_INVALID


FRAME = {"wage": [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0], "g": ["a", "b"] * 4,
         "x": [1.0, 2.0, 1.5, 2.5, 3.0, 1.0, 0.5, 2.0], "w": [1.0, 2.0, 0.5, 1.0, 1.5, 1.0, 2.0, 1.0]}


def _builder(ob, frame=FRAME, weights=True):
    b = ob.OaxacaBuilder(frame, "wage", "g", "b").predictors(["x"]).bootstrap_reps(4).seed(1)
    return b.weights("w") if weights else b


def _prepare_rc(N, b, spec):
    cols, ncol, nrow = b._frame.as_c()
    cfg, keep = b._config()
    h = C.c_void_p()
    rc = N.lib().ob_builder_prepare_reweighted_statistic(None, cols, ncol, nrow, C.byref(cfg), C.byref(spec), C.byref(h))
    return rc, N.lib().ob_last_error().decode()


def _run_rc(N, b, specs):
    cols, ncol, nrow = b._frame.as_c()
    cfg, keep = b._config()
    arr = (N.ob_rif_spec * max(len(specs), 1))(*specs)
    hs = (C.c_void_p * max(len(specs), 1))()
    rc = N.lib().ob_builder_run_reweighted_statistics(None, cols, ncol, nrow, C.byref(cfg), arr, len(specs),
                                                      C.cast(hs, C.POINTER(C.c_void_p)))
    return rc, N.lib().ob_last_error().decode()


def test_builder_errors_need_no_device(ob, N):
    var, gini, q = _spec(N, N.OB_RIF_VARIANCE), _spec(N, N.OB_RIF_GINI), _spec(N, N.OB_RIF_QUANTILE, 0.5)
    b = _builder(ob)
    assert _prepare_rc(N, b, q) == (N.OB_E_INVALID, "null pointer: ctx")  # good arguments
    assert _prepare_rc(N, b, _spec(N, 9))[0] == N.OB_E_INVALID
    assert _prepare_rc(N, b, _spec(N, N.OB_RIF_QUANTILE, 1.5))[0] == N.OB_E_INVALID
    rc, msg = _prepare_rc(N, _builder(ob, dict(FRAME, wage=[1.0, 2.0, 3.0, -4.0, 5.0, 6.0, 7.0, 8.0])), gini)
    assert rc == N.OB_E_INVALID and "negative" in msg
    rc, msg = _prepare_rc(N, _builder(ob).normalize(["x"]), var)
    assert rc == N.OB_E_UNSUPPORTED and "normalized" in msg
    assert _run_rc(N, b, [var, gini, q]) == (N.OB_E_INVALID, "null pointer: ctx")
    assert _run_rc(N, b, [])[0] == N.OB_E_INVALID
    assert _run_rc(N, b, [var, _spec(N, 5)])[0] == N.OB_E_INVALID
    rc, msg = _run_rc(N, b, [var] * 17)
    assert rc == N.OB_E_UNSUPPORTED and "at most 16" in msg
    assert N.lib().ob_prepared_reweight_statistics(None, None) == N.OB_E_INVALID
    with pytest.raises(N.OaxacaError) as e:
        _builder(ob).cluster("x").prepare_reweighted("gini")
    assert e.value.code == N.OB_E_UNSUPPORTED


def test_python_surface_parses(ob, N):
    p = ob.parse_weighted_rif_statistic
    assert p("variance") == (N.OB_RIF_VARIANCE, 0.0, 0.0)
    assert p("gini") == (N.OB_RIF_GINI, 0.0, 0.0)
    assert p("iqr", upper=0.75, lower=0.25) == (N.OB_RIF_IQR, 0.75, 0.25)
    assert p("quantile") == (N.OB_RIF_QUANTILE, 0.5, 0.0)
    assert p("quantile", tau=0.1) == (N.OB_RIF_QUANTILE, 0.1, 0.0)
    assert p(("quantile", {"tau": 0.9})) == (N.OB_RIF_QUANTILE, 0.9, 0.0)
    assert p({"stat": "quantile", "tau": 0.25}) == (N.OB_RIF_QUANTILE, 0.25, 0.0)
    assert p({"stat": "iqr", "upper": 0.8}) == (N.OB_RIF_IQR, 0.8, 0.1)
    for bad in ("theil", "Quantile", None, 3):
        with pytest.raises(N.OaxacaError) as e:
            p(bad)
        assert e.value.code == N.OB_E_INVALID
    with pytest.raises(ValueError):
        p("quantile", upper=0.9)
    with pytest.raises(ValueError):
        p("gini", tau=0.5)
    with pytest.raises(ValueError):
        _builder(ob).prepare_reweighted(tau=0.5)  # parameters without a statistic
    with pytest.raises(ValueError):
        _builder(ob).decompose_reweighted_statistics([])
    with pytest.raises(N.OaxacaError) as e:
        ob.rif_statistic_weighted([1.0, 2.0], [1.0, -1.0], "variance")
    assert e.value.code == N.OB_E_INVALID
    with pytest.raises(N.OaxacaError) as e:
        ob.rif_statistic_weighted([1.0, 2.0, 3.0], [1.0, 1.0, 1.0], "quantile", tau=0.0)
    assert e.value.code == N.OB_E_INVALID
    with pytest.raises(ValueError):
        ob.rif_statistic_weighted([1.0, 2.0], [1.0], "variance")
    r = ob.ReweightedDecompositionResults
    assert r.__dataclass_fields__["statistic"].default is None and r.__dataclass_fields__["statistics"].default is None


def test_unit_weights_are_the_unweighted_reference():
    gap = W.unit_weight_gap()
    for stat, e in gap.items():
        assert e <= U.TOL[stat], (stat, e)
    for name, y in U.inputs().items():  # the quantile alone against the host path's restatement
        for tau in W.TAUS:
            rif, q = W.quantile(y, np.ones(len(y)), tau)
            ref, ref_q, _ = U.quantile_rif(y, tau)
            assert U.mixed_error(rif, q, ref, ref_q) <= U.TOL["iqr"], (name, tau)


def test_integer_weights_are_repeated_rows():
    """The variance and the Gini of (y, w) with integer w are those of the sample with row i repeated w_i times; the
    RIF of a row is the RIF of its copies. (The quantile's type-7 position (n - 1) tau depends on the row count, so
    it has no such identity.)"""
    rng = np.random.default_rng(5)
    y = np.concatenate([U.wages(200, 77), [3.0, 3.0, 3.0]])
    w = rng.integers(0, 5, len(y)).astype(float)
    rep = np.repeat(np.arange(len(y)), w.astype(int))
    first = np.array([np.flatnonzero(rep == i)[0] if w[i] else -1 for i in range(len(y))])
    for stat in ("variance", "gini"):
        rif, value = W.rif_statistic(y, w, stat)
        ref, ref_value = U.rif_statistic(y[rep], stat)
        assert abs(value - ref_value) <= U.TOL[stat] * abs(ref_value), stat
        keep = first >= 0
        scale = np.maximum(np.abs(ref[first[keep]]), abs(ref_value))
        assert np.all(np.abs(rif[keep] - ref[first[keep]]) <= U.TOL[stat] * scale), stat


def test_step_margins_of_the_inputs():
    """Every quantile input stays clear of a step of Y(t) (wrif_ref.step_margins): the GPU test relies on it."""
    taus = sorted({t for s, kw in W.STATS for t in W.stat_taus(s, kw)})
    for name, (y, w) in W.inputs().items():
        m_t, m_q = W.step_margins(y, w, taus)
        assert m_t >= 1e-9 and m_q >= 1e-9, (name, m_t, m_q)
    y = U.inputs()["n257"]
    m_t, m_q = W.step_margins(y, np.ones(len(y)), taus)  # unit weights: every t is an S, exactly
    assert m_t >= 1e-9 and m_q >= 1e-9
