"""RIF statistics without a GPU: the identities of tests/rif_stat_ref.py, the argument errors
of ob_rif_stat / ob_builder_decompose_statistics (they come back with no device present, which is the proof that
the checks precede device work) and the Python stat / params surface."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rif_stat_ref as R  # noqa: E402


@pytest.mark.parametrize("name", R.DISTINCT)
def test_variance_and_gini_identities(name):
    """mean(variance RIF) = sigma^2 and, on distinct values, mean(gini RIF) = G + 2/n, within the
    longdouble-measured E of the largest RIF value (the mixed error's own scale)."""
    y = R.inputs()[name]
    n = len(y)
    v, s2 = R.variance(y)
    assert abs(np.mean(v) - s2) <= R.E_MEASURED["variance"] * max(np.max(np.abs(v)), s2)
    g, gini = R.gini(y)
    assert -1.0 / n <= gini < 1.0  # this G is the usual Gini less 1/n: the sum to y_i includes y_i itself
    assert abs(np.mean(g) - (gini + 2.0 / n)) <= R.E_MEASURED["gini"] * max(np.max(np.abs(g)), gini)


@pytest.mark.parametrize("name", R.DISTINCT)
@pytest.mark.parametrize("pair", R.IQR_PAIRS)
def test_iqr_identity_within_the_indicator_bound(name, pair):
    """mean(iqr RIF) = q_hi - q_lo up to the indicator terms: |tau - #{y <= q} / n| < 1/n per quantile on distinct
    values, so the gap is at most (1 / f(q_hi) + 1 / f(q_lo)) / n (rif_stat_ref.iqr_identity_bound; the script
    prints gap and bound: 2.4e-4 against 2.0e-3 at n = 70,001, 5.6e1 against 7.1e1 at n = 2)."""
    y = R.inputs()[name]
    rif, stat = R.iqr(y, *pair)
    bound = R.iqr_identity_bound(y, *pair)
    assert abs(np.mean(rif) - stat) <= bound * (1 + 1e-12)
    hi, q_hi, _ = R.quantile_rif(y, pair[0])
    lo, q_lo, _ = R.quantile_rif(y, pair[1])
    assert stat == q_hi - q_lo and np.array_equal(rif, hi - lo)


def test_iqr_reference_matches_the_host_quantile_rif(ob):
    """The second yardstick: ob_rif(tau_hi) - ob_rif(tau_lo) of the host code, ties and fallbacks included."""
    for name, y in R.inputs().items():
        for hi, lo in R.IQR_PAIRS:
            rif, stat = R.iqr(y, hi, lo)
            host = ob.rif(y, hi) - ob.rif(y, lo)
            scale = np.maximum(np.abs(host), abs(stat))
            assert np.all(np.abs(rif - host) <= R.TOL["iqr"] * scale), name


def test_ties_share_the_last_rank_and_constant_panels():
    y = np.array([2.0, 1.0, 2.0, 3.0, 2.0])
    g, gini = R.gini(y)
    gl = np.array([7.0, 1.0, 7.0, 10.0, 7.0]) / 5  # the scan at the run's end
    p = np.array([4, 1, 4, 5, 4]) / 5
    big_r = gl.mean()
    assert np.allclose(g, 1 + 2 * big_r / 4 * y - (2 / 2.0) * (y * (1 - p) + gl), rtol=1e-15)
    c = R.inputs()["constant"]
    assert np.array_equal(R.variance(c)[0], np.zeros(len(c))) and R.variance(c)[1] == 0.0
    assert np.all(np.isfinite(R.gini(c)[0]))
    assert np.all(np.isfinite(R.iqr(c)[0])) and R.iqr(c)[1] == 0.0


def _spec(N, stat, p0=0.0, p1=0.0):
    return N.ob_rif_spec(stat, p0, p1)


def _stat_rc(N, y, spec):
    y = np.ascontiguousarray(y, dtype=np.float64)
    out, val = np.zeros(max(len(y), 1)), C.c_double()
    rc = N.lib().ob_rif_stat(None, y.ctypes.data_as(C.POINTER(C.c_double)), len(y), C.byref(spec),
                             out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(val))
    return rc, N.lib().ob_last_error().decode()


def test_array_errors_need_no_device(N):
    """Every check of ob_rif_stat runs before the context is looked at: a NULL context gets the same codes."""
    good = np.array([1.0, 2.0, 4.0])
    cases = [
        (good[:1], _spec(N, N.OB_RIF_VARIANCE), N.OB_E_INSUFFICIENT, "at least 2 rows"),
        (good[:0], _spec(N, N.OB_RIF_GINI), N.OB_E_INSUFFICIENT, "at least 2 rows"),
        (np.array([1.0, np.nan, 2.0]), _spec(N, N.OB_RIF_VARIANCE), N.OB_E_INVALID, "not finite"),
        (np.array([1.0, np.inf]), _spec(N, N.OB_RIF_IQR, 0.9, 0.1), N.OB_E_INVALID, "not finite"),
        (good, _spec(N, 3), N.OB_E_INVALID, "unknown RIF statistic"),
        (good, _spec(N, -1), N.OB_E_INVALID, "unknown RIF statistic"),
        (good, _spec(N, N.OB_RIF_IQR, 0.1, 0.9), N.OB_E_INVALID, "0 < lower < upper < 1"),
        (good, _spec(N, N.OB_RIF_IQR, 1.0, 0.1), N.OB_E_INVALID, "0 < lower < upper < 1"),
        (good, _spec(N, N.OB_RIF_IQR, 0.9, 0.0), N.OB_E_INVALID, "0 < lower < upper < 1"),
        (good, _spec(N, N.OB_RIF_IQR, np.nan, 0.1), N.OB_E_INVALID, "0 < lower < upper < 1"),
        (np.array([1.0, -0.5, 2.0]), _spec(N, N.OB_RIF_GINI), N.OB_E_INVALID, "negative"),
        (np.zeros(4), _spec(N, N.OB_RIF_GINI), N.OB_E_INVALID, "mean outcome must be positive"),
        (good, _spec(N, N.OB_RIF_GINI), N.OB_E_INVALID, "null pointer"),  # good arguments: only the context is missing
    ]
    for y, spec, code, text in cases:
        rc, msg = _stat_rc(N, y, spec)
        assert rc == code and text in msg, (rc, msg)
    assert N.lib().ob_rif_last_timing(None) == N.OB_E_INVALID
    assert N.lib().ob_rif_scan_block() == R.SCAN_BLOCK


FRAME = {"wage": [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0], "g": ["a", "b"] * 4,
         "x": [1.0, 2.0, 1.5, 2.5, 3.0, 1.0, 0.5, 2.0]}


def _builder_rc(ob, N, frame, specs, cluster=None):
    b = ob.OaxacaBuilder(frame, "wage", "g", "b").predictors(["x"]).bootstrap_reps(4).seed(1)
    cols, ncol, nrow = b._frame.as_c()
    cfg, keep = b._config()
    arr = (N.ob_rif_spec * len(specs))(*specs)
    hs = (C.c_void_p * max(len(specs), 1))()
    out = C.cast(hs, C.POINTER(C.c_void_p))
    if cluster:
        cc = b.cluster(cluster)._cluster_config()
        rc = N.lib().ob_builder_decompose_statistics_clustered(None, cols, ncol, nrow, C.byref(cfg), C.byref(cc), arr,
                                                               len(specs), out)
    else:
        rc = N.lib().ob_builder_decompose_statistics(None, cols, ncol, nrow, C.byref(cfg), arr, len(specs), out)
    return rc, N.lib().ob_last_error().decode()


def test_builder_errors_need_no_device(ob, N):
    var, gini = _spec(N, N.OB_RIF_VARIANCE), _spec(N, N.OB_RIF_GINI)
    assert _builder_rc(ob, N, FRAME, [var, _spec(N, 7)])[0] == N.OB_E_INVALID
    assert _builder_rc(ob, N, FRAME, [_spec(N, N.OB_RIF_IQR, 0.5, 0.5)])[0] == N.OB_E_INVALID
    assert _builder_rc(ob, N, FRAME, [])[0] == N.OB_E_INVALID
    one = dict(FRAME, g=["a"] + ["b"] * 7)  # group a has one row
    rc, msg = _builder_rc(ob, N, one, [var])
    assert rc == N.OB_E_INSUFFICIENT and "at least 2 rows" in msg
    bad = dict(FRAME, wage=[1.0, 2.0, float("nan"), 4.0, 5.0, 6.0, 7.0, 8.0])
    rc, msg = _builder_rc(ob, N, bad, [var])
    assert rc == N.OB_E_INVALID and "not finite" in msg
    neg = dict(FRAME, wage=[1.0, 2.0, 3.0, -4.0, 5.0, 6.0, 7.0, 8.0])
    assert _builder_rc(ob, N, neg, [var, gini])[0] == N.OB_E_INVALID
    assert _builder_rc(ob, N, neg, [var]) == (N.OB_E_INVALID, "null pointer")  # legal for the variance
    assert _builder_rc(ob, N, dict(FRAME, g=["a"] * 8), [var])[0] == N.OB_E_GROUP
    rc, msg = _builder_rc(ob, N, dict(FRAME, c=[1, 1, 2, 2, 3, 3, 4, 4]), [gini], cluster="c")
    assert (rc, msg) == (N.OB_E_INVALID, "null pointer")


def test_python_surface_parses(ob, N):
    p = ob.parse_rif_statistic
    assert p("variance") == (N.OB_RIF_VARIANCE, 0.0, 0.0)
    assert p("gini") == (N.OB_RIF_GINI, 0.0, 0.0)
    assert p("iqr") == (N.OB_RIF_IQR, 0.9, 0.1)
    assert p("iqr", upper=0.75, lower=0.25) == (N.OB_RIF_IQR, 0.75, 0.25)
    assert p(("iqr", {"lower": 0.2})) == (N.OB_RIF_IQR, 0.9, 0.2)
    assert p({"stat": "iqr", "upper": 0.8}) == (N.OB_RIF_IQR, 0.8, 0.1)
    for bad in ("theil", "Variance", None, 3):
        with pytest.raises(N.OaxacaError) as e:
            p(bad)
        assert e.value.code == N.OB_E_INVALID
    with pytest.raises(ValueError):
        p("gini", upper=0.9)
    with pytest.raises(ValueError):
        p("iqr", tau=0.5)
    with pytest.raises(ValueError):
        p(("iqr", 0.9))
    b = ob.OaxacaBuilder(FRAME, "wage", "g", "b").predictors(["x"])
    with pytest.raises(ValueError):
        b.decompose_statistics([])
    with pytest.raises(N.OaxacaError) as e:
        b.decompose_statistic("iqr", upper=0.1, lower=0.9)  # the library's check, before any device is needed
    assert e.value.code == N.OB_E_INVALID
    with pytest.raises(N.OaxacaError) as e:
        ob.rif_statistic([1.0], "variance")
    assert e.value.code == N.OB_E_INSUFFICIENT
    assert hasattr(ob.OaxacaBlinder, "fit_statistic") and hasattr(ob.OaxacaBuilder, "statistic_builder")
