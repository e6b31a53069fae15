"""Host pieces of the jackknife / BCa inference: ob_bca_stats, ob_aggregate_bca,
ob_jackknife_finish and the argument checks made before any device work. No GPU."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jackknife_ref as J  # noqa: E402


def _skewed(n, seed):
    rng = np.random.default_rng(seed)
    return rng.gamma(2.0, 0.7, n) - 1.1


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _check_bca(ob, v, point, accel, level=0.95):
    got, ref = ob.bca_stats(v, point, accel, level), J.bca(v, point, accel, level)
    assert got["flag"] == ref["flag"]
    if ref["flag"] == 0:
        n = len(v)
        for key in ("alpha_lo", "alpha_hi"):  # the floor must not sit on an integer: then both sides index alike
            assert abs(ref[key] * n - round(ref[key] * n)) > 1e-6
            assert abs(got[key] - ref[key]) <= 1e-12
        assert abs(got["z0"] - ref["z0"]) <= 1e-12 * max(1.0, abs(ref["z0"]))
    assert _same(got["ci_lower"], ref["ci_lower"]) and _same(got["ci_upper"], ref["ci_upper"])
    return got


@pytest.mark.parametrize("n", [1, 2, 999, 1000])
@pytest.mark.parametrize("accel", [0.0, 0.05, -0.05])
def test_bca_stats_matches_python(ob, n, accel):
    v = _skewed(n, 100 + n)
    point = float(np.median(v)) + 0.03 if n > 2 else float(v.mean())
    got = _check_bca(ob, v, point, accel)
    if n > 2:
        assert got["flag"] == 0 and got["ci_lower"] < got["ci_upper"]
    _check_bca(ob, v, point, accel, level=0.9)


def test_bca_reduces_to_percentile(ob):
    """a = 0 and p0 exactly 1/2: z0 = 0, alpha' = alpha, so the endpoints are ob_bootstrap_stats's at n = 999."""
    v = _skewed(999, 7)
    point = float(np.median(v))  # one value equal to it, 499 on either side
    got = ob.bca_stats(v, point, 0.0)
    assert got["flag"] == 0 and got["z0"] == 0.0
    _, _, (lo, hi) = ob.bootstrap_stats(v)
    assert got["ci_lower"] == lo and got["ci_upper"] == hi


def test_bca_flags(ob):
    v = _skewed(200, 3)
    assert ob.bca_stats(v, v.max() + 1.0, 0.0)["flag"] == 2   # all replicates below the point estimate
    assert ob.bca_stats(v, v.min() - 1.0, 0.0)["flag"] == 2   # all above
    assert ob.bca_stats(np.zeros(0), 0.0, 0.0)["flag"] == 1   # n = 0
    assert ob.bca_stats(v, float(np.median(v)), float("nan"))["flag"] == 3
    assert ob.bca_stats(v, float(np.median(v)), float("inf"))["flag"] == 3
    g = ob.bca_stats(v, float(np.median(v)), 0.6)  # 1 - a q <= 0 at the upper end: q = 1.96
    assert g["flag"] == 4 and math.isnan(g["ci_lower"]) and math.isnan(g["ci_upper"])
    for case in (ob.bca_stats(v, v.max() + 1.0, 0.0), ob.bca_stats(np.zeros(0), 0.0, 0.0)):
        assert math.isnan(case["ci_lower"]) and math.isnan(case["ci_upper"])
    for args in ((v, v.max() + 1.0, 0.0), (np.zeros(0), 0.0, 0.0), (v, float(np.median(v)), float("nan")),
                 (v, float(np.median(v)), 0.6)):
        assert J.bca(*args)["flag"] == ob.bca_stats(*args)["flag"]


def test_aggregate_bca_matches_per_column(ob):
    rng = np.random.default_rng(5)
    rows = rng.gamma(2.0, 1.0, (999, 7)) - 1.7
    ok = (rng.random(999) > 0.1).astype(np.uint8)
    cols = [0, 3, 6]
    point = [float(np.median(rows[:, c])) + 0.02 for c in cols]
    accel = [0.0, 0.05, -0.05]
    out = ob.aggregate_bca(rows, ok, cols, point, accel, 0.95)
    for j, c in enumerate(cols):
        v = rows[ok.astype(bool), c]
        ref = J.bca(v, point[j], accel[j])
        for key in ("alpha_lo", "alpha_hi"):
            assert abs(ref[key] * len(v) - round(ref[key] * len(v))) > 1e-6
        assert out[j, 5] == 0 and out[j, 0] == ref["ci_lower"] and out[j, 1] == ref["ci_upper"]
        assert abs(out[j, 2] - ref["z0"]) <= 1e-12
        one = ob.bca_stats(v, point[j], accel[j])
        assert [one[k] for k in ("ci_lower", "ci_upper", "z0", "alpha_lo", "alpha_hi")] == list(out[j, :5])


def test_jackknife_finish_matches_closed_form(ob):
    rng = np.random.default_rng(9)
    c, m = 5, (40, 57)
    d = [rng.gamma(2.0, 1e-3, (m[0], c)) - 2e-3, rng.normal(0.0, 2e-3, (m[1], c))]
    d[0][:, 3] = 0.25   # a constant component: zero denominator in both groups
    d[1][:, 3] = -0.5
    sums = np.zeros((2, c, 3))
    for g in (0, 1):
        sums[g, :, 0], sums[g, :, 1], sums[g, :, 2] = d[g].sum(0), (d[g] ** 2).sum(0), (d[g] ** 3).sum(0)
    sums[:, 3, 1] = [m[0] * 0.25 ** 2, m[1] * 0.5 ** 2]  # exact, so that sum u^2 is exactly 0
    got, ref = ob.jackknife_finish(sums, m), J.finish(sums, m)
    assert np.allclose(got, ref, rtol=1e-12, atol=0)
    assert got[3, 0] == 0.0 and got[3, 1] == 0.0
    assert got[3, 2] == (m[0] - 1) * 0.25 + (m[1] - 1) * -0.5
    # against the definition, from the deviations themselves
    theta = np.vstack(d)
    a_dir, se_dir = J.finish_direct(np.delete(theta, 3, 1), np.ones(len(theta), bool), m[0])
    assert np.allclose(np.delete(got, 3, 0)[:, 0], a_dir, rtol=1e-9)
    assert np.allclose(np.delete(got, 3, 0)[:, 1], se_dir, rtol=1e-9)
    # one empty group adds nothing
    only_a = ob.jackknife_finish(sums, (m[0], 0))
    sums_a = sums.copy()
    sums_a[1] = 0.0
    assert np.array_equal(only_a, J.finish(sums_a, (m[0], 0)))


def test_checks_before_device_work(ob, N):
    lib = N.lib()

    def code(fn):
        with pytest.raises(N.OaxacaError) as e:
            fn()
        return e.value.code

    ob.jackknife_check_shape(6, 100, 100)
    ob.jackknife_check_shape(N.OB_JACK_MAX_K, 200, 200)
    assert code(lambda: ob.jackknife_check_shape(6, 100, 100, heckman=True)) == N.OB_E_UNSUPPORTED
    assert code(lambda: ob.jackknife_check_shape(6, 100, 100, n_norm=1)) == N.OB_E_UNSUPPORTED
    assert code(lambda: ob.jackknife_check_shape(6, 100, 100, n_y=2)) == N.OB_E_UNSUPPORTED
    assert code(lambda: ob.jackknife_check_shape(N.OB_JACK_MAX_K + 1, 500, 500)) == N.OB_E_UNSUPPORTED
    assert code(lambda: ob.jackknife_check_shape(6, 2 ** 24, 1, want_rows=True)) == N.OB_E_UNSUPPORTED
    ob.jackknife_check_shape(6, 2 ** 24, 8)  # the sums output has no such limit
    assert code(lambda: ob.jackknife_check_shape(6, 7, 100)) == N.OB_E_INSUFFICIENT
    assert code(lambda: ob.jackknife_check_shape(6, 100, 7)) == N.OB_E_INSUFFICIENT
    ob.jackknife_check_shape(6, 8, 8)
    assert code(lambda: ob.jackknife_check_shape(0, 8, 8)) == N.OB_E_INVALID
    assert code(lambda: ob.jackknife_check_shape(6, -1, 8)) == N.OB_E_INVALID
    # null handles and bad arguments of the entry points
    o = N.ob_jackknife_out()
    assert lib.ob_jackknife(None, 0, C.byref(o)) == N.OB_E_INVALID
    assert lib.ob_jackknife(None, 0, None) == N.OB_E_INVALID
    assert lib.ob_jackknife_rows(None, 0, None, None, None) == N.OB_E_INVALID
    assert lib.ob_prepared_jackknife(None, C.byref(o)) == N.OB_E_INVALID
    h = C.c_void_p()
    assert lib.ob_prepared_finish_bca(None, None, None, 0, 0.95, C.byref(h)) == N.OB_E_INVALID
    assert lib.ob_builder_run_bca(None, None, 0, 0, None, 0.95, C.byref(h)) == N.OB_E_INVALID
    assert lib.ob_results_jackknife(None, 0, 0, None) == N.OB_E_INVALID
    out = np.zeros(6)
    v = np.ones(3)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    for level in (0.0, 1.0, -0.5, float("nan")):
        assert lib.ob_bca_stats(dp(v), 3, 0.0, 0.0, level, dp(out)) == N.OB_E_INVALID
    assert lib.ob_bca_stats(None, 3, 0.0, 0.0, 0.95, dp(out)) == N.OB_E_INVALID
    assert lib.ob_bca_stats(dp(v), -1, 0.0, 0.0, 0.95, dp(out)) == N.OB_E_INVALID
    assert lib.ob_bca_stats(dp(v), 3, 0.0, 0.0, 0.95, None) == N.OB_E_INVALID
    assert lib.ob_jackknife_finish(None, None, 3, None) == N.OB_E_INVALID
    cols = np.array([9], dtype=np.int32)
    ok = np.ones(3, dtype=np.uint8)
    rows = np.zeros((3, 2))
    rc = lib.ob_aggregate_bca(dp(rows), ok.ctypes.data_as(C.POINTER(C.c_uint8)), 3, 2,
                              cols.ctypes.data_as(C.POINTER(C.c_int32)), 1, dp(v), dp(v), 0.95, dp(out))
    assert rc == N.OB_E_INVALID
    ms = C.c_double(-1.0)
    assert lib.ob_jackknife_last_timing(C.byref(ms)) == N.OB_OK and ms.value >= 0.0
