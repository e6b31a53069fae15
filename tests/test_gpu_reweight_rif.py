"""The reweighted decomposition of a statistic on the GPU (csrc/ob_reweight.hip with the weighted RIF pass of
csrc/ob_rif.hip) against the numpy restatement tests/reweight_rif_ref.py: the point row, 67
replicate rows and the three statistics; bitwise determinism; several statistics in one run; agreement with
decompose_quantile; the mean path as it was; the refusals.

Panels: reweight_ref.panel at 130 + 257 rows, K = 3 and K = 9, weighted and unweighted (4 added to y for the Gini).
Statistics: quantile(0.5), variance, gini, iqr(0.9, 0.1). The rows' tolerance is the parity suite's RTOL (1e-6
relative to max(|ref|, |total_gap|)); nu_A, nu_B, nu_C are held to wrif_ref.TOL.

decompose_quantile. `python tests/reweight_rif_ref.py` measures the difference between the group coefficients of the
two numpy restatements of an unweighted quantile RIF regression (wrif_ref at w = 1 and rif_stat_ref.quantile_rif) on
these panels: 0 at K = 3 and K = 9, so the bound is the floor, 1e-9 relative to the largest coefficient."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reweight_ref as R  # noqa: E402
import reweight_rif_ref as RR  # noqa: E402
import wrif_ref as W  # noqa: E402
from test_gpu_parity import RTOL, SEED, close  # noqa: E402
from test_gpu_reweight import frame_of  # noqa: E402

pytestmark = pytest.mark.gpu

REPS = 64 + 3
QUANTILE_BETA_TOL = max(8 * 0.0, 1e-9)
MEAN_JSON_KEYS = ["total_gap", "aggregate", "detailed_pure_explained", "detailed_specification_error",
                  "detailed_pure_unexplained", "detailed_reweighting_error", "names", "beta_a", "beta_b", "beta_c",
                  "gamma", "xa_mean", "xb_mean", "xc_mean", "y_means", "effective_sample_size", "logit_passes", "n_a",
                  "n_b", "n_failed"]


def builder(ob, k, weighted, stat, reps=REPS):
    f, xs = frame_of(*RR.panel(k, weighted, stat))
    b = ob.OaxacaBuilder(f, "y", "g", "B").predictors(xs).bootstrap_reps(reps).seed(SEED)
    return b.weights("w") if weighted else b


_ref = {}


def ref_run(O, k, weighted, stat, kw):
    """The restatement's point row, its REPS rows from replicate 0 and nu, computed once and shared (read-only)."""
    key = (k, weighted, stat, tuple(sorted(kw.items())))
    if key not in _ref:
        point, rows, ok, nu, norms = RR.run(O, k, weighted, stat, kw, SEED, 0, REPS)
        assert ok.all() and max(len(v) for v in norms) <= 25
        for a in (point, rows):
            a.setflags(write=False)
        _ref[key] = (point, rows, nu)
    return _ref[key]


@pytest.mark.parametrize("stat,kw", RR.STATS, ids=[s for s, _ in RR.STATS])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("k", [3, 9])
def test_rows_match_ref(ob, O, k, weighted, stat, kw):
    point, rows, nu = ref_run(O, k, weighted, stat, kw)
    pr = builder(ob, k, weighted, stat).prepare_reweighted(stat, **kw)
    try:
        assert pr.row_len == R.row_len(k)
        got_point = pr.point_row()
        got, ok = pr.boot(0, REPS)
        got_nu = pr.reweight_statistics()
    finally:
        pr.close()
    assert ok.all() and np.isfinite(got_point).all()
    good, worst = close(got_point, point, point[0])
    print(f"k={k} weighted={weighted} {stat}: point worst {worst:.3e}")
    assert good, worst
    assert got_point[-1] == point[-1]
    worst_all = 0.0
    for r in range(REPS):
        good, worst = close(got[r], rows[r], rows[r][0])
        worst_all = max(worst_all, worst)
        assert good, (r, worst)
    assert np.array_equal(got[:, -1], rows[:, -1])  # the pass counts
    e_nu = max(abs(a - b) / abs(b) for a, b in zip(got_nu, nu))
    print(f"k={k} weighted={weighted} {stat}: replicate worst {worst_all:.3e}, nu worst {e_nu:.3e}")
    assert e_nu <= W.TOL[stat], (got_nu, nu)
    # the row's ybar entries are the weighted means of the RIFs, not nu
    sc = got_point[7 + 11 * k:]
    assert all(np.isfinite(sc[:3]))


@pytest.mark.parametrize("stat,kw", [RR.STATS[0], RR.STATS[2]], ids=["quantile", "gini"])
def test_rows_are_deterministic(ob, N, stat, kw):
    """Bitwise: replicate 5 alone, in a batch of 67, at a shifted first_rep, at hk_batch 1; a repeated call; a second
    handle."""
    b = builder(ob, 3, True, stat, reps=200)
    pr = b.prepare_reweighted(stat, **kw)
    pr2 = b.prepare_reweighted(stat, **kw)
    try:
        r0, k0 = pr.boot(0, 200)
        r1, k1 = pr.boot(0, REPS)
        r2, k2 = pr.boot(5, 1)
        r3, k3 = pr.boot(3, 130)
        r4, k4 = pr.boot(0, 200)
        with N.option("hk_batch", 1):
            r5, k5 = pr.boot(0, 200)
        r6, k6 = pr2.boot(0, REPS)
        assert pr.point_row().tobytes() == pr2.point_row().tobytes()
        assert pr.reweight_statistics() == pr2.reweight_statistics()
    finally:
        pr.close()
        pr2.close()
    assert k0.all()
    assert r0.tobytes() == r4.tobytes() and np.array_equal(k0, k4)
    assert r0[:REPS].tobytes() == r1.tobytes() == r6.tobytes() and np.array_equal(k0[:REPS], k1)
    assert r0[5:6].tobytes() == r2.tobytes() and np.array_equal(k0[5:6], k2)
    assert r0[3:133].tobytes() == r3.tobytes() and np.array_equal(k0[3:133], k3)
    assert r0.tobytes() == r5.tobytes() and np.array_equal(k0, k5)


def _numbers(res):
    comps = (res.aggregate + res.detailed_pure_explained + res.detailed_specification_error +
             res.detailed_pure_unexplained + res.detailed_reweighting_error)
    v = [[c.estimate, c.std_err, c.ci_lower, c.ci_upper, c.t_stat, c.p_value] for c in comps]
    return np.concatenate([np.ravel(v), [res.total_gap, res.effective_sample_size, res.logit_passes], res.beta_a,
                           res.beta_b, res.beta_c, res.gamma, res.xa_mean, res.xb_mean, res.xc_mean, res.y_means,
                           res.statistics])


def test_several_statistics_in_one_run(ob):
    stats = [("gini", {}), ("quantile", {"tau": 0.5}), ("iqr", {"upper": 0.9, "lower": 0.1})]
    b = builder(ob, 3, True, "gini", reps=REPS)
    many = b.decompose_reweighted_statistics(stats)
    assert len(many) == 3
    for (stat, kw), res in zip(stats, many):
        one = b.decompose_reweighted(stat, **kw)
        assert one.statistic == (stat, kw) == res.statistic
        assert (one.n_a, one.n_b, one.n_failed, one.names) == (res.n_a, res.n_b, res.n_failed, res.names)
        assert _numbers(one).tobytes() == _numbers(res).tobytes(), stat
        js = json.loads(one.to_json())
        assert js["statistic"] == {"stat": stat, **kw} and js["statistics"] == list(one.statistics)
    # the three statistics differ, so equality above is not that of one column read three times
    assert len({m.total_gap for m in many}) == 3


def test_quantile_agrees_with_decompose_quantile(ob):
    """Unweighted: beta_A and beta_B of the reweighted quantile decomposition are the group coefficients of
    decompose_quantile (the host's RIF, the OLS engine's Gram and solve), read as its beta_star under GroupA and
    GroupB."""
    for k in (3, 9):
        b = builder(ob, k, False, "quantile", reps=4)
        res = b.decompose_reweighted("quantile", tau=0.5)
        qa = b.reference_coefficients(ob.ReferenceCoefficients.GroupA).decompose_quantile(0.5)
        qb = b.reference_coefficients(ob.ReferenceCoefficients.GroupB).decompose_quantile(0.5)
        for got, want in ((res.beta_a, qa.beta_star), (res.beta_b, qb.beta_star)):
            assert got.shape == want.shape == (k,)
            e = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
            print(f"k={k}: against decompose_quantile {e:.3e} (bound {QUANTILE_BETA_TOL:.1e})")
            assert e <= QUANTILE_BETA_TOL


def test_mean_path_is_untouched(ob):
    b = builder(ob, 3, True, "variance", reps=8)
    res = b.decompose_reweighted()
    assert res.statistic is None and res.statistics is None
    assert list(json.loads(res.to_json()).keys()) == MEAN_JSON_KEYS
    pr = b.prepare_reweighted()
    try:
        with pytest.raises(ob._native.OaxacaError) as e:
            pr.reweight_statistics()
        assert e.value.code == ob._native.OB_E_INVALID
    finally:
        pr.close()


def test_refusals(ob, N):
    b = builder(ob, 3, False, "gini", reps=4)
    with pytest.raises(N.OaxacaError) as e:
        b.cluster("x1").decompose_reweighted("gini")
    assert e.value.code == N.OB_E_UNSUPPORTED
    b = builder(ob, 3, False, "gini", reps=4)
    with pytest.raises(N.OaxacaError) as e:
        b.normalize(["x1"]).decompose_reweighted("gini")
    assert e.value.code == N.OB_E_UNSUPPORTED
    pr = builder(ob, 3, False, "gini", reps=4).prepare_reweighted("gini")
    try:
        with pytest.raises(N.OaxacaError) as e:
            pr.boot_sharded(0, 4)
        assert e.value.code == N.OB_E_UNSUPPORTED
        with pytest.raises(N.OaxacaError) as e:
            pr.jackknife()
        assert e.value.code == N.OB_E_UNSUPPORTED
        rows, ok = pr.boot(0, 4)
        with pytest.raises(N.OaxacaError) as e:
            pr.finish_bca(rows, ok)
        assert e.value.code == N.OB_E_UNSUPPORTED
    finally:
        pr.close()
