"""The delete-one-cluster jackknife on the MI355X against tests/cluster_jack_ref.py: the `rows`
output against brute-force refits (the oracle's single_pass on the frame without the cluster), the `sums` output
against the numpy deviations form, the dropped clusters, determinism, BCa intervals of a clustered run, and the
cluster jackknife standard error as an independent check of the cluster bootstrap's. All tests need an MI355X.

Tolerances. theta_(c): R.TOL = max(8 E, 1e-12) in the mixed error max|got - ref| / max(|ref|, |total_gap|), E measured
on the CPU (cluster_jack_ref.py). Power sums over m kept clusters: every d_c carries at most delta_j = TOL max(|theta_hat_j|,
|total_gap|), so with D_j = max_c |d_cj|: |sum d| <= m delta_j, |sum d^2| <= 2.5 D_j m delta_j, |sum d^3| <= 3.5 D_j^2 m
delta_j (first order in delta_j, the constants 2 and 3 rounded up for the second-order terms)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_jack_ref as R  # noqa: E402
import jackknife_ref as J  # noqa: E402

pytestmark = pytest.mark.gpu


def builder(ob, f, p, ref, weighted, stratified=False, reps=20, extra=(), cluster=True, xs=None):
    xs = [f"x{j}" for j in range(p)] + list(extra) if xs is None else xs
    b = ob.OaxacaBuilder(f, "y", "g", "B").predictors(xs).bootstrap_reps(reps).reference_coefficients(ref).seed(R.SEED)
    if weighted:
        b = b.weights("w")
    return b.cluster("firm", stratified) if cluster else b


def check_sums(jk, refb, ref):
    """The `sums` output against the numpy deviations form, within the bounds of the module docstring."""
    d, kept, hat = R.closed_form(refb, ref, deviations=True, with_point=True)
    sums, used, dropped = R.power_sums(d, kept, R.n_strata_ranges(refb))
    assert jk.n_used == tuple(used) and jk.n_dropped == tuple(dropped), (jk.n_used, used, jk.n_dropped, dropped)
    gap = abs(hat[5])
    delta = R.TOL * np.maximum(np.abs(hat), gap)
    worst = 0.0
    for s, (lo, hi) in enumerate(R.n_strata_ranges(refb)):
        m = max(used[s], 1)
        big = np.abs(d[lo:hi][kept[lo:hi]]).max(0) if used[s] else np.zeros(len(hat))
        bound = np.stack([m * delta, 2.5 * big * m * delta, 3.5 * big ** 2 * m * delta], axis=1)
        err = np.abs(jk.sums[s] - sums[s])
        print(f"stratum {s}: m = {m}, worst |err| / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3e}")
        assert (err <= bound).all(), (s, float((err / np.maximum(bound, 1e-300)).max()))
        worst = max(worst, float((err[:, 0] / (m * np.maximum(np.abs(hat), gap))).max()))
    want = J.finish(sums, used)
    got = np.stack([jk.accel, jk.std_err, jk.bias], axis=1)
    # the handle's statistics are ob_jackknife_finish of its own sums, a stratum taken as a group (a few f64 roundings)
    own = J.finish(jk.sums, jk.n_used)
    live = got[:, 1] > 1e-9 * np.maximum(np.abs(hat), gap)  # explained:intercept is 0 in every fit: its accel is noise
    assert np.allclose(got[:, 1:], own[:, 1:], rtol=1e-7, atol=1e-13 * gap) and np.allclose(got[live, 0], own[live, 0], rtol=1e-6)
    mtot = sum(used)
    assert (np.abs(got[:, 2] - want[:, 2]) <= max(mtot - 1, 1) * delta).all()              # bias = sum_s (m_s - 1) dbar_s
    assert (np.abs(got[:, 1] - want[:, 1]) <= 2 * mtot ** 0.5 * delta).all()               # se: |u|_2 moves by <= 2 delta sqrt(m)
    return worst


def check_rows(pr, refb, clusters=None):
    """The `rows` output against brute force on `clusters` (all by default) -> (theta, kept, full rows)."""
    theta, kept, dropped, dev = pr.cluster_jackknife_rows(deviations=True)
    bt, bk = R.brute(refb, clusters)
    idx = np.arange(refb.n_clusters) if clusters is None else np.asarray(clusters)
    assert np.array_equal(kept[idx], bk), (kept[idx].tolist(), bk.tolist())
    assert np.isnan(theta[~kept]).all()
    if clusters is None:
        want = [int((~bk[lo:hi]).sum()) for lo, hi in R.n_strata_ranges(refb)] + [0]
        assert dropped == tuple(want[:2])
    if bk.any():
        gap = refb.b.point(refb.prep)[0][5]
        e = R.mixed_error(theta[idx][bk], bt[bk], gap)
        print(f"rows vs brute force: mixed error {e:.3e} (TOL {R.TOL:.3e})")
        assert e <= R.TOL, e
        # the sums path's own deviations, cluster by cluster: d + theta_hat is theta_(c) as well
        hat = pr.point_row()[:theta.shape[1]]
        e = R.mixed_error(dev[idx][bk] + hat[None, :], bt[bk], gap)
        print(f"deviations + point vs brute force: mixed error {e:.3e}")
        assert e <= R.TOL, e
    assert np.isnan(dev[~kept]).all()
    return theta, kept


@pytest.mark.parametrize("ref", R.REF_RULES)
@pytest.mark.parametrize("shape,weighted,stratified", R.CASES)
def test_rows_and_sums(ob, O, N, shape, weighted, stratified, ref):
    n_a, n_b, p, c = shape
    f = R.case_frame(shape, weighted, stratified)
    refb = R.reference(O, f, p, ref, weighted, stratified)
    pr = builder(ob, f, p, ref, weighted, stratified).prepare()
    try:
        assert pr.cluster_info["n_clusters"] == c == refb.n_clusters
        theta, kept = check_rows(pr, refb)
        if c == 2:  # a stratum with fewer than 2 kept clusters has no jackknife variance
            assert not kept.all()
            with pytest.raises(ob.OaxacaError) as e:
                pr.cluster_jackknife()
            assert e.value.code == N.OB_E_INSUFFICIENT
            return
        assert kept.all()
        if not stratified:  # the panel mixes clusters that span both groups with clusters that lie in one
            sizes = np.array([[len(refb.members[g][cc]) for g in (0, 1)] for cc in range(c)])
            assert ((sizes > 0).all(1)).any() and (sizes[:, 0] == 0).any() and (sizes[:, 1] == 0).any()
        else:  # a deleted A-cluster leaves B's beta bitwise at the point estimate, and the other way round
            full, _, _ = pr.cluster_jackknife_rows(full=True)
            k, point = p + 1, pr.point_row()
            tail = 6 + 2 * k
            a_rows, b_rows = full[:refb.c_a], full[refb.c_a:]
            assert (a_rows[:, tail + k:tail + 2 * k] == point[tail + k:tail + 2 * k]).all()
            assert (b_rows[:, tail:tail + k] == point[tail:tail + k]).all()
            assert (a_rows[:, tail + 3 * k:tail + 4 * k] == point[tail + 3 * k:tail + 4 * k]).all()
            assert not (a_rows[:, tail:tail + k] == point[tail:tail + k]).all()
        check_sums(pr.cluster_jackknife(), refb, ref)
        assert ob.cluster_jackknife_last_timing() > 0.0
    finally:
        pr.close()


def test_singleton_clusters(ob, O):
    """C = 1,030 on 3,000 rows, the last 103 clusters singletons: brute force on 16 sampled clusters."""
    f = R.singleton_frame()
    refb = R.reference(O, f, 3, 2, True, False)
    assert refb.n_clusters == 1030
    sizes = np.array([len(refb.members[0][c]) + len(refb.members[1][c]) for c in range(1030)])
    assert (sizes == 1).sum() >= 100
    sample = sorted(set(np.random.default_rng(1).choice(1030, 12, replace=False).tolist())
                    | set(np.flatnonzero(sizes == 1)[:4].tolist()) | {0})[:16]
    pr = builder(ob, f, 3, 2, True).prepare()
    try:
        check_rows(pr, refb, sample)
        check_sums(pr.cluster_jackknife(), refb, 2)
    finally:
        pr.close()


@pytest.mark.parametrize("ref", [0, 2, 4])
def test_one_cluster_holds_most_rows(ob, O, ref):
    f = R.big_cluster_frame()
    refb = R.reference(O, f, 3, ref, True, False)
    big = refb.labels.index("f0")
    assert len(refb.members[0][big]) > 150 and len(refb.members[1][big]) > 155  # more than half of 300 / 310
    pr = builder(ob, f, 3, ref, True).prepare()
    try:
        check_rows(pr, refb)
        check_sums(pr.cluster_jackknife(), refb, ref)
    finally:
        pr.close()


def test_many_clusters_deterministic(ob, O):
    """C = 5,000 on 20,000 + 20,001 rows, p = 5, WLS: many blocks and slots; two handles return equal bytes."""
    f = R.many_cluster_frame()
    refb = R.reference(O, f, 5, 2, True, False)
    assert refb.n_clusters == 5000
    out = []
    for _ in range(2):
        pr = builder(ob, f, 5, 2, True).prepare()
        try:
            out.append(pr.cluster_jackknife())
        finally:
            pr.close()
    assert out[0].sums.tobytes() == out[1].sums.tobytes() and out[0].n_used == out[1].n_used == (5000, 0)
    for key in ("accel", "std_err", "bias"):
        assert getattr(out[0], key).tobytes() == getattr(out[1], key).tobytes()
    check_sums(out[0], refb, 2)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ref", [0, 2])
def test_dummy_confined_to_one_cluster(ob, O, weighted, ref):
    """The dummy's ones all lie in cluster `f3`: that cluster is dropped, and the oracle's refit fails on exactly it."""
    f = R.dummy_frame(weighted)
    refb = R.reference(O, f, 2, ref, weighted, False, extra=("d",))
    _, bk = R.brute(refb)
    assert (~bk).tolist() == [lab == "f3" for lab in refb.labels]
    pr = builder(ob, f, 2, ref, weighted, extra=("d",)).prepare()
    try:
        theta, kept = check_rows(pr, refb)
        assert kept.tolist() == bk.tolist()
        jk = pr.cluster_jackknife()
        assert jk.n_dropped == (1, 0) and jk.n_used == (8, 0)
        check_sums(jk, refb, ref)
    finally:
        pr.close()


def test_zero_weight_cluster_is_kept(ob, O):
    """Every weight of cluster `f4` is zero: it is kept and moves nothing. r_c = 0, S_c = 0, W_c = 0, so every
    deviation the sums kernel forms for it is 0.0 exactly, on the device as in the numpy form; its theta_(c) from the
    solve kernel (T_g - 0 in place of G_g) stays within TOL of the point estimate."""
    f = R.zero_weight_frame()
    refb = R.reference(O, f, 2, 4, True, False)
    d, kept = R.closed_form(refb, 4, deviations=True)
    z = refb.labels.index("f4")
    assert kept[z] and (d[z] == 0.0).all()
    pr = builder(ob, f, 2, 4, True).prepare()
    try:
        theta, gk = check_rows(pr, refb)
        assert gk[z]
        _, _, _, dev = pr.cluster_jackknife_rows(deviations=True)
        assert (dev[z] == 0.0).all() and all((dev[c] != 0.0).any() for c in range(5) if c != z)
        point = pr.point_row()[:theta.shape[1]]
        assert R.mixed_error(theta[z], point, point[5]) <= R.TOL
        jk = pr.cluster_jackknife()
        assert jk.n_used == (5, 0)
        check_sums(jk, refb, 4)
    finally:
        pr.close()


def _group_q(ob, refb, g):
    """cluster_gram of group g over the restatement's clusters (rows sorted stably by cluster id)."""
    p = refb.prep
    x, y, w = (p["xa"], p["ya"], p["wa"]) if g == 0 else (p["xb"], p["yb"], p["wb"])
    ids = np.empty(len(y), dtype=np.int64)
    for c, m in enumerate(refb.members[g]):
        ids[m] = c
    perm = np.argsort(ids, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=refb.n_clusters))])
    return ob.cluster_gram(np.ascontiguousarray(x[:, 1:]), y, w, perm, off)


@pytest.mark.parametrize("ref", [0, 2, 4])
@pytest.mark.parametrize("stratified", [False, True])
def test_array_entry_points(ob, O, ref, stratified):
    """cluster_gram()'s output fed to ob_cluster_jackknife / ob_cluster_jackknife_rows: the same clusters kept, the
    sums within the bounds of the numpy form (the point Gram is the sum of Q here, the unit Gram on the handle: only
    rounding differs), theta_(c) within TOL of brute force, and the prepared handle's result beside it."""
    shape, weighted = (400, 417, 16, 67), True
    f = R.case_frame(shape, weighted, stratified)
    refb = R.reference(O, f, 16, ref, weighted, stratified)
    p = refb.prep
    (qa, ra), (qb, rb) = _group_q(ob, refb, 0), _group_q(ob, refb, 1)
    panel = ob.Panel(p["xa"][:, 1:], p["ya"], p["xb"][:, 1:], p["yb"], p["wa"], p["wb"], device=0)
    row = panel.point_estimate(ref)
    k, c = 17, 6 + 2 * 17
    nca = refb.c_a if stratified else None
    jk = ob.cluster_jackknife(qa, qb, ra, rb, row[c:c + 5 * k], len(p["ya"]), len(p["yb"]), weighted, ref, n_clusters_a=nca)
    check_sums(jk, refb, ref)
    theta, kept, dropped, dev = ob.cluster_jackknife_rows(panel, qa, qb, ra, rb, ref, n_clusters_a=nca, deviations=True)
    bt, bk = R.brute(refb)
    assert np.array_equal(kept, bk) and dropped == (0, 0)
    gap = refb.b.point(refb.prep)[0][5]
    assert R.mixed_error(theta[:, :c], bt, gap) <= R.TOL
    assert R.mixed_error(dev + row[None, :c], bt, gap) <= R.TOL
    pr = builder(ob, f, 16, ref, weighted, stratified).prepare()
    try:
        own = pr.cluster_jackknife()
        ptheta, pkept, _ = pr.cluster_jackknife_rows(full=True)
    finally:
        pr.close()
    assert own.n_used == jk.n_used and np.array_equal(pkept, kept)
    assert R.mixed_error(theta, ptheta, gap) <= R.TOL  # two summation orders of the same panel
    scale = np.maximum(np.abs(own.estimate), abs(gap))
    assert (np.abs(jk.estimate - own.estimate) <= R.TOL * scale).all()
    assert (np.abs(jk.std_err - own.std_err) <= 2 * 2 * 67 ** 0.5 * R.TOL * scale).all()  # each within 2 delta sqrt(m) of numpy


def test_run_cluster_bca(ob, O, N):
    from test_gpu_cluster import make_frame

    f = make_frame(3000, 3, 67, 21, True)
    preds = ["x0", "x1", "x2"]
    mk = lambda: builder(ob, f, 3, 2, True, reps=999)
    plain, bca = mk().run(), mk().run_cluster_bca(0.95)
    assert plain.jackknife is None and bca.jackknife and bca.n_clusters == 67 == plain.n_clusters
    tables = lambda r: {"two_fold": r.two_fold.aggregate, "three_fold": r.three_fold.aggregate,
                        "detailed_explained": r.two_fold.detailed_explained,
                        "detailed_unexplained": r.two_fold.detailed_unexplained}
    pr = mk().prepare()
    try:
        rows, ok = pr.boot(0, 999)
        assert ok.all()
        jk = pr.cluster_jackknife()
        assert jk.n_dropped == (0, 0) and jk.n_used == (67, 0)
        again = pr.finish_cluster_bca(rows, ok, 0.95)
        with pytest.raises(ob.OaxacaError) as e:  # the delete-one-row forms keep refusing a clustered handle
            pr.finish_bca(rows, ok)
        assert e.value.code == N.OB_E_UNSUPPORTED
    finally:
        pr.close()
    col = {("two_fold", "explained"): 0, ("two_fold", "unexplained"): 1, ("three_fold", "endowments"): 2,
           ("three_fold", "coefficients"): 3, ("three_fold", "interaction"): 4}
    names = ["__ob_intercept__"] + preds
    for j, nm in enumerate(names):
        col[("detailed_explained", nm)] = 6 + j
        col[("detailed_unexplained", nm)] = 6 + len(names) + j
    for t, comps in tables(bca).items():
        for c0, c1, c2 in zip(tables(plain)[t], comps, tables(again)[t]):
            assert (c0.name, c0.estimate, c0.std_err, c0.p_value, c0.t_stat) == \
                   (c1.name, c1.estimate, c1.std_err, c1.p_value, c1.t_stat)
            j = col[(t, c1.name)]
            info = bca.jackknife[(t, c1.name)]
            assert info["accel"] == jk.accel[j] and info["std_err"] == jk.std_err[j] and info["bias"] == jk.bias[j]
            want = J.bca(rows[:, j], c1.estimate, jk.accel[j], 0.95)
            assert want["flag"] == info["flag"]
            if want["flag"] == 0:
                for key in ("alpha_lo", "alpha_hi"):
                    assert abs(want[key] * 999 - round(want[key] * 999)) > 1e-6
                assert (c1.ci_lower, c1.ci_upper) == (want["ci_lower"], want["ci_upper"])
            else:
                assert np.isnan(c1.ci_lower) and np.isnan(c1.ci_upper)
            assert (c2.ci_lower, c2.ci_upper) == (c1.ci_lower, c1.ci_upper) or want["flag"] != 0
    # the reference acceleration: the numpy deviations form gives the same one to the sums' bounds
    refb = R.reference(O, f, 3, 2, True, False, reps=999)
    check_sums(jk, refb, 2)


def test_statistic_builder_runs_cluster_bca(ob):
    from test_gpu_cluster import make_frame

    f = make_frame(3000, 3, 67, 9, False)
    b = builder(ob, f, 3, 1, False, reps=60).statistic_builder("variance")
    res = b.run_cluster_bca()
    assert res.n_clusters == 67 and res.jackknife
    assert all(np.isfinite(v["std_err"]) and v["std_err"] > 0 for (t, _), v in res.jackknife.items() if t == "two_fold")


def test_cluster_shock_jackknife_se(ob, O):
    """A strong per-cluster shock: the cluster jackknife SE of total_gap exceeds the delete-one-row jackknife SE of the
    same panel run unclustered, and lies closer (in log ratio) to the cluster bootstrap SE than to the row bootstrap
    SE. The restatements alone satisfy both conditions at this seed (test_cluster_jack_host.py checks that)."""
    f = R.shock_frame()
    xs = ["x0"]
    b = builder(ob, f, 1, 0, False, reps=200, xs=xs)
    plain = builder(ob, f, 1, 0, False, reps=200, xs=xs, cluster=False)
    cj = b.cluster_jackknife().std_err[5]
    rj = plain.jackknife().std_err[5]
    pr = b.prepare()
    try:
        rows, ok = pr.boot(0, 200)
    finally:
        pr.close()
    pp = plain.prepare()
    try:
        prow, pok = pp.boot(0, 200)
        with pytest.raises(ob.OaxacaError) as e:
            pp.cluster_jackknife()
        assert e.value.code == ob._native.OB_E_INVALID
        with pytest.raises(ob.OaxacaError) as e:
            pp.finish_cluster_bca(prow, pok)
        assert e.value.code == ob._native.OB_E_INVALID
    finally:
        pp.close()
    se_c, se_r = rows[ok.astype(bool), 5].std(ddof=1), prow[pok.astype(bool), 5].std(ddof=1)
    print(f"cluster jack {cj:.5f}, row jack {rj:.5f}, cluster boot {se_c:.5f}, row boot {se_r:.5f}")
    assert cj > rj
    assert abs(np.log(cj / se_c)) < abs(np.log(cj / se_r))
