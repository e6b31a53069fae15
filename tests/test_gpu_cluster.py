"""The cluster bootstrap on the MI355X against the numpy restatement of tests/cluster_ref.py:
the OBRC-1 counts exactly, the per-cluster Grams and counts x Q to 1e-12 of sqrt(G_aa G_bb) (only the summation
order differs), bytewise determinism over batches and first_rep, replicate rows / ok masks against explicitly
gathered frames to test_gpu_parity's 1e-6 * max(|ref|, |total_gap|), dropped replicates, and the builder end to end.
All tests need an MI355X."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_ref as R  # noqa: E402
from test_gpu_parity import close, compare_results  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 0x0B5EED
FAR = 2 ** 32 - 40


def make_frame(n, p, c, seed, weighted, ints=False, sector=False):
    """~n rows in c clusters: cluster 0 holds ~700 rows (several 256-row pieces) of both groups, cluster 1 (c >= 5)
    lies in group A only and cluster 2 in B only, the last c // 10 clusters are singletons, rows are shuffled."""
    rng = np.random.default_rng(seed)
    single = c // 10
    sizes = np.ones(c, dtype=np.int64)
    big = min(700, n // 3)
    sizes[0] = big
    mid = c - 1 - single
    if mid > 0:
        sizes[1:1 + mid] += rng.multinomial(n - big - (c - 1), np.ones(mid) / mid)
    cl = rng.permutation(np.repeat(np.arange(c), sizes))
    m = len(cl)
    g = np.where(rng.random(m) < 0.45, "A", "B")
    if c >= 5:
        g[cl == 1], g[cl == 2] = "A", "B"
    x = rng.normal(size=(m, p)) + (g == "A")[:, None] * 0.3
    y = 1.0 + x @ rng.normal(0.2, 0.1, p) + (g == "A") * 0.25 + rng.normal(0, 0.5, m)
    f = {"y": y.tolist(), "g": g.tolist(), "firm": (cl + 100).tolist() if ints else [f"f{v}" for v in cl]}
    for j in range(p):
        f[f"x{j}"] = x[:, j].tolist()
    if weighted:
        f["w"] = rng.uniform(0.5, 2.0, m).tolist()
    if sector:
        f["sector"] = rng.choice(["agri", "manu", "serv"], m).tolist()
    return f


def builders(ob, O, f, p, ref, weighted, reps=37, stratified=False, cluster="firm", cats=(), norm=()):
    """(the row-bootstrap builder, the same builder with .cluster(), the restatement)."""
    xs = [f"x{j}" for j in range(p)]

    def mk():
        b = (ob.OaxacaBuilder(f, "y", "g", "B").predictors(xs).categorical_predictors(list(cats))
             .normalize(list(norm)).bootstrap_reps(reps).reference_coefficients(ref).seed(SEED))
        return b.weights("w") if weighted else b

    ref_b = R.ClusterRef(O, f, "y", "g", "B", cluster, stratified, predictors=xs, categorical=list(cats),
                         normalize=list(norm), reps=reps, ref_mode=ref, weights="w" if weighted else None, seed=SEED)
    return mk(), mk().cluster(cluster, stratified), ref_b


# ---- the three kernels ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,reps", [(2, 37), (5, 37), (67, 1), (67, 300), (1030, 37), (13000, 3)])
def test_counts_match_obrc1(ob, O, c, reps):
    """Both modes, at first_rep 0 and 2^32 - 40; C = 13000 runs the global-atomics kernel (beyond one block's LDS)."""
    ca = max(1, c // 3)
    for first, n in ((0, reps), (FAR, min(reps, 40))):  # replicate ids end at 2^32 - 1
        assert np.array_equal(ob.cluster_counts(SEED, first, n, c), R.counts(O, SEED, first, n, c))
        got = ob.cluster_counts(SEED, first, n, ca, c - ca, stratified=True)
        assert np.array_equal(got, R.counts(O, SEED, first, n, ca, c - ca, True))


def _pairs(k1):
    return [(a, b) for a in range(k1) for b in range(a, k1)]


def _check_gram(got, want, k1):
    """|got - want| <= 1e-12 sqrt(G_aa G_bb) entry by entry (test_gpu_gram_i8.py's mixed tolerance)."""
    pairs = _pairs(k1)
    diag = [i for i, (a, b) in enumerate(pairs) if a == b]
    d = np.abs(want[..., diag])
    worst = 0.0
    for e, (a, b) in enumerate(pairs):
        scale = np.sqrt(d[..., a] * d[..., b])
        err = np.abs(got[..., e] - want[..., e])
        assert ((err <= 1e-12 * scale) | (scale == 0)).all(), (a, b, float((err / np.maximum(scale, 1e-300)).max()))
        worst = max(worst, float((err / np.maximum(scale, 1e-300))[scale > 0].max(initial=0.0)))
    return worst


def _group_arrays(f, p, weighted, which):
    rows = [i for i, g in enumerate(f["g"]) if g == which]
    x = np.array([[f[f"x{j}"][i] for j in range(p)] for i in rows]).reshape(len(rows), p)
    y = np.array([f["y"][i] for i in rows])
    w = np.array([f["w"][i] for i in rows]) if weighted else None
    return rows, x, y, w


@pytest.mark.parametrize("p", [3, 20])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("c", [5, 1030])
def test_cluster_gram_matches_numpy(ob, p, weighted, c):
    f = make_frame(3000, p, c, 11 + p, weighted)
    grp = [0 if g == "A" else 1 for g in f["g"]]
    ix = ob.cluster_index(f["firm"], grp)
    assert ix["n_clusters"] == c and ix["max_cluster_rows"] >= 600
    pairs = _pairs(p + 2)
    for key, which in (("a", "A"), ("b", "B")):
        _, x, y, w = _group_arrays(f, p, weighted, which)
        q, rows = ob.cluster_gram(x, y, w, ix["perm_" + key], ix["off_" + key])
        v = np.hstack([np.ones((len(y), 1)), x, y[:, None]])
        if weighted:
            v = v * np.sqrt(w)[:, None]
        want = np.zeros((c, len(pairs)))
        off, perm = ix["off_" + key], ix["perm_" + key]
        for cc in range(c):
            vc = v[perm[off[cc]:off[cc + 1]]]
            want[cc] = [(vc[:, a] * vc[:, b]).sum() for a, b in pairs]
        assert np.array_equal(rows, np.diff(off))
        assert (rows == 0).any() and (c == 5 or (rows == 1).any())  # one-group clusters; singletons at C = 1030
        _check_gram(q, want, p + 2)
        q2, _ = ob.cluster_gram(x, y, w, ix["perm_" + key], ix["off_" + key])
        assert np.array_equal(q, q2)


@pytest.mark.parametrize("c,reps,k1", [(2, 37, 5), (5, 1, 22), (67, 300, 22), (1030, 37, 5), (8200, 37, 5)])
def test_cluster_apply_matches_numpy(ob, c, reps, k1):
    """counts x Q against numpy; C = 8200 crosses the 8192-cluster run, so partial sums are reduced."""
    rng = np.random.default_rng(c)
    e = k1 * (k1 + 1) // 2
    v = rng.normal(size=(c, 3, k1))
    pairs = _pairs(k1)
    q = np.stack([(v[:, :, a] * v[:, :, b]).sum(1) for a, b in pairs], 1)  # a PSD Gram per cluster
    counts = rng.multinomial(c, np.ones(c) / c, size=reps).astype(np.uint32)
    got = ob.cluster_apply(counts, q)
    want = counts.astype(np.float64) @ q
    assert got.shape == (reps, e)
    _check_gram(got, want, k1)
    assert np.array_equal(got, ob.cluster_apply(counts, q))
    sub = ob.cluster_apply(counts[reps // 2:reps // 2 + 1], q)  # a replicate alone: the same bytes
    assert np.array_equal(sub[0], got[reps // 2])


# ---- replicate rows ---------------------------------------------------------------------------------------------
def _compare_rows(pr, refb, first, n):
    rows, ok = pr.boot(first, n)
    rrows, rok = refb.rows(first, n)
    assert np.array_equal(ok, rok), (ok.tolist(), rok.tolist())
    gap = refb.b.point(refb.prep)[0][5]
    m = ok.astype(bool)
    good, worst = close(rows[m], rrows[m], gap)
    assert good, worst
    assert np.isnan(rows[~m]).all()
    return rows, ok


@pytest.mark.parametrize("ref", [0, 1, 2, 4])  # GroupA, GroupB, Pooled, Cotton: the four distinct beta* rules
@pytest.mark.parametrize("p,weighted,c", [(3, False, 67), (20, True, 67)])
def test_rows_match_gathered_frames(ob, O, ref, p, weighted, c):
    f = make_frame(3000, p, c, 5 + p, weighted)
    _, b, refb = builders(ob, O, f, p, ref, weighted)
    pr = b.prepare()
    try:
        assert pr.cluster_info["n_clusters"] == c == refb.n_clusters
        _compare_rows(pr, refb, 0, 37)
    finally:
        pr.close()


@pytest.mark.parametrize("c,ints", [(2, False), (5, True), (1030, False)])
def test_rows_other_cluster_counts(ob, O, c, ints):
    """C = 2 and 5 (below / no multiple of the MFMA k-step; at C = 5 replicates that miss a group's clusters are
    dropped on both sides), C = 1030 with integer ids elsewhere; a normalized categorical rides along."""
    f = make_frame(3000, 3, c, 40 + c, True, ints=ints, sector=True)
    _, b, refb = builders(ob, O, f, 3, 2, True, cats=["sector"], norm=["sector"])
    pr = b.prepare()
    try:
        _compare_rows(pr, refb, 0, 37)
        _compare_rows(pr, refb, FAR, 5)
    finally:
        pr.close()


def test_determinism(ob, O):
    import torch

    f = make_frame(3000, 3, 67, 8, True)
    _, b, _ = builders(ob, O, f, 3, 2, True)
    pr = b.prepare()
    try:
        alone = pr.boot(100, 37)
        inside = pr.boot(0, 300)
        assert np.array_equal(alone[0], inside[0][100:137], equal_nan=True) and np.array_equal(alone[1], inside[1][100:137])
        again = pr.boot(100, 37)
        assert np.array_equal(alone[0], again[0], equal_nan=True) and np.array_equal(alone[1], again[1])
        dev = torch.device("cuda", 0)
        rows = torch.empty((37, pr.row_len), dtype=torch.float64, device=dev)
        ok = torch.empty(37, dtype=torch.uint8, device=dev)
        s = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(s):
            pr.boot_device(100, 37, rows.data_ptr(), ok.data_ptr(), s.cuda_stream)
        pr.sync()
        assert np.array_equal(rows.cpu().numpy(), alone[0], equal_nan=True) and np.array_equal(ok.cpu().numpy(), alone[1])
        t = ob.cluster_last_timing()
        assert t["apply_ms"] > 0 and t["counts_ms"] > 0 and t["solve_ms"] > 0
    finally:
        pr.close()
    pr2 = b.prepare()  # a fresh handle: Q formed again, the same bytes
    try:
        fresh = pr2.boot(100, 37)
        assert np.array_equal(alone[0], fresh[0], equal_nan=True)
    finally:
        pr2.close()


DROP_SEED = 3  # the restatement drops some and keeps some of its 64 replicates at this seed (asserted below)


def test_dropped_replicates(ob, O):
    """C = 3, joint: cluster `b` holds all of group B, so a replicate that misses it (p = (2/3)^3 ~ 30 %) has no B
    rows and is dropped (the reference's InsufficientData)."""
    rng = np.random.default_rng(1)
    n = 300
    firm = np.where(np.arange(n) < 120, "b", np.where(np.arange(n) % 2 == 0, "a1", "a2"))
    g = np.where(firm == "b", "B", "A")
    x = rng.normal(size=n)
    f = {"y": (1 + 0.5 * x + (g == "A") * 0.3 + rng.normal(0, 0.4, n)).tolist(), "g": g.tolist(), "x0": x.tolist(),
         "firm": firm.tolist()}
    refb = R.ClusterRef(O, f, "y", "g", "B", "firm", predictors=["x0"], reps=64, ref_mode=3, seed=DROP_SEED)
    rrows, rok = refb.rows(0, 64)
    assert 0 < rok.sum() < 64  # on the CPU: the seed gives both kinds
    b = (ob.OaxacaBuilder(f, "y", "g", "B").predictors(["x0"]).bootstrap_reps(64).reference_coefficients(3)
         .seed(DROP_SEED).cluster("firm"))
    pr = b.prepare()
    try:
        rows, ok = pr.boot(0, 64)
    finally:
        pr.close()
    assert np.array_equal(ok, rok)
    res = b.run()
    assert res.n_failed == int(64 - rok.sum()) and res.n_clusters == 3
    compare_results(res, refb.run())


# ---- the builder end to end -------------------------------------------------------------------------------------
def test_run_matches_restatement_and_keeps_estimates(ob, O):
    f = make_frame(3000, 3, 67, 21, True, sector=True)
    plain, _, _ = builders(ob, O, f, 3, 2, True, reps=150, cats=["sector"])
    base = plain.run()
    assert base.n_clusters is None
    _, b, refb = builders(ob, O, f, 3, 2, True, reps=150, cats=["sector"])
    res = b.run()
    compare_results(res, refb.run())
    assert res.n_clusters == 67
    for t in ("aggregate", "detailed_explained", "detailed_unexplained"):
        assert [c.estimate for c in getattr(res.two_fold, t)] == [c.estimate for c in getattr(base.two_fold, t)]
    assert res.total_gap == base.total_gap and np.array_equal(res.residuals, base.residuals)
    via = ob.OaxacaBlinder(f, "y", "g", "B", ["x0", "x1", "x2"], ["sector"], bootstrap_reps=150, weights="w", seed=SEED,
                           cluster="firm")
    assert via._create_builder()._cluster == "firm"


def test_cluster_shock_widens_the_interval(ob, O):
    """A strong per-cluster shock in the outcome: the clustered SE of total_gap agrees with the restatement's and
    both exceed the row bootstrap's from the same builder."""
    rng = np.random.default_rng(4)
    n, c = 3000, 40
    cl = rng.integers(0, c, n)
    g = np.where(rng.random(n) < 0.5, "A", "B")
    x = rng.normal(size=n)
    y = 1 + 0.5 * x + (g == "A") * 0.3 + rng.normal(0, 1.0, c)[cl] * np.where(g == "A", 1.0, -1.0) + rng.normal(0, 0.3, n)
    f = {"y": y.tolist(), "g": g.tolist(), "x0": x.tolist(), "firm": cl.tolist()}
    plain, _, _ = builders(ob, O, f, 1, 0, False, reps=200)
    se_rows = plain.run()
    _, b, refb = builders(ob, O, f, 1, 0, False, reps=200)
    res, want = b.run(), refb.run()
    compare_results(res, want)
    # total_gap = explained + unexplained; its replicate column is row[5]
    pr = b.prepare()
    try:
        rows, ok = pr.boot(0, 200)
    finally:
        pr.close()
    rrows, rok = refb.rows(0, 200)
    se_c, se_r = rows[ok.astype(bool), 5].std(ddof=1), rrows[rok.astype(bool), 5].std(ddof=1)
    assert abs(se_c - se_r) <= 1e-6 * max(se_r, abs(want["total_gap"]))
    pp = plain.prepare()
    try:
        prow, pok = pp.boot(0, 200)
    finally:
        pp.close()
    se_plain = prow[pok.astype(bool), 5].std(ddof=1)
    assert se_c > se_plain and se_r > se_plain, (se_c, se_r, se_plain)
    assert res.unexplained().std_err > se_rows.unexplained().std_err


def test_stratified_nested_ids(ob, O):
    f = make_frame(3000, 3, 67, 33, False)
    f["worker"] = [(7 * i) % 400 * 2 + (0 if g == "A" else 1) for i, g in enumerate(f["g"])]  # nested in the groups
    _, b, refb = builders(ob, O, f, 3, 3, False, stratified=True, cluster="worker")
    pr = b.prepare()
    try:
        info = pr.cluster_info
        assert info["stratified"] == 1 and info["n_clusters_a"] + info["n_clusters_b"] == info["n_clusters"]
        assert (info["n_clusters_a"], info["n_clusters_b"]) == (refb.c_a, refb.c_b)
        _compare_rows(pr, refb, 0, 37)
    finally:
        pr.close()
    compare_results(b.run(), refb.run())
    with pytest.raises(ob.OaxacaError) as e:
        b.cluster("firm", stratified=True).run()
    assert e.value.code == ob._native.OB_E_INVALID and "both groups" in str(e.value)


def test_decompose_quantile_clustered(ob, O):
    f = make_frame(3000, 3, 67, 9, False)
    plain, _, _ = builders(ob, O, f, 3, 1, False, reps=60)
    base = plain.decompose_quantile(0.5)
    _, b, _ = builders(ob, O, f, 3, 1, False, reps=60)
    res = b.decompose_quantile(0.5)
    assert res.n_clusters == 67 and base.n_clusters is None
    assert [c.estimate for c in res.two_fold.aggregate] == [c.estimate for c in base.two_fold.aggregate]
    assert all(np.isfinite(c.std_err) and c.std_err > 0 for c in res.two_fold.aggregate)
    many = b.decompose_quantiles([0.25, 0.5])
    assert [c.std_err for c in many[1].two_fold.aggregate] == [c.std_err for c in res.two_fold.aggregate]


def test_unsupported_on_a_clustered_builder(ob, O):
    N = ob._native
    f = make_frame(3000, 3, 67, 9, False)
    _, b, _ = builders(ob, O, f, 3, 0, False)
    for call in (b.run_bca, b.jackknife):
        with pytest.raises(ob.OaxacaError) as e:
            call()
        assert e.value.code == N.OB_E_UNSUPPORTED
    pr = b.prepare()
    try:
        rows, ok = pr.boot(0, 8)
        for call in (lambda: pr.boot_sharded(0, 8), pr.jackknife, lambda: pr.finish_bca(rows, ok)):
            with pytest.raises(ob.OaxacaError) as e:
                call()
            assert e.value.code == N.OB_E_UNSUPPORTED
        assert pr.finish(rows, ok).n_clusters == 67
    finally:
        pr.close()
