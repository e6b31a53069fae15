"""References for the delete-one-cluster jackknife tests, plain numpy plus the oracle.

1. brute(): drop every row of cluster c and call oracle.single_pass on what is left. This is the reference's
   own algorithm on a frame without the cluster and the yardstick; a group left with rows <= K, or a pass that
   fails, is a dropped cluster.
2. closed_form(): the downdate formulas of the device pass in numpy f64. For cluster c and group g, with
   Q^xx_c, b_c, S_c, W_c, Y_c the cluster's sums of w x x', w x y, w x, w, w y:
     M = G_g - Q^xx_c,  r_c = b_c - Q^xx_c beta_g,  beta_g(c) - beta_g = -M^-1 r_c,
     xbar_g(c) - xbar_g = (W_c xbar_g - S_c) / (W_g - W_c), the mean outcome likewise,
   Pooled: the same downdate of the pooled Gram on [x, 1[g = A]] with the indicator's coefficient removed,
   Weighted: s from W_g - W_c. A group without a row of the cluster stays at the point estimate. A cluster is
   dropped when n_g - rows <= K for a group it touches, W_g - W_c <= 0, or a Cholesky pivot of M (of the pooled
   downdate) is at most 2^-40 times the same pivot of the point estimate's factor.
   closed_form(deviations=True) gives d = theta_(c) - theta_hat formed from the changes themselves (u'v' - uv =
   du v' + u dv), which is what the power sums need: jack_bias multiplies d's mean by m - 1.

Tolerance. E = the largest mixed error max|closed - brute| / max(|brute|, |total_gap|) over the panels of
tests/test_gpu_cluster_jack.py (every shape, reference rule, weighting and mode of CASES, the dummy and the
zero-weight panels), measured on x86-64 by `python tests/cluster_jack_ref.py`:
    E = 1.65e-14
The device sums the same f64 terms in another order; the GPU tests allow 8 E with a floor of 1e-12:
    TOL = 1e-12
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_ref as CR  # noqa: E402
import jackknife_ref as JR  # noqa: E402

E_MEASURED = 1.65e-14
TOL = max(8 * E_MEASURED, 1e-12)
TINY = 2.0 ** -40
SEED = 0x0B5EED
REF_RULES = [0, 1, 2, 4]  # GroupA, GroupB, Pooled, Cotton: the four distinct beta* rules


def _rule(ref):
    return {4: 3, 5: 2}.get(ref, ref)  # Cotton == Weighted, Neumark == Pooled


def n_strata_ranges(refb):
    if refb.stratified:
        return [(0, refb.c_a), (refb.c_a, refb.n_clusters)]
    return [(0, refb.n_clusters)]


def brute(refb, clusters=None):
    """theta_(c) by refitting without cluster c -> (theta (len, 6 + 2K), kept)."""
    p, O = refb.prep, refb.O
    k = p["cfg"].k
    c_ = JR.n_components(k)
    clusters = range(refb.n_clusters) if clusters is None else clusters
    out = np.full((len(clusters), c_), np.nan)
    kept = np.zeros(len(clusters), dtype=bool)
    for t, c in enumerate(clusters):
        m = [np.ones(len(p["ya"]), bool), np.ones(len(p["yb"]), bool)]
        for g in (0, 1):
            m[g][refb.members[g][c]] = False
        if m[0].sum() <= k or m[1].sum() <= k:  # ols.rs:98-105
            continue
        wa = None if p["wa"] is None else p["wa"][m[0]]
        wb = None if p["wb"] is None else p["wb"][m[1]]
        rc, row = O.single_pass(p["cfg"], p["xa"][m[0]], p["ya"][m[0]], wa, p["xb"][m[1]], p["yb"][m[1]], wb)
        if rc == 0:
            out[t], kept[t] = row[:c_], True
    return out, kept


def _pivots(m):
    """The Cholesky pivots d_j = L_jj^2 of m, or None where the factorisation fails."""
    try:
        return np.diag(np.linalg.cholesky(m)) ** 2
    except np.linalg.LinAlgError:
        return None


def closed_form(refb, ref, deviations=False, with_point=False):
    """-> (theta (C, 6 + 2K), kept[, theta_hat]); deviations=True returns d = theta_(c) - theta_hat instead of
    theta. theta_hat is this closed form's own point estimate (jackknife_ref.closed_form's convention)."""
    p, ref = refb.prep, _rule(ref)
    xs = [np.asarray(p["xa"], float), np.asarray(p["xb"], float)]
    ys = [np.asarray(p["ya"], float), np.asarray(p["yb"], float)]
    weighted = p["wa"] is not None
    ws = [np.asarray(p["wa"], float), np.asarray(p["wb"], float)] if weighted else [np.ones(len(y)) for y in ys]
    k = xs[0].shape[1]
    n = [len(y) for y in ys]
    G = [(x * w[:, None]).T @ x for x, w in zip(xs, ws)]
    b = [(x * w[:, None]).T @ y for x, y, w in zip(xs, ys, ws)]
    beta = [np.linalg.solve(g, v) for g, v in zip(G, b)]
    S = [(x * w[:, None]).sum(0) for x, w in zip(xs, ws)]
    W = [s[0] for s in S]
    SY = [(w * y).sum() for w, y in zip(ws, ys)]
    xbar = [s / wt for s, wt in zip(S, W)]
    ybar = [s / wt for s, wt in zip(SY, W)]
    piv = [_pivots(g) for g in G]
    pooled = ref == 2
    if pooled:
        zs = [np.hstack([xs[0], np.ones((n[0], 1))]), np.hstack([xs[1], np.zeros((n[1], 1))])]
        P = sum((z * w[:, None]).T @ z for z, w in zip(zs, ws))
        rp = sum((z * w[:, None]).T @ y for z, y, w in zip(zs, ys, ws))
        bp = np.linalg.solve(P, rp)
        piv_p = _pivots(P)
    w_a0 = W[0] / (W[0] + W[1])
    star = [beta[0], beta[1], bp[:k] if pooled else None, beta[0] * w_a0 + beta[1] * (1.0 - w_a0)][ref]
    hat = JR._components(xbar[0][None, :], xbar[1][None, :], beta[0][None, :], beta[1][None, :], star[None, :],
                         np.array([ybar[0] - ybar[1]]))[0]
    nc = refb.n_clusters
    theta = np.full((nc, JR.n_components(k)), np.nan)
    kept = np.zeros(nc, dtype=bool)
    zero = np.zeros(k)
    for c in range(nc):
        keep = True
        db, dx, dy, wc = [zero, zero], [zero, zero], [0.0, 0.0], [0.0, 0.0]
        Pc, rpc = (np.zeros((k + 1, k + 1)), np.zeros(k + 1)) if pooled else (None, None)
        for g in (0, 1):
            idx = refb.members[g][c]
            if len(idx) == 0:
                continue
            if n[g] - len(idx) <= k:
                keep = False
                break
            x, y, w = xs[g][idx], ys[g][idx], ws[g][idx]
            Q, bc, Sc = (x * w[:, None]).T @ x, (x * w[:, None]).T @ y, (x * w[:, None]).sum(0)
            wc[g] = w.sum() if weighted else float(len(idx))
            wm = W[g] - wc[g]
            if not wm > 0.0:
                keep = False
                break
            M = G[g] - Q
            d = _pivots(M)
            if d is None or (d <= TINY * piv[g]).any():
                keep = False
                break
            db[g] = -np.linalg.solve(M, bc - Q @ beta[g])
            dx[g] = (wc[g] * xbar[g] - Sc) / wm
            dy[g] = (wc[g] * ybar[g] - (w * y).sum()) / wm
            if pooled:
                z = zs[g][idx]
                Pc += (z * w[:, None]).T @ z
                rpc += (z * w[:, None]).T @ y
        dbs = None
        if keep and pooled:
            M = P - Pc
            d = _pivots(M)
            if d is None or (d <= TINY * piv_p).any():
                keep = False
            else:
                dbs = (-np.linalg.solve(M, rpc - Pc @ bp))[:k]
        if not keep:
            continue
        kept[c] = True
        pa, pb, qa, qb = beta[0], beta[1], xbar[0], xbar[1]
        dba, dbb, dxa, dxb = db[0], db[1], dx[0], dx[1]
        if ref == 0:
            dbs = dba
        elif ref == 1:
            dbs = dbb
        elif ref == 3:
            rest = (W[0] + W[1]) - wc[0] - wc[1]
            w_a = (W[0] - wc[0]) / rest
            if deviations:
                d_wa = (W[0] * wc[1] - wc[0] * W[1]) / (rest * (W[0] + W[1]))
                dbs = dba * w_a + dbb * (1.0 - w_a) + (pa - pb) * d_wa
            else:
                dbs = (pa + dba) * w_a + (pb + dbb) * (1.0 - w_a) - star
        if not deviations:
            gap = (ybar[0] + dy[0]) - (ybar[1] + dy[1])
            theta[c] = JR._components((qa + dxa)[None, :], (qb + dxb)[None, :], (pa + dba)[None, :], (pb + dbb)[None, :],
                                      (star + dbs)[None, :], np.array([gap]))[0]
            continue
        na_, nb_, ns_ = pa + dba, pb + dbb, star + dbs  # the values without the cluster
        pdx, ddx, pdb, ddb = qa - qb, dxa - dxb, pa - pb, dba - dbb
        dex = ddx * ns_ + pdx * dbs
        dun = dxa * (na_ - ns_) + qa * (dba - dbs) + dxb * (ns_ - nb_) + qb * (dbs - dbb)
        d_expl = dex.sum()
        six = np.array([d_expl, ((dxa * na_ + qa * dba).sum() - (dxb * nb_ + qb * dbb).sum()) - d_expl,
                        (ddx * nb_ + pdx * dbb).sum(), (dxb * (pdb + ddb) + qb * ddb).sum(),
                        (ddx * (pdb + ddb) + pdx * ddb).sum(), dy[0] - dy[1]])
        theta[c] = np.concatenate([six, dex, dun])
    return (theta, kept, hat) if with_point else (theta, kept)


def power_sums(d, kept, ranges):
    """-> sums (2, C, 3), n_used [2], n_dropped [2] of the deviations d over the kept clusters of each stratum."""
    out = np.zeros((2, d.shape[1], 3))
    used, dropped = [0, 0], [0, 0]
    for s, (lo, hi) in enumerate(ranges):
        v = d[lo:hi][kept[lo:hi]]
        used[s], dropped[s] = len(v), (hi - lo) - len(v)
        out[s, :, 0], out[s, :, 1], out[s, :, 2] = v.sum(0), (v ** 2).sum(0), (v ** 3).sum(0)
    return out, used, dropped


def stats(refb, ref):
    """accel, jack_se, jack_bias (C, 3), n_used and n_dropped per stratum, from the deviations form."""
    d, kept = closed_form(refb, ref, deviations=True)
    sums, used, dropped = power_sums(d, kept, n_strata_ranges(refb))
    return JR.finish(sums, used), used, dropped, sums


# ---- the test panels (shared by tests/test_gpu_cluster_jack.py, the host test and the measurement below) -------
SHAPES = [(37, 53, 2, 5), (37, 53, 2, 2), (400, 417, 16, 67), (900, 950, 31, 67)]  # n_a, n_b, p, C
CASES = [(s, w, strat) for s in SHAPES for w in (False, True) for strat in (False, True)]


def frame(n_a, n_b, p, c, seed, weighted, stratified):
    """n_a + n_b shuffled rows in c clusters. Joint: cluster 0 spans both groups, cluster 1 lies in A only and
    cluster 2 in B only (c >= 5), the others mix; at c = 2 cluster 0 holds all but two of A's rows, so the fit
    without it has rows <= K. Stratified: ids nested in the groups, A's clusters first."""
    rng = np.random.default_rng(seed)
    n = n_a + n_b
    g = rng.permutation(np.array(["A"] * n_a + ["B"] * n_b))
    is_a = g == "A"
    if stratified:
        ca = max(1, c // 2)
        cl = np.where(is_a, rng.integers(0, ca, n), ca + rng.integers(0, c - ca, n))
        cl[np.flatnonzero(is_a)[:ca]] = np.arange(ca)            # every cluster has a row
        cl[np.flatnonzero(~is_a)[:c - ca]] = ca + np.arange(c - ca)
    elif c == 2:
        cl = rng.integers(0, 2, n)
        cl[is_a] = 0
        cl[np.flatnonzero(is_a)[:2]] = 1
    else:
        cl = rng.integers(0, c, n)
        cl[:c] = np.arange(c)
        if c >= 5:
            cl[(cl == 1) & ~is_a] = 0
            cl[(cl == 2) & is_a] = 0
            cl[np.flatnonzero(is_a)[0]] = 1
            cl[np.flatnonzero(~is_a)[0]] = 2
    x = rng.normal(size=(n, p)) + is_a[:, None] * 0.3
    shock = rng.normal(0, 0.3, c)[cl]
    y = 1.0 + x @ rng.normal(0.2, 0.1, p) + is_a * 0.25 + shock + rng.normal(0, 0.5, n)
    f = {"y": y.tolist(), "g": g.tolist(), "firm": [f"f{v}" for v in cl]}
    for j in range(p):
        f[f"x{j}"] = x[:, j].tolist()
    if weighted:
        f["w"] = rng.uniform(0.5, 2.0, n).tolist()
    return f


def case_frame(shape, weighted, stratified):
    n_a, n_b, p, c = shape
    return frame(n_a, n_b, p, c, 100 + 7 * p + c, weighted, stratified)


def reference(O, f, p, ref, weighted, stratified, reps=20, extra=()):
    xs = [f"x{j}" for j in range(p)] + list(extra)
    return CR.ClusterRef(O, f, "y", "g", "B", "firm", stratified, predictors=xs, reps=reps, ref_mode=ref,
                         weights="w" if weighted else None, seed=SEED)


def dummy_frame(weighted):
    """(61 + 45, 2, 9) with a dummy column whose ones all lie in cluster 3 (rows of both groups): without that
    cluster the column is zero and no fit exists."""
    f = frame(61, 45, 2, 9, 5, weighted, False)
    f["d"] = [1.0 if v == "f3" else 0.0 for v in f["firm"]]
    on = [i for i, v in enumerate(f["firm"]) if v == "f3"]
    for i in on[::2]:  # not collinear with anything while the cluster is there
        f["d"][i] = 0.0
    return f


def zero_weight_frame():
    """(37 + 53, 2, 5) WLS in which every row of cluster 4 has weight zero."""
    f = frame(37, 53, 2, 5, 13, True, False)
    f["w"] = [0.0 if v == "f4" else w for v, w in zip(f["firm"], f["w"])]
    return f


def big_cluster_frame():
    """(300 + 310, 3, 12) in which cluster 0 holds more than half the rows of each group."""
    f = frame(300, 310, 3, 12, 21, True, False)
    rng = np.random.default_rng(2)
    f["firm"] = ["f0" if rng.random() < 0.6 else v for v in f["firm"]]
    return f


def singleton_frame():
    """3,000 rows in 1,030 clusters, the last 103 of them singletons (test_gpu_cluster.py's make_frame)."""
    from test_gpu_cluster import make_frame

    return make_frame(3000, 3, 1030, 17, True)


def many_cluster_frame():
    """20,000 + 20,001 rows, p = 5, WLS, C = 5,000."""
    return frame(20000, 20001, 5, 5000, 77, True, False)


def shock_frame():
    """The strong per-cluster shock panel of test_gpu_cluster.py's test_cluster_shock_widens_the_interval."""
    rng = np.random.default_rng(4)
    n, c = 3000, 40
    cl = rng.integers(0, c, n)
    g = np.where(rng.random(n) < 0.5, "A", "B")
    x = rng.normal(size=n)
    y = 1 + 0.5 * x + (g == "A") * 0.3 + rng.normal(0, 1.0, c)[cl] * np.where(g == "A", 1.0, -1.0) + rng.normal(0, 0.3, n)
    return {"y": y.tolist(), "g": g.tolist(), "x0": x.tolist(), "firm": cl.tolist()}


def mixed_error(got, ref, gap):
    return JR.mixed_error(got, ref, gap)


if __name__ == "__main__":  # the measurement of E
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
    import oracle as O

    O.build()
    worst = 0.0
    todo = [(f"{s} weighted={w} stratified={st}", case_frame(s, w, st), s[2], w, st, ()) for s, w, st in CASES]
    todo += [(f"dummy weighted={w}", dummy_frame(w), 2, w, False, ("d",)) for w in (False, True)]
    todo += [("zero weight", zero_weight_frame(), 2, True, False, ()), ("big cluster", big_cluster_frame(), 3, True, False, ())]
    for name, f, p, w, st, extra in todo:
        for ref in REF_RULES:
            refb = reference(O, f, p, ref, w, st, extra=extra)
            bt, bk = brute(refb)
            cf, ck = closed_form(refb, ref)
            dv, dk, hat = closed_form(refb, ref, deviations=True, with_point=True)
            assert np.array_equal(bk, ck) and np.array_equal(bk, dk), (name, ref, bk, ck)
            if not bk.any():
                print(f"{name} ref={ref}: every cluster dropped")
                continue
            gap = refb.b.point(refb.prep)[0][5]
            e = max(mixed_error(cf[bk], bt[bk], gap), mixed_error(dv[bk] + hat[None, :], bt[bk], gap))
            worst = max(worst, e)
            print(f"{name} ref={ref}: kept {int(bk.sum())}/{len(bk)}  E = {e:.3e}")
    print(f"E = {worst:.3e}")
