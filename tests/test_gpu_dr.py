"""The distribution-regression decomposition on the GPU (csrc/ob_dr.hip) against the numpy
restatement tests/dr_ref.py: the threshold logit pass and the distribution pass alone, the point row and the
replicate rows on the same counts, bitwise determinism, the failure path, the builder end to end and the bytes of
the older paths after a run.

Pieces: the stacked 387 rows of reweight_ref.panel(k) (a ragged last 64-row sub-tile, two chunks), K = 3, 9, 16, 17
and 32, T = 2, 16, 17 and 64 (both sides of a 16-fit block, and the limit), weighted and unweighted, with counts and
without. The tolerance is 8 E, E the largest error of the f64 restatement against its longdouble run on the same
inputs, relative to sqrt(G_aa G_bb), to sqrt(G_jj sum cw) and to sum cw; the figures are in DESIGN.md §5.16.

Rows: reweight_ref.panel(k, weighted, n_a=650, n_b=1285), K = 3, 9 and 17, thresholds at 5 and at 17 evenly spaced
pooled quantiles of [0.1, 0.9], 67 replicates at first_rep 0 and the 39 that exist from 2^32 - 40. A CPU scan with
the oracle's OBRS-3 counts over the six (K, T, weighted) cases below -- the point pass, 67 and 39 replicates each,
14,124 fits -- found every fit converged and every replicate ok, the longest fit 10 passes; 5,698 of the fits have
a step norm within a factor 10 of 1e-6 (Newton's norms square from pass to pass, as test_gpu_reweight.py explains),
which the tests print again per case. At the point estimate four (tau, distribution) pairs of every case lie
outside the grid's range (tau = 0.1 and 0.9 against thresholds at the pooled 0.1 and 0.9 quantiles), so the edge
cases are compared as well. The tests assert that scan's result on the restatement (every replicate ok, at most 25
passes) before they compare."""
import json
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dr_ref as D  # noqa: E402
import reweight_ref as R  # noqa: E402
from test_gpu_parity import RTOL, SEED, close  # noqa: E402  (the Heckman and binary tests' row tolerance)
from test_gpu_reweight import frame_of  # noqa: E402

pytestmark = pytest.mark.gpu

REPS = 64 + 3  # a ragged replicate batch
HIGH = 2 ** 32 - 40
TAUS = np.array([0.1, 0.25, 0.5, 0.75, 0.9])
N_A, N_B = 650, 1285
ROW_CASES = [(3, 5, False), (3, 17, True), (9, 5, True), (9, 17, False), (17, 5, False), (17, 17, True)]


def row_panel(k, weighted):
    return R.panel(k, weighted, n_a=N_A, n_b=N_B)


def builder(ob, k, weighted, reps=REPS, panel=None):
    f, xs = frame_of(*(row_panel(k, weighted) if panel is None else panel))
    b = ob.OaxacaBuilder(f, "y", "g", "B").predictors(xs).bootstrap_reps(reps).seed(SEED)
    return b.weights("w") if weighted else b


_ref = {}


def ref_rows(O, k, T, weighted):
    """The restatement's thresholds, point row, REPS rows from replicate 0 and 39 from HIGH, computed once and
    shared (read-only)."""
    key = (k, T, weighted)
    if key not in _ref:
        xa, ya, xb, yb, wa, wb = row_panel(k, weighted)
        thr = D.thresholds(np.concatenate([ya, yb]), T, 0.1, 0.9)
        point, info = D.decompose(xa, ya, xb, yb, thr, TAUS, wa, wb)
        assert point is not None and len(thr) == T
        lo = D.boot(O, xa, ya, xb, yb, wa, wb, thr, TAUS, SEED, 0, REPS)
        hi = D.boot(O, xa, ya, xb, yb, wa, wb, thr, TAUS, SEED, HIGH, 39)
        norms = info["norms"] + [f for rep in lo[2] + hi[2] for f in rep]
        assert lo[1].all() and hi[1].all() and max(len(v) for v in norms) <= 25
        print(f"k={k} T={T} weighted={weighted}: {sum(not R.margin_ok(v) for v in norms)} of {len(norms)} fits have "
              f"a step norm within a factor 10 of 1e-6")
        for a in (thr, point, lo[0], hi[0], info["beta"], info["passes"], info["edge"]):
            a.setflags(write=False)
        _ref[key] = (thr, point, lo[0], hi[0], info)
    return _ref[key]


def piece_inputs(O, k, weighted):
    """Stacked rows of the small panel, a zero-weight row, counts with a zero-count row."""
    xa, ya, xb, yb, wa, wb = R.panel(k, weighted)
    x, y = np.vstack([xa, xb]), np.concatenate([ya, yb])
    w = np.concatenate([wa, wb]) if weighted else np.ones(len(y))
    w[7] = 0.0
    c = np.concatenate([R.counts(O, SEED, 5, 0, len(ya)), R.counts(O, SEED, 5, 1, len(yb))])
    c[11] = 0
    return x, y, w, c


def piece_thresholds(y, T, cw):
    """T thresholds: one below every y, one above every y, one exactly equal to the y of a row that counts (the <=
    must hold), the others spread over the outcome's range -> (thresholds, the index of the equal one or None)."""
    thr = np.linspace(np.quantile(y, 0.05), np.quantile(y, 0.95), T)
    thr[0] = y.min() - 1.0
    thr[-1] = y.max() + 1.0
    if T == 2:
        return thr, None
    counted = np.flatnonzero(cw > 0)
    inner = y[counted[np.argsort(y[counted])[len(counted) // 2]]]
    thr[T // 2] = inner
    thr = np.sort(thr)
    assert len(np.unique(thr)) == T
    return thr, int(np.flatnonzero(thr == inner)[0])


def piece_betas(x, k, T, which):
    """(T, k) coefficient sets: 0, a fitted-size one, one that drives p into the clamp."""
    rng = np.random.default_rng(1000 * k + T)
    if which == 0:
        return np.zeros((T, k))
    b = rng.normal(size=(T, k)) * 0.4 / np.sqrt(k)
    if which == 2:
        b = b * (40.0 / np.abs(x @ b.T).max(0))[:, None]  # |x'beta| up to 40: p beyond the clamp
        p = R.sigmoid_clamped(x @ b.T)
        assert (p == R.HI).any() or (p == R.LO).any()
    return b


def rel_err(got, want):
    """The largest error relative to sqrt(G_aa G_bb) of a symmetric matrix."""
    dg = np.sqrt(np.abs(np.diag(want)))
    return float(np.max(np.abs(got - want) / np.outer(dg, dg)))


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("k,T", [(3, 2), (3, 17), (9, 16), (16, 17), (17, 64), (32, 2), (32, 16), (9, 64)])
def test_pieces_match_numpy(ob, O, k, T, weighted):
    x, y, w, c = piece_inputs(O, k, weighted)
    thr, t_eq = piece_thresholds(y, T, c * w)
    L = np.longdouble
    for counts in (None, c):
        cw = (np.ones(len(y)) if counts is None else counts.astype(float)) * w
        for which in range(3):
            betas = piece_betas(x, k, T, which)
            info, grad = ob.dr_logit_pass(x, y, thr, betas, w=w, counts=counts)
            i64, g64 = D.logit_pass(x, y, cw, thr, betas)
            iL, gL = D.logit_pass(x, y, cw, thr, betas, dtype=L)
            e_info = dev_info = e_grad = dev_grad = 0.0
            for t in range(T):
                e_info = max(e_info, rel_err(i64[t].astype(L), iL[t]))
                dev_info = max(dev_info, rel_err(info[t].astype(L), iL[t]))
                gscale = np.sqrt(np.abs(np.diag(iL[t])) * np.sum(cw))  # |sum cw (d - p) x_j| <= sqrt(sum cw x_j^2 sum cw)
                gscale = np.maximum(gscale, np.abs(gL[t]))
                e_grad = max(e_grad, float(np.max(np.abs(g64[t] - gL[t]) / gscale)))
                dev_grad = max(dev_grad, float(np.max(np.abs(grad[t] - gL[t]) / gscale)))
                assert np.array_equal(info[t], info[t].T)
            both = np.vstack([betas, betas[::-1] * 0.5])  # 2 T vectors, as a run's pass takes
            sums, wsum = ob.dr_cdf(x, both, w=w, counts=counts)
            s64, ws64 = D.cdf_sums(x, cw, both)
            sL, wsL = D.cdf_sums(x, cw, both, dtype=L)
            e_f = float(max(np.max(np.abs(s64 - sL)), abs(ws64 - wsL)) / wsL)
            dev_f = float(max(np.max(np.abs(sums - sL)), abs(wsum - wsL)) / wsL)
            print(f"k={k} T={T} w={weighted} counts={counts is not None} beta#{which}: E info {e_info:.2e} dev "
                  f"{dev_info:.2e} | E grad {e_grad:.2e} dev {dev_grad:.2e} | E F {e_f:.2e} dev {dev_f:.2e}")
            E = max(e_info, e_grad, e_f)
            assert E > 0.0
            assert dev_info <= 8 * E and dev_grad <= 8 * E and dev_f <= 8 * E
    # the extreme thresholds: d = 0 for every row, d = 1 for every row; and the row that equals a threshold
    info, grad = ob.dr_logit_pass(x, y, thr, np.zeros((T, k)), w=w, counts=c)
    cw = c * w
    assert abs(grad[0][0] + 0.5 * cw.sum()) <= 1e-12 * cw.sum() and abs(grad[-1][0] - 0.5 * cw.sum()) <= 1e-12 * cw.sum()
    if t_eq is not None:
        want = np.sum(cw * ((y <= thr[t_eq]) - 0.5))
        strict = np.sum(cw * ((y < thr[t_eq]) - 0.5))
        assert want != strict and abs(grad[t_eq][0] - want) <= 1e-12 * cw.sum()


@pytest.mark.parametrize("k,T,weighted", ROW_CASES)
def test_rows_match_ref(ob, O, N, k, T, weighted):
    thr, point, lo, hi, info = ref_rows(O, k, T, weighted)
    nq = len(TAUS)
    pr = builder(ob, k, weighted).prepare_distribution(TAUS, n_thresholds=T, lo=0.1, hi=0.9)
    try:
        assert pr.row_len == D.row_len(T, nq) == ob.dr_row_len(T, nq)
        got_point = pr.point_row()
        got_info = pr.dr_info()
        got_lo, ok_lo = pr.boot(0, REPS)
        got_hi, ok_hi = pr.boot(HIGH, 39)
    finally:
        pr.close()
    assert np.array_equal(got_info["thresholds"], thr) and got_info["n_thresholds_requested"] == T
    assert ok_lo.all() and ok_hi.all() and np.isfinite(got_point).all()
    scale = point[nq // 2]  # the total gap at the median
    assert TAUS[nq // 2] == 0.5 and scale != 0.0
    good, worst = close(got_point, point, scale)
    print(f"k={k} T={T} weighted={weighted}: point worst {worst:.3e}")
    assert good, worst
    assert got_point[-1] == point[-1]
    assert np.array_equal(got_info["passes"], info["passes"])
    assert np.array_equal(got_info["out_of_range"], info["edge"])
    assert got_info["n_out_of_range"] == int((info["edge"] != 0).sum())
    assert np.all(np.abs(got_info["beta"] - info["beta"]) <= RTOL * np.maximum(np.abs(info["beta"]), 1.0))
    for got, want in ((got_lo, lo), (got_hi, hi)):
        worst_all = 0.0
        for r in range(len(want)):
            good, worst = close(got[r], want[r], scale)
            worst_all = max(worst_all, worst)
            assert good, (r, worst)
        assert np.array_equal(got[:, -1], want[:, -1])  # the pass counts
        print(f"k={k} T={T} weighted={weighted}: replicate worst {worst_all:.3e}")


@pytest.mark.parametrize("k,T", [(3, 17), (17, 5)])
def test_rows_are_deterministic(ob, N, k, T):
    """Bitwise: replicate 5 alone, in the batch of 67, in a longer run, at a shifted first_rep, at two batch sizes
    forced through hk_batch; a repeated call."""
    pr = builder(ob, k, True, reps=200).prepare_distribution(TAUS, n_thresholds=T, lo=0.1, hi=0.9)
    try:
        r0, k0 = pr.boot(0, 200)
        r1, k1 = pr.boot(0, REPS)
        r2, k2 = pr.boot(5, 1)
        r3, k3 = pr.boot(3, 130)
        r4, k4 = pr.boot(0, 200)
        with N.option("hk_batch", 1):
            r5, k5 = pr.boot(0, 200)
        with N.option("hk_batch", 2):
            r6, k6 = pr.boot(0, 200)
    finally:
        pr.close()
    assert k0.all()
    assert r0.tobytes() == r4.tobytes() and np.array_equal(k0, k4)
    assert r0[:REPS].tobytes() == r1.tobytes() and np.array_equal(k0[:REPS], k1)
    assert r0[5:6].tobytes() == r2.tobytes() and np.array_equal(k0[5:6], k2)
    assert r0[3:133].tobytes() == r3.tobytes() and np.array_equal(k0[3:133], k3)
    assert r0.tobytes() == r5.tobytes() == r6.tobytes() and np.array_equal(k0, k5) and np.array_equal(k0, k6)


def rare_panel():
    """The K = 3 row panel with three rows of group A, the ones nearest A's covariate mean, moved far below every
    other outcome: the threshold between them and the rest has three rows of A under it (and none of B's, whose
    three lowest outcomes are moved likewise so that B's fit at that threshold exists). A central point cannot be
    separated from the cloud around it, so a replicate that draws at least one of the three converges; one that
    draws none has d = 0 on every row of A, its intercept runs off at one unit a pass and the fit is still
    iterating at pass 100."""
    xa, ya, xb, yb, wa, wb = row_panel(3, False)
    ya, yb = ya.copy(), yb.copy()
    ia = np.argsort(np.sum((xa[:, 1:] - xa[:, 1:].mean(0)) ** 2, axis=1))[:3]
    ib = np.argsort(np.sum((xb[:, 1:] - xb[:, 1:].mean(0)) ** 2, axis=1))[:40]
    low = min(ya.min(), yb.min())
    ya[ia] = low - 10.0
    yb[ib] = low - 10.0
    thr = np.concatenate([[low - 5.0], D.thresholds(np.concatenate([ya, yb]), 5, 0.1, 0.9)])
    return (xa, ya, xb, yb, wa, wb), ia, thr


def test_failed_replicates(ob, O, N):
    """A user threshold below every outcome of group A is OB_E_LINALG at prepare. With three rows of A under a
    threshold, the replicates that draw none of them come back ok = 0 with NaN rows, exactly the ones the
    restatement fails, and their neighbours' rows are bitwise those of runs that hold no failed replicate."""
    xa, ya, xb, yb, wa, wb = row_panel(3, False)
    below_a = np.concatenate([[ya.min() - 1.0], D.thresholds(np.concatenate([ya, yb]), 5, 0.1, 0.9)])
    yb2 = yb.copy()
    yb2[:5] = ya.min() - 2.0  # B has rows under it, A has none
    with pytest.raises(N.OaxacaError) as e:
        builder(ob, 3, False, panel=(xa, ya, xb, yb2, wa, wb)).prepare_distribution(TAUS, thresholds=below_a)
    assert e.value.code == N.OB_E_LINALG
    panel, ia, thr = rare_panel()
    xa, ya, xb, yb, wa, wb = panel
    assert (ya <= thr[0]).sum() == 3
    # the seed, from the oracle's counts: the first at or after SEED with a replicate among the 67 that draws none
    seed = SEED
    while True:
        none = [r for r in range(REPS) if R.counts(O, seed, r, 0, len(ya))[ia].sum() == 0]
        if none and len(none) < REPS:
            break
        seed += 1
    rows, ok, _ = D.boot(O, xa, ya, xb, yb, wa, wb, thr, TAUS, seed, 0, REPS)
    failed = np.flatnonzero(ok == 0)
    print(f"seed {seed}: replicates that draw none of the three rows {none}, the restatement fails {failed.tolist()}")
    assert set(none) <= set(failed.tolist()) and 1 <= len(failed) < REPS
    b = builder(ob, 3, False, panel=panel).seed(seed)
    pr = b.prepare_distribution(TAUS, thresholds=thr)
    try:
        got, gok = pr.boot(0, REPS)
        alone = {int(r): pr.boot(int(r), 1) for r in np.flatnonzero(ok)[:6]}
    finally:
        pr.close()
    assert np.array_equal(gok, ok)
    assert np.isnan(got[failed]).all() and np.isfinite(got[ok.astype(bool)]).all()
    scale = rows[ok.astype(bool)][0][len(TAUS) // 2]
    for r in np.flatnonzero(ok):
        good, worst = close(got[r], rows[r], scale)
        assert good, (r, worst)
    for r, (row1, ok1) in alone.items():
        assert ok1[0] == 1 and row1[0].tobytes() == got[r].tobytes()


def test_decompose_distribution_end_to_end(ob, O, N):
    k, T, weighted, reps = 3, 17, True, 200
    thr, point, lo, hi, info = ref_rows(O, k, T, weighted)
    xa, ya, xb, yb, wa, wb = row_panel(k, weighted)
    rows, ok, _ = D.boot(O, xa, ya, xb, yb, wa, wb, thr, TAUS, SEED, 0, reps)
    assert ok.all()
    b = builder(ob, k, weighted, reps=reps)
    n_edge = int((info["edge"] != 0).sum())
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = b.decompose_distribution(TAUS, n_thresholds=T, lo=0.1, hi=0.9)
    assert sum("outside the range" in str(w.message) for w in caught) == (1 if n_edge else 0)
    pr = b.prepare_distribution(TAUS, n_thresholds=T, lo=0.1, hi=0.9)
    try:
        got_point = pr.point_row()
    finally:
        pr.close()
    nq = len(TAUS)
    assert res.n_a == N_A and res.n_b == N_B and res.n_failed == 0 and res.n_out_of_range == n_edge
    assert np.array_equal(res.out_of_range, info["edge"])
    assert np.array_equal(res.thresholds, thr) and np.array_equal(res.quantiles, TAUS)
    assert res.beta_a.shape == res.beta_b.shape == (T, k) and res.names == ["__ob_intercept__", "x1", "x2"]
    comps = []
    for table, parts in ((res.quantile_effects, D.EFFECTS), (res.quantile_values, ("A", "B", "C")),
                         (res.distribution_effects, D.EFFECTS), (res.cdf, ("AA", "BB", "AB", "BA"))):
        for part in parts:
            comps += table[part]
    assert len(comps) == len(got_point) - 1
    assert [c.estimate for c in comps] == got_point[:-1].tolist()  # the estimates are the point row's
    for table in (res.quantile_effects, res.distribution_effects):
        for tot, comp, st in zip(table["total"], table["composition"], table["structure"]):
            assert abs(tot.estimate - comp.estimate - st.estimate) <= 1e-12
    for key in ("AA", "BB", "AB"):
        assert np.all(np.diff(res.cdf_rearranged[key]) >= 0.0)
        assert np.array_equal(res.cdf_rearranged[key], np.sort([c.estimate for c in res.cdf[key]]))
    want = D.aggregate(O, point, rows, ok)
    scale = point[nq // 2]
    for c, w in zip(comps, want):
        for got, exp in ((c.estimate, w[0]), (c.std_err, w[1]), (c.ci_lower, w[2]), (c.ci_upper, w[3])):
            assert abs(got - exp) <= RTOL * max(abs(exp), abs(scale)), (c.name, got, exp)
    js = json.loads(res.to_json())
    back = json.loads(json.dumps(js))
    assert back == js and js["n_failed"] == 0 and js["thresholds"] == [float(v) for v in thr]
    assert js["quantile_effects"]["structure"][2]["estimate"] == res.quantile_effects["structure"][2].estimate
    assert js["beta_b"] == [[float(v) for v in r] for r in res.beta_b]
    t = ob.dr_last_timing()
    assert t["passes"] >= 2 and t["launches"] >= t["passes"]
    assert t["pass_ms"] > 0.0 and t["cdf_ms"] > 0.0 and t["row_ms"] > 0.0
    # a tau outside the grid's range is counted and warned about
    with pytest.warns(RuntimeWarning, match="outside the range"):
        edge = builder(ob, k, weighted, reps=4).decompose_distribution([0.02, 0.5, 0.98], n_thresholds=5, lo=0.1, hi=0.9)
    assert edge.n_out_of_range == 6 and edge.out_of_range[:, 1].sum() == 0
    assert all(c.estimate == 0.0 for c in edge.quantile_effects["total"][:1])  # both quantiles are the grid's first point


def test_refusals_on_a_dr_handle(ob, N):
    pr = builder(ob, 3, False).prepare_distribution(TAUS, n_thresholds=5, lo=0.1, hi=0.9)
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


def test_older_paths_keep_their_bytes(ob, N):
    """The reweighted and the binary point rows before and after a distribution-regression run in this process."""
    xa, ya, xb, yb, wa, wb = R.panel(9, True)
    f, xs = frame_of(xa, ya, xb, yb, wa, wb)
    rw = ob.OaxacaBuilder(f, "y", "g", "B").predictors(xs).weights("w").bootstrap_reps(4).seed(SEED)
    fb = dict(f)
    cut = float(np.median(np.concatenate([ya, yb])))
    fb["y"] = [1.0 if v > cut else 0.0 for v in f["y"]]
    del fb["w"]
    bn = ob.OaxacaBuilder(fb, "y", "g", "B").predictors(xs).bootstrap_reps(4).seed(SEED)

    def rows():
        out = []
        for pr in (rw.prepare_reweighted(), bn.prepare_binary()):
            try:
                out.append(pr.point_row().tobytes())
            finally:
                pr.close()
        return out

    before = rows()
    res = builder(ob, 9, True, reps=8).decompose_distribution(TAUS, n_thresholds=5, lo=0.1, hi=0.9)
    assert res.n_failed == 0
    after = rows()
    assert before[0] == after[0]
    assert before[1] == after[1]


@pytest.mark.parametrize("n", [65, 257])
@pytest.mark.parametrize("k", [1, 5, 6, 11, 31, 32])
def test_pass_edges_match_numpy(ob, k, n):
    """The pass kernel's edges under the tolerance of test_pieces_match_numpy: one pair tile with
    three idle waves (k = 1), 15 and 21 pairs either side of the first tile boundary, a wave's second pair tile
    (k = 11), 496 and 528 pairs without a padding lane and all 9 tiles of a wave (k = 32); a one-row last sub-tile
    (n = 65) and a one-row second tile (n = 257); 17 thresholds: a partly filled block of 16."""
    rng = np.random.default_rng(1000 * n + k)
    T = 17
    x = np.column_stack([np.ones(n), rng.normal(size=(n, k - 1))])
    y = rng.normal(size=n)
    w = rng.uniform(0.5, 2.0, n)
    c = rng.integers(0, 4, n).astype(np.uint8)
    cw = c * w
    thr = np.linspace(np.quantile(y, 0.1), np.quantile(y, 0.9), T)
    betas = rng.normal(size=(T, k)) * 0.4 / np.sqrt(k)
    L = np.longdouble
    info, grad = ob.dr_logit_pass(x, y, thr, betas, w=w, counts=c)
    i64, g64 = D.logit_pass(x, y, cw, thr, betas)
    iL, gL = D.logit_pass(x, y, cw, thr, betas, dtype=L)
    E = dev = 0.0
    for t in range(T):
        gscale = np.maximum(np.sqrt(np.abs(np.diag(iL[t])) * np.sum(cw)), np.abs(gL[t]))
        E = max(E, rel_err(i64[t].astype(L), iL[t]), float(np.max(np.abs(g64[t] - gL[t]) / gscale)))
        dev = max(dev, rel_err(info[t].astype(L), iL[t]), float(np.max(np.abs(grad[t] - gL[t]) / gscale)))
        assert np.array_equal(info[t], info[t].T)
    print(f"k={k} n={n}: E {E:.2e} dev {dev:.2e}")
    assert E > 0.0 and dev <= 8 * E
