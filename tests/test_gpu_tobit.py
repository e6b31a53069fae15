"""Tobit decomposition on the GPU against the numpy restatement tests/tobit_ref.py: one pass and the
means pass alone, the point row and every replicate row on the same counts, bitwise determinism, the dropped replicate
and the builder end to end.

Groups of 130 and 257 rows: a ragged last 64-row sub-tile, more than one tile, and B spanning two chunks. The
restatement runs the kernels' iteration in f64, so rows are compared under the project's row tolerance (RTOL of
test_gpu_parity.py); a pass count is compared where no step norm of the restatement's fit lies within a factor 10 of
the stopping threshold (tobit_ref.margin_ok), since there rounding cannot decide it."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tobit_ref as R  # noqa: E402
from test_gpu_parity import RTOL, SEED, close  # noqa: E402

pytestmark = pytest.mark.gpu

REPS = 64 + 3  # a ragged replicate batch
LIMITS = {"both": (True, True), "lower": (True, False), "none": (False, False)}


def panel(k, weighted, limits="both"):
    """tobit_ref.panel under a limit configuration: without a limit the rows that sat at it are ordinary values."""
    xa, ya, xb, yb, wa, wb, lower, upper = R.panel(k, weighted)
    lo, hi = LIMITS[limits]
    return xa, ya, xb, yb, wa, wb, (lower if lo else None), (upper if hi else None)


def builder(ob, k, weighted, ref, limits="both", reps=REPS):
    xa, ya, xb, yb, wa, wb, lower, upper = panel(k, weighted, limits)
    f = {"y": np.concatenate([ya, yb]).tolist(), "g": ["A"] * len(ya) + ["B"] * len(yb)}
    xs = [f"x{j}" for j in range(1, k)]
    for j in range(1, k):
        f[f"x{j}"] = np.concatenate([xa[:, j], xb[:, j]]).tolist()
    if weighted:
        f["w"] = np.concatenate([wa, wb]).tolist()
    b = ob.OaxacaBuilder(f, "y", "g", "B").predictors(xs).bootstrap_reps(reps).seed(SEED).reference_coefficients(ref)
    return (b.weights("w") if weighted else b), lower, upper


_ref = {}


def ref_rows(O, k, weighted, ref, limits="both"):
    """The restatement's point row, its REPS replicate rows and the margins of their pass counts, computed once and
    shared (read-only)."""
    key = (k, weighted, ref, limits)
    if key not in _ref:
        xa, ya, xb, yb, wa, wb, lower, upper = panel(k, weighted, limits)
        point, etas, pn = R.decompose(O, xa, ya, xb, yb, wa, wb, None, None, ref, lower, upper)
        assert point is not None
        rows, ok, norms = R.boot(O, xa, ya, xb, yb, wa, wb, SEED, 0, REPS, etas, ref, lower, upper)
        assert ok.all() and max(len(v) for pair in [pn] + norms for v in pair) <= 25
        margins = np.array([[R.margin_ok(v) for v in pair] for pair in [pn] + norms])
        for a in (point, rows, margins):
            a.setflags(write=False)
        _ref[key] = (point, rows, margins)
    return _ref[key]


def piece_inputs(O, k, weighted):
    """Group B of a panel with a zero-weight row, counts with a zero-count row, and three parameter vectors: the
    least-squares start, the restatement's fit and a far one that drives u deep into both tails."""
    _, _, x, y, _, w, lower, upper = R.panel(k, weighted)
    w = np.ones(len(y)) if w is None else w.copy()
    w[7] = 0.0
    c = R.counts(O, SEED, 5, 1, len(y))
    c[11] = 0
    start = R.ols_start(x, y, w)
    fitted = R.fit(O, x, y, w, np.ones(len(y)), start, lower, upper)[0]
    far = start.copy()
    far[:k] *= -4.0
    far[k] *= 6.0
    return x, y, w, c, np.stack([start, fitted, far]), lower, upper


def rel_err(got, want):
    return float(np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-300))


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("k", [3, 9, 31])
def test_pass_and_means_match_numpy(ob, O, k, weighted):
    """Sums of at most 257 * 255 terms in f64 against numpy's: 1e-11 of the largest entry leaves four orders of
    magnitude over n eps and is far below any error in s, h or m. The gradient vanishes at a fit, so its error is
    measured against the size of its terms, sum c w |s v| + N_unc / theta, which is what bounds a sum's rounding."""
    x, y, w, c, etas, lower, upper = piece_inputs(O, k, weighted)
    for counts in (None, c):
        cf = np.ones(len(y)) if counts is None else counts.astype(float)
        info, grad, nunc = ob.tobit_pass(x, y, etas, lower, upper, w=w, counts=counts)
        for i, eta in enumerate(etas):
            want_info, want_grad, want_nunc = R.tobit_pass(O, x, y, cf * w, eta, lower, upper)
            _, sc, _ = R.score_weights(O, x, y, eta, lower, upper)
            terms = np.abs(np.column_stack([x, -y]) * (cf * w * sc)[:, None]).sum(0).max() + want_nunc / eta[k]
            e_info, e_grad = rel_err(info[i], want_info), float(np.max(np.abs(grad[i] - want_grad)) / terms)
            print(f"k={k} w={weighted} counts={counts is not None} eta#{i}: info {e_info:.2e} grad {e_grad:.2e}")
            assert np.isfinite(info[i]).all() and np.isfinite(grad[i]).all()
            assert e_info <= 1e-11 and e_grad <= 1e-11 and abs(nunc[i] - want_nunc) <= 1e-11 * want_nunc
            assert np.array_equal(info[i], info[i].T)
        got = ob.tobit_means(x, y, etas[:2], lower, upper, w=w, counts=counts)
        want = R.means(O, x, y, cf * w, etas[:2], lower, upper)
        flat_got = np.concatenate([got["means"], [got["y_mean"], got["n"], *got["censored_share"]], got["x_mean"]])
        flat_want = np.concatenate([want[:6], want[6]])
        print(f"k={k} w={weighted} counts={counts is not None}: means {np.max(np.abs(flat_got - flat_want)):.2e}")
        assert np.max(np.abs(flat_got - flat_want) / np.maximum(np.abs(flat_want), 1.0)) <= 1e-11


CASES = [(k, w, ref, "both") for k in (3, 9) for w in (False, True) for ref in (R.GROUP_A, R.GROUP_B)]
CASES += [(3, False, R.GROUP_A, "lower"), (3, True, R.GROUP_B, "none")]
# D = 17, 18 and 32, the size of the step kernel's arrays; at K = 31 a row is 240 doubles
CASES += [(16, True, R.GROUP_A, "both"), (17, False, R.GROUP_B, "both"), (31, True, R.GROUP_A, "both"), (31, False, R.GROUP_B, "lower")]


@pytest.mark.parametrize("k,weighted,ref,limits", CASES)
def test_rows_match_ref(ob, O, k, weighted, ref, limits):
    point, rows, margins = ref_rows(O, k, weighted, ref, limits)
    b, lower, upper = builder(ob, k, weighted, ref, limits)
    pr = b.prepare_tobit(lower, upper)
    try:
        assert pr.row_len == R.row_len(k)
        got_point = pr.point_row()
        got, ok = pr.boot(0, REPS)
        info = pr.tobit_info()
    finally:
        pr.close()
    assert ok.all() and np.isfinite(got_point).all() and np.isfinite(got).all()
    assert (info["lower"], info["upper"]) == (lower, upper)
    good, worst = close(got_point[:-2], point[:-2], point[5])
    print(f"k={k} weighted={weighted} ref={ref} {limits}: point worst {worst:.3e}")
    assert good, worst
    worst_all = 0.0
    for r in range(REPS):
        good, worst = close(got[r][:-2], rows[r][:-2], rows[r][5])
        worst_all = max(worst_all, worst)
        assert good, (r, worst)
    print(f"k={k} weighted={weighted} ref={ref} {limits}: replicate worst {worst_all:.3e}")
    got_passes = np.vstack([got_point[-2:], got[:, -2:]])
    want_passes = np.vstack([point[-2:], rows[:, -2:]])
    print(f"  {int((~margins).sum())} of {margins.size} fits have a step norm within a factor 10 of 1e-6")
    assert np.array_equal(got_passes[margins], want_passes[margins])
    assert (np.abs(got_passes - want_passes) <= 1).all()


def test_rows_are_deterministic(ob, N):
    """Bitwise: replicate 5 alone, in a boot of 67, at a shifted first_rep, on a repeated call and under a batch of
    one 64-replicate block forced through hk_batch."""
    b, lower, upper = builder(ob, 9, True, R.GROUP_A, reps=200)
    pr = b.prepare_tobit(lower, upper)
    try:
        r0, k0 = pr.boot(0, 200)
        r1, k1 = pr.boot(0, REPS)
        r2, k2 = pr.boot(5, 1)
        r3, k3 = pr.boot(3, 130)
        r4, k4 = pr.boot(0, 200)
        with N.option("hk_batch", 1):
            r5, k5 = pr.boot(0, 200)
    finally:
        pr.close()
    assert k0.all()
    assert r0.tobytes() == r4.tobytes() and np.array_equal(k0, k4)
    assert r0[:REPS].tobytes() == r1.tobytes() and np.array_equal(k0[:REPS], k1)
    assert r0[5:6].tobytes() == r2.tobytes() and np.array_equal(k0[5:6], k2)
    assert r0[3:133].tobytes() == r3.tobytes() and np.array_equal(k0[3:133], k3)
    assert r0.tobytes() == r5.tobytes() and np.array_equal(k0, k5)


def test_censored_only_resample_is_dropped(ob, O, N):
    """Counts that select only censored rows of a K + 2-row group: the fit is flagged failed before any step, with
    nothing non-finite, and the same counts through the row kernel give ok = 0; then counts of that kind on the whole
    group A, beside a replicate that is kept."""
    k = 3
    xa, ya, xb, yb, _, _, lower, upper = R.panel(k)
    cens = np.flatnonzero((ya == lower) | (ya == upper))[:3]
    unc = np.flatnonzero((ya != lower) & (ya != upper))[:2]
    take = np.concatenate([cens, unc])  # K + 2 rows, two of them uncensored
    x, y = xa[take], ya[take]
    counts = np.array([[2, 1, 3, 0, 0], [1, 1, 1, 1, 1]])
    eta0 = R.ols_start(xa, ya)
    eta, flags, passes = ob.tobit_fit(x, y, lower, upper, counts=counts, eta0=eta0)
    assert flags[0] == N.OB_TOBIT_DONE | N.OB_TOBIT_FAILED and passes[0] == 0
    assert np.isfinite(eta).all() and np.array_equal(eta[0], eta0)
    assert R.fit(O, x, y, counts[0].astype(float), counts[0], eta0, lower, upper)[1:3] == (0, False)
    # the same group and counts as A through the row kernel: replicate 0 holds no uncensored row, replicate 1 two (<= K)
    cb = np.ones((2, len(yb)), dtype=int)
    rows, ok = ob.tobit_rows(x, y, xb, yb, lower, upper, counts_a=counts, counts_b=cb)
    assert list(ok) == [0, 0] and np.isnan(rows).all()
    # and beside a kept replicate: replicate 0 leaves the whole A without an uncensored row, replicate 1 counts every
    # row once
    ca = np.zeros((2, len(ya)), dtype=int)
    ca[0, cens] = [40, 40, 50]
    ca[1] = 1
    cb = np.ones((2, len(yb)), dtype=int)
    rows, ok = ob.tobit_rows(xa, ya, xb, yb, lower, upper, counts_a=ca, counts_b=cb)
    assert list(ok) == [0, 1] and np.isnan(rows[0]).all() and np.isfinite(rows[1]).all()
    want = R.decompose(O, xa, ya, xb, yb, None, None, None, None, R.GROUP_A, lower, upper)[0]
    assert close(rows[1][:-2], want[:-2], want[5])[0]


def test_refusals_on_a_tobit_handle(ob, N):
    """What a Tobit handle does not serve, each with its code and message: the generic refusals of a model handle
    read this front end's label and plural from ob_model.hpp's table. (A failed point fit, OB_E_LINALG, is reached on
    the host in test_tobit_host.py.)"""
    b, lower, upper = builder(ob, 3, False, R.GROUP_A)
    pr = b.prepare_tobit(lower, upper)
    try:
        with pytest.raises(N.OaxacaError) as e:
            pr.boot_sharded(0, 4)
        assert e.value.code == N.OB_E_UNSUPPORTED and str(e.value) == "tobit decomposition: sharded runs are outside its scope"
        with pytest.raises(N.OaxacaError) as e:
            pr.jackknife()
        assert e.value.code == N.OB_E_UNSUPPORTED
        assert str(e.value) == "jackknife: tobit decompositions (BCa included) are outside its scope"
        rows, ok = pr.boot(0, 4)
        with pytest.raises(N.OaxacaError) as e:
            pr.finish_bca(rows, ok)
        assert e.value.code == N.OB_E_UNSUPPORTED
        assert str(e.value) == "jackknife: tobit decompositions (BCa included) are outside its scope"
        assert pr.cluster_info is None
    finally:
        pr.close()
    with pytest.raises(N.OaxacaError) as e:
        b.cluster("x1").prepare_tobit(lower, upper)
    assert e.value.code == N.OB_E_UNSUPPORTED and str(e.value) == "tobit decomposition: the cluster bootstrap is outside its scope"


def test_decompose_tobit_end_to_end(ob, O, N):
    k = 9
    b, lower, upper = builder(ob, k, True, R.GROUP_B)
    res = b.decompose_tobit(lower, upper)
    with b.prepare_tobit(lower, upper) as pr:
        point = pr.point_row()
        rows, ok = pr.boot(0, REPS)
    assert res.n_failed == 0 and ok.all() and res.n_a == 130 and res.n_b == 257
    want = ob.tobit_finish_rows(point, k, rows, ok)
    tables = ("two_fold", "three_fold", "latent", "detailed_explained", "detailed_unexplained")
    cols = ([0, 1], [2, 3, 4], range(6 + 7 * k, 6 + 7 * k + 3), range(6, 6 + k), range(6 + k, 6 + 2 * k))
    for name, cc in zip(tables, cols):
        for c, w, col in zip(getattr(res, name), getattr(want, name), cc):
            assert c.estimate == point[col]
            assert (c.std_err, c.p_value, c.ci_lower, c.ci_upper) == (w.std_err, w.p_value, w.ci_lower, w.ci_upper)
            assert c.std_err > 0.0 or name.startswith("detailed")
    assert len(res.names) == k and res.names[1:] == [f"x{j}" for j in range(1, k)]
    assert res.total_gap == point[5] and res.raw_gap == point[6 + 7 * k + 7] - point[6 + 7 * k + 8]
    ref_point = ref_rows(O, k, True, R.GROUP_B)[0]
    assert close(point[:-2], ref_point[:-2], ref_point[5])[0]
    assert abs(res.sigma_a - ref_point[6 + 7 * k + 9]) <= RTOL * res.sigma_a
    assert 0.1 < res.censored_share[("A", "left")] < 0.45 and 0.02 < res.censored_share[("B", "right")] < 0.25
    back = json.loads(res.to_json())
    assert back["total_gap"] == res.total_gap and back["n_failed"] == 0 and back["upper"] == upper
    assert [c["estimate"] for c in back["latent"]] == [c.estimate for c in res.latent]
    assert back["expected_values"]["A|beta_a"] == res.expected_values[("A", "beta_a")]
    t = ob.tobit_last_timing()
    assert 1 <= t["passes"] <= N.OB_TOBIT_MAX_PASSES and t["pass_launches"] >= 1


@pytest.mark.parametrize("n", [65, 257])
@pytest.mark.parametrize("k", [1, 5, 6, 11, 30, 31])
def test_pass_edges_match_numpy(ob, O, k, n):
    """The pass's edges at dimension D = k + 1 under the bound of test_pass_and_means_match_numpy: three pairs in one
    tile (k = 1), 21 and 28 pairs either side of a tile boundary, a wave's second pair tile (k = 11), 496 and 528
    pairs without a padding lane and all 9 tiles of a wave (k = 31); a one-row last sub-tile (n = 65) and a one-row
    second tile (n = 257); 17 parameter vectors: a partly filled block of 16."""
    rng = np.random.default_rng(1000 * n + k)
    x = np.column_stack([np.ones(n), rng.normal(size=(n, k - 1))])
    ystar = 0.5 + x[:, 1:] @ (0.5 / np.sqrt(max(k - 1, 1)) * np.ones(k - 1)) + rng.normal(size=n)
    lower, upper = 0.0, float(np.round(np.quantile(ystar, 0.9), 2))
    y = np.clip(ystar, lower, upper)
    w = rng.uniform(0.5, 2.0, n)
    c = rng.integers(0, 4, n).astype(np.uint8)
    start = R.ols_start(x, y, w)
    etas = start[None, :] * rng.uniform(0.8, 1.25, size=(17, k + 1))
    info, grad, nunc = ob.tobit_pass(x, y, etas, lower, upper, w=w, counts=c)
    for i, eta in enumerate(etas):
        want_info, want_grad, want_nunc = R.tobit_pass(O, x, y, c * w, eta, lower, upper)
        _, sc, _ = R.score_weights(O, x, y, eta, lower, upper)
        terms = np.abs(np.column_stack([x, -y]) * (c * w * sc)[:, None]).sum(0).max() + want_nunc / eta[k]
        e_info, e_grad = rel_err(info[i], want_info), float(np.max(np.abs(grad[i] - want_grad)) / terms)
        print(f"k={k} n={n} eta#{i}: info {e_info:.2e} grad {e_grad:.2e}")
        assert e_info <= 1e-11 and e_grad <= 1e-11 and abs(nunc[i] - want_nunc) <= 1e-11 * want_nunc
        assert np.array_equal(info[i], info[i].T)
