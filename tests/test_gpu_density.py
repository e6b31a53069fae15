"""The bootstrapped DFL density decomposition on the GPU (csrc/ob_density.hip) against the numpy
restatement tests/density_ref.py: the density pass alone, the point row and the replicate rows on the same counts,
bitwise determinism, a boot across a segment boundary, run_dfl's two densities, the builder end to end and the
refusals on a handle.

Groups of 130 and 257 rows (a ragged last 64-row sub-tile, two chunks in B). The tolerance is the project's RTOL
through test_gpu_parity.close, on the scale of the case's largest point density (of the largest direct sum for the
pass alone), so a deep-tail density is compared on that absolute scale.

Rounding can decide a logit's pass count only where a step norm lies within a factor 10 of 1e-6
(reweight_ref.margin_ok). At these row counts that is not so for every replicate (the CPU scan behind
reweight_ref.panel left 7 to 49 of 67 outside, by panel), so the pass count is compared on the replicates whose logits
pass margin_ok -- the test asserts that it holds for each replicate it keeps, and that some are kept -- while ok and
every other entry are compared on all replicates: an extra Newton pass at a step norm of 1e-6 moves gamma by about
1e-12."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_ref as D  # noqa: E402
import reweight_ref as R  # noqa: E402
from test_gpu_parity import RTOL, SEED, close  # noqa: E402
from test_gpu_reweight import frame_of  # noqa: E402

pytestmark = pytest.mark.gpu

REPS = 64 + 3  # a ragged replicate batch, and three replicate groups of 32 in the pass
FIT_SEG = 4096  # kFitSegReps (csrc/ob_model.hpp)


def builder(ob, k, weighted, reps=REPS):
    f, xs = frame_of(*R.panel(k, weighted))
    b = ob.OaxacaBuilder(f, "y", "g", "B").predictors(xs).bootstrap_reps(reps).seed(SEED)
    return b.weights("w") if weighted else b


_ref = {}


def ref_rows(O, k, weighted, G):
    """The restatement's grid, bandwidths, point row and REPS rows from replicate 0 with their logits' margin flags,
    computed once and shared (read-only)."""
    key = (k, weighted, G)
    if key not in _ref:
        xa, ya, xb, yb, wa, wb = R.panel(k, weighted)
        grid = D.default_grid(np.concatenate([ya, yb]), G)
        h_a, h_b = D.silverman(ya), D.silverman(yb)
        point, pn = D.decompose(xa, ya, xb, yb, grid, h_a, h_b, wa, wb)
        assert point is not None
        rows, ok, norms = D.boot(O, xa, ya, xb, yb, grid, h_a, h_b, wa, wb, SEED, 0, REPS)
        margin = np.array([R.margin_ok(v) for v in [pn] + norms])
        assert ok.all() and margin[1:].any()
        for a in (grid, point, rows, ok, margin):
            a.setflags(write=False)
        _ref[key] = (grid, h_a, h_b, point, rows, ok, margin)
    return _ref[key]


@pytest.mark.parametrize("G", [2, 17, 100, 256])  # one column, a tile and a column, 12 padding columns, the limit
@pytest.mark.parametrize("k", [3, 9, 32])
def test_pass_matches_numpy(ob, O, k, G):
    xa, ya, xb, yb, wa, wb = R.panel(k, True)
    x, y, n = xb, yb, len(yb)
    grid = np.linspace(y.min() - 0.3, y.max() + 0.2, G)
    h = D.silverman(y)
    c = R.counts(O, SEED, 5, 1, n)
    c[11] = 0
    wt = wb.copy()
    wt[7] = 0.0
    rng = np.random.default_rng(100 * k + G)
    g1 = rng.normal(size=(64, k)) * 0.4 / np.sqrt(k)
    g1[0] = 0.0
    g1[1] *= 40.0 / np.abs(x @ g1[1]).max()  # |x'gamma| up to 40: p beyond the clamp
    p = R.sigmoid_clamped(x @ g1[1])
    assert (p == R.HI).any() or (p == R.LO).any()
    worst = 0.0
    for counts in (None, c):
        cf = np.ones(n) if counts is None else counts.astype(float)
        for w in (None, wt):
            wv = np.ones(n) if w is None else w
            for gammas in (None, g1[1:2], g1):
                num, den, den2 = ob.density_pass(x, y, grid, h, gammas=gammas, w=w, counts=counts)
                gs = [None] if gammas is None else list(gammas)
                assert num.shape == (len(gs), G) and den.shape == den2.shape == (len(gs),)
                for i, g in enumerate(gs):
                    psi = np.ones(n)
                    if g is not None:
                        pp = R.sigmoid_clamped(x @ g)
                        psi = pp / (1 - pp)
                    v = wv * psi
                    want = D.kernel_sums(y, cf * v, grid, h)
                    good, err = close(num[i], want, want.max())
                    worst = max(worst, err)
                    assert good, (counts is not None, w is not None, i, err)
                    assert abs(den[i] - np.sum(cf * v)) <= RTOL * np.sum(cf * v)
                    assert abs(den2[i] - np.sum(cf * v * v)) <= RTOL * np.sum(cf * v * v)
                if counts is None and w is None and gammas is None:
                    kde = ob.kde(y, grid, h)
                    good, err = close(num[0] / (h * den[0]), kde, kde.max())
                    assert good, err
    print(f"k={k} G={G}: worst {worst:.3e}")


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("G", [17, 100])
@pytest.mark.parametrize("k", [3, 9])
def test_rows_match_ref(ob, O, N, k, G, weighted):
    grid, h_a, h_b, point, rows, ok, margin = ref_rows(O, k, weighted, G)
    pr = builder(ob, k, weighted).prepare_density(grid_size=G)
    try:
        assert pr.row_len == D.row_len(k, G) == ob.density_row_len(k, G)
        info = pr.density_info()
        got_point = pr.point_row()
        got, got_ok = pr.boot(0, REPS)
    finally:
        pr.close()
    assert np.array_equal(info["grid"], grid) and (info["k"], info["n_a"], info["n_b"]) == (k, 130, 257)
    assert abs(info["bandwidth_a"] - h_a) <= 1e-14 * h_a and abs(info["bandwidth_b"] - h_b) <= 1e-14 * h_b
    assert np.array_equal(got_ok, ok) and np.isfinite(got_point).all()
    scale = point[:3 * G].max()
    good, worst = close(got_point[:-1], point[:-1], scale)
    print(f"k={k} G={G} weighted={weighted}: point worst {worst:.3e}, scale {scale:.3f}, "
          f"{int(margin[1:].sum())} of {REPS} replicate logits clear of 1e-6")
    assert good, worst
    if margin[0]:
        assert got_point[-1] == point[-1]
    worst_all = 0.0
    for r in range(REPS):
        good, worst = close(got[r][:-1], rows[r][:-1], scale)
        worst_all = max(worst_all, worst)
        assert good, (r, worst)
        if margin[1 + r]:  # one of the kept cases: its pass count is not rounding's to decide
            assert got[r][-1] == rows[r][-1], r
    print(f"k={k} G={G} weighted={weighted}: replicate worst {worst_all:.3e}")


def test_rows_are_deterministic(ob, N):
    """Bitwise: replicate 5 alone, in a boot of 67, at a shifted first_rep, a repeated call, and two batch sizes forced
    through hk_batch."""
    pr = builder(ob, 9, True, reps=200).prepare_density(grid_size=100)
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


@pytest.mark.parametrize("hk_batch", [0, 1])
def test_a_boot_across_a_segment_boundary(ob, N, hk_batch):
    """A boot of one segment and three replicates equals its two halves booted apart and a short boot, byte for byte,
    as tests/test_gpu_boot_segments.py has it for the other kinds; with hk_batch = 1 a batch ends inside the second
    segment's three replicates."""
    seg = FIT_SEG
    pr = builder(ob, 3, True).prepare_density(grid_size=17)
    try:
        def boots():
            return pr.boot(0, seg + 3), pr.boot(0, seg), pr.boot(seg, 3), pr.boot(0, 67)

        if hk_batch:
            with N.option("hk_batch", hk_batch):
                (full, ok), (r0, k0), (r1, k1), (rs, ks) = boots()
        else:
            (full, ok), (r0, k0), (r1, k1), (rs, ks) = boots()
    finally:
        pr.close()
    assert full.shape == (seg + 3, D.row_len(3, 17)) and ok.shape == (seg + 3,)
    assert full.tobytes() == np.concatenate([r0, r1]).tobytes()
    assert ok.tobytes() == np.concatenate([k0, k1]).tobytes()
    assert np.ascontiguousarray(full[:67]).tobytes() == rs.tobytes() and ok[:67].tobytes() == ks.tobytes()
    assert ok.any()


def test_densities_of_a_and_b_are_those_of_run_dfl(ob, N):
    """No logit is involved in f_A and f_B, and both entry points use the grid rule and the bandwidths of dfl.rs."""
    k = 3
    f, xs = frame_of(*R.panel(k, False))
    dfl = ob.run_dfl(f, "y", "g", "B", xs)
    res = builder(ob, k, False, reps=4).decompose_density()
    assert np.array_equal(res.grid, dfl.grid) and len(res.grid) == 100
    assert abs(res.bandwidth_a - dfl.bandwidth_a) <= 1e-14 * dfl.bandwidth_a
    assert abs(res.bandwidth_b - dfl.bandwidth_b) <= 1e-14 * dfl.bandwidth_b
    scale = max(dfl.density_a.max(), dfl.density_b.max())
    for got, want in ((res.density_a.estimate, dfl.density_a), (res.density_b.estimate, dfl.density_b)):
        good, worst = close(got, want, scale)
        print(f"against run_dfl: worst {worst:.3e}")
        assert good, worst


def test_decompose_density_end_to_end(ob, O, N):
    """A frame with a categorical and sample weights; A's outcome lies to the right of B's, so the uniform band of the
    total curve excludes zero on both sides. Every field is that of the restatement on the same seeds."""
    rng = np.random.default_rng(21)
    n = 600
    g = np.where(rng.random(n) < 0.45, "A", "B")
    x1 = rng.normal(size=n) + 0.6 * (g == "A")
    x2 = rng.uniform(0, 2, n)
    cat = rng.choice(["lo", "mid", "hi"], size=n)
    y = 1.0 + 0.8 * x1 - 0.3 * x2 + 0.2 * (cat == "mid") + 0.4 * (g == "A") + 0.3 * rng.normal(size=n)
    w = rng.uniform(0.5, 2.0, n)
    f = {"y": y.tolist(), "g": g.tolist(), "x1": x1.tolist(), "x2": x2.tolist(), "cat": cat.tolist(), "w": w.tolist()}
    reps, G = 60, 40
    b = (ob.OaxacaBuilder(f, "y", "g", "B").predictors(["x1", "x2"]).categorical_predictors(["cat"]).weights("w")
         .bootstrap_reps(reps).seed(SEED))
    res = b.decompose_density(grid_size=G, bandwidth=(0.2, 0.25))
    xa, ya, xb, yb, names = b.get_data_matrices()
    k = xa.shape[1]
    wa, wb = w[g == "A"], w[g == "B"]
    grid = D.default_grid(y, G)
    point, _ = D.decompose(xa, ya, xb, yb, grid, 0.2, 0.25, wa, wb)
    rows, ok, _ = D.boot(O, xa, ya, xb, yb, grid, 0.2, 0.25, wa, wb, SEED, 0, reps)
    assert point is not None and ok.all()
    want = D.aggregate(O, point, rows, ok, G)
    assert np.array_equal(res.grid, grid) and (res.bandwidth_a, res.bandwidth_b) == (0.2, 0.25)
    assert res.names == names and (res.n_a, res.n_b, res.n_failed) == (len(ya), len(yb), 0)
    scale = point[:3 * G].max()
    assert close(res.gamma, point[6 * G:6 * G + k], 1.0)[0]
    assert abs(res.effective_sample_size - point[6 * G + k]) <= RTOL * point[6 * G + k]
    for name in D.CURVES:
        got, w_ = getattr(res, name), want[name]
        for field in ("estimate", "std_err", "ci_lower", "ci_upper", "band_lower", "band_upper"):
            good, worst = close(getattr(got, field), w_[field], scale)
            assert good, (name, field, worst)
        assert np.array_equal(got.p_value, w_["p_value"]), name
        assert abs(got.band_critical - w_["band_critical"]) <= 1e-6 * w_["band_critical"], name
    total, comp = res.total, res.composition
    print(f"total: crit {total.band_critical:.3f}, {(np.sign(total.band_lower) == np.sign(total.band_upper)).sum()} of "
          f"{G} grid points off zero; composition: crit {comp.band_critical:.3f}")
    assert (total.band_lower > 0.0).any() and (total.band_upper < 0.0).any()  # A's density is shifted to the right
    js = json.loads(res.to_json())
    assert js["n_failed"] == 0 and js["names"] == names and js["grid"] == [float(v) for v in res.grid]
    for name in D.CURVES:
        c = getattr(res, name)
        assert js[name]["estimate"] == [float(v) for v in c.estimate]
        assert js[name]["band_lower"] == [float(v) for v in c.band_lower] and js[name]["band_critical"] == c.band_critical
    assert js["gamma"] == [float(v) for v in res.gamma] and js["effective_sample_size"] == res.effective_sample_size
    t = ob.density_last_timing()
    assert t["logit_passes"] >= 2 and t["logit_launches"] >= t["logit_passes"]
    assert t["logit_ms"] > 0.0 and t["density_ms"] > 0.0 and t["finish_ms"] > 0.0


def test_separated_groups_fail_like_the_reweighted_decomposition(ob, N):
    rng = np.random.default_rng(3)
    n = 200
    g = np.where(np.arange(n) < 80, "A", "B")
    x1 = np.where(g == "A", 1.0, -1.0) * (0.5 + rng.random(n))
    f = {"y": (1.0 + rng.normal(size=n)).tolist(), "g": g.tolist(), "x1": x1.tolist()}
    b = ob.OaxacaBuilder(f, "y", "g", "B").predictors(["x1"]).bootstrap_reps(8).seed(SEED)
    with pytest.raises(N.OaxacaError) as e:
        b.decompose_density()
    assert e.value.code == N.OB_E_LINALG
    assert str(e.value) == "Nalgebra error: Failed to solve Information Matrix in Logit. Perfect separation?"


def test_refusals_on_a_density_handle(ob, N):
    b = builder(ob, 3, False)
    pr = b.prepare_density(grid_size=17)
    try:
        with pytest.raises(N.OaxacaError) as e:
            pr.boot_sharded(0, 4)
        assert e.value.code == N.OB_E_UNSUPPORTED and str(e.value) == "density decomposition: sharded runs are outside its scope"
        with pytest.raises(N.OaxacaError) as e:
            pr.jackknife()
        assert e.value.code == N.OB_E_UNSUPPORTED
        assert str(e.value) == "jackknife: density decompositions (BCa included) are outside its scope"
        rows, ok = pr.boot(0, 4)
        with pytest.raises(N.OaxacaError) as e:
            pr.finish_bca(rows, ok)
        assert e.value.code == N.OB_E_UNSUPPORTED
        assert pr.cluster_info is None
    finally:
        pr.close()
    f, xs = frame_of(*R.panel(3, False))
    f["firm"] = [f"f{i % 7}" for i in range(len(f["y"]))]
    c = ob.OaxacaBuilder(f, "y", "g", "B").predictors(xs).cluster("firm")
    with pytest.raises(N.OaxacaError) as e:
        c.prepare_density()
    assert e.value.code == N.OB_E_UNSUPPORTED
