"""The binary (probit) Oaxaca-Blinder decomposition on the GPU (csrc/ob_binary.hip) against
the numpy restatement tests/binary_ref.py: the mean-probability pass alone, the point pass and 64 + 3
replicates row for row under every supported beta*, bitwise determinism, and the builder end to end.

Panels come from a probit DGP with P(y = 1) between 0.3 and 0.7 in both groups (binary_ref.panel asserts it);
the restatement drops no replicate of them and asserts that every probit converged. Groups of 130 and 257 rows:
a ragged last 64-row sub-tile, more than one tile, and -- by the chunk rule of the panel's chunk table, which
gives a group of two tiles two chunks when both groups together have three -- group B spans two chunks while
group A has one (257 is the smallest row count that does so).

No test makes a replicate fail: oracle.probit's ridge keeps the Hessian solvable even where a group's
resample has a constant outcome (checked on the CPU with a group of K + 2 rows: 100 iterations, no failure), so no
small case exists. Dropping and counting an ok = 0 replicate is ob_prepared_finish's code, shared with run()."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import binary_ref as R  # noqa: E402
from test_gpu_parity import RTOL, SEED, close  # noqa: E402  (the Heckman tests' tolerance for gamma and rows)

pytestmark = pytest.mark.gpu

REPS = 64 + 3  # a ragged replicate batch


def frame_of(xa, ya, xb, yb):
    k = xa.shape[1]
    f = {"y": np.concatenate([ya, yb]).tolist(), "g": ["A"] * len(ya) + ["B"] * len(yb)}
    for j in range(1, k):
        f[f"x{j}"] = np.concatenate([xa[:, j], xb[:, j]]).tolist()
    return f, [f"x{j}" for j in range(1, k)]


def builder(ob, k, ref, reps=REPS):
    f, xs = frame_of(*R.panel(k))
    return (ob.OaxacaBuilder(f, "y", "g", "B").predictors(xs).bootstrap_reps(reps).reference_coefficients(ref)
            .seed(SEED))


_ref_rows = {}


def ref_rows(O, k, ref):
    """The restatement's point row and REPS replicate rows of a case, computed once and shared (read-only)."""
    if (k, ref) not in _ref_rows:
        xa, ya, xb, yb = R.panel(k)
        point, conv = R.decompose(O, xa, ya, xb, yb, ref)
        assert conv
        rows, ok = R.boot(O, xa, ya, xb, yb, ref, SEED, 0, REPS)
        assert ok.all()  # the restatement drops no replicate of these panels
        for a in (point, rows):
            a.setflags(write=False)
        _ref_rows[(k, ref)] = (point, rows)
    return _ref_rows[(k, ref)]


@pytest.mark.parametrize("k", [3, 9, 32])
def test_means_pass_alone(ob, O, k):
    xa, ya, xb, yb = R.panel(k)
    rng = np.random.default_rng(k)
    betas = rng.normal(size=(3, k)) * 0.5 / np.sqrt(k)
    for x, y, g in ((xa, ya, 0), (xb, yb, 1)):
        for c in (None, R.counts(O, SEED, 5, g, len(y))):
            got = ob.binary_means(x, y, betas, counts=c)
            w = np.ones(len(y)) if c is None else c.astype(float)
            want = np.array([np.sum(w * O._ncdf(x @ b)) / w.sum() for b in betas])
            print(f"k={k} g={g} counts={c is not None}: max |dP| = {np.abs(got['probabilities'] - want).max():.3e}")
            assert np.all(np.abs(got["probabilities"] - want) <= RTOL * np.maximum(np.abs(want), 1e-300))
            assert got["n"] == w.sum()
            assert abs(got["y_mean"] - np.sum(w * y) / w.sum()) <= RTOL
            xm = (w[:, None] * x).sum(0) / w.sum()
            assert got["x_mean"][0] == 1.0 and np.all(np.abs(got["x_mean"] - xm) <= RTOL * np.maximum(np.abs(xm), 1.0))


@pytest.mark.parametrize("ref", R.REFS, ids=["group_a", "group_b", "weighted", "cotton"])
@pytest.mark.parametrize("k", [3, 9])
def test_rows_match_ref(ob, O, N, k, ref):
    point, rows = ref_rows(O, k, ref)
    pr = builder(ob, k, ref).prepare_binary()
    try:
        assert pr.row_len == R.row_len(k)
        got_point = pr.point_row()
        got, ok = pr.boot(0, REPS)
    finally:
        pr.close()
    assert ok.all() and np.isfinite(got).all() and np.isfinite(got_point).all()
    good, worst = close(got_point, point, point[5])
    print(f"k={k} ref={ref}: point worst {worst:.3e}")
    assert good, worst
    worst_all = 0.0
    for r in range(REPS):
        good, worst = close(got[r], rows[r], rows[r][5])
        worst_all = max(worst_all, worst)
        assert good, (r, worst)
    print(f"k={k} ref={ref}: replicate worst {worst_all:.3e}")
    if ref == R.GROUP_A:  # U_A's zero denominator: 0.0, not NaN; P(A, beta_A) == P(A, beta*)
        assert np.array_equal(got[:, 6 + 7 * k], got[:, 6 + 7 * k + 2])
    if ref == R.GROUP_B:
        assert np.array_equal(got[:, 6 + 7 * k + 4], got[:, 6 + 7 * k + 5])


def test_group_b_spans_two_chunks(ob, N):
    pr = builder(ob, 3, R.GROUP_A).prepare_binary()
    try:
        table = (C.c_uint32 * 96)()
        n = C.c_int32()
        N.check(N.lib().ob_debug_chunks(N.lib().ob_prepared_panel(pr._h), table, 32, C.byref(n)))
    finally:
        pr.close()
    assert [tuple(table[3 * i:3 * i + 3]) for i in range(n.value)] == [(0, 0, 1), (1, 0, 1), (1, 1, 2)]


@pytest.mark.parametrize("k", [3, 9])
def test_rows_are_deterministic(ob, N, k):
    """Bitwise: replicate r's row in a boot of 1, of 67 and at a shifted first_rep; a repeated call; and, where
    the wide path batches replicates, forced batches of 64."""
    b = builder(ob, k, R.WEIGHTED, reps=200)
    pr = b.prepare_binary()
    try:
        r0, k0 = pr.boot(0, 200)
        r1, k1 = pr.boot(0, REPS)
        r2, k2 = pr.boot(66, 1)
        r3, k3 = pr.boot(41, 130)
        r4, k4 = pr.boot(0, 200)
    finally:
        pr.close()
    assert k0.all()
    assert r0.tobytes() == r4.tobytes() and np.array_equal(k0, k4)
    assert r0[:REPS].tobytes() == r1.tobytes() and np.array_equal(k0[:REPS], k1)
    assert r0[66:67].tobytes() == r2.tobytes() and np.array_equal(k0[66:67], k2)
    assert r0[41:171].tobytes() == r3.tobytes() and np.array_equal(k0[41:171], k3)
    if k > 8:
        with N.option("hk_batch", 1):
            pr = b.prepare_binary()
            try:
                rb, kb = pr.boot(0, 200)
            finally:
                pr.close()
        assert r0.tobytes() == rb.tobytes() and np.array_equal(k0, kb)


def test_library_erfc_matches_ref(ob, O, N):
    """Option hk_erfc = 0: the probit and the means pass both take the library erfc."""
    point, rows = ref_rows(O, 3, R.WEIGHTED)
    with N.option("hk_erfc", 0):
        pr = builder(ob, 3, R.WEIGHTED).prepare_binary()
        try:
            got, ok = pr.boot(0, 8)
        finally:
            pr.close()
    assert ok.all()
    for r in range(8):
        good, worst = close(got[r], rows[r], rows[r][5])
        assert good, (r, worst)


def test_decompose_binary_end_to_end(ob, O, N):
    """A dict frame with one categorical: names and estimates equal the point row, the standard errors equal
    bootstrap_stats of the restatement's replicate rows; ob_builder_run_binary gives the same tables."""
    rng = np.random.default_rng(21)
    n = 400
    g = np.where(rng.random(n) < 0.45, "A", "B")
    x1, x2 = rng.normal(size=n), rng.uniform(0, 2, n)
    cat = rng.choice(["lo", "mid", "hi"], size=n)
    idx = -0.2 + 0.5 * x1 - 0.3 * x2 + 0.3 * (cat == "mid") + 0.35 * (g == "A")
    y = (idx + rng.normal(size=n) > 0).astype(float)
    f = {"y": y.tolist(), "g": g.tolist(), "x1": x1.tolist(), "x2": x2.tolist(), "cat": cat.tolist()}
    reps = 40
    b = (ob.OaxacaBuilder(f, "y", "g", "B").predictors(["x1", "x2"]).categorical_predictors(["cat"])
         .bootstrap_reps(reps).reference_coefficients(ob.ReferenceCoefficients.Weighted).seed(SEED))
    res = b.decompose_binary()
    xa, ya, xb, yb, names = b.get_data_matrices()
    k = xa.shape[1]
    assert names == ["__ob_intercept__", "x1", "x2", "cat_lo", "cat_mid"] == res.names and k == 5
    assert 0.3 <= ya.mean() <= 0.7 and 0.3 <= yb.mean() <= 0.7
    point, conv = R.decompose(O, xa, ya, xb, yb, R.WEIGHTED)
    rows, ok = R.boot(O, xa, ya, xb, yb, R.WEIGHTED, SEED, 0, reps)
    assert conv and ok.all()
    scale = abs(point[5])
    assert res.n_a == len(ya) and res.n_b == len(yb) and res.n_failed == 0 and res.model == "probit"
    assert abs(res.total_gap - point[5]) <= RTOL * scale
    assert abs(res.raw_gap - (ya.mean() - yb.mean())) <= 1e-15
    tail = point[6 + 2 * k:]
    for got, want in ((res.beta_a, tail[:k]), (res.beta_b, tail[k:2 * k]), (res.beta_star, tail[4 * k:5 * k])):
        assert np.all(np.abs(got - want) <= RTOL * np.maximum(np.abs(want), 1.0))
    keys = [(gg, bb) for gg in ("A", "B") for bb in ("beta_a", "beta_b", "beta_star")]
    assert list(res.probabilities) == keys
    for key, want in zip(keys, tail[5 * k:5 * k + 6]):
        assert abs(res.probabilities[key] - want) <= RTOL * want

    def check(comps, cols, cnames):
        assert [c.name for c in comps] == cnames
        for c, col in zip(comps, cols):
            se, p, (lo, hi) = O.bootstrap_stats(rows[:, col])
            assert abs(c.estimate - point[col]) <= RTOL * max(abs(point[col]), scale), c.name
            for a, w in ((c.std_err, se), (c.ci_lower, lo), (c.ci_upper, hi)):
                assert abs(a - w) <= RTOL * max(abs(w), scale), (c.name, a, w)

    check(res.two_fold, [0, 1], ["explained", "unexplained"])
    check(res.three_fold, [2, 3, 4], ["endowments", "coefficients", "interaction"])
    check(res.detailed_explained, list(range(6, 6 + k)), names)
    check(res.detailed_unexplained, list(range(6 + k, 6 + 2 * k)), names)
    assert '"model": "probit"' in res.to_json()
    # the C entry point that runs everything: the same tables, bitwise (same seed, same kernels)
    cols, ncol, nrow = b._frame.as_c()
    cfg, keep = b._config()
    h = C.c_void_p()
    N.check(N.lib().ob_builder_run_binary(N.context(None), cols, ncol, nrow, C.byref(cfg), N.OB_BINARY_PROBIT, C.byref(h)))
    from importlib import import_module
    r2 = import_module("oaxaca-blinder-rs_amd.api")._results_from_c(h)
    assert r2.total_gap == res.total_gap
    for c, d in zip(res.two_fold + res.detailed_unexplained, r2.two_fold.aggregate + r2.two_fold.detailed_unexplained):
        assert (c.name, c.estimate, c.std_err, c.ci_lower, c.ci_upper) == (d.name, d.estimate, d.std_err, d.ci_lower,
                                                                         d.ci_upper)
    t = ob.binary_last_timing()
    assert t["probit_launches"] >= 1 and t["means_ms"] > 0.0 and t["epilogue_ms"] > 0.0


def test_refusals_on_a_binary_handle(ob, N):
    pr = builder(ob, 3, R.GROUP_A).prepare_binary()
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
