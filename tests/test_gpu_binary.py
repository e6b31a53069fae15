"""The binary (probit) Oaxaca-Blinder decomposition on the GPU (csrc/ob_binary.hip) against
the numpy restatement tests/binary_ref.py: the mean-probability pass alone, the point pass and 64 + 3
replicates row for row under every supported beta*, bitwise determinism, and the builder end to end.

Widths 1, 2, 3, 8, 9, 16, 17 and 32 (binary_ref.SIZES gives each the smallest panel on which every resampled probit
converges), a steep, an outlier and a lopsided panel, a panel whose probits run out of iterations, and the means
pass against mpmath at the row counts, count bytes and index ranges where its loops change shape.

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


def builder(ob, case, ref, reps=REPS):
    """case: a width (binary_ref.SIZES' panel of it) or the name of a hard panel (binary_ref.case_panel)."""
    f, xs = frame_of(*R.case_panel(case))
    return (ob.OaxacaBuilder(f, "y", "g", "B").predictors(xs).bootstrap_reps(reps).reference_coefficients(ref)
            .seed(SEED))


def ref_rows(O, case, ref):
    """The restatement's point row and REPS replicate rows of a case that converges everywhere, computed once and
    shared (read-only) with test_binary_host.py."""
    point, conv, rows, ok, cv = R.case_rows(O, case, ref, SEED, REPS)
    assert conv
    assert ok.all() and cv.all()  # the restatement drops no replicate of these panels and every probit converges
    return point, rows


def boot_handle(ob, case, ref, reps=REPS):
    pr = builder(ob, case, ref).prepare_binary()
    try:
        assert pr.row_len == R.row_len(R.case_panel(case)[0].shape[1])
        got_point = pr.point_row()
        got, ok = pr.boot(0, reps)
    finally:
        pr.close()
    return got_point, got, ok


def compare_rows(label, got_point, got, point, rows, which=None):
    """close() on the point row and on the replicate rows in `which` (default: all); prints the worst of each."""
    good, worst = close(got_point, point, point[5])
    print(f"{label}: point worst {worst:.3e}")
    assert good, worst
    worst_all = 0.0
    for r in range(len(rows)) if which is None else which:
        good, worst = close(got[r], rows[r], rows[r][5])
        worst_all = max(worst_all, worst)
        assert good, (r, worst)
    print(f"{label}: replicate worst {worst_all:.3e}")


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


REF_IDS = {R.GROUP_A: "group_a", R.GROUP_B: "group_b", R.WEIGHTED: "weighted", R.COTTON: "cotton"}
# K = 3 and 9 under every rule; the other widths under Weighted (both coefficient vectors) and GroupA; K = 32 also
# under GroupB, so that the row kernel's second gather trip feeds a row whose U_B denominator is 0 too. Widths: 1 and
# 2 (gs = k | 1, the <1> and <2> probits), 8 (the last register-resident probit: a segment whole), 16, 17 and 32 (the
# MFMA probit in batches).
ROW_CASES = [(k, ref) for k in (3, 9) for ref in R.REFS]
ROW_CASES += [(k, ref) for k in (1, 2, 8, 16, 17, 32) for ref in (R.WEIGHTED, R.GROUP_A)] + [(32, R.GROUP_B)]


def second_trip_check(O, k, got_point, got):
    """K >= 28: the row kernel gathers 2 (5 + K) > 64 chunk sums, the second trip of its lanes carries group B's
    covariate sums of columns 22 .. 31. Those means against the resample's counts, so that a failure names the trip."""
    xb = R.case_panel(k)[2]
    lo = 6 + 2 * k + 3 * k + 22
    for r in range(-1, len(got)):
        row = got_point if r < 0 else got[r]
        w = np.ones(len(xb)) if r < 0 else R.counts(O, SEED, r, 1, len(xb)).astype(float)
        want = (w[:, None] * xb[:, 22:32]).sum(0) / w.sum()
        assert np.all(np.abs(row[lo:lo + 10] - want) <= RTOL * np.maximum(np.abs(want), 1.0)), (r, row[lo:lo + 10], want)


@pytest.mark.parametrize("k,ref", [pytest.param(k, ref, id=f"{k}-{REF_IDS[ref]}") for k, ref in ROW_CASES])
def test_rows_match_ref(ob, O, N, k, ref):
    point, rows = ref_rows(O, k, ref)
    got_point, got, ok = boot_handle(ob, k, ref)
    assert ok.all() and np.isfinite(got).all() and np.isfinite(got_point).all()
    if k >= 28:
        second_trip_check(O, k, got_point, got)
    compare_rows(f"k={k} ref={ref}", got_point, got, point, rows)
    if ref == R.GROUP_A:  # U_A's zero denominator: 0.0, not NaN; P(A, beta_A) == P(A, beta*)
        assert np.array_equal(got[:, 6 + 7 * k], got[:, 6 + 7 * k + 2])
    if ref == R.GROUP_B:
        assert np.array_equal(got[:, 6 + 7 * k + 4], got[:, 6 + 7 * k + 5])


def chunk_table(ob, N, case):
    pr = builder(ob, case, R.GROUP_A).prepare_binary()
    try:
        table = (C.c_uint32 * 96)()
        n = C.c_int32()
        N.check(N.lib().ob_debug_chunks(N.lib().ob_prepared_panel(pr._h), table, 32, C.byref(n)))
    finally:
        pr.close()
    return [tuple(table[3 * i:3 * i + 3]) for i in range(n.value)]


def test_chunk_tables_of_the_wider_panels(ob, N):
    """300 / 513 and 600 / 1025 rows: 2 + 3 and 3 + 5 tiles, a chunk a tile. A panel of at most 32 tiles never gets a
    chunk of two (the engine cuts about 32 chunks), so through a handle the means kernel's walk over a second tile
    needs more than 8,192 rows; test_means_row_counts runs it at 33,025 rows through ob_binary_means."""
    assert chunk_table(ob, N, 16) == [(0, 0, 1), (0, 1, 2), (1, 0, 1), (1, 1, 2), (1, 2, 3)]
    assert chunk_table(ob, N, 32) == [(0, 0, 1), (0, 1, 2), (0, 2, 3), (1, 0, 1), (1, 1, 2), (1, 2, 3), (1, 3, 4),
                                      (1, 4, 5)]


def test_group_b_spans_two_chunks(ob, N):
    pr = builder(ob, 3, R.GROUP_A).prepare_binary()
    try:
        table = (C.c_uint32 * 96)()
        n = C.c_int32()
        N.check(N.lib().ob_debug_chunks(N.lib().ob_prepared_panel(pr._h), table, 32, C.byref(n)))
    finally:
        pr.close()
    assert [tuple(table[3 * i:3 * i + 3]) for i in range(n.value)] == [(0, 0, 1), (1, 0, 1), (1, 1, 2)]


@pytest.mark.parametrize("k", [3, 8, 9, 32])
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


@pytest.mark.parametrize("case", ["steep", "lopsided"])
def test_hard_panels_match_ref(ob, O, case):
    """steep: fitted indices beyond the probit's clamp (clamp_phi, the one reciprocal, both branches of lambda) at
    the point fit and in most replicates. lopsided: y-bar near 0.04 and 0.97, every Phi of the means pass in Cody's
    middle and outer regions and Yun's shares over small denominators. test_binary_host.py proves both properties."""
    point, rows = ref_rows(O, case, R.WEIGHTED)
    got_point, got, ok = boot_handle(ob, case, R.WEIGHTED)
    assert ok.all() and np.isfinite(got).all() and np.isfinite(got_point).all()
    compare_rows(case, got_point, got, point, rows)


def test_steep_panel_library_erfc(ob, O, N):
    """The clamp beside the library erfc (option hk_erfc = 0)."""
    point, rows = ref_rows(O, "steep", R.WEIGHTED)
    with N.option("hk_erfc", 0):
        got_point, got, ok = boot_handle(ob, "steep", R.WEIGHTED, reps=8)
    assert ok.all()
    compare_rows("steep, library erfc", got_point, got, point, rows[:8])


def unconverged_case(ob, O, case, expected, compare_all):
    """A panel on which the restatement's probits run out of iterations in exactly the replicates `expected`. The
    device keeps such a replicate (ok = 1, a finite row): equal ok flags and finite rows everywhere, close() on
    every replicate the restatement converged on. The others' deviation is printed; compare_all asserts it too."""
    point, conv, rows, ok_ref, cv = R.case_rows(O, case, R.WEIGHTED, SEED, REPS)
    assert conv and tuple(np.flatnonzero(cv == 0)) == expected  # more or others: fail, do not compare fewer rows
    got_point, got, ok = boot_handle(ob, case, R.WEIGHTED)
    assert np.array_equal(ok, ok_ref) and ok.all()
    assert np.isfinite(got).all() and np.isfinite(got_point).all()
    compare_rows(case, got_point, got, point, rows, which=None if compare_all else np.flatnonzero(cv))
    for r in expected:
        print(f"{case}: replicate {r} (out of iterations) deviates by {close(got[r], rows[r], rows[r][5])[1]:.3e}")


def test_outlier_panel_matches_ref(ob, O):
    """(x_1 = 40, y = 0) and (x_1 = -40, y = 0) in each group: beyond the clamp at the point fit, where phi underflows
    and the rows get neither weight nor score; replicates that did not draw them are compared like the rest. In 21
    replicates the restatement's iteration does not settle in 100 passes (binary_ref.outlier_panel); ten of those rows
    still agree to 1e-12, the others carry rounding differences forward and differ by 5e-12 to 3.5 in units of the
    gap (measured on an MI355X), so they are left out of the value comparison, and only they."""
    unconverged_case(ob, O, "outliers", R.OUTLIER_UNCONVERGED, compare_all=False)


def test_out_of_iterations_keeps_the_replicate(ob, O):
    """K = 16 at 130 / 257 rows: two replicates have a probit at its 100th iteration. Their rows agree with the
    restatement to 1.2e-15 and 7.9e-14 (measured on an MI355X), so all 67 replicates are compared."""
    unconverged_case(ob, O, "k16_small", R.K16_SMALL_UNCONVERGED, compare_all=True)


def hard_probit_xy(case, g, k):
    """Group g's design of a hard K = 3 panel, for K = 9 padded with six mild N(0, 1) columns."""
    p = R.case_panel(case)
    x, y = p[2 * g], p[2 * g + 1]
    if k > 3:
        x = np.column_stack([x, np.random.default_rng(31 * k + g).normal(size=(len(y), k - 3))])
    return x, y


@pytest.mark.parametrize("k", [3, 9])
@pytest.mark.parametrize("g", [0, 1])
@pytest.mark.parametrize("case", ["steep", "outliers"])
def test_probit_piece_on_hard_designs(ob, O, case, g, k):
    """ob_probit beyond the clamp, on the narrow (K = 3) and the MFMA (K = 9) kernels: the convergence flag, the
    iteration count and the coefficients, as test_gpu_heckman_wide.test_probit_piece_matches_oracle on mild shapes."""
    x, y = hard_probit_xy(case, g, k)
    want = O.probit(y, x, full=True)
    assert want["converged"] and want["iterations"] < 100
    assert R.clamped_rows(x, want["coefficients"]) >= 1
    beta, conv, iters = ob.probit(x, y)
    dev = np.abs(beta - want["coefficients"]) / np.maximum(np.abs(want["coefficients"]), 1.0)
    print(f"{case} g={g} k={k}: {iters} iterations (restatement {want['iterations']}), worst {dev.max():.3e}")
    assert conv == want["converged"] and iters == want["iterations"]
    assert np.all(dev <= RTOL)


_means_designs = {}


def means_design(n, k):
    """x, y, three coefficient vectors whose indices span about +-3, +-8 and +-40 (Cody's three regions, and in the
    last exact 0 and 1, inside one sum) and the mpmath Phi of every row under each; computed once (read-only)."""
    if (n, k) not in _means_designs:
        rng = np.random.default_rng(100 * n + k)
        x = np.column_stack([np.ones(n), rng.normal(size=(n, k - 1))])
        y = (rng.random(n) < 0.4).astype(float)
        d = rng.normal(size=k - 1)
        t = x[:, 1:] @ d
        d *= -np.sign(t[np.argmax(np.abs(t))]) / np.abs(t).max()  # the extreme row's index is -span
        betas = np.array([np.concatenate([[0.0], s * d]) for s in (3.0, 8.0, 40.0)])
        for a in (x, y, betas):
            a.setflags(write=False)
        _means_designs[(n, k)] = (x, y, betas, (R.phi_hp if n <= MP_ROWS else R.phi_fsum)(x, betas))
    return _means_designs[(n, k)]


MP_ROWS = 4096  # up to here the reference is mpmath at 50 digits; the one longer design takes erfc in an exact sum


def check_means(ob, n, k, c, label):
    """n, y_mean and x_mean[0] are ratios of exactly summed integers: ==. The probabilities to RTOL relative."""
    x, y, betas, phis = means_design(n, k)
    got = ob.binary_means(x, y, betas, counts=c)
    w = np.ones(n) if c is None else np.asarray(c, dtype=float)
    want = (R.means_hp if n <= MP_ROWS else R.means_fsum)(phis, c)
    dev = np.abs(got["probabilities"] - want) / np.maximum(np.abs(want), 1e-300)
    print(f"n={n} k={k} {label}: P = {want}, worst relative {dev.max():.3e}")
    assert got["n"] == w.sum()
    assert got["y_mean"] == np.sum(w * y) / w.sum()
    assert np.all(dev <= RTOL)
    xm = (w[:, None] * x).sum(0) / w.sum()
    assert got["x_mean"][0] == 1.0 and np.all(np.abs(got["x_mean"] - xm) <= RTOL * np.maximum(np.abs(xm), 1.0))


# 33,025 rows are 130 tiles in ob_binary_means' 128 chunks: two chunks of two tiles, the smallest row count at which a
# thread's register sums cross a tile boundary. K = 28 is the first width with a fifth reduction round, 32 the limit.
@pytest.mark.parametrize("n,k", [(1, 3), (63, 3), (64, 3), (65, 3), (256, 3), (257, 3), (33025, 3), (257, 28), (257, 32)])
def test_means_row_counts(ob, O, n, k):
    check_means(ob, n, k, None, "unit counts")
    check_means(ob, n, k, R.counts(O, SEED, 5, 0, n), "resample counts")


def test_means_counts_in_the_byte_lanes(ob):
    """255 in each byte of a count word, whole four-row groups at 0 (the thread skips the sub-tile before the
    barrier), a whole 64-row sub-tile at 0, and a single counted row: the last one."""
    n = 257
    c = np.random.default_rng(3).integers(0, 4, n)
    c[[12, 13, 14, 15, 129, 200, 256]] = 255
    c[16:24] = 0
    c[64:128] = 0
    check_means(ob, n, 3, c, "255s and zero groups")
    last = np.zeros(n, dtype=np.int64)
    last[-1] = 3
    check_means(ob, n, 3, last, "the last row alone")


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
