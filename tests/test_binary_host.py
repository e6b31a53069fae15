"""Host pieces of the binary (probit) Oaxaca-Blinder decomposition: the identities of the
numpy restatement, the row length, the shape limits and every argument error before any device work. No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import binary_ref as R  # noqa: E402


def _code(N, fn):
    with pytest.raises(N.OaxacaError) as e:
        fn()
    return e.value.code, str(e.value)


@pytest.mark.parametrize("ref", R.REFS)
@pytest.mark.parametrize("k", [3, 9])
def test_ref_identities(O, k, ref):
    xa, ya, xb, yb = R.panel(k)
    row, conv = R.decompose(O, xa, ya, xb, yb, ref)
    assert conv and np.isfinite(row).all()
    expl, unex, endow, coef, inter, total = row[:6]
    dex, dun = row[6:6 + k], row[6 + k:6 + 2 * k]
    paa, pab, pas, pba, pbb, pbs = row[6 + 7 * k:6 + 7 * k + 6]
    eps = 8 * np.finfo(float).eps  # sums of at most 2 K terms of magnitude below 1
    assert abs(expl + unex - total) <= eps
    assert abs(endow + coef + inter - total) <= eps
    assert abs(dex.sum() - expl) <= 4 * k * eps
    assert abs(dun.sum() - ((paa - pas) + (pbs - pbb))) <= 4 * k * eps
    assert abs(total - (paa - pbb)) <= eps and 0.0 <= min(paa, pab, pas, pba, pbb, pbs) <= 1.0
    if ref == R.GROUP_A:  # U_A = 0 exactly, its zero denominator contributes 0.0 and not NaN
        assert paa == pas and abs(dun.sum() - (pbs - pbb)) <= 4 * k * eps
    if ref == R.GROUP_B:
        assert pbb == pbs and abs(dun.sum() - (paa - pas)) <= 4 * k * eps
    assert abs(row[-2] - ya.mean()) == 0.0 and abs(row[-1] - yb.mean()) == 0.0


def test_ref_weighted_is_cotton_and_between(O):
    xa, ya, xb, yb = R.panel(3)
    w, _ = R.decompose(O, xa, ya, xb, yb, R.WEIGHTED)
    c, _ = R.decompose(O, xa, ya, xb, yb, R.COTTON)
    assert np.array_equal(w, c)
    ba, bb, bs = w[12:15], w[15:18], w[24:27]
    wa = len(ya) / (len(ya) + len(yb))
    assert np.allclose(bs, wa * ba + (1 - wa) * bb, rtol=1e-15)


SEED, REPS = 0x0B5EED, 64 + 3  # test_gpu_binary.py's: the properties below are those of the rows it compares


def test_panel_defaults_are_unchanged():
    """panel()'s new arguments leave the panels of the earlier tests as they were (first values recorded before)."""
    xa, ya, xb, yb = R.panel(3)
    assert xa.shape == (130, 3) and xb.shape == (257, 3)
    assert (ya.sum(), yb.sum()) == (80.0, 126.0)
    assert np.array_equal(R.panel(3)[0], R.panel(3, slope=1.0, x_scale=1.0, c0_shift=(0.0, 0.0), planted=())[0])
    with pytest.raises(AssertionError):
        R.panel(32, 1000, 2049)  # the mild band fails there (0.706), so K = 32 stays at 600 / 1025


@pytest.mark.parametrize("k", [1, 2, 8, 16, 17, 32])
def test_width_panels_converge_everywhere(O, k):
    """The sizes of R.SIZES: the point fit and all 134 resampled probits converge and no replicate is dropped."""
    point, conv, rows, ok, cv = R.case_rows(O, k, R.WEIGHTED, SEED, REPS)
    assert conv and ok.all() and cv.all() and np.isfinite(rows).all() and np.isfinite(point).all()


def test_k16_at_the_small_size_runs_out_of_iterations(O):
    point, conv, rows, ok, cv = R.case_rows(O, "k16_small", R.WEIGHTED, SEED, REPS)
    assert conv and ok.all() and np.isfinite(rows).all()
    assert tuple(np.flatnonzero(cv == 0)) == R.K16_SMALL_UNCONVERGED


def _clamped_in_both(O, p, row, rep=None):
    k = p[0].shape[1]
    tail = row[6 + 2 * k:]
    n = []
    for g, (x, beta) in enumerate(((p[0], tail[:k]), (p[2], tail[k:2 * k]))):
        n.append(R.clamped_rows(x, beta, None if rep is None else R.counts(O, SEED, rep, g, len(x))))
    return min(n)


def test_steep_panel_reaches_the_clamp(O):
    """From the restatement's fitted coefficients: rows beyond |z| = 6.3613 in both groups at the point fit and in at
    least half of the replicates; every probit converges."""
    p = R.steep_panel()
    point, conv, rows, ok, cv = R.case_rows(O, "steep", R.WEIGHTED, SEED, REPS)
    assert conv and ok.all() and cv.all()
    assert _clamped_in_both(O, p, point) >= 1
    assert sum(_clamped_in_both(O, p, rows[r], r) >= 1 for r in range(REPS)) >= (REPS + 1) // 2


def test_outlier_panel_rows_sit_beyond_the_clamp(O):
    """The planted rows lie beyond the clamp at the converged point fit of each group. Not every replicate converges
    (binary_ref.outlier_panel): exactly the listed ones run out of iterations, and none is dropped."""
    xa, ya, xb, yb = p = R.outlier_panel()
    for x, y in ((xa, ya), (xb, yb)):
        assert [tuple(r) for r in x[-2:, 1:]] == [(-40.0, 0.0), (40.0, 0.0)] and not y[-2:].any()
    point, conv, rows, ok, cv = R.case_rows(O, "outliers", R.WEIGHTED, SEED, REPS)
    assert conv and ok.all() and np.isfinite(rows).all()
    tail = point[6 + 2 * 3:]
    for x, beta in ((xa, tail[:3]), (xb, tail[3:6])):
        assert np.all(np.abs(x[-2:] @ beta) > R.CLAMP_Z)
    assert tuple(np.flatnonzero(cv == 0)) == R.OUTLIER_UNCONVERGED


def test_lopsided_panel_bands_and_convergence(O):
    xa, ya, xb, yb = R.lopsided_panel()
    assert (len(ya), len(yb)) == R.LOPSIDED_SIZES
    assert 0.02 <= ya.mean() <= 0.06 and 0.94 <= yb.mean() <= 0.98
    point, conv, rows, ok, cv = R.case_rows(O, "lopsided", R.WEIGHTED, SEED, REPS)
    assert conv and ok.all() and cv.all()


def test_means_hp_agrees_with_the_restatement(O):
    """The mpmath reference of the means pass against oracle._ncdf at mild indices (both are exact to rounding)."""
    xa, ya, _, _ = R.panel(3)
    betas = np.array([[0.1, 0.4, -0.3], [0.0, 0.2, 0.2], [-0.2, 0.1, 0.5]])
    w = R.counts(O, SEED, 5, 0, len(ya))
    got = R.means_hp(R.phi_hp(xa, betas), w)
    want = np.array([np.sum(w * O._ncdf(xa @ b)) / w.sum() for b in betas])
    assert np.all(np.abs(got - want) <= 1e-15)
    # the erfc-in-fsum stand-in for very long designs, at indices out to +-40: a few ulp of the mpmath value
    steep = betas * 60.0
    hp, fs = R.phi_hp(xa, steep), R.phi_fsum(xa, steep)
    assert max(abs(float(h) - f) for a, b in zip(hp, fs) for h, f in zip(a, b)) <= 1e-15
    # relative, in the far tail: the products' rounding, 3 * 2^-53 |z|, times |z| = 40 is 5e-13
    assert all(abs(float(h) - f) <= 1e-12 * float(h) for a, b in zip(hp, fs) for h, f in zip(a, b) if float(h) > 1e-300)
    assert np.all(np.abs(R.means_hp(hp, w) - R.means_fsum(fs, w)) <= 1e-15)


def test_row_len_and_shape(ob, N):
    for k in (1, 3, 9, 32):
        assert ob.binary_row_len(k) == 6 + 7 * k + 8 == R.row_len(k)
    assert N.OB_BINARY_MAX_K == 32
    ob.binary_check_shape(32, 33, 33)
    ob.binary_check_shape(1, 2, 2)
    assert _code(N, lambda: ob.binary_check_shape(33, 100, 100))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.binary_check_shape(3, 3, 100))[0] == N.OB_E_INSUFFICIENT
    assert _code(N, lambda: ob.binary_check_shape(3, 100, 3))[0] == N.OB_E_INSUFFICIENT
    assert _code(N, lambda: ob.binary_check_shape(0, 100, 100))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.binary_check_shape(3, -1, 100))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.binary_check_shape(3, 2 ** 31, 100))[0] == N.OB_E_UNSUPPORTED


def _frame(n=80, n_x=2, y=None):
    rng = np.random.default_rng(4)
    f = {"y": (rng.random(n) < 0.5).astype(float).tolist() if y is None else list(y),
         "g": np.where(np.arange(n) % 2 == 0, "A", "B").tolist(),
         "w": rng.uniform(0.5, 2.0, n).tolist(), "s": (rng.random(n) < 0.7).astype(float).tolist(),
         "firm": [f"f{i % 5}" for i in range(n)], "cat": [("u", "v", "w")[i % 3] for i in range(n)]}
    for j in range(n_x):
        f[f"x{j}"] = rng.normal(size=n).tolist()
    return f


def test_argument_errors_before_device_work(ob, N):
    lib = N.lib()
    fake = C.create_string_buffer(4096)  # no context at all: every check must come before it is read
    ctx = C.cast(fake, C.c_void_p)

    def prepare(builder, model=N.OB_BINARY_PROBIT, run=False):
        cols, ncol, nrow = builder._frame.as_c()
        cfg, keep = builder._config()
        h = C.c_void_p()
        fn = lib.ob_builder_run_binary if run else lib.ob_builder_prepare_binary
        rc = fn(ctx, cols, ncol, nrow, C.byref(cfg), model, C.byref(h))
        assert not h.value and fake.raw == bytes(4096)
        return rc, lib.ob_last_error().decode()

    def base(f, xs=("x0", "x1")):
        return ob.OaxacaBuilder(f, "y", "g", "B").predictors(list(xs)).seed(1)

    f = _frame()
    for run in (False, True):
        assert prepare(base(f), model=N.OB_BINARY_LOGIT, run=run)[0] == N.OB_E_UNSUPPORTED
        assert prepare(base(f).weights("w"), run=run)[0] == N.OB_E_UNSUPPORTED
        assert prepare(base(f).categorical_predictors(["cat"]).normalize(["cat"]), run=run)[0] == N.OB_E_UNSUPPORTED
        assert prepare(base(f).heckman_selection("s", ["x1"]), run=run)[0] == N.OB_E_UNSUPPORTED
        for ref in (ob.ReferenceCoefficients.Pooled, ob.ReferenceCoefficients.Neumark):
            assert prepare(base(f).reference_coefficients(ref), run=run)[0] == N.OB_E_UNSUPPORTED
    assert prepare(base(f), model=7)[0] == N.OB_E_INVALID
    assert prepare(base(f, ["x0", "nope"]))[0] == N.OB_E_COLUMN
    # outcome values other than exactly 0.0 or 1.0
    y = np.array(f["y"])
    for bad in (0.5, 2.0, -1.0, float("nan")):
        yy = y.copy()
        yy[7] = bad
        rc, msg = prepare(base(_frame(y=yy)))
        assert rc == N.OB_E_INVALID and "0.0 or 1.0" in msg
    # a null in a named column (outcome, predictor, categorical, group)
    for col in ("y", "x1", "cat", "g"):
        fn = _frame()
        fn[col] = list(fn[col])
        fn[col][5] = None
        rc, msg = prepare(base(fn).categorical_predictors(["cat"]))
        assert rc == N.OB_E_INVALID and f"`{col}`" in msg
    # a group whose outcome is constant
    yy = y.copy()
    yy[1::2] = 1.0  # group B
    rc, msg = prepare(base(_frame(y=yy)))
    assert rc == N.OB_E_INVALID and "group B" in msg
    # K > 32: 32 predictors and the intercept
    wide = _frame(n=200, n_x=32)
    assert prepare(base(wide, [f"x{j}" for j in range(32)]))[0] == N.OB_E_UNSUPPORTED
    # a group with rows <= K: 3 rows a group, K = 3
    small = _frame(n=6)
    small["y"] = [0.0, 1.0, 1.0, 0.0, 1.0, 1.0]
    assert prepare(base(small))[0] == N.OB_E_INSUFFICIENT
    # null pointers
    cols, ncol, nrow = base(f)._frame.as_c()
    cfg, keep = base(f)._config()
    h = C.c_void_p()
    assert lib.ob_builder_prepare_binary(ctx, cols, ncol, nrow, C.byref(cfg), 0, None) == N.OB_E_INVALID
    assert lib.ob_builder_prepare_binary(None, cols, ncol, nrow, C.byref(cfg), 0, C.byref(h)) == N.OB_E_INVALID
    assert lib.ob_builder_run_binary(None, cols, ncol, nrow, C.byref(cfg), 0, C.byref(h)) == N.OB_E_INVALID
    assert lib.ob_builder_prepare_binary(ctx, cols, ncol, nrow, None, 0, C.byref(h)) == N.OB_E_INVALID
    assert lib.ob_binary_last_timing(None) == N.OB_E_INVALID
    assert lib.ob_prepared_point_row(None, None, None) == N.OB_E_INVALID
    assert fake.raw == bytes(4096)


def test_python_refusals_before_a_context(ob, N):
    f = _frame()
    b = ob.OaxacaBuilder(f, "y", "g", "B").predictors(["x0"]).seed(1)
    assert _code(N, lambda: b.cluster("firm").decompose_binary())[0] == N.OB_E_UNSUPPORTED
    b.cluster(None)
    assert _code(N, lambda: b.decompose_binary(model="logit"))[0] == N.OB_E_UNSUPPORTED
    with pytest.raises(ValueError):
        b.decompose_binary(model="cloglog")
    assert _code(N, lambda: b.weights("w").decompose_binary())[0] == N.OB_E_UNSUPPORTED


def test_binary_means_argument_errors(ob, N):
    x = np.column_stack([np.ones(10), np.arange(10.0)])
    y = (np.arange(10) % 2).astype(float)
    betas = np.zeros((3, 2))
    assert _code(N, lambda: ob.binary_means(np.ones((10, 33)), y, np.zeros((3, 33))))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.binary_means(x[:, ::-1], y, betas))[0] == N.OB_E_UNSUPPORTED  # no intercept column
    assert _code(N, lambda: ob.binary_means(x, y, betas, counts=np.zeros(10, dtype=int)))[0] == N.OB_E_INVALID
    with pytest.raises(ValueError):
        ob.binary_means(x, y, np.zeros((2, 2)))
    with pytest.raises(ValueError):
        ob.binary_means(x, y, betas, counts=np.full(10, 256))


def test_results_to_json(ob):
    import json

    c = ob.ComponentResult("explained", 0.1, 0.02, 5.0, 0.0, 0.06, 0.14)
    r = ob.BinaryDecompositionResults(
        "probit", 0.12, 0.11, [c], [c], [c], [c], {("A", "beta_a"): 0.6, ("B", "beta_b"): float("nan")},
        np.array([0.1, 0.2]), np.array([0.0, 0.3]), np.array([0.1, 0.2]), np.array([1.0, 0.4]), np.array([1.0, 0.1]),
        ["__ob_intercept__", "x"], 10, 12, 1)
    d = json.loads(r.to_json())
    assert d["model"] == "probit" and d["total_gap"] == 0.12 and d["raw_gap"] == 0.11 and d["n_failed"] == 1
    assert d["probabilities"] == {"A|beta_a": 0.6, "B|beta_b": None}
    assert d["two_fold"][0]["name"] == "explained" and d["beta_b"] == [0.0, 0.3]
