"""Host pieces of the reweighted Oaxaca-Blinder decomposition: the identities of the numpy
restatement, the row length, the shape limits and every refusal before any device work. No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reweight_ref as R  # noqa: E402


def _code(N, fn):
    with pytest.raises(N.OaxacaError) as e:
        fn()
    return e.value.code, str(e.value)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("k", [3, 9, 17])
def test_ref_identities(k, weighted):
    xa, ya, xb, yb, wa, wb = R.panel(k, weighted)
    rng = np.random.default_rng(k)
    for ca, cb in ((None, None), (rng.poisson(1.0, len(ya)), rng.poisson(1.0, len(yb)))):
        row, norms = R.decompose(xa, ya, xb, yb, wa, wb, ca, cb)
        assert row is not None and np.isfinite(row).all() and norms[-1] < R.TOL
        total, comp, struct, pe, se, pu, re = row[:7]
        tol = 1e-12 * abs(total)
        assert abs(comp + struct - total) <= tol
        assert abs(pe + se - comp) <= tol
        assert abs(pu + re - struct) <= tol
        det = row[7:7 + 4 * k].reshape(4, k)
        assert np.all(np.abs(det.sum(1) - row[3:7]) <= tol)
        tail = row[7 + 4 * k:]
        bc, mc, yc = tail[2 * k:3 * k], tail[5 * k:6 * k], tail[7 * k + 2]
        assert abs(yc - mc @ bc) <= tol  # the intercept's normal equation in sample C
        assert 1.0 < tail[7 * k + 3] <= (len(yb) if cb is None else cb.sum()) * (1 + 1e-12)
        assert tail[7 * k + 4] == len(norms)


@pytest.mark.parametrize("k", [3, 9])
def test_ref_gamma_zero_is_plain_ob(k):
    xa, ya, xb, yb, wa, wb = R.panel(k, True)
    row, _ = R.decompose(xa, ya, xb, yb, wa, wb, force_gamma=np.zeros(k))
    tail = row[7 + 4 * k:]
    assert np.array_equal(tail[k:2 * k], tail[2 * k:3 * k])  # beta_C = beta_B
    assert row[4] == 0.0 and np.all(row[7 + k:7 + 2 * k] == 0.0)  # specification_error
    assert row[3] == 0.0 and abs(row[1]) <= 1e-12 * abs(row[0])  # psi = 1: no composition effect at all


def test_row_len_and_shape(ob, N):
    for k in (1, 3, 9, 32):
        assert ob.reweight_row_len(k) == 7 + 11 * k + 5 == R.row_len(k)
    assert ob.reweight_row_len(0) == 0
    assert N.OB_REWEIGHT_MAX_K == 32
    ob.reweight_check_shape(32, 33, 33)
    ob.reweight_check_shape(1, 2, 2)
    assert _code(N, lambda: ob.reweight_check_shape(33, 100, 100))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.reweight_check_shape(3, 3, 100))[0] == N.OB_E_INSUFFICIENT
    assert _code(N, lambda: ob.reweight_check_shape(3, 100, 3))[0] == N.OB_E_INSUFFICIENT
    assert _code(N, lambda: ob.reweight_check_shape(0, 100, 100))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.reweight_check_shape(3, -1, 100))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.reweight_check_shape(3, 2 ** 31, 100))[0] == N.OB_E_UNSUPPORTED


def _frame(n=80, n_x=2):
    rng = np.random.default_rng(4)
    f = {"y": rng.normal(size=n).tolist(), "g": np.where(np.arange(n) % 2 == 0, "A", "B").tolist(),
         "w": rng.uniform(0.5, 2.0, n).tolist(), "s": (rng.random(n) < 0.7).astype(float).tolist(),
         "firm": [f"f{i % 5}" for i in range(n)], "cat": [("u", "v", "w")[i % 3] for i in range(n)]}
    for j in range(n_x):
        f[f"x{j}"] = rng.normal(size=n).tolist()
    return f


def test_refusals_before_device_work(ob, N):
    lib = N.lib()
    fake = C.create_string_buffer(4096)  # no context at all: every check must come before it is read
    ctx = C.cast(fake, C.c_void_p)

    def prepare(builder, run=False):
        cols, ncol, nrow = builder._frame.as_c()
        cfg, keep = builder._config()
        h = C.c_void_p()
        fn = lib.ob_builder_run_reweighted if run else lib.ob_builder_prepare_reweighted
        rc = fn(ctx, cols, ncol, nrow, C.byref(cfg), C.byref(h))
        assert not h.value and fake.raw == bytes(4096)
        return rc, lib.ob_last_error().decode()

    def base(f=None, xs=("x0", "x1")):
        return ob.OaxacaBuilder(_frame() if f is None else f, "y", "g", "B").predictors(list(xs)).seed(1)

    for run in (False, True):
        assert prepare(base().categorical_predictors(["cat"]).normalize(["cat"]), run)[0] == N.OB_E_UNSUPPORTED
        assert prepare(base().heckman_selection("s", ["x0"]), run)[0] == N.OB_E_UNSUPPORTED
    rc, msg = prepare(base().normalize(["cat"]))
    assert rc == N.OB_E_UNSUPPORTED and "normalized" in msg
    rc, msg = prepare(base().heckman_selection("s", ["x0"]))
    assert rc == N.OB_E_UNSUPPORTED and "Heckman" in msg
    # K = 33 > OB_REWEIGHT_MAX_K
    wide = _frame(n=200, n_x=32)
    rc, msg = prepare(base(wide, [f"x{j}" for j in range(32)]))
    assert rc == N.OB_E_UNSUPPORTED and "32" in msg
    # a null and a non-finite value in a named column (the weights column included)
    for col, bad in (("x0", None), ("x1", float("nan")), ("y", float("inf")), ("w", None), ("w", float("nan"))):
        f = _frame()
        f[col][3] = bad
        rc, msg = prepare(base(f).weights("w"))
        assert rc == N.OB_E_INVALID and f"`{col}`" in msg, (col, bad, msg)
    f = _frame()
    f["g"][5] = None
    assert prepare(base(f))[0] == N.OB_E_INVALID
    assert prepare(base(xs=("x0", "nope")))[0] == N.OB_E_COLUMN
    # a group with rows <= K
    small = _frame(n=8, n_x=3)
    rc, msg = prepare(base(small, ["x0", "x1", "x2"]))
    assert rc == N.OB_E_INSUFFICIENT, msg
    # sample weights, categoricals and any reference_coefficients pass every check: the null context is what is left
    good = base().weights("w").categorical_predictors(["cat"]).reference_coefficients(ob.ReferenceCoefficients.Pooled)
    cols, ncol, nrow = good._frame.as_c()
    cfg, keep = good._config()
    h = C.c_void_p()
    rc = lib.ob_builder_prepare_reweighted(None, cols, ncol, nrow, C.byref(cfg), C.byref(h))
    assert rc == N.OB_E_INVALID and "null pointer" in lib.ob_last_error().decode()
    assert lib.ob_builder_prepare_reweighted(None, cols, ncol, nrow, C.byref(cfg), None) == N.OB_E_INVALID


def test_cluster_is_refused(ob, N):
    b = ob.OaxacaBuilder(_frame(), "y", "g", "B").predictors(["x0", "x1"]).cluster("firm")
    for fn in (b.prepare_reweighted, b.decompose_reweighted):
        code, msg = _code(N, fn)
        assert code == N.OB_E_UNSUPPORTED and "cluster" in msg


def test_piece_argument_errors(ob, N):
    x = np.column_stack([np.ones(10), np.arange(10.0)])
    d = (np.arange(10) % 2).astype(float)
    g = np.zeros((1, 2))
    assert _code(N, lambda: ob.reweight_logit_pass(x[:, ::-1], d, g))[0] == N.OB_E_UNSUPPORTED  # no intercept
    assert _code(N, lambda: ob.reweight_logit_pass(x, d + 0.5, g))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.reweight_logit_pass(x, d, np.zeros((65, 2))))[0] == N.OB_E_INVALID
    wide = np.column_stack([np.ones(40)] + [np.arange(40.0)] * 32)
    assert _code(N, lambda: ob.reweight_gram(wide, np.zeros(40), np.zeros((1, 33))))[0] == N.OB_E_UNSUPPORTED
    with pytest.raises(ValueError):
        ob.reweight_gram(x, d, g, counts=np.full(10, 256))
