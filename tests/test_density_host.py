"""Host pieces of the bootstrapped DFL density decomposition: the row length and shape limits, the
default grid, the aggregation of given rows with its uniform bands, and every refusal before any device work.
No GPU."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_ref as D  # noqa: E402


def _code(N, fn):
    with pytest.raises(N.OaxacaError) as e:
        fn()
    return e.value.code, str(e.value)


def test_row_len_and_shape(ob, N):
    for k, G in ((1, 2), (3, 17), (4, 100), (32, 256)):
        assert ob.density_row_len(k, G) == 6 * G + k + 2 == D.row_len(k, G)
    assert ob.density_row_len(0, 100) == 0 and ob.density_row_len(3, 1) == 0 and ob.density_row_len(3, 257) == 0
    assert (N.OB_DENSITY_MAX_GRID, N.OB_REWEIGHT_MAX_K) == (D.MAX_GRID, D.MAX_K) == (256, 32)
    ob.density_check_shape(32, 33, 33, 256)
    ob.density_check_shape(1, 2, 2, 2)
    assert _code(N, lambda: ob.density_check_shape(3, 100, 100, 1))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.density_check_shape(3, 100, 100, 257))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.density_check_shape(33, 100, 100, 100))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.density_check_shape(3, 3, 100, 100))[0] == N.OB_E_INSUFFICIENT
    assert _code(N, lambda: ob.density_check_shape(3, 100, 3, 100))[0] == N.OB_E_INSUFFICIENT
    assert _code(N, lambda: ob.density_check_shape(0, 100, 100, 100))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.density_check_shape(3, 2 ** 31, 100, 100))[0] == N.OB_E_UNSUPPORTED


def test_grid_is_the_rule_of_dfl(ob, N):
    rng = np.random.default_rng(5)
    y = rng.normal(size=1935) * 3.0 + 0.7
    for G in (2, 17, 100, 256):
        got = ob.density_grid(y, G)
        assert np.array_equal(got, D.default_grid(y, G)) and len(got) == G
        assert got[0] == y.min() and got[-1] < y.max() and np.all(np.diff(got) > 0)
        assert abs(got[-1] + (y.max() - y.min()) / G - y.max()) <= 1e-12 * np.abs(y).max()
    assert np.array_equal(ob.density_grid(y, 0), D.default_grid(y, 100))
    assert _code(N, lambda: ob.density_grid(y, 1))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.density_grid(y, 257))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.density_grid(np.array([1.0, np.nan]), 10))[0] == N.OB_E_INVALID


def _synthetic_rows(k, G, reps, dropped, flat, seed):
    """A point row and replicate rows around it; entry `flat` of every curve does not move (se = 0: the value 0.5
    keeps the mean of any number of copies exact)."""
    rng = np.random.default_rng(seed)
    point = rng.normal(size=D.row_len(k, G))
    point[flat:6 * G:G] = 0.5
    rows = point[None, :] + 0.1 * rng.normal(size=(reps, len(point))) * (1.0 + np.arange(len(point)) % 3)
    for c in range(6):
        rows[:, c * G + flat] = point[c * G + flat]
    ok = np.ones(reps, dtype=np.uint8)
    for r in dropped:
        rows[r], ok[r] = np.nan, 0
    return point, rows, ok


# kept replicates R: floor(0.95 R) is R - 1 for R = 19 and is not for R = 40 (38) and R = 21 (19)
@pytest.mark.parametrize("reps,dropped", [(19, ()), (40, ()), (24, (3, 17, 20))])
def test_finish_rows_match_ref(ob, O, N, reps, dropped):
    k, G, flat = 3, 17, 5
    point, rows, ok = _synthetic_rows(k, G, reps, dropped, flat, seed=reps)
    R = reps - len(dropped)
    assert (int(np.floor(0.95 * R)) == R - 1) == (reps == 19)
    grid = np.linspace(-1.0, 2.0, G)
    res = ob.density_finish_rows(point, k, grid, rows, ok, 0.3, 0.4)
    want = D.aggregate(O, point, rows, ok, G)
    assert res.n_failed == len(dropped) and np.array_equal(res.grid, grid)
    assert (res.bandwidth_a, res.bandwidth_b) == (0.3, 0.4)
    assert np.array_equal(res.gamma, point[6 * G:6 * G + k]) and res.effective_sample_size == point[6 * G + k]
    for name in D.CURVES:
        got, w = getattr(res, name), want[name]
        assert np.array_equal(got.estimate, w["estimate"]), name
        for f in ("std_err", "p_value", "ci_lower", "ci_upper", "band_lower", "band_upper"):
            a, b = getattr(got, f), w[f]
            assert np.all(np.abs(a - b) <= 1e-12 * np.maximum(np.abs(b), 1.0)), (name, f)
        assert abs(got.band_critical - w["band_critical"]) <= 1e-12 * w["band_critical"], name
        assert got.std_err[flat] == 0.0 and got.band_lower[flat] == got.band_upper[flat] == got.estimate[flat]
        live = np.arange(G) != flat
        assert np.all(got.std_err[live] > 0.0) and np.all(got.band_upper[live] > got.band_lower[live])
        # the uniform band is no narrower than 95 % of the replicates' largest deviation asks for
        kept = rows[ok.astype(bool)][:, D.CURVES.index(name) * G:][:, :G]
        inside = np.all((kept >= got.band_lower - 1e-12) & (kept <= got.band_upper + 1e-12), axis=1)
        assert inside.mean() >= 0.95 - 1.0 / R
    js = json.loads(res.to_json())
    assert js["n_failed"] == len(dropped) and js["grid"] == [float(v) for v in grid]
    assert js["total"]["band_critical"] == res.total.band_critical
    assert js["structure"]["band_upper"] == [float(v) for v in res.structure.band_upper]
    with pytest.raises(ValueError):
        ob.density_finish_rows(point[:-1], k, grid, rows, ok)


def test_finish_rows_without_replicates(ob, N):
    k, G = 2, 4
    point = np.arange(D.row_len(k, G), dtype=float)
    res = ob.density_finish_rows(point, k, np.arange(4.0), np.empty((0, len(point))), np.empty(0, dtype=np.uint8))
    assert res.n_failed == 0 and np.array_equal(res.total.estimate, point[3 * G:4 * G])
    assert np.isnan(res.total.band_critical) and np.isnan(res.total.std_err).all()
    lib = N.lib()
    h = C.c_void_p()
    dp = C.POINTER(C.c_double)
    assert lib.ob_density_finish_rows(point.ctypes.data_as(dp), 33, G, None, None, 0, C.byref(h)) == N.OB_E_INVALID
    assert lib.ob_density_finish_rows(point.ctypes.data_as(dp), k, 257, None, None, 0, C.byref(h)) == N.OB_E_INVALID
    assert lib.ob_density_finish_rows(None, k, G, None, None, 0, C.byref(h)) == N.OB_E_INVALID


def _frame(n=80, n_x=2):
    rng = np.random.default_rng(4)
    f = {"y": rng.normal(size=n).tolist(), "g": np.where(np.arange(n) % 2 == 0, "A", "B").tolist(),
         "w": rng.uniform(0.5, 2.0, n).tolist(), "s": (rng.random(n) < 0.7).astype(float).tolist(),
         "firm": [f"f{i % 5}" for i in range(n)], "cat": [("u", "v", "w")[i % 3] for i in range(n)]}
    for j in range(n_x):
        f[f"x{j}"] = rng.normal(size=n).tolist()
    return f


def _density_config(N, grid_size=0, grid=None, bandwidth_a=0.0, bandwidth_b=0.0):
    keep = None
    dc = N.ob_density_config()
    dc.grid_size, dc.grid = grid_size, None
    if grid is not None:
        keep = np.ascontiguousarray(grid, dtype=np.float64)
        dc.grid, dc.grid_size = keep.ctypes.data_as(C.POINTER(C.c_double)), len(keep)
    dc.bandwidth_a, dc.bandwidth_b = bandwidth_a, bandwidth_b
    return dc, keep


def test_refusals_before_device_work(ob, N):
    lib = N.lib()
    fake = C.create_string_buffer(4096)  # no context at all: every check must come before it is read
    ctx = C.cast(fake, C.c_void_p)

    def prepare(builder, run=False, **kw):
        cols, ncol, nrow = builder._frame.as_c()
        cfg, keep = builder._config()
        dc, keep2 = _density_config(N, **kw)
        h = C.c_void_p()
        fn = lib.ob_builder_run_density if run else lib.ob_builder_prepare_density
        rc = fn(ctx, cols, ncol, nrow, C.byref(cfg), C.byref(dc), C.byref(h))
        assert not h.value and fake.raw == bytes(4096)
        return rc, lib.ob_last_error().decode()

    def base(f=None, xs=("x0", "x1")):
        return ob.OaxacaBuilder(_frame() if f is None else f, "y", "g", "B").predictors(list(xs)).seed(1)

    for run in (False, True):
        rc, msg = prepare(base().categorical_predictors(["cat"]).normalize(["cat"]), run)
        assert rc == N.OB_E_UNSUPPORTED and msg == "density decomposition: normalized categoricals are outside its scope"
        rc, msg = prepare(base().heckman_selection("s", ["x0"]), run)
        assert rc == N.OB_E_UNSUPPORTED and msg == "density decomposition: Heckman selection settings are outside its scope"
        assert prepare(base(), run, grid_size=257)[0] == N.OB_E_UNSUPPORTED
        assert prepare(base(), run, grid_size=1)[0] == N.OB_E_INVALID
    # K = 33 > OB_REWEIGHT_MAX_K
    wide = _frame(n=200, n_x=32)
    rc, msg = prepare(base(wide, [f"x{j}" for j in range(32)]))
    assert rc == N.OB_E_UNSUPPORTED and "32" in msg
    # a grid that is not finite and strictly increasing, or too short or too long
    for grid in ([0.0, 0.0, 1.0], [1.0, 0.5], [0.0, np.nan, 1.0], [0.0, np.inf], [0.3]):
        rc, msg = prepare(base(), grid=grid)
        assert rc == N.OB_E_INVALID and "grid" in msg, (grid, msg)
    assert prepare(base(), grid=np.arange(257.0))[0] == N.OB_E_UNSUPPORTED
    assert prepare(base(), grid_size=-1)[0] == N.OB_E_INVALID
    # a bandwidth that is not finite and > 0
    for bad in (-0.5, float("nan"), float("inf")):
        for kw in ({"bandwidth_a": bad}, {"bandwidth_b": bad}):
            rc, msg = prepare(base(), **kw)
            assert rc == N.OB_E_INVALID and "bandwidth" in msg, (kw, msg)
    # a null and a non-finite value in a named column (the weights column included), a negative weight
    for col, bad in (("x0", None), ("x1", float("nan")), ("y", float("inf")), ("w", None), ("w", float("nan"))):
        f = _frame()
        f[col][3] = bad
        rc, msg = prepare(base(f).weights("w"))
        assert rc == N.OB_E_INVALID and f"`{col}`" in msg, (col, bad, msg)
    f = _frame()
    f["w"][6] = -1.0
    rc, msg = prepare(base(f).weights("w"))
    assert rc == N.OB_E_INVALID and "negative weight" in msg and "`w`" in msg
    f = _frame()
    f["g"][5] = None
    assert prepare(base(f))[0] == N.OB_E_INVALID
    assert prepare(base(xs=("x0", "nope")))[0] == N.OB_E_COLUMN
    # a group with rows <= K, and one without positive weight
    small = _frame(n=8, n_x=3)
    rc, msg = prepare(base(small, ["x0", "x1", "x2"]))
    assert rc == N.OB_E_INSUFFICIENT, msg
    f = _frame()
    f["w"] = [0.0 if g == "A" else w for g, w in zip(f["g"], f["w"])]
    rc, msg = prepare(base(f).weights("w"))
    assert rc == N.OB_E_INSUFFICIENT and "positive weight" in msg
    # a constant outcome has no default grid and no Silverman bandwidth
    const = _frame()
    const["y"] = [1.0] * 80
    assert prepare(base(const))[0] == N.OB_E_INVALID
    assert prepare(base(const), grid=[0.0, 1.0, 2.0])[0] == N.OB_E_INVALID
    # sample weights, categoricals, any reference_coefficients, a grid and bandwidths pass every check: the null
    # context is what is left
    good = base().weights("w").categorical_predictors(["cat"]).reference_coefficients(ob.ReferenceCoefficients.Pooled)
    cols, ncol, nrow = good._frame.as_c()
    cfg, keep = good._config()
    h = C.c_void_p()
    for kw in ({}, {"grid": [-1.0, 0.0, 0.5, 2.0], "bandwidth_a": 0.3, "bandwidth_b": 0.25}, {"grid_size": 256}):
        dc, keep2 = _density_config(N, **kw)
        rc = lib.ob_builder_prepare_density(None, cols, ncol, nrow, C.byref(cfg), C.byref(dc), C.byref(h))
        assert rc == N.OB_E_INVALID and "null pointer" in lib.ob_last_error().decode(), kw
    rc = lib.ob_builder_prepare_density(None, cols, ncol, nrow, C.byref(cfg), None, C.byref(h))  # NULL: every default
    assert rc == N.OB_E_INVALID and "null pointer: ctx" in lib.ob_last_error().decode()
    assert lib.ob_builder_prepare_density(None, cols, ncol, nrow, C.byref(cfg), C.byref(dc), None) == N.OB_E_INVALID


def test_cluster_is_refused(ob, N):
    b = ob.OaxacaBuilder(_frame(), "y", "g", "B").predictors(["x0", "x1"]).cluster("firm")
    for fn in (b.prepare_density, b.decompose_density):
        code, msg = _code(N, fn)
        assert code == N.OB_E_UNSUPPORTED and msg == "density decomposition: the cluster bootstrap is outside its scope"


def test_python_argument_errors(ob, N):
    b = ob.OaxacaBuilder(_frame(), "y", "g", "B").predictors(["x0", "x1"])
    with pytest.raises(ValueError):
        b.prepare_density(bandwidth=[0.1, 0.2, 0.3])
    with pytest.raises(ValueError):
        b.prepare_density(bandwidth=0.0)
    with pytest.raises(ValueError):
        b.prepare_density(grid=np.zeros((2, 2)))
    # through the Python layer the argument errors still come before the missing device
    assert _code(N, lambda: b.prepare_density(grid=[1.0, 0.0]))[0] == N.OB_E_INVALID
    assert _code(N, lambda: b.prepare_density(bandwidth=-1.0))[0] == N.OB_E_INVALID
    assert _code(N, lambda: b.prepare_density(grid_size=300))[0] == N.OB_E_UNSUPPORTED


def test_pass_argument_errors(ob, N):
    x = np.column_stack([np.ones(10), np.arange(10.0)])
    y = np.arange(10.0)
    grid = np.linspace(0.0, 9.0, 5)
    assert _code(N, lambda: ob.density_pass(x[:, ::-1], y, grid, 1.0))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.density_pass(x, y, grid, 0.0))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.density_pass(x, y, grid, float("nan")))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.density_pass(x, y, grid[:1], 1.0))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.density_pass(x, y, np.arange(257.0), 1.0))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.density_pass(x, y, [0.0, np.inf], 1.0))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.density_pass(x, y, grid, 1.0, gammas=np.zeros((65, 2))))[0] == N.OB_E_INVALID
    wide = np.column_stack([np.ones(40)] + [np.arange(40.0)] * 32)
    assert _code(N, lambda: ob.density_pass(wide, np.arange(40.0), grid, 1.0))[0] == N.OB_E_UNSUPPORTED
    with pytest.raises(ValueError):
        ob.density_pass(x, y, grid, 1.0, counts=np.full(10, 256))
    with pytest.raises(ValueError):
        ob.density_pass(x, y[:-1], grid, 1.0)
    with pytest.raises(ValueError):
        ob.density_pass(x, y, grid, 1.0, gammas=np.zeros((1, 3)))
