"""Host pieces of Nopo's matching decomposition: the cells and their order, the shape limits, every
refusal before any device work, the aggregation of given rows and the restatement's own identity. No GPU."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nopo_ref as R  # noqa: E402


def _code(N, fn):
    with pytest.raises(N.OaxacaError) as e:
        fn()
    return e.value.code, str(e.value)


def test_row_len_and_shape(ob, N):
    assert ob.nopo_row_len() == R.ROW_LEN == 13
    ob.nopo_check_shape(1, 1, 1)
    ob.nopo_check_shape(522240, 2 ** 31 - 1, 2 ** 31 - 1)
    assert _code(N, lambda: ob.nopo_check_shape(522241, 10, 10))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.nopo_check_shape(5, 2 ** 31, 10))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.nopo_check_shape(5, 10, 2 ** 31))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.nopo_check_shape(5, 0, 10))[0] == N.OB_E_INSUFFICIENT
    assert _code(N, lambda: ob.nopo_check_shape(5, 10, 0))[0] == N.OB_E_INSUFFICIENT
    assert _code(N, lambda: ob.nopo_check_shape(-1, 10, 10))[0] == N.OB_E_INVALID


@pytest.mark.parametrize("name", ["main", "tiny"])
def test_cells_match_ref(ob, name):
    p = R.panel(name, False)
    row_cell, n_cells = ob.nopo_cells(p.frame, "y", "g", "B", ["x"], ["s"])
    assert n_cells == p.n_cells == len({"main": R.MAIN_CELLS, "tiny": R.TINY_CELLS}[name])
    assert row_cell.dtype == np.int32 and np.array_equal(row_cell, p.row_cell)
    if name == "main":  # the keys in id order are the specification's; -0.0 and 0.0 share cell 2
        assert [(float(x), s) for x, s in p.keys] == [(x, s) for x, s, _, _ in R.MAIN_CELLS]
        x, s = np.array(p.frame["x"]), np.array(p.frame["s"])
        zero = (x == 0.0) & (s == "p")
        assert np.signbit(x[zero]).any() and not np.signbit(x[zero]).all() and set(row_cell[zero]) == {2}


def test_cells_order_strings_integers_third_level_and_bins(ob):
    f = {"y": [1.0] * 8, "g": ["A", "B", "A", "B", "C", "A", "B", "A"],
         "age": [31, 25, 25, 47, 25, 39, 31, 20], "s": ["b", "a", "a", "b", "a", "Z", "b", "a"]}
    # strings by bytes ("Z" < "a"), then integers; the row of level C has no cell
    row_cell, n_cells = ob.nopo_cells(f, "y", "g", "B", [], ["s"])
    assert n_cells == 3 and row_cell.tolist() == [2, 1, 1, 2, -1, 0, 2, 1]
    row_cell, n_cells = ob.nopo_cells(f, "y", "g", "B", ["age"], ["s"])
    used = [i for i in range(8) if f["g"][i] != "C"]
    ids, n_ref, keys = R.cells([np.array(f["age"])[used], np.array(f["s"])[used]])
    assert n_cells == n_ref == 5 and row_cell[used].tolist() == ids.tolist() and row_cell[4] == -1
    assert keys == sorted(keys) == [(20, "a"), (25, "a"), (31, "b"), (39, "Z"), (47, "b")]  # predictors come first
    # bins: the column is replaced by its numpy.digitize index
    row_cell, n_cells = ob.nopo_cells(f, "y", "g", "B", ["age"], [], bins={"age": [30, 40]})
    idx = np.digitize(np.array(f["age"], dtype=float), [30, 40])
    assert n_cells == 3 and row_cell[used].tolist() == idx[used].tolist()
    with pytest.raises(ValueError):
        ob.nopo_cells(f, "y", "g", "B", ["age"], ["s"], bins={"s": [1]})


def _frame(n=80):
    rng = np.random.default_rng(4)
    return {"y": rng.normal(size=n).tolist(), "g": np.where(np.arange(n) % 2 == 0, "A", "B").tolist(),
            "w": rng.uniform(0.5, 2.0, n).tolist(), "sel": (rng.random(n) < 0.7).astype(float).tolist(),
            "firm": [f"f{i % 5}" for i in range(n)], "cat": [("u", "v", "w")[i % 3] for i in range(n)],
            "x0": rng.integers(0, 4, n).astype(float).tolist(), "x1": rng.integers(0, 3, n).tolist()}


def test_refusals_before_device_work(ob, N):
    lib = N.lib()
    fake = C.create_string_buffer(4096)  # no context at all: every check must come before it is read
    ctx = C.cast(fake, C.c_void_p)

    def prepare(builder, run=False):
        cols, ncol, nrow = builder._frame.as_c()
        cfg, keep = builder._config()
        h = C.c_void_p()
        fn = lib.ob_builder_run_nopo if run else lib.ob_builder_prepare_nopo
        rc = fn(ctx, cols, ncol, nrow, C.byref(cfg), C.byref(h))
        assert not h.value and fake.raw == bytes(4096)
        return rc, lib.ob_last_error().decode()

    def base(f=None, xs=("x0", "x1")):
        return ob.OaxacaBuilder(_frame() if f is None else f, "y", "g", "B").predictors(list(xs)).seed(1)

    for run in (False, True):
        rc, msg = prepare(base().categorical_predictors(["cat"]).normalize(["cat"]), run)
        assert rc == N.OB_E_UNSUPPORTED and "normalized" in msg
        rc, msg = prepare(base().heckman_selection("sel", ["x0"]), run)
        assert rc == N.OB_E_UNSUPPORTED and "Heckman" in msg
        rc, msg = prepare(base(xs=()), run)
        assert rc == N.OB_E_INVALID and "no matching column" in msg
    # a null and a non-finite value in a named column, a negative or non-finite weight
    for col, bad in (("x0", None), ("x0", float("nan")), ("y", float("inf")), ("w", None), ("w", float("nan")),
                     ("w", float("inf")), ("cat", None), ("x1", None)):
        f = _frame()
        f[col][3] = bad
        rc, msg = prepare(base(f).categorical_predictors(["cat"]).weights("w"))
        assert rc == N.OB_E_INVALID and f"`{col}`" in msg, (col, bad, msg)
    f = _frame()
    f["w"][7] = -0.5
    rc, msg = prepare(base(f).weights("w"))
    assert rc == N.OB_E_INVALID and "negative" in msg
    f = _frame()
    f["g"][5] = None
    assert prepare(base(f))[0] == N.OB_E_INVALID
    assert prepare(base(xs=("x0", "nope")))[0] == N.OB_E_COLUMN
    assert prepare(base().categorical_predictors(["x0"]))[0] == N.OB_E_POLARS  # a categorical column holds strings
    assert prepare(base(xs=("cat",)))[0] == N.OB_E_POLARS  # a numeric one does not
    # a group without rows, or without positive weight
    f = _frame()
    f["g"] = ["A" if i else "C" for i in range(80)]
    f["g"][1] = "C"
    rc, msg = prepare(ob.OaxacaBuilder(f, "y", "g", "B").predictors(["x0"]))
    assert rc == N.OB_E_INSUFFICIENT and "no rows" in msg, msg  # B is absent
    f = _frame()
    f["w"] = [0.0 if g == "A" else 1.0 for g in f["g"]]
    rc, msg = prepare(base(f).weights("w"))
    assert rc == N.OB_E_INSUFFICIENT and "positive weight" in msg
    # a point pass with an empty support: no cell holds weight of both groups
    f = _frame()
    f["x0"] = [float(i % 2) for i in range(80)]  # A's rows are the even ones
    rc, msg = prepare(base(f, xs=("x0",)))
    assert rc == N.OB_E_INSUFFICIENT and "no common support" in msg
    f["x0"] = [0.0] * 80  # one cell, but A's weight in it is zero except where B's is
    f["w"] = [0.0 if g == "A" else 1.0 for g in f["g"]]
    f["w"][0] = 1.0
    f["x0"][0] = 5.0
    rc, msg = prepare(base(f, xs=("x0",)).weights("w"))
    assert rc == N.OB_E_INSUFFICIENT and "no common support" in msg
    # sample weights, categoricals and any reference_coefficients pass every check: the null context is what is left
    good = base().weights("w").categorical_predictors(["cat"]).reference_coefficients(ob.ReferenceCoefficients.Pooled)
    cols, ncol, nrow = good._frame.as_c()
    cfg, keep = good._config()
    h = C.c_void_p()
    rc = lib.ob_builder_prepare_nopo(None, cols, ncol, nrow, C.byref(cfg), C.byref(h))
    assert rc == N.OB_E_INVALID and "null pointer" in lib.ob_last_error().decode()
    assert lib.ob_builder_prepare_nopo(None, cols, ncol, nrow, C.byref(cfg), None) == N.OB_E_INVALID
    assert lib.ob_builder_run_nopo(None, cols, ncol, nrow, C.byref(cfg), None) == N.OB_E_INVALID


def test_cluster_is_refused(ob, N):
    b = ob.OaxacaBuilder(_frame(), "y", "g", "B").predictors(["x0", "x1"]).cluster("firm")
    for fn in (b.prepare_nopo, b.decompose_nopo):
        code, msg = _code(N, fn)
        assert code == N.OB_E_UNSUPPORTED and "cluster" in msg


def test_sums_argument_errors(ob, N):
    y, cell = np.arange(6.0), np.array([0, 0, 1, 1, 2, 2])
    assert _code(N, lambda: ob.nopo_sums(y, cell[::-1].copy(), 3))[0] == N.OB_E_INVALID  # not ascending
    assert _code(N, lambda: ob.nopo_sums(y, cell, 2))[0] == N.OB_E_INVALID  # an id outside [0, n_cells)
    assert _code(N, lambda: ob.nopo_sums(y, cell, 3, w=-np.ones(6)))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.nopo_sums(y, cell, 522241))[0] == N.OB_E_UNSUPPORTED
    with pytest.raises(ValueError):
        ob.nopo_sums(y, cell, 3, counts=np.full((2, 6), 256))
    with pytest.raises(ValueError):
        ob.nopo_sums(y, cell[:5], 3)


def test_finish_rows_match_bootstrap_stats(ob, O, N):
    """nopo_finish_rows on rows of the restatement, the failed ones among them: every component is the point entry
    with the oracle's bootstrap statistics of its column over the rows kept."""
    point, okp, rows, ok, _ = R.boot(O, "tiny", True)
    assert okp and 0 < ok.sum() < len(ok)
    res = ob.nopo_finish_rows(point, rows, ok)
    want = R.aggregate(O, point, rows, ok)
    assert res.n_failed == int(len(ok) - ok.sum()) and tuple(res.components) == R.COMPONENTS
    for name, w in zip(R.COMPONENTS, want):
        c = res.components[name]
        assert c.name == name and c.estimate == w[0] and getattr(res, name) is c
        for got, exp in ((c.std_err, w[1]), (c.ci_lower, w[2]), (c.ci_upper, w[3])):
            assert abs(got - exp) <= 1e-12 * max(abs(exp), 1.0), (name, got, exp)
    js = json.loads(res.to_json())
    assert js["n_failed"] == res.n_failed and js["components"]["unexplained"]["estimate"] == res.unexplained.estimate
    with pytest.raises(ValueError):
        ob.nopo_finish_rows(point[:-1], rows, ok)


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("name", ["main", "tiny"])
def test_ref_identity(O, name, weighted):
    """D = D_X + D_0 + D_A + D_B in the restatement, on the GPU tests' panels: the point row and every replicate
    kept; both unmatched terms are non-zero at the main panel's point."""
    p = R.panel(name, weighted)
    point, okp, rows, ok, sup = R.boot(O, name, weighted)
    assert okp
    for row in [point] + [r for r, k in zip(rows, ok) if k]:
        assert abs(row[0] - row[1:5].sum()) <= p.tol, row
        assert abs(row[0] - (row[5] - row[6])) <= p.tol
    assert np.isnan(rows[~ok.astype(bool)]).all()
    if name == "main":
        assert point[3] != 0.0 and point[4] != 0.0 and point[12] == 6 and ok.all()
    else:
        assert point[4] == 0.0 and point[11] == 1.0 and np.all(rows[ok.astype(bool), 4] == 0.0)
