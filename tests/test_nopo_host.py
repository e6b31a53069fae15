"""Host pieces of Nopo's matching decomposition: the cells and their order, the shape limits, every
refusal before any device work, the aggregation of given rows and the restatement's own identity; the exact
reference beside the restatement, and the stated property of every panel and group the GPU tests rely on (zero
weights, the offset, a cell per row, the edge shapes, the 33,025-row group's exact products, the count bytes). No GPU."""
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


@pytest.mark.parametrize("name,weighted", [("main", True), ("main", False), ("tiny", True), ("offset", True)])
def test_exact_reference_beside_the_restatement(O, name, weighted):
    """The Fraction reference and the numpy restatement are two computations of one definition: equal ok flags and
    supports, rows within the panel's tolerance of each other, N bit for bit where the weights are dyadic."""
    p = R.panel(name, weighted)
    point, okp, rows, ok, sup = R.boot_exact(O, name, weighted)
    rpoint, rokp, rrows, rok, rsup = (R.boot(O, name, weighted) if name != "offset" else
                                      (*p.point(), *p.boot(O, 0, R.REPS)))
    assert okp == rokp == 1 and np.array_equal(ok, rok) and np.array_equal(sup[:-1], rsup)
    keep = ok.astype(bool)
    assert np.isnan(rows[~keep]).all()
    assert np.abs(point - rpoint).max() <= p.tol and np.abs(rows[keep] - rrows[keep]).max() <= p.tol
    assert np.array_equal(rows[keep, 12], rrows[keep, 12])
    if name != "offset":
        assert np.array_equal(rows[keep][:, [10, 11]], rrows[keep][:, [10, 11]])
    for g in (0, 1):
        c = p.counts(O, 1, g)
        n_ex, s_ex = R.sums_exact(p.y[g], p.w[g], p.cell[g], p.n_cells, c)
        n_np, s_np = R.sums(p.y[g], p.w[g], p.cell[g], p.n_cells, c)
        assert np.abs(s_ex - s_np).max() <= p.tol
        assert np.array_equal(n_ex, n_np) if name != "offset" else np.abs(n_ex - n_np).max() <= p.tol
        assert not np.array_equal(s_ex, s_np) or name == "tiny"  # the order of a sum does show in its last bits


def test_zero_w_panel(O):
    """The zero_w panel's properties (nopo_ref: (a) .. (d)), by weight, before any GPU test relies on them."""
    p, m = R.panel("zero_w", True), R.panel("main", True)
    assert p.n == m.n == [130, 257] and p.n_cells == len(R.MAIN_CELLS) and np.array_equal(p.row_cell, m.row_cell)
    assert all(np.array_equal(p.y[g], m.y[g]) for g in (0, 1))
    wa, wb, ca, cb = p.w[0], p.w[1], p.cell[0], p.cell[1]
    assert np.all(wa[ca == R.ZERO_A_CELL] == 0.0) and (ca == R.ZERO_A_CELL).sum() == 20  # (a)
    assert np.all(wb[cb == R.ZERO_A_CELL] > 0.0) and (cb == R.ZERO_A_CELL).sum() == 70
    one = wa[ca == R.ONE_ROW_CELL]
    assert len(one) == 30 and (one > 0.0).sum() == 1 and wb[cb == R.ONE_ROW_CELL].sum() > 0.0  # (b)
    for w, c in ((wa, ca), (wb, cb)):  # (c)
        inside = w[c == R.MIXED_CELL]
        assert (inside == 0.0).sum() >= 10 and (inside > 0.0).sum() >= 20
    (na, sa), (nb, sb) = p.fractions()
    sup = np.array([a > 0 and b > 0 for a, b in zip(na, nb)])
    rows_a = np.bincount(ca, minlength=p.n_cells)
    outside = np.flatnonzero(~sup & (rows_a > 0))
    assert set(outside) == {R.ZERO_A_CELL, *R.A_ONLY_CELLS} and all(na[x] == 0 for x in outside)  # (d)
    assert sup.sum() == 5 and not sup[R.ZERO_A_CELL] and sup[R.ONE_ROW_CELL] and sup[R.MIXED_CELL]
    # the support by rows differs from the support by weight, at the point pass and in the replicates
    assert (rows_a[R.ZERO_A_CELL] > 0) and np.bincount(cb, minlength=p.n_cells)[R.ZERO_A_CELL] > 0
    point, okp, rows, ok, rsup = R.boot_exact(O, "zero_w", True)
    assert okp and ok.all() and point[3] == 0.0 and point[12] == 5 and point[4] != 0.0
    assert np.array_equal(rsup[-1], sup) and not rsup[:, R.ZERO_A_CELL].any()
    kept = rsup[:-1, R.ONE_ROW_CELL]  # (b): the replicates that draw the one weighted row keep the cell, the others lose it
    the_row = np.flatnonzero((ca == R.ONE_ROW_CELL) & (wa > 0.0))[0]
    drawn = np.array([p.counts(O, r, 0)[the_row] > 0 for r in range(R.REPS)])
    rows_drawn = np.array([p.counts(O, r, 0)[ca == R.ONE_ROW_CELL].sum() > 0 for r in range(R.REPS)])
    assert np.array_equal(kept, drawn) and 10 <= kept.sum() <= R.REPS - 10 and rows_drawn.all()
    zero_out = rows[:, 3] == 0.0  # N_A^out == 0 with rows present: in some replicates and not in others
    assert 5 <= zero_out.sum() <= R.REPS - 5


def test_offset_panel():
    p, m = R.panel("offset", True), R.panel("main", True)
    assert np.array_equal(p.row_cell, m.row_cell)
    for g in (0, 1):
        assert np.array_equal(p.y[g], m.y[g] + 2.0 ** 20) and np.all(p.y[g] > 2.0 ** 20)
        k = np.round(p.w[g] * 7.0)
        assert np.array_equal(p.w[g], k / 7.0) and k.min() >= 1 and k.max() <= 16
        assert np.any(p.w[g] * 8.0 != np.round(p.w[g] * 8.0))  # not dyadic: sums of c w round
    assert 4e-7 < p.tol < 6e-7
    q = R.panel("offset", False)
    assert np.all(q.w[0] == 1.0) and np.array_equal(q.y[1], p.y[1])


def test_singletons_panel():
    p = R.panel("singletons", True)
    assert p.n == [65, 321] and p.n_cells == 353 >= 321
    for g in (0, 1):
        assert np.array_equal(np.bincount(p.cell[g], minlength=p.n_cells).max(), 1)  # every row its own cell
        assert len(R.fragments(p.cell[g], [(0, 1), (1, 2)][:1 + g])) == p.n[g]  # a fragment per row
    in_a, in_b = np.isin(np.arange(p.n_cells), p.cell[0]), np.isin(np.arange(p.n_cells), p.cell[1])
    assert (in_a & in_b).sum() == 33 and (in_a & ~in_b).sum() == 32 and (~in_a & in_b).sum() == 288
    shared = np.flatnonzero(in_a & in_b)  # the keys interleave: shared cells and cells of one group alternate
    assert np.all(np.diff(shared) > 1) and in_a[shared[3] + 1:shared[4]].any() and in_b[shared[3] + 1:shared[4]].any()


@pytest.mark.parametrize("name", list(R.EDGE_NAMES))
def test_edges_panels(O, name):
    n_a, n_b = R.EDGE_NAMES[name]
    p = R.panel(name, True)
    assert p.n == [n_a, n_b]
    ends = set((np.flatnonzero(np.diff(p.cell[1])) + 1).tolist()) | {n_b}  # the rows after which a run of B ends
    assert {r for r in (64, 256, 512) if r <= n_b} <= ends
    if n_a == 1:  # A's single row: drawn exactly once in every replicate, w = 1/2
        assert p.w[0][0] == 0.5 and all(p.counts(O, r, 0).tolist() == [1] for r in range(R.REPS))
    point, okp, rows, ok, sup = R.boot_exact(O, name, True)
    assert okp and ok.all() and point[4] != 0.0


def test_long_group_premise():
    """The 33,025-row group: the chunk table restated from group_chunks has what the GPU test is there for, and
    every product c (w y) and every cell's sum is exact in f64, so math.fsum is the exact reference."""
    gr = R.long_group()
    T = R.TILE
    assert gr.n == 33025 and len(gr.chunks) == 128 and gr.chunks[-1][1] == 130
    two = [c for c in gr.chunks if c[1] - c[0] == 2]
    assert two == [(63, 65), (128, 130)] and all(c[1] - c[0] in (1, 2) for c in gr.chunks)
    assert gr.cell[64 * T - 1] == gr.cell[64 * T]  # a cell across the tile boundary inside chunk 63
    assert gr.cell[129 * T - 1] != gr.cell[129 * T] and gr.cell[129 * T - 2] == gr.cell[129 * T - 1]  # one ends on it
    assert gr.n - 1 == 129 * T and gr.cell[-1] == gr.n_cells - 1 and (gr.cell == gr.cell[-1]).sum() == 1
    assert np.all(np.diff(gr.cell) >= 0) and set(np.diff(gr.cell).tolist()) == {0, 1}
    c = gr.counts
    assert set(np.unique(c).tolist()) == {0, 1, 2, 3, 255} and (c == 255).sum() >= 300
    assert not c[3, 64 * T:65 * T].any() and c[3, 63 * T:64 * T].any() and not c[5, 63 * T:64 * T].any()
    assert not c[7, 128 * T:129 * T].any() and not c[64, 17 * T:18 * T].any() and c[9, -1] == 0 and c[11, -1] == 255
    # the bit budget, from the arrays: 8 w and 2^20 y are integers, so 2^23 c w y is one; f64 holds it and its sums
    w8, y20 = gr.w * 8.0, gr.y * 2.0 ** 20
    assert np.array_equal(w8, np.round(w8)) and w8.min() == 0 and w8.max() == 16
    assert np.array_equal(y20, np.round(y20)) and np.abs(gr.y).max() < 32.0
    exact = c.astype(np.int64) * (w8.astype(np.int64) * y20.astype(np.int64))[None, :]  # 2^23 c w y, exactly
    prod = c.astype(np.float64) * (gr.w * gr.y)[None, :]
    assert np.array_equal(prod * 2.0 ** 23, exact.astype(np.float64)) and np.abs(exact).max() < 2 ** 38
    longest = np.bincount(gr.cell).max()
    assert longest * 2 ** 38 < 2 ** 53  # every partial sum of a cell, in any order, is an integer below 2^53 / 2^23
    # and on a few cells the Fraction sum itself
    n_fs, s_fs = R.long_sums(gr, c[11])
    rows = np.flatnonzero(np.isin(gr.cell, [0, 5, gr.cell[64 * T], gr.n_cells - 1]))
    n_fr, s_fr = R.sums_exact(gr.y[rows], gr.w[rows], gr.cell[rows], gr.n_cells, c[11][rows])
    for x in (0, 5, int(gr.cell[64 * T]), gr.n_cells - 1):
        assert n_fs[x] == n_fr[x] and s_fs[x] == s_fr[x]


def test_byte_group_property():
    gr = R.byte_group()
    assert gr.n == 257 and gr.counts.shape == (131, 257) and gr.chunks == [(0, 1), (1, 2)]
    for j in range(4):  # every byte value in every byte lane of a count word
        assert set(np.unique(gr.counts[:, j::4]).tolist()) == set(range(256)), j
    words = gr.counts[:, :256].reshape(131, 64, 4)
    assert (words.min(axis=2) >= 128).sum() >= 100  # words whose four bytes all have the high bit
    assert any(f[0] == 9 and f[2] == 257 for f in R.fragments(gr.cell, gr.chunks))  # cell 9 across the chunk boundary


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
