"""Nopo's matching decomposition on the GPU (csrc/ob_nopo.hip) against the numpy restatement
tests/nopo_ref.py: the cell pass alone, the point pass and 64 + 3 replicates row for row, weighted and unweighted,
bitwise determinism, and the builder end to end.

The main panel has groups of 130 and 257 rows (a ragged last sub-tile, more than one tile, B in two chunks and A in
one) with cells across a sub-tile boundary and across the chunk boundary, one-row cells and cells of one group only
(nopo_ref.MAIN_CELLS); the tiny panel of 3 and 4 rows has a single shared cell holding one row of A, so a third of
its replicates have an empty support (ok = 0).

Tolerance (derived): every quantity is a ratio or difference of ordered f64 sums of at most n terms, and both sides
carry that error: |got - want| <= 16 n_max 2^-53 max|y| (Panel.tol). The matched shares and the support-cell count
are compared with ==: the panels' weights are multiples of 1/8, so every N is exact in f64 in any order.

Beside the restatement, which adds the same f64 terms in the same order and so shares the device's error, stands an
exact reference (nopo_ref.sums_exact, terms_exact, long_sums): test_cell_pass_long_chunks (chunks of two tiles),
test_cell_pass_counts_and_batches (every count byte in every lane, three batches, unused cell ids) and
test_rows_match_exact (zero weights, an offset of 2^20 with weights k / 7, a cell per row, groups of exactly 1, 64,
256 and 512 rows). Their bounds are the device's alone: per cell (m + f) 2^-53 times the absolute sum for the cell
pass (nopo_ref.sum_bounds), Panel.tol for the rows. test_nopo_host.py proves each panel's property without a GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nopo_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [("main", False), ("main", True), ("tiny", False), ("tiny", True)]
IDS = ["main", "main_weighted", "tiny", "tiny_weighted"]
EXACT = [10, 11, 12]  # the matched shares and the support-cell count


def check_rows(p, got, ok, want, want_ok, what):
    """Every row against the restatement's: the ok flags equal, NaN rows as NaN, no replicate left out."""
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    assert np.array_equal(np.atleast_1d(ok).astype(bool), np.atleast_1d(want_ok).astype(bool)), what
    worst = 0.0
    for r in range(len(want)):
        if not np.atleast_1d(want_ok)[r]:
            assert np.isnan(got[r]).all() and np.isnan(want[r]).all(), (what, r)
            continue
        worst = max(worst, np.abs(got[r] - want[r]).max())
        assert np.all(np.abs(got[r] - want[r]) <= p.tol), (what, r, got[r] - want[r])
        assert np.array_equal(got[r][EXACT], want[r][EXACT]), (what, r)
    print(f"{what}: largest deviation {worst:.3e} (bound {p.tol:.3e})")


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_cell_pass_alone(ob, O, weighted):
    p = R.panel("main", weighted)
    for g in (0, 1):
        w = p.w[g] if weighted else None
        counts = np.stack([p.counts(O, r, g) for r in range(R.REPS)])
        for c in (None, counts):
            n_got, s_got = ob.nopo_sums(p.y[g], p.cell[g], p.n_cells, w=w, counts=c)
            reps = 1 if c is None else len(c)
            assert n_got.shape == s_got.shape == (reps, p.n_cells)
            for r in range(reps):
                n_want, s_want = R.sums(p.y[g], p.w[g], p.cell[g], p.n_cells, None if c is None else c[r])
                assert np.array_equal(n_got[r], n_want), (g, r)  # integers (unweighted) or multiples of 1/8: exact
                if not weighted:
                    assert np.all(n_got[r] == np.round(n_got[r]))
                assert np.all(np.abs(s_got[r] - s_want) <= p.tol), (g, r)
    t = ob.nopo_last_timing()
    assert t["cell_ms"] > 0.0 and t["row_ms"] >= 0.0


def stack(pairs):
    """[(N, S) per replicate] -> [N [reps][cells], S [reps][cells]]."""
    return [np.stack(v) for v in zip(*pairs)]


def check_sums(gr, got, want, want_abs, what):
    """N and S of ob.nopo_sums ([reps][cells]) against the exact sums, per cell within nopo_ref.sum_bounds; want_abs:
    the exact sums with |y| for y. Prints the worst deviation and the bound of that cell."""
    bounds = R.sum_bounds(gr.cell, gr.n_cells, gr.chunks, *want_abs)
    line = []
    for i in (0, 1):
        assert got[i].shape == want[i].shape == bounds[i].shape, what
        dev = np.abs(got[i] - want[i])
        r, x = np.unravel_index(np.argmax(dev), dev.shape)
        line.append(f"{'NS'[i]} {dev[r, x]:.3e} (bound there {bounds[i][r, x]:.3e})")
        bad = np.argwhere(dev > bounds[i])
        assert len(bad) == 0, (what, "NS"[i], bad[:4], dev[tuple(bad[0])], bounds[i][tuple(bad[0])])
    print(f"{what}: largest deviation {', '.join(line)}")


def test_cell_pass_long_chunks(ob):
    """One group of 33,025 rows: 130 tiles in 128 chunks, so chunks 63 and 127 hold two tiles and the kernel steps
    from a chunk's first tile to its second with the next image prefetched across the step. Against math.fsum of
    exact products (test_nopo_host.py::test_long_group_premise); bound per cell (nopo_ref.sum_bounds)."""
    gr = R.long_group()
    T = R.TILE
    # restated from group_chunks (t0 = tiles * c // nc), before any device call
    tiles = (gr.n + T - 1) // T
    chunks = [(tiles * c // 128, tiles * (c + 1) // 128) for c in range(128)]
    assert tiles == 130 and chunks == gr.chunks
    two = [(t0, t1) for t0, t1 in chunks if t1 - t0 == 2]
    assert two == [(63, 65), (128, 130)]  # at least one chunk holds two tiles
    b0, b1 = (two[0][0] + 1) * T, (two[1][0] + 1) * T  # the tile boundaries inside them
    assert gr.cell[b0 - 1] == gr.cell[b0]  # one cell spans the first
    assert gr.cell[b1 - 1] != gr.cell[b1] and gr.cell[b1 - 2] == gr.cell[b1 - 1]  # another ends exactly on the second
    assert b1 == gr.n - 1 and (gr.cell == gr.cell[-1]).sum() == 1  # the last row, alone in its tile, is its own cell
    assert not gr.counts[3, b0:b0 + T].any()  # a replicate whose second tile of a two-tile chunk is all zeros
    for c in (None, gr.counts):
        got = ob.nopo_sums(gr.y, gr.cell, gr.n_cells, w=gr.w, counts=c)
        reps = 1 if c is None else len(c)
        assert got[0].shape == got[1].shape == (reps, gr.n_cells)
        want = stack(R.long_sums(gr, None if c is None else c[r]) for r in range(reps))
        want_abs = stack(R.long_sums(gr, None if c is None else c[r], absolute=True) for r in range(reps))
        check_sums(gr, got, want, want_abs, f"long chunks, {'point' if c is None else '65 replicates'}")
        # every product and every partial sum of a cell is exact in f64 (the host test proves it from the arrays), so
        # no order of the sum rounds at all
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_cell_pass_counts_and_batches(ob, N):
    """257 rows, 131 replicates whose counts hold every byte value in every byte lane of a count word, against
    sums_exact; in one batch and in three (hk_batch = 1, the last ragged), bitwise equal; and with unused cell ids
    between the used ones and past the highest."""
    gr = R.byte_group()
    want = stack(R.sums_exact(gr.y, gr.w, gr.cell, gr.n_cells, c) for c in gr.counts)
    want_abs = stack(R.sums_exact(np.abs(gr.y), gr.w, gr.cell, gr.n_cells, c) for c in gr.counts)
    got = ob.nopo_sums(gr.y, gr.cell, gr.n_cells, w=gr.w, counts=gr.counts)
    check_sums(gr, got, want, want_abs, "bytes, one batch")
    assert np.array_equal(got[0], want[0])  # dyadic weights: N is exact in any order
    with N.option("hk_batch", 1):
        forced = ob.nopo_sums(gr.y, gr.cell, gr.n_cells, w=gr.w, counts=gr.counts)
    check_sums(gr, forced, want, want_abs, "bytes, three batches")
    assert forced[0].tobytes() == got[0].tobytes() and forced[1].tobytes() == got[1].tobytes()
    # ids 3 x + 2 of 3 n_cells + 5: unused ids before, between and past the used ones
    wide, n_wide = 3 * gr.cell + 2, 3 * gr.n_cells + 5
    used = np.zeros(n_wide, dtype=bool)
    used[3 * np.arange(gr.n_cells) + 2] = True
    for batch in (None, 1):  # the default batch, and three
        with N.option("hk_batch", batch):
            spread = ob.nopo_sums(gr.y, wide, n_wide, w=gr.w, counts=gr.counts)
        for i in (0, 1):
            assert spread[i].shape == (len(gr.counts), n_wide)
            assert spread[i][:, used].tobytes() == got[i].tobytes(), (batch, i)
            assert np.all(spread[i][:, ~used] == 0.0) and not np.signbit(spread[i][:, ~used]).any(), (batch, i)


def chunk_table(N, pr):
    table = (C.c_uint32 * 96)()
    n = C.c_int32()
    N.check(N.lib().ob_debug_chunks(N.lib().ob_prepared_panel(pr._h), table, 32, C.byref(n)))
    return [tuple(table[3 * i:3 * i + 3]) for i in range(n.value)]


EXACT_CASES = [("main", False), ("main", True), ("zero_w", True), ("offset", False), ("offset", True),
               ("singletons", False), ("singletons", True)] + [(e, wt) for e in R.EDGE_NAMES for wt in (False, True)]


@pytest.mark.parametrize("name,weighted", EXACT_CASES, ids=[f"{n}{'_weighted' if wt else ''}" for n, wt in EXACT_CASES])
def test_rows_match_exact(ob, O, N, name, weighted):
    """The point row and 67 replicates against the Fraction reference (nopo_ref.terms_exact): the reference is exact,
    so Panel.tol bounds the device alone. Unweighted zero_w is unweighted main."""
    p = R.panel(name, weighted)
    point, okp, rows, ok, sup = R.boot_exact(O, name, weighted)
    assert okp and ok.all()
    dyadic = not (name == "offset" and weighted)
    with p.builder(ob).prepare_nopo() as pr:
        got_point = pr.point_row()
        got, got_ok = pr.boot(0, R.REPS)
        info = pr.nopo_info()
        chunks = chunk_table(N, pr)
    for what, g, gok, w, wok in (("point", got_point, 1, point, okp), ("replicates", got, got_ok, rows, ok)):
        g, w = np.atleast_2d(g), np.atleast_2d(w)
        assert np.array_equal(np.atleast_1d(gok).astype(bool), np.atleast_1d(wok).astype(bool)), what
        dev = np.abs(g - w)
        print(f"{name} weighted={weighted} {what}: largest deviation {dev.max():.3e} (bound {p.tol:.3e})")
        assert np.all(dev <= p.tol), (what, np.argwhere(dev > p.tol)[:4])
        assert np.array_equal(g[:, 12], w[:, 12]), what  # the support-cell count
        if dyadic:
            assert np.array_equal(g[:, [10, 11]], w[:, [10, 11]]), what  # the matched shares: every N is exact
    assert np.array_equal(info["in_support"], sup[-1]) and info["n_support_cells"] == int(point[12])
    if name not in R.EDGE_NAMES:  # (the edges' cells are large) the support is decided again in the replicates
        assert any(not np.array_equal(s, sup[-1]) for s in sup[:-1])
    if name == "zero_w":
        (na, _), (nb, _) = p.fractions()
        by_weight = np.array([a > 0 and b > 0 for a, b in zip(na, nb)])
        assert np.array_equal(info["in_support"].astype(bool), by_weight)
        x = R.ZERO_A_CELL  # rows, but no weight and no mean
        assert np.isnan(info["mean_a"][x]) and info["w_a"][x] == 0.0 and info["n_cell_a"][x] == 20
        assert not info["in_support"][x] and info["w_b"][x] > 0.0 and np.isfinite(info["mean_b"][x])
        assert got_point[3] == 0.0 and not np.signbit(got_point[3])  # N_A^out == 0.0 with rows present
        zero = rows[:, 3] == 0.0
        assert zero.any() and np.array_equal(got[:, 3] == 0.0, zero)
    if name in R.EDGE_NAMES:
        n_a, n_b = R.EDGE_NAMES[name]
        ends = set((np.flatnonzero(np.diff(p.cell[1])) + 1).tolist()) | {n_b}
        b_chunks = [c for c in chunks if c[0] == 1]
        assert {c[2] * R.TILE for c in b_chunks if c[2] * R.TILE <= n_b} <= ends  # a fragment ends on each boundary
        assert len(b_chunks) == (n_b + R.TILE - 1) // R.TILE and (n_b < 512 or (1, 0, 1) in b_chunks)
        if n_a == 1:  # A's single row is drawn once in every replicate: ybar_A is its y, exactly
            assert got_point[5] == p.y[0][0] and np.all(got[:, 5] == p.y[0][0])


@pytest.mark.parametrize("name,weighted", CASES, ids=IDS)
def test_rows_match_ref(ob, O, name, weighted):
    p = R.panel(name, weighted)
    point, okp, rows, ok, sup = R.boot(O, name, weighted)
    # on the CPU, before any GPU call: the replicates exercise what they are here for
    assert okp
    (na, _), (nb, _) = p.cell_sums()
    point_sup = (na > 0) & (nb > 0)
    if name == "main":
        assert ok.all() and any(not np.array_equal(s, point_sup) for s in sup)
    else:
        assert (ok == 0).any() and (ok == 1).any()
    with p.builder(ob).prepare_nopo() as pr:
        assert pr.row_len == R.ROW_LEN
        got_point = pr.point_row()
        got, got_ok = pr.boot(0, R.REPS)
        info = pr.nopo_info()
    check_rows(p, got_point, 1, point, okp, f"{name} weighted={weighted} point")
    check_rows(p, got, got_ok, rows, ok, f"{name} weighted={weighted} replicates")
    assert np.array_equal(info["in_support"], point_sup) and info["n_support_cells"] == int(point[12])
    if name == "tiny":  # all of B lies in the support: D_B is exactly 0.0, its share exactly 1
        keep = got_ok.astype(bool)
        assert got_point[4] == 0.0 and np.all(got[keep, 4] == 0.0) and np.all(got[keep, 11] == 1.0)


@pytest.mark.parametrize("name,weighted", [("main", True), ("tiny", False), ("zero_w", True), ("singletons", True)],
                         ids=["main_weighted", "tiny", "zero_w", "singletons"])
def test_bitwise_properties(ob, N, name, weighted):
    p = R.panel(name, weighted)
    with p.builder(ob).prepare_nopo() as pr:
        rows, ok = pr.boot(0, R.REPS)
        again, ok2 = pr.boot(0, R.REPS)
        assert rows.tobytes() == again.tobytes() and ok.tobytes() == ok2.tobytes()  # a repeated call
        for r in (0, 5, 63, 64, 66):  # alone
            one, ok1 = pr.boot(r, 1)
            assert one[0].tobytes() == rows[r].tobytes() and ok1[0] == ok[r], r
        part, okp = pr.boot(5, 62)  # another first_rep: the replicates sit in other lanes and blocks
        assert part.tobytes() == rows[5:67].tobytes() and okp.tobytes() == ok[5:67].tobytes()
        with N.option("hk_batch", 1):  # one-block batches
            forced, okf = pr.boot(0, R.REPS)
        assert forced.tobytes() == rows.tobytes() and okf.tobytes() == ok.tobytes()
    with p.builder(ob).prepare_nopo() as pr2:  # another handle
        other, _ = pr2.boot(0, R.REPS)
    assert other.tobytes() == rows.tobytes()


def test_handle_refusals(ob, N):
    p = R.panel("main", False)
    with p.builder(ob).prepare_nopo() as pr:
        rows, ok = pr.boot(0, 8)
        for fn in (lambda: pr.boot_sharded(0, 8), pr.jackknife, lambda: pr.finish_bca(rows, ok)):
            with pytest.raises(N.OaxacaError) as e:
                fn()
            assert e.value.code == N.OB_E_UNSUPPORTED


@pytest.mark.parametrize("name,weighted", [("main", True), ("tiny", False)], ids=["main_weighted", "tiny"])
def test_decompose_end_to_end(ob, O, name, weighted):
    p = R.panel(name, weighted)
    with p.builder(ob).prepare_nopo() as pr:
        point = pr.point_row()
        rows, ok = pr.boot(0, R.REPS)
    res = p.builder(ob).decompose_nopo(relative=True)
    want = R.aggregate(O, point, rows, ok)
    assert res.n_failed == int(len(ok) - ok.sum()) and (res.n_a, res.n_b) == tuple(p.n)
    for cname, w in zip(R.COMPONENTS, want):
        c = res.components[cname]
        assert c.estimate == w[0], cname
        for got, exp in ((c.std_err, w[1]), (c.ci_lower, w[2]), (c.ci_upper, w[3])):
            assert abs(got - exp) <= 1e-12 * max(abs(exp), 1.0), (cname, got, exp)
    # the cells and every row's cell are the restatement's
    assert res.n_cells == p.n_cells and np.array_equal(res.row_cell, p.row_cell)
    assert res.n_support_cells == int(point[12])
    (na, sa), (nb, sb) = p.cell_sums()
    assert [c["key"] for c in res.cells] == [(float(x), s) for x, s in p.keys]
    for x, c in enumerate(res.cells):
        assert (c["n_a"], c["n_b"]) == (int((p.cell[0] == x).sum()), int((p.cell[1] == x).sum()))
        assert c["in_support"] == bool(na[x] > 0 and nb[x] > 0)
        for got, n, s in ((c["mean_a"], na[x], sa[x]), (c["mean_b"], nb[x], sb[x])):
            assert np.isnan(got) if n == 0 else abs(got - s / n) <= p.tol
    # relative: each term over ybar_B, per replicate
    keep = rows[ok.astype(bool)]
    for i, cname in enumerate(R.COMPONENTS[:5]):
        c = res.relative[cname]
        se, _, (lo, hi) = O.bootstrap_stats(keep[:, i] / keep[:, 6])
        assert c.estimate == point[i] / point[6]
        for got, exp in ((c.std_err, se), (c.ci_lower, lo), (c.ci_upper, hi)):
            assert abs(got - exp) <= 1e-12 * max(abs(exp), 1.0), (cname, got, exp)
    assert not p.builder(ob).decompose_nopo().relative


def test_bins_end_to_end(ob):
    """bins coarsens a numeric column on the host: the decomposition is that of the digitized frame."""
    p = R.panel("main", False)
    edges = [0.5, 2.5]
    binned = dict(p.frame)
    binned["x"] = np.digitize(np.array(p.frame["x"]), edges).tolist()
    a = p.builder(ob, reps=8).decompose_nopo(bins={"x": edges})
    b = ob.OaxacaBuilder(binned, "y", "g", "B").predictors(["x"]).categorical_predictors(["s"]).bootstrap_reps(8)
    b = b.seed(R.SEED).decompose_nopo()
    assert a.n_cells == b.n_cells < p.n_cells and np.array_equal(a.row_cell, b.row_cell)
    for name in R.COMPONENTS:
        assert a.components[name].__dict__ == b.components[name].__dict__
