"""Nopo's matching decomposition on the GPU (csrc/ob_nopo.hip) against the numpy restatement
tests/nopo_ref.py: the cell pass alone, the point pass and 64 + 3 replicates row for row, weighted and unweighted,
bitwise determinism, and the builder end to end.

The main panel has groups of 130 and 257 rows (a ragged last sub-tile, more than one tile, B in two chunks and A in
one) with cells across a sub-tile boundary and across the chunk boundary, one-row cells and cells of one group only
(nopo_ref.MAIN_CELLS); the tiny panel of 3 and 4 rows has a single shared cell holding one row of A, so a third of
its replicates have an empty support (ok = 0).

Tolerance (derived): every quantity is a ratio or difference of ordered f64 sums of at most n terms, and both sides
carry that error: |got - want| <= 16 n_max 2^-53 max|y| (Panel.tol). The matched shares and the support-cell count
are compared with ==: the panels' weights are multiples of 1/8, so every N is exact in f64 in any order."""
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


@pytest.mark.parametrize("name,weighted", [("main", True), ("tiny", False)], ids=["main_weighted", "tiny"])
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
