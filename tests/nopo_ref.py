"""numpy f64 restatement of Nopo's matching decomposition of include/oaxaca_boot.h: the cells by
numpy.unique over the key tuples, the per-cell sums by numpy.bincount with weights over the oracle's OBRS-3 counts,
the terms exactly as the header defines them. Shared by test_nopo_host.py and test_gpu_nopo.py.

Beside it stands an exact reference, which shares no rounding with the device: sums_exact and terms_exact work in
fractions.Fraction on the f64 inputs (the product w y rounded to f64 first, as the host does before the upload) and
round once at the end; the 33,025-row group (long_group) has products and sums that are exact in f64, so math.fsum
is its exact sum."""
import math
from fractions import Fraction

import numpy as np

# Both panels, weighted and unweighted, were checked on the CPU (test_gpu_nopo.py asserts it before any GPU call):
# with this seed replicates 0 .. 66 of the main panel hold supports that differ from the point pass's, and those of
# the tiny panel hold both ok = 0 and ok = 1 replicates. With a one-row cell either holds for about a third of the
# replicates, so nearly any seed does.
SEED = 0x0B5EED
REPS = 64 + 3  # a ragged replicate batch
ROW_LEN = 13
TILE = 256  # OB_TILE_ROWS: rows of a tile, four 64-row sub-tiles
COMPONENTS = ("total_gap", "composition", "unexplained", "unmatched_a", "unmatched_b", "matched_share_a",
              "matched_share_b")
COLUMNS = (0, 1, 2, 3, 4, 10, 11)  # their row entries


def cells(keycols):
    """Key columns (numeric arrays match on value, -0.0 = 0.0; string columns on their bytes) -> (id per row, number
    of cells, the key tuples in id order): ids number the distinct tuples in lexicographic order."""
    codes, levels = [], []
    for col in keycols:
        a = np.asarray(col)
        if a.dtype.kind in "USO":
            a = np.array([v.encode() if isinstance(v, str) else v for v in a.tolist()], dtype=bytes)
        lv, inv = np.unique(a, return_inverse=True)
        codes.append(inv.reshape(-1))
        levels.append(lv)
    tuples, ids = np.unique(np.column_stack(codes), axis=0, return_inverse=True)
    keys = [tuple(lv[c].decode() if isinstance(lv[c], bytes) else lv[c].item() for lv, c in zip(levels, t))
            for t in tuples]
    return ids.reshape(-1).astype(np.int32), len(tuples), keys


def sort_group(cell):
    """Sorted position -> row of the group: stable ascending order of cell id (the OBRS-3 row order)."""
    return np.argsort(cell, kind="stable")


def sums(y, w, cell, n_cells, c=None):
    """N(x) = sum c w and S(x) = sum c (w y) over rows in ascending order of cell."""
    c = np.ones(len(y)) if c is None else np.asarray(c, dtype=np.float64)
    return (np.bincount(cell, weights=c * w, minlength=n_cells), np.bincount(cell, weights=c * (w * y), minlength=n_cells))


def terms(na, sa, nb, sb):
    """Per-cell sums of A and B -> (row, ok): the header's aggregates and terms; a NaN row and ok = 0 for an empty
    support or a group without weight."""
    sup = (na > 0) & (nb > 0)
    NA, SA, NB, SB = na.sum(), sa.sum(), nb.sum(), sb.sum()
    if not sup.any() or not NA > 0 or not NB > 0:
        return np.full(ROW_LEN, np.nan), 0
    NAs, SAs, NBs, SBs = na[sup].sum(), sa[sup].sum(), nb[sup].sum(), sb[sup].sum()
    NAo, SAo, NBo, SBo = na[~sup].sum(), sa[~sup].sum(), nb[~sup].sum(), sb[~sup].sum()
    cf = np.sum(nb[sup] * (sa[sup] / na[sup])) / NBs
    eas, ebs = SAs / NAs, SBs / NBs
    da = 0.0 if NAo == 0 else (NAo / NA) * (SAo / NAo - eas)
    db = 0.0 if NBo == 0 else (NBo / NB) * (ebs - SBo / NBo)
    return np.array([SA / NA - SB / NB, eas - cf, cf - ebs, da, db, SA / NA, SB / NB, eas, ebs, cf, NAs / NA, NBs / NB,
                     float(sup.sum())]), 1


def sums_fractions(y, w, cell, n_cells, c=None):
    """Per-cell N = sum c w and S = sum c fl(w y) as lists of Fractions: no rounding but that of the product w y."""
    wy = np.asarray(w, dtype=np.float64) * np.asarray(y, dtype=np.float64)  # one f64 rounding, as upload_wy's
    c = [1] * len(wy) if c is None else [int(v) for v in c]
    n, s = [Fraction(0)] * n_cells, [Fraction(0)] * n_cells
    for ci, wi, ti, x in zip(c, np.asarray(w, dtype=np.float64).tolist(), wy.tolist(), np.asarray(cell).tolist()):
        if ci:
            n[x] += ci * Fraction(wi)
            s[x] += ci * Fraction(ti)
    return n, s


def sums_exact(y, w, cell, n_cells, c=None):
    """sums_fractions, each sum rounded to f64 once."""
    n, s = sums_fractions(y, w, cell, n_cells, c)
    return np.array([float(v) for v in n]), np.array([float(v) for v in s])


def terms_exact(na, sa, nb, sb):
    """terms on exact per-cell sums (lists of Fractions), every aggregate and term in Fraction arithmetic, the row
    rounded to f64 once: the same support rule and the same ok rule."""
    sup = [a > 0 and b > 0 for a, b in zip(na, nb)]
    NA, SA, NB, SB = sum(na), sum(sa), sum(nb), sum(sb)
    if not any(sup) or not NA > 0 or not NB > 0:
        return np.full(ROW_LEN, np.nan), 0
    inside = [x for x, k in enumerate(sup) if k]
    NAs, SAs, NBs, SBs = (sum(v[x] for x in inside) for v in (na, sa, nb, sb))
    NAo, SAo, NBo, SBo = NA - NAs, SA - SAs, NB - NBs, SB - SBs  # exact: the sums over the other cells
    cf = sum(nb[x] * (sa[x] / na[x]) for x in inside) / NBs
    eas, ebs = SAs / NAs, SBs / NBs
    da = Fraction(0) if NAo == 0 else (NAo / NA) * (SAo / NAo - eas)
    db = Fraction(0) if NBo == 0 else (NBo / NB) * (ebs - SBo / NBo)
    row = [SA / NA - SB / NB, eas - cf, cf - ebs, da, db, SA / NA, SB / NB, eas, ebs, cf, NAs / NA, NBs / NB,
           Fraction(len(inside))]
    return np.array([float(v) for v in row]), 1


def group_chunks(tiles, max_chunks=128):
    """ob::group_chunks of one group: [(t0, t1)] with t0 = tiles * c // nc over nc = min(tiles, max_chunks) chunks."""
    nc = min(tiles, max_chunks)
    return [(tiles * c // nc, tiles * (c + 1) // nc) for c in range(nc)]


def fragments(cell, chunks):
    """The fragments (a cell's rows within one chunk) of a sorted group under the chunk table [(t0, t1)], as
    ob::nopo_fragments cuts them: [(cell, first row, end row)] in row order."""
    cell, n, out = np.asarray(cell), len(cell), []
    for t0, t1 in chunks:
        r0, r1 = t0 * TILE, min(t1 * TILE, n)
        cuts = [r0] + [i for i in range(r0 + 1, r1) if cell[i] != cell[i - 1]] + [r1]
        out += [(int(cell[a]), a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    return out


def sum_bounds(cell, n_cells, chunks, abs_n, abs_s):
    """The cell pass's derived bounds against the exact sums: a fragment is a serial sum of rounded products, a cell
    adds a fragment per chunk, so |N - N*| <= (m + f) 2^-53 sum c w and |S - S*| <= (m + f) 2^-53 sum c |w y| with m
    the cell's rows and f its fragments. abs_n, abs_s: the exact sums with |y| for y ([reps][n_cells]; w is not
    negative)."""
    m = np.bincount(cell, minlength=n_cells)
    f = np.bincount([x for x, _, _ in fragments(cell, chunks)], minlength=n_cells)
    return (m + f) * 2.0 ** -53 * abs_n, (m + f) * 2.0 ** -53 * abs_s


class Panel:
    """A frame with its restatement: cells, each group's sorted rows, y and w in the sorted order."""

    def __init__(self, frame, predictors, categorical, weighted):
        self.frame, self.predictors, self.categorical, self.weighted = frame, list(predictors), list(categorical), weighted
        g = np.array(frame["g"])
        used = np.flatnonzero((g == "A") | (g == "B"))
        ids, self.n_cells, self.keys = cells([np.asarray(frame[c])[used] for c in (*predictors, *categorical)])
        self.row_cell = np.full(len(g), -1, dtype=np.int32)
        self.row_cell[used] = ids
        y, w = np.asarray(frame["y"], dtype=np.float64), np.asarray(frame["w"], dtype=np.float64)
        self.rows, self.cell, self.y, self.w = [], [], [], []
        for name in ("A", "B"):
            rows = np.flatnonzero(g == name)
            rows = rows[sort_group(self.row_cell[rows])]
            self.rows.append(rows)
            self.cell.append(self.row_cell[rows])
            self.y.append(y[rows])
            self.w.append(w[rows] if weighted else np.ones(len(rows)))
        self.n = [len(r) for r in self.rows]
        self.tol = 16 * max(self.n) * 2.0 ** -53 * np.abs(y).max()  # the issue's bound, for this panel's shape

    def builder(self, ob, reps=REPS):
        b = ob.OaxacaBuilder(self.frame, "y", "g", "B").predictors(self.predictors)
        b = b.categorical_predictors(self.categorical).bootstrap_reps(reps).seed(SEED)
        return b.weights("w") if self.weighted else b

    def cell_sums(self, counts=(None, None)):
        return [sums(self.y[g], self.w[g], self.cell[g], self.n_cells, counts[g]) for g in (0, 1)]

    def point(self):
        (na, sa), (nb, sb) = self.cell_sums()
        return terms(na, sa, nb, sb)

    def counts(self, O, rep, g):
        return np.bincount(O.resample_indices(SEED, rep, g, self.n[g]), minlength=self.n[g])

    def boot(self, O, first_rep, n_reps):
        """Replicates first_rep .. -> (rows, ok, support flags per replicate and cell)."""
        rows, ok = np.full((n_reps, ROW_LEN), np.nan), np.zeros(n_reps, dtype=np.uint8)
        sup = np.zeros((n_reps, self.n_cells), dtype=bool)
        for r in range(n_reps):
            (na, sa), (nb, sb) = self.cell_sums([self.counts(O, first_rep + r, g) for g in (0, 1)])
            rows[r], ok[r] = terms(na, sa, nb, sb)
            sup[r] = (na > 0) & (nb > 0)
        return rows, ok, sup

    def fractions(self, counts=(None, None)):
        """Both groups' exact per-cell sums: [(N, S) of A, (N, S) of B], lists of Fractions."""
        return [sums_fractions(self.y[g], self.w[g], self.cell[g], self.n_cells, counts[g]) for g in (0, 1)]

    def boot_exact(self, O, n_reps):
        """The exact reference's point row and replicates 0 .. -> (point, its ok, rows, ok, support flags, with the
        point pass's as entry n_reps)."""
        rows, ok = np.full((n_reps, ROW_LEN), np.nan), np.zeros(n_reps, dtype=np.uint8)
        sup = np.zeros((n_reps + 1, self.n_cells), dtype=bool)
        for r in range(n_reps + 1):
            point = r == n_reps
            (na, sa), (nb, sb) = self.fractions([None if point else self.counts(O, r, g) for g in (0, 1)])
            sup[r] = [a > 0 and b > 0 for a, b in zip(na, nb)]
            if point:
                prow, pok = terms_exact(na, sa, nb, sb)
            else:
                rows[r], ok[r] = terms_exact(na, sa, nb, sb)
        return prow, pok, rows, ok, sup


# The main panel, per cell in key order: (x, s, rows of A, rows of B). Groups of 130 and 257 rows (the binary tests'
# shape: a ragged last sub-tile, more than one tile, B in two chunks of one tile each and A in one). In B's sorted
# order cell 3 holds rows 2 .. 71, cell 5 rows 72 .. 171 and cell 7 rows 178 .. 247 (each across a 64-row sub-tile
# boundary) and cell 9 rows 249 .. 256 (across the chunk boundary at row 256). Cells 0, 4 and 10 exist in A only, 1
# and 6 in B only; 2 and 8 hold one row of each group, 0 and 10 one row of A, 1 one row of B. Cell 2's key is -0.0
# in A's row and 0.0 in B's.
MAIN_CELLS = ((-2.0, "p", 1, 0), (-1.0, "p", 0, 1), (0.0, "p", 1, 1), (0.0, "q", 20, 70), (1.0, "p", 5, 0),
              (1.5, "p", 40, 100), (2.0, "p", 0, 6), (2.0, "q", 30, 70), (3.0, "p", 1, 1), (3.5, "q", 31, 8),
              (4.0, "p", 1, 0))
# The tiny panel: 3 rows of A, 4 of B; the single shared cell holds one row of A, so a replicate that does not draw
# it has an empty support. All of B lies in the support: D_B is exactly 0.0.
TINY_CELLS = ((1.0, "p", 2, 0), (2.0, "p", 1, 4))


# zero_w: the main panel (same rows, same y) with zero weights planted; cell ids are MAIN_CELLS' positions.
#   (a) ZERO_A_CELL: all 20 rows of A carry w = 0 while B has weight: rows, but no weight and no mean, outside the
#       support;
#   (b) ONE_ROW_CELL: of A's 30 rows only the first keeps its weight: a replicate that does not draw it loses the cell;
#   (c) MIXED_CELL: every third row of A and every fourth of B carry w = 0 inside a well-supported cell;
#   (d) the cells of A alone (0, 4, 10) carry w = 0 throughout, so with (a) every cell outside the support has no
#       weight of A: N_A^out == 0.0 with rows present, at the point pass and in every replicate that keeps cells 2
#       and 8 (one row of each group) matched or unmatched on A's side alone.
ZERO_A_CELL, ONE_ROW_CELL, MIXED_CELL, A_ONLY_CELLS = 3, 7, 5, (0, 4, 10)
# singletons: every row is its own cell (one fragment per row: the table pointer advances on every row). B holds
# x = 0 .. 320 (321 rows, two tiles), A every tenth of them (33 shared cells) and 32 keys of its own between them
# (x = 5.5, 15.5, ..): 65 rows, 353 cells, 288 of B alone.
SINGLETON_CELLS = tuple(sorted([(float(j), "p", int(j % 10 == 0), 1) for j in range(321)]
                               + [(j + 0.5, "p", 1, 0) for j in range(5, 321, 10)]))
# edges: groups of exactly (1, 64), (64, 256) and (256, 512) rows. B's runs end exactly at row 64 (a sub-tile), at
# row 256 (a tile; the chunk boundary of the 512-row group) and at the group's last row, where the kernel reads the
# sentinel after a full sub-tile, tile or chunk. In (1, 64) A's single row (w = 1/2, so w y and its quotient are
# exact) is drawn exactly once in every replicate.
EDGE_CELLS = {(1, 64): ((0.0, "p", 1, 40), (1.0, "p", 0, 24)),
              (64, 256): ((0.0, "p", 30, 64), (1.0, "p", 34, 100), (2.0, "p", 0, 92)),
              (256, 512): ((0.0, "p", 64, 64), (1.0, "p", 100, 192), (2.0, "p", 92, 100), (3.0, "p", 0, 156))}
EDGE_NAMES = {f"edges_{a}_{b}": (a, b) for a, b in EDGE_CELLS}
OFFSET = 2.0 ** 20


def _plant_zero_w(ci, g, w):
    a = g == "A"
    w[a & np.isin(ci, (ZERO_A_CELL,) + A_ONLY_CELLS)] = 0.0
    w[np.flatnonzero(a & (ci == ONE_ROW_CELL))[1:]] = 0.0
    w[np.flatnonzero(a & (ci == MIXED_CELL))[::3]] = 0.0
    w[np.flatnonzero(~a & (ci == MIXED_CELL))[::4]] = 0.0


def _plant_half(ci, g, w):
    w[g == "A"] = 0.5


def _frame(spec, seed, w_div=8.0, offset=0.0, plant=None):
    rng = np.random.default_rng(seed)
    x, s, g, ci = [], [], [], []
    for i, (xv, sv, n_a, n_b) in enumerate(spec):
        for name, n in (("A", n_a), ("B", n_b)):
            x += [(-0.0 if name == "A" and xv == 0.0 and sv == "p" else xv)] * n
            s += [sv] * n
            g += [name] * n
            ci += [i] * n
    n = len(x)
    x, g = np.array(x), np.array(g)
    y = 10.0 + 0.7 * x + (g == "A") * (0.5 + 0.2 * x) + rng.normal(size=n) + offset
    w = rng.integers(1, 17, size=n) / w_div  # / 8: dyadic, every sum of c w is exact in f64, whatever its order
    if plant:
        plant(np.array(ci), g, w)
    order = rng.permutation(n)  # the frame's row order is not the cells'
    return {"y": y[order].tolist(), "g": g[order].tolist(), "x": x[order].tolist(), "s": np.array(s)[order].tolist(),
            "w": w[order].tolist()}


_panels = {}


def panel(name, weighted):
    """A panel by name (main, tiny, zero_w, offset, singletons, edges_1_64, edges_64_256, edges_256_512), built
    once and shared (read-only)."""
    if (name, weighted) not in _panels:
        if name in EDGE_NAMES:
            shape = EDGE_NAMES[name]
            args = (EDGE_CELLS[shape], 15 + shape[0]), {"plant": _plant_half if shape[0] == 1 else None}
        else:
            args = {"main": ((MAIN_CELLS, 11), {}), "tiny": ((TINY_CELLS, 12), {}),
                    "zero_w": ((MAIN_CELLS, 11), {"plant": _plant_zero_w}),
                    "offset": ((MAIN_CELLS, 11), {"w_div": 7.0, "offset": OFFSET}),  # w = k / 7: not dyadic
                    "singletons": ((SINGLETON_CELLS, 13), {})}[name]
        _panels[(name, weighted)] = Panel(_frame(*args[0], **args[1]), ["x"], ["s"], weighted)
    return _panels[(name, weighted)]


_boots = {}


def boot(O, name, weighted):
    """The restatement's point row and REPS replicates of a panel, computed once and shared (read-only)."""
    if (name, weighted) not in _boots:
        p = panel(name, weighted)
        point, okp = p.point()
        rows, ok, sup = p.boot(O, 0, REPS)
        for a in (point, rows, ok, sup):
            a.setflags(write=False)
        _boots[(name, weighted)] = (point, okp, rows, ok, sup)
    return _boots[(name, weighted)]


_exact = {}


def boot_exact(O, name, weighted):
    """The exact reference's point row and REPS replicates of a panel (Panel.boot_exact), computed once and shared
    (read-only)."""
    if (name, weighted) not in _exact:
        out = panel(name, weighted).boot_exact(O, REPS)
        for a in out:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _exact[(name, weighted)] = out
    return _exact[(name, weighted)]


# The long group of ob_nopo_sums: 33,025 rows are 130 tiles in 128 chunks, the smallest row count with a chunk of two
# tiles (chunks 63 and 127: tiles 63 .. 64 and 128 .. 129) and with the last row alone in its tile. Runs of 1 to a
# few hundred rows; the run over row 64 * 256 spans the tile boundary inside chunk 63, a run ends exactly on the
# tile boundary 129 * 256 inside chunk 127, and the last row is a cell of its own.
LONG_N, LONG_REPS = 33025, 65


class Group:
    """One sorted group for ob_nopo_sums: y, w, cell, n_cells and u8 counts [reps][n]."""

    def __init__(self, y, w, cell, n_cells, counts):
        self.y, self.w, self.cell, self.n_cells, self.counts = y, w, cell, n_cells, counts
        self.n = len(y)
        self.chunks = group_chunks((self.n + TILE - 1) // TILE)
        for a in (y, w, cell, counts):
            a.setflags(write=False)


_groups = {}


def long_group():
    """w a multiple of 1/8 up to 2 (zeros among them), y a multiple of 2^-20 below 32 in magnitude, counts below 256:
    c (w y) takes at most 8 + 5 + 25 bits, so every product is exact in f64 and, a run being short, so is every sum:
    math.fsum over a cell's terms is the exact sum (test_nopo_host.py proves the premise from the arrays)."""
    if "long" not in _groups:
        rng = np.random.default_rng(21)
        n = LONG_N
        cut = np.zeros(n, dtype=bool)
        cut[rng.choice(np.arange(1, n), size=700, replace=False)] = True
        cut[[64, 256, 512, 63 * TILE, 65 * TILE, 129 * TILE]] = True  # runs that end on a sub-tile, a tile, a chunk
        cut[64 * TILE - 40:64 * TILE + 40] = False  # one run across the tile boundary inside chunk 63
        cell = np.cumsum(cut).astype(np.int32)
        y = rng.integers(-2 ** 25 + 1, 2 ** 25, size=n) / 2.0 ** 20
        w = rng.integers(0, 17, size=n) / 8.0
        counts = rng.integers(0, 4, size=(LONG_REPS, n)).astype(np.uint8)
        counts[rng.integers(0, LONG_REPS, 400), rng.integers(0, n, 400)] = 255
        counts[3, 64 * TILE:65 * TILE] = 0    # the second tile of the two-tile chunk 63, all zeros
        counts[5, 63 * TILE:64 * TILE] = 0    # its first tile
        counts[7, 128 * TILE:129 * TILE] = 0  # the first tile of chunk 127
        counts[64, 17 * TILE:18 * TILE] = 0   # a one-tile chunk, in the second replicate block
        counts[9, n - 1] = 0                  # the last row, alone in its tile
        counts[11, n - 1] = 255
        _groups["long"] = Group(y, w, cell, int(cell[-1]) + 1, counts)
    return _groups["long"]


def long_sums(gr, c=None, absolute=False):
    """The exact N and S of the long group for one replicate's counts (None: the point pass): math.fsum per cell.
    absolute: with |y| for y."""
    c = np.ones(gr.n) if c is None else c.astype(np.float64)
    first = np.flatnonzero(np.diff(gr.cell, prepend=-1))
    tn, ts = (c * gr.w).tolist(), (c * (gr.w * (np.abs(gr.y) if absolute else gr.y))).tolist()
    ends = first.tolist()[1:] + [gr.n]
    return (np.array([math.fsum(tn[a:b]) for a, b in zip(first.tolist(), ends)]),
            np.array([math.fsum(ts[a:b]) for a, b in zip(first.tolist(), ends)]))


# The byte group: group B of the main panel (257 rows: two tiles, two chunks, a ragged last sub-tile of one row) with
# counts that hold every byte value in each of the four byte lanes of a count word.
BYTE_REPS = 2 * 64 + 3  # three replicate blocks, the last ragged


def byte_group():
    if "byte" not in _groups:
        p = panel("main", True)
        rng = np.random.default_rng(22)
        counts = rng.integers(0, 256, size=(BYTE_REPS, p.n[1])).astype(np.uint8)
        counts[2, 8:12] = (128, 255, 129, 254)  # whole words of high bytes
        counts[70, 252:256] = 255
        counts[130, 256] = 255  # the last row of the last replicate
        _groups["byte"] = Group(p.y[1].copy(), p.w[1].copy(), p.cell[1].copy(), p.n_cells, counts)
    return _groups["byte"]


def aggregate(O, point, rows, ok):
    """(estimate, std_err, ci_lower, ci_upper) per component: the oracle's bootstrap statistics over the rows kept."""
    kept = np.asarray(rows)[np.asarray(ok).astype(bool)]
    out = []
    for c in COLUMNS:
        se, _, (lo, hi) = O.bootstrap_stats(kept[:, c])
        out.append((point[c], se, lo, hi))
    return out
