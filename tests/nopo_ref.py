"""numpy f64 restatement of Nopo's matching decomposition of include/oaxaca_boot.h: the cells by
numpy.unique over the key tuples, the per-cell sums by numpy.bincount with weights over the oracle's OBRS-3 counts,
the terms exactly as the header defines them. Shared by test_nopo_host.py and test_gpu_nopo.py."""
import numpy as np

# Both panels, weighted and unweighted, were checked on the CPU (test_gpu_nopo.py asserts it before any GPU call):
# with this seed replicates 0 .. 66 of the main panel hold supports that differ from the point pass's, and those of
# the tiny panel hold both ok = 0 and ok = 1 replicates. With a one-row cell either holds for about a third of the
# replicates, so nearly any seed does.
SEED = 0x0B5EED
REPS = 64 + 3  # a ragged replicate batch
ROW_LEN = 13
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


def _frame(spec, seed):
    rng = np.random.default_rng(seed)
    x, s, g = [], [], []
    for xv, sv, n_a, n_b in spec:
        for name, n in (("A", n_a), ("B", n_b)):
            x += [(-0.0 if name == "A" and xv == 0.0 and sv == "p" else xv)] * n
            s += [sv] * n
            g += [name] * n
    n = len(x)
    x, g = np.array(x), np.array(g)
    y = 10.0 + 0.7 * x + (g == "A") * (0.5 + 0.2 * x) + rng.normal(size=n)
    w = rng.integers(1, 17, size=n) / 8.0  # dyadic: every sum of c w is exact in f64, whatever its order
    order = rng.permutation(n)  # the frame's row order is not the cells'
    return {"y": y[order].tolist(), "g": g[order].tolist(), "x": x[order].tolist(), "s": np.array(s)[order].tolist(),
            "w": w[order].tolist()}


_panels = {}


def panel(name, weighted):
    """The main or the tiny panel, built once and shared (read-only)."""
    if (name, weighted) not in _panels:
        spec, seed = {"main": (MAIN_CELLS, 11), "tiny": (TINY_CELLS, 12)}[name]
        _panels[(name, weighted)] = Panel(_frame(spec, seed), ["x"], ["s"], weighted)
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


def aggregate(O, point, rows, ok):
    """(estimate, std_err, ci_lower, ci_upper) per component: the oracle's bootstrap statistics over the rows kept."""
    kept = np.asarray(rows)[np.asarray(ok).astype(bool)]
    out = []
    for c in COLUMNS:
        se, _, (lo, hi) = O.bootstrap_stats(kept[:, c])
        out.append((point[c], se, lo, hi))
    return out
