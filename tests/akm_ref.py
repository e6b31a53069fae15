"""NumPy restatement of the reference's AKM module (akm.rs), written from its description.

f64 mode: ``np.bincount(idx, weights=v)`` adds its weights in row order, the reference's own order,
so ``demean`` and ``recover_fe`` are the reference operation for operation (sums, the division by the
count, the subtraction, and the change norm added row by row). Each loop returns its result, its
iteration count, the whole ``diff`` sequence and ``V``, the largest magnitude that entered a group
sum over the run.

High-precision mode (``hi=True``): the same recursions in ``np.longdouble`` (64-bit significand here),
stopped at the iteration counts the f64 mode found. ``math.fsum`` rounds its arguments to f64, so it
cannot add longdouble values; the group sums are longdouble ``np.add.reduceat`` sums over the rows
sorted by group instead, 2^11 times finer than the f64 rounding the bars are about.

Connected set: components by label propagation (the result does not depend on the order of the
edges); the engine's tie rule (most nodes, then the smallest sorted worker id).
"""
import numpy as np

U = 2.0 ** -53


def _seq_sum(x):
    """x[0] + x[1] + ... in order, as a Rust `for` loop adds them."""
    x = np.asarray(x, dtype=np.float64)
    return float(np.bincount(np.zeros(len(x), dtype=np.intp), weights=x, minlength=1)[0])


class _Groups:
    """Group sums of one grouping in either precision."""

    def __init__(self, idx, n_groups):
        self.idx = np.asarray(idx, dtype=np.intp)
        self.n = int(n_groups)
        self.counts = np.bincount(self.idx, minlength=self.n)
        self.order = np.argsort(self.idx, kind="stable")
        self.present = np.flatnonzero(self.counts > 0)
        self.starts = (np.cumsum(self.counts) - self.counts)[self.present]

    def sums(self, v):
        if v.dtype == np.float64:
            return np.bincount(self.idx, weights=v, minlength=self.n)
        out = np.zeros(self.n, dtype=v.dtype)
        if len(v):
            out[self.present] = np.add.reduceat(v[self.order], self.starts)
        return out

    def means(self, v, keep=None):
        s = self.sums(v)
        out = np.zeros(self.n, dtype=v.dtype) if keep is None else keep.copy()
        nz = self.counts > 0
        out[nz] = s[nz] / self.counts[nz].astype(v.dtype)
        return out


def demean(v, widx, fidx, n_workers, n_firms, tol=1e-8, max_iters=1000, hi=False, stop_at=None):
    """akm.rs:452-527 -> (v, iterations, diffs, V). converged is ``iterations < max_iters``."""
    dt = np.longdouble if hi else np.float64
    v = np.array(v, dtype=dt)
    gw, gf = _Groups(widx, n_workers), _Groups(fidx, n_firms)
    diffs, big, it = [], 0.0, 0
    diff = tol + 1.0
    while (it < stop_at) if stop_at is not None else (diff > tol and it < max_iters):
        prev = v.copy()
        big = max(big, float(np.max(np.abs(v))) if len(v) else 0.0)
        v = v - gw.means(v)[gw.idx]
        big = max(big, float(np.max(np.abs(v))) if len(v) else 0.0)
        v = v - gf.means(v)[gf.idx]
        d = v - prev
        diff = float(np.sqrt(_seq_sum((d * d).astype(np.float64)))) if not hi else float(np.sqrt(np.sum(d * d)))
        diffs.append(diff)
        it += 1
    return v, it, diffs, big


def recover_fe(r, widx, fidx, n_workers, n_firms, tol=1e-8, max_iters=1000, hi=False, stop_at=None, normalise=True):
    """akm.rs:530-621 -> (alpha, psi, iterations, diffs, V)."""
    dt = np.longdouble if hi else np.float64
    r = np.array(r, dtype=dt)
    gw, gf = _Groups(widx, n_workers), _Groups(fidx, n_firms)
    alpha, psi = np.zeros(n_workers, dtype=dt), np.zeros(n_firms, dtype=dt)
    diffs, big, it = [], 0.0, 0
    diff = tol + 1.0
    while (it < stop_at) if stop_at is not None else (diff > tol and it < max_iters):
        pa, pp = alpha.copy(), psi.copy()
        t = r - psi[gf.idx]
        big = max(big, float(np.max(np.abs(t))) if len(t) else 0.0)
        alpha = gw.means(t, keep=alpha)
        t = r - alpha[gw.idx]
        big = max(big, float(np.max(np.abs(t))) if len(t) else 0.0)
        psi = gf.means(t, keep=psi)
        da, dp = alpha - pa, psi - pp
        sq = np.concatenate([da * da, dp * dp])
        diff = float(np.sqrt(_seq_sum(sq.astype(np.float64)))) if not hi else float(np.sqrt(np.sum(sq)))
        diffs.append(diff)
        it += 1
    if normalise and n_firms > 0:
        ref = psi[0]
        psi = psi - ref
        alpha = alpha + ref
    return alpha, psi, it, diffs, big


def connected_set(workers, firms):
    """akm.rs:151-303 over two lists of id strings (None: null) -> dict like ``ob.akm_connected_set``."""
    n = len(workers)
    both = np.array([w is not None and f is not None for w, f in zip(workers, firms)], dtype=bool)
    wall = sorted({w for w in workers if w is not None}, key=lambda s: s.encode())
    fall = sorted({f for f in firms if f is not None}, key=lambda s: s.encode())
    wpos = {s: i for i, s in enumerate(wall)}
    fpos = {s: i for i, s in enumerate(fall)}
    nw, nf = len(wall), len(fall)
    ew = np.array([wpos[w] for w, b in zip(workers, both) if b], dtype=np.intp)
    ef = np.array([fpos[f] + nw for f, b in zip(firms, both) if b], dtype=np.intp)
    lab = np.arange(nw + nf)
    while True:
        m = np.minimum(lab[ew], lab[ef])
        new = lab.copy()
        np.minimum.at(new, ew, m)
        np.minimum.at(new, ef, m)
        new = new[new]  # pointer jumping
        if np.array_equal(new, lab):
            break
        lab = new
    keep = np.zeros(n, dtype=bool)
    out = {"keep": keep, "worker_idx": np.zeros(0, np.int32), "firm_idx": np.zeros(0, np.int32), "worker_ids": [],
           "firm_ids": [], "n_components": int(len(np.unique(lab)))}
    if nw + nf == 0:
        return out
    roots, counts = np.unique(lab, return_counts=True)
    best, best_key = None, None
    for root, cnt in zip(roots, counts):
        members = np.flatnonzero(lab == root)
        wmin = members[members < nw].min() if (members < nw).any() else np.iinfo(np.int64).max
        key = (-int(cnt), int(wmin))
        if best_key is None or key < best_key:
            best, best_key = root, key
    edge_keep = lab[ew] == best
    keep[np.flatnonzero(both)[edge_keep]] = True
    kw, kf = ew[edge_keep], ef[edge_keep] - nw
    uw, uf = np.unique(kw), np.unique(kf)
    out.update(worker_idx=np.searchsorted(uw, kw).astype(np.int32), firm_idx=np.searchsorted(uf, kf).astype(np.int32),
               worker_ids=[wall[i] for i in uw], firm_ids=[fall[i] for i in uf])
    return out


class AkmRefError(Exception):
    def __init__(self, kind, message):
        super().__init__(message)
        self.kind = kind  # "insufficient" | "convergence"


def run(workers, firms, y, controls, tol=1e-8, max_iters=1000):
    """AkmBuilder::run (akm.rs:89-449). y: floats or None; controls: list of columns, None reads as 0.0."""
    cs = connected_set(workers, firms)
    keep = cs["keep"]
    if not keep.any():
        raise AkmRefError("insufficient", "No connected set found")
    wi, fi = cs["worker_idx"], cs["firm_idx"]
    nw, nf = len(cs["worker_ids"]), len(cs["firm_ids"])
    yk = [v for v, k in zip(y, keep) if k]
    if any(v is None for v in yk):
        raise AkmRefError("insufficient", "Null outcome encountered")
    yk = np.array(yk, dtype=np.float64)
    xs = [np.array([0.0 if v is None else v for v, k in zip(col, keep) if k], dtype=np.float64) for col in controls]
    iters = []

    def dm(v):
        out, it, _, _ = demean(v, wi, fi, nw, nf, tol, max_iters)
        iters.append(it)
        if it >= max_iters:
            raise AkmRefError("convergence", f"demean_vector failed to converge within {max_iters} iterations")
        return out

    yr = dm(yk)
    xr = [dm(x) for x in xs]
    beta = np.zeros(0)
    if xs:
        xm = np.stack(xr, axis=1)
        xtx, xty = xm.T @ xm, xm.T @ yr
        try:
            l = np.linalg.cholesky(xtx)
        except np.linalg.LinAlgError:
            raise AkmRefError("convergence", "OLS design matrix is singular") from None
        beta = np.linalg.solve(l.T, np.linalg.solve(l, xty))
    r = yk.copy()
    for j, x in enumerate(xs):
        r = r - x * beta[j]
    alpha, psi, it, _, _ = recover_fe(r, wi, fi, nw, nf, tol, max_iters)
    if it >= max_iters:
        raise AkmRefError("convergence", f"recover_fe failed to converge within {max_iters} iterations")
    tss = float(np.sum((yk - yk.sum() / len(yk)) ** 2))
    pred = alpha[wi] + psi[fi]
    for j, x in enumerate(xs):
        pred = pred + x * beta[j]
    rss = float(np.sum((yk - pred) ** 2))
    return {"beta": beta, "worker_effects": dict(zip(cs["worker_ids"], alpha.tolist())),
            "firm_effects": dict(zip(cs["firm_ids"], psi.tolist())), "r2": 1.0 - rss / tss,
            "demean_iterations": iters, "recover_iterations": it, "set": cs}


def panel(n, n_workers, n_firms, n_controls, seed, zipf=False):
    """The reference test's recipe (tests/test_akm.rs): uniform worker draws, uniform (or Zipf 1.3) firm
    draws, x in (0, 10), beta = 2.5 per control, alpha in (-1, 1), psi in (-0.5, 0.5), noise +-0.01; then
    the largest connected set with dense indices. -> dict(widx, fidx, nw, nf, y, x (n, n_controls))."""
    rng = np.random.default_rng(seed)
    alpha, psi = rng.uniform(-1, 1, n_workers), rng.uniform(-0.5, 0.5, n_firms)
    w = rng.integers(0, n_workers, n)
    if zipf:
        p = 1.0 / np.arange(1, n_firms + 1) ** 1.3
        f = rng.choice(n_firms, size=n, p=p / p.sum())
    else:
        f = rng.integers(0, n_firms, n)
    x = rng.uniform(0, 10, (n, n_controls))
    y = 2.5 * x.sum(axis=1) + alpha[w] + psi[f] + rng.uniform(-0.01, 0.01, n)
    return dense(w, f, y, x)


def dense(w, f, y, x):
    """Largest connected set of integer-labelled rows and dense indices (label order is irrelevant to
    the loops, so integers are ranked as integers here)."""
    uw, wi = np.unique(w, return_inverse=True)
    uf, fi = np.unique(f, return_inverse=True)
    nw = len(uw)
    lab = np.arange(nw + len(uf))
    ew, ef = wi, fi + nw
    while True:
        m = np.minimum(lab[ew], lab[ef])
        new = lab.copy()
        np.minimum.at(new, ew, m)
        np.minimum.at(new, ef, m)
        new = new[new]
        if np.array_equal(new, lab):
            break
        lab = new
    roots, counts = np.unique(lab, return_counts=True)
    keep = lab[ew] == roots[np.argmax(counts)]
    kw, kf = np.unique(wi[keep], return_inverse=True)[1], np.unique(fi[keep], return_inverse=True)[1]
    return {"widx": kw.astype(np.int32), "fidx": kf.astype(np.int32), "nw": int(kw.max()) + 1, "nf": int(kf.max()) + 1,
            "y": np.ascontiguousarray(y[keep]), "x": np.ascontiguousarray(x[keep])}


def sized_firms(sizes, n_workers, seed):
    """A panel whose firm k has exactly sizes[k] rows, rows shuffled, workers drawn uniformly."""
    rng = np.random.default_rng(seed)
    f = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    n = len(f)
    w = rng.integers(0, n_workers, n)
    alpha, psi = rng.uniform(-1, 1, n_workers), rng.uniform(-0.5, 0.5, len(sizes))
    x = rng.uniform(0, 10, (n, 1))
    y = 2.5 * x[:, 0] + alpha[w] + psi[f] + rng.uniform(-0.01, 0.01, n)
    return dense(w, f, y, x)


# The schedule boundaries of csrc/ob_akm.hpp (kAkmLaneMax, kAkmWaveMax): lane <= 32 < wave <= 2048 < block.
LANE_MAX, WAVE_MAX = 32, 2048
BOUNDARY_SIZES = [1, 63, 64, 65, LANE_MAX - 1, LANE_MAX, LANE_MAX + 1, WAVE_MAX - 1, WAVE_MAX, WAVE_MAX + 1]

_CACHE = {}


def case(name):
    """The inputs tests/test_gpu_akm.py uses, by name; built once per process and never modified."""
    if name not in _CACHE:
        _CACHE[name] = _build(name)
    return _CACHE[name]


CASES = ["p1000", "p5000", "zipf70k", "zipf300k", "four", "singletons", "boundaries", "wide65"]


def _build(name):
    if name == "p1000":
        return panel(1000, 100, 20, 1, 7)
    if name == "p5000":
        return panel(5000, 1500, 60, 5, 7)
    if name == "zipf70k":
        return panel(70000, 9000, 300, 1, 7, zipf=True)
    if name == "zipf300k":
        return panel(300000, 40000, 2000, 1, 7, zipf=True)
    if name == "four":
        return {"widx": np.array([0, 1, 0, 1], np.int32), "fidx": np.array([0, 0, 1, 1], np.int32), "nw": 2, "nf": 2,
                "y": np.array([1.0, 2.0, 3.0, 4.0]), "x": np.array([[1.0], [0.0], [0.5], [2.0]])}
    if name == "singletons":
        rng = np.random.default_rng(11)
        n = 777
        return {"widx": rng.permutation(n).astype(np.int32), "fidx": rng.integers(0, 9, n).astype(np.int32), "nw": n,
                "nf": 9, "y": rng.normal(size=n), "x": rng.normal(size=(n, 1))}
    if name == "boundaries":
        return sized_firms(BOUNDARY_SIZES, 1500, 5)
    if name == "wide65":
        d = dict(panel(1000, 100, 20, 1, 7))
        rng = np.random.default_rng(65)
        d["x"] = np.concatenate([d["x"], rng.normal(size=(len(d["y"]), 63)) * 3.0], axis=1)
        return d
    raise KeyError(name)


def batch(d):
    """(n, 1 + controls): the outcome, then the controls."""
    return np.concatenate([d["y"][:, None], d["x"]], axis=1)


def max_group(d):
    return int(max(np.bincount(d["widx"]).max(), np.bincount(d["fidx"]).max()))


_REF = {}


def ref_demean(name, tol=1e-8, max_iters=1000):
    """The f64 restatement of every column of a case: list of (v, iterations, diffs, V)."""
    key = ("d", name, tol, max_iters)
    if key not in _REF:
        d = case(name)
        b = batch(d)
        _REF[key] = [demean(b[:, c], d["widx"], d["fidx"], d["nw"], d["nf"], tol, max_iters) for c in range(b.shape[1])]
    return _REF[key]


def residual(d):
    return d["y"] - 2.5 * d["x"][:, 0]


def ref_recover(name, tol=1e-8, max_iters=1000):
    key = ("r", name, tol, max_iters)
    if key not in _REF:
        d = case(name)
        _REF[key] = recover_fe(residual(d), d["widx"], d["fidx"], d["nw"], d["nf"], tol, max_iters)
    return _REF[key]


def margin_ok(diffs, tol):
    """The stopping margin: the last diff <= tol (1 - 1e-6), every earlier one >= tol (1 + 1e-6)."""
    return len(diffs) >= 1 and diffs[-1] <= tol * (1 - 1e-6) and all(x >= tol * (1 + 1e-6) for x in diffs[:-1])


def demean_bar(t, m, n, big):
    return 4.0 * t * (m + 2) * U * np.sqrt(n) * big


def recover_bar(t, m, big):
    return 4.0 * t * (m + 3) * U * big
