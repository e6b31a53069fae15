"""numpy restatement of the per-replicate RIF of a quantile over resample counts (csrc/ob_rifq.hip).

A group's rows stand in stable ascending order of y; a replicate is its counts c_i over those rows. `restate` gives
what rif.rs:14-88 (oracle.rif) returns on the expanded resample np.repeat(y_sorted, c), computed over the counts: the
quantile q (bitwise), the bandwidth, the density, N_le, the masked sums T_a and the y-pairs of the extended Gram. With
dtype=np.longdouble everything but q and the row prefix p (exact by definition) runs in extended precision: that
run measures the f64 restatement's own error E, from which the GPU tests take their bound (8 E, floor 1e-12).

`python tests/rifq_ref.py` prints E over the GPU tests' inputs."""
import os
import sys

import numpy as np

SEED = 0x0B5EED
TAUS = (0.1, 0.5, 0.9)
SIZES = (2, 130, 256, 257, 513)
FLOOR = 1e-12


def order_stat(y_sorted, csum, k):
    """Y(k): the y of the first sorted position whose inclusive count prefix exceeds k."""
    return y_sorted[int(np.searchsorted(csum, k, side="right"))]


def quantile(y_sorted, csum, n, tau):
    """Type-7 quantile of the expanded resample, the multiply and the add rounded separately (f64)."""
    h = (np.float64(n) - 1.0) * np.float64(tau)
    hf, hc = np.floor(h), np.ceil(h)
    y0 = order_stat(y_sorted, csum, int(hf))
    if hf == hc:
        return y0
    y1 = order_stat(y_sorted, csum, int(hc))
    return y0 + (h - hf) * (y1 - y0)


def restate(y_sorted, c, taus, x=None, dtype=np.float64):
    """-> dict of q, p, bw, f_raw, f, floored, n_le, t, gy (per tau where it applies), iqr, spread."""
    y64 = np.ascontiguousarray(y_sorted, dtype=np.float64)
    c = np.asarray(c, dtype=np.int64)
    n = int(c.sum())
    assert n == len(y64) and n >= 2
    csum = np.cumsum(c)
    y, cw, nf = y64.astype(dtype), c.astype(dtype), dtype(n)
    v = np.ones((n, 1), dtype=dtype) if x is None else np.hstack([np.ones((n, 1), dtype=dtype), np.asarray(x, dtype=dtype)])
    mean = (cw * y).sum() / nf
    sd = np.sqrt((cw * (y - mean) ** 2).sum() / (nf - 1))
    i75, i25 = max(int(np.ceil(0.75 * n)) - 1, 0), max(int(np.ceil(0.25 * n)) - 1, 0)
    iqr = dtype(order_stat(y64, csum, min(i75, n - 1))) - dtype(order_stat(y64, csum, min(i25, n - 1)))
    spread = min(sd, iqr / dtype(1.34)) if iqr > 1e-8 else sd
    spread_used = dtype(1.0) if spread < 1e-8 else spread
    bw = dtype(0.9) * spread_used * dtype(np.float64(n) ** -0.2)
    out = {"bw": bw, "iqr": iqr, "spread": spread, "mean": mean, "sd": sd, "q": [], "p": [], "f_raw": [], "f": [],
           "floored": [], "n_le": [], "t": [], "gy": [], "A": [], "B": []}
    g0 = (cw[:, None] * v).sum(0)
    for tau in taus:
        q = quantile(y64, csum, n, tau)
        p = int(np.searchsorted(y64, q, side="right"))
        u = (dtype(q) - y) / bw
        f_raw = (cw * (dtype(1.0) / np.sqrt(dtype(2.0) * dtype(np.pi))) * np.exp(dtype(-0.5) * (u * u))).sum() / (nf * bw)
        f = dtype(1e-8) if f_raw < 1e-8 else f_raw
        B = dtype(1.0) / f
        A = dtype(q) + dtype(tau) * B
        t = (cw[:p, None] * v[:p]).sum(0)
        gy = np.concatenate([A * g0 - B * t, [A * A * nf - (2 * A * B - B * B) * t[0]]])
        for key, val in (("q", q), ("p", p), ("f_raw", f_raw), ("f", f), ("floored", bool(f_raw < 1e-8)),
                         ("n_le", int(c[:p].sum())), ("t", t), ("gy", gy), ("A", A), ("B", B)):
            out[key].append(val)
    return out


def rif_values(y_sorted, r, t):
    """RIF of every sorted row at tau index t of a restatement."""
    return np.where(np.asarray(y_sorted) <= r["q"][t], r["A"][t] - r["B"][t], r["A"][t])


def check_steps(r):
    """rif.rs branches on iqr > 1e-8, spread < 1e-8 and density < 1e-8: each must sit exactly at its degenerate value
    or clear of the threshold, so that no rounding decides a branch."""
    def clear(vv, degenerate):
        vv = float(vv)
        return vv == degenerate or not (0.5e-8 <= vv <= 2e-8)
    assert clear(r["iqr"], 0.0), r["iqr"]
    assert clear(r["spread"], 0.0), r["spread"]
    for fr in r["f_raw"]:
        assert clear(fr, 0.0), fr


def panel(n, p, seed=11, decimals=None):
    """Sorted log-wage-like y with p predictors correlated with it -> (y_sorted, x in y's order)."""
    rng = np.random.default_rng(1000 * seed + 7 * n + p)
    x = rng.normal(size=(n, p))
    y = 2.5 + x @ (0.4 / np.sqrt(max(p, 1)) * np.ones(p)) + 0.5 * rng.normal(size=n) if p else 2.5 + 0.6 * rng.normal(size=n)
    if decimals is not None:
        y = np.round(y, decimals)
    order = np.argsort(y, kind="stable")
    return np.ascontiguousarray(y[order]), np.ascontiguousarray(x[order])


def stream_counts(O, n, reps, seed=SEED, g=0, first=0):
    return np.stack([np.bincount(O.resample_indices(seed, first + r, g, n), minlength=n) for r in range(reps)])


def hand_counts(n):
    """Long zero runs and one count of 200 (where n allows it); sums to n."""
    c = np.zeros(n, dtype=np.int64)
    if n < 210:
        c[n // 2] = n - 1 if n > 2 else 1
        c[n - 1] += 1
        return c
    c[n // 3] = 200
    rest = n - 200
    c[5] = rest // 2
    c[n - 2] = rest - rest // 2
    return c


def taus_for(n):
    """0.1 / 0.5 / 0.9 and a tau whose h = (n - 1) tau is whole in f64 (0.25 or 0.75 when n - 1 divides by 4,
    else 0.5 on odd n)."""
    extra = [t for t in (0.25, 0.75) if ((n - 1) * t) == np.floor((n - 1) * t)]
    return tuple(sorted(set(TAUS) | set(extra[:1])))


def cases(O, reps=5):
    """(name, y_sorted, x, counts [reps'][n], taus) of the rifq_pass tests."""
    out = []
    for n in SIZES:
        y, x = panel(n, 2)
        c = np.vstack([stream_counts(O, n, reps), hand_counts(n)[None, :]])
        out.append((f"n{n}", y, x, c, taus_for(n)))
    y, x = panel(257, 2, decimals=1)  # every quantile falls inside a tie run
    out.append(("ties257", y, x, stream_counts(O, 257, reps), TAUS))
    y, x = panel(130, 2)
    out.append(("const130", np.full(130, 3.25), x, stream_counts(O, 130, reps), TAUS))
    return out


def mixed_err(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), np.longdouble(1e-300)))


def restatement_error(O):
    """E per quantity: the f64 restatement against the longdouble run over every case and replicate."""
    E = {"bw": 0.0, "f": 0.0, "t": 0.0, "gy": 0.0}
    for _, y, x, cs, taus in cases(O):
        for c in cs:
            r64, rld = restate(y, c, taus, x), restate(y, c, taus, x, dtype=np.longdouble)
            check_steps(r64)
            assert r64["q"] == rld["q"] and r64["p"] == rld["p"]
            E["bw"] = max(E["bw"], mixed_err(r64["bw"], rld["bw"]))
            for key in ("f", "t", "gy"):
                E[key] = max(E[key], mixed_err(np.array(r64[key], dtype=np.float64), np.array(rld[key])))
    return E


def bound(E):
    return max(8.0 * E, FLOOR)


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "oracle"))
    import oracle

    oracle.build()
    for key, val in restatement_error(oracle).items():
        print(f"E[{key}] = {val:.3e}   bound {bound(val):.3e}")


# ---- the refitted decomposition (ob_builder_prepare_quantiles_refit) ----------------------------------------------
def frame(k, n_a=130, n_b=257, seed=5):
    """A wage-like frame with K = k design columns: k - 2 - (k > 3) numeric predictors and one categorical with 2
    (k = 3) or 3 levels -> (dict frame, numeric names, categorical names)."""
    rng = np.random.default_rng(100 * seed + k)
    n = n_a + n_b
    levels = 2 if k == 3 else 3
    n_num = k - 1 - (levels - 1)
    g = np.array(["A"] * n_a + ["B"] * n_b)
    x = rng.normal(size=(n, n_num)) + 0.3 * (g == "A")[:, None]
    cat = rng.integers(0, levels, n)
    y = 2.4 + 0.25 * (g == "A") + x @ (0.3 / np.sqrt(n_num) * np.ones(n_num)) + 0.15 * cat + 0.5 * rng.normal(size=n)
    f = {"y": y.tolist(), "g": g.tolist(), "c": [f"l{v}" for v in cat]}
    for j in range(n_num):
        f[f"x{j}"] = x[:, j].tolist()
    return f, [f"x{j}" for j in range(n_num)], ["c"]


def sorted_designs(xa, ya, xb, yb):
    oa, ob_ = np.argsort(ya, kind="stable"), np.argsort(yb, kind="stable")
    return xa[oa], ya[oa], xb[ob_], yb[ob_], oa, ob_


def tail_of(y, tau):
    """q, f, N_le of rif.rs on the array y (a resample, any order), through the restatement over unit counts."""
    ys = np.sort(y, kind="stable")
    r = restate(ys, np.ones(len(ys), dtype=np.int64), (tau,))
    check_steps(r)
    return r["q"][0], float(r["f"][0]), float(r["n_le"][0])


def oracle_row(O, cfg, xa, ya, xb, yb, tau, ia=None, ib=None):
    """The refitted row of one (re)sample: O.rif on the resampled outcome, O.single_pass on the resampled designs,
    then q_A, q_B, f_A, f_B, N_le,A, N_le,B. xa .. yb are y-sorted; ia / ib index them (None: the sample itself)."""
    xa_, ya_ = (xa, ya) if ia is None else (xa[ia], ya[ia])
    xb_, yb_ = (xb, yb) if ib is None else (xb[ib], yb[ib])
    rc, row = O.single_pass(cfg, xa_, O.rif(ya_, tau), None, xb_, O.rif(yb_, tau), None)
    ta, tb = tail_of(ya_, tau), tail_of(yb_, tau)
    return rc, np.concatenate([row, [ta[0], tb[0], ta[1], tb[1], ta[2], tb[2]]])


def oracle_boot(O, cfg, xa, ya, xb, yb, taus, seed, first_rep, n_reps):
    """-> rows (T, n_reps, row_len + 6), ok (T, n_reps): OBRS-3 position i of group g is the i-th y-sorted row."""
    rows = np.full((len(taus), n_reps, cfg.row_len + 6), np.nan)
    ok = np.zeros((len(taus), n_reps), dtype=np.uint8)
    for r in range(n_reps):
        ia = O.resample_indices(seed, first_rep + r, 0, len(ya))
        ib = O.resample_indices(seed, first_rep + r, 1, len(yb))
        for t, tau in enumerate(taus):
            rc, row = oracle_row(O, cfg, xa, ya, xb, yb, tau, ia, ib)
            ok[t, r] = 1 if rc == 0 else 0
            rows[t, r] = row
    return rows, ok
