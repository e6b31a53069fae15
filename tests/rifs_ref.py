"""numpy restatement of the per-replicate RIFs of the variance, the Gini and quantile ranges over resample counts
(csrc/ob_rifs.hip).

A group's rows stand in stable ascending order of y; a replicate is its counts c_i over those rows. `restate` gives,
per statistic, its value nu on the expanded resample np.repeat(y_sorted, c) and the y-pairs G[a, RIF] = sum c v_a RIF,
G[RIF, RIF] = sum c RIF^2 over v = [1, x], computed over the counts by the formulas of §5.19 -- no sort, no n-length
RIF column. With dtype=np.longdouble everything but a range's q and row prefix (exact by definition) runs in extended
precision: that run measures the f64 restatement's own error E, from which the GPU tests take their bound
(8 E, floor 1e-12: the rule of §5.10).

`python tests/rifs_ref.py` prints E per statistic and quantity over the GPU tests' inputs and asserts that the counts
form equals tests/rif_stat_ref.py's variance, gini and iqr on the expanded resample to that bound. Measured on x86-64:
    variance  E[nu] = 8.0e-16  E[gy] = 6.6e-16      gini  E[nu] = 5.4e-16  E[gy] = 3.2e-15
    iqr       E[nu] = 0        E[gy] = 1.5e-15
so 8 E is below the floor for every quantity and the GPU bound is 1e-12."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rif_stat_ref as S  # noqa: E402
import rifq_ref as R  # noqa: E402

FLOOR = 1e-12
SIZES = R.SIZES
STATS = (("variance", {}), ("gini", {}), ("iqr", {"upper": 0.9, "lower": 0.1}), ("iqr", {"upper": 0.9, "lower": 0.5}),
         ("iqr", {"upper": 0.75, "lower": 0.25}))
E_MEASURED = {"variance": {"nu": 8.0e-16, "gy": 6.6e-16}, "gini": {"nu": 5.4e-16, "gy": 3.2e-15},
              "iqr": {"nu": 0.0, "gy": 1.5e-15}}


def tie_runs(y_sorted):
    """(row0, row1) of every run of equal y that spans more than one row."""
    y = np.asarray(y_sorted)
    edges = np.flatnonzero(np.concatenate([[True], y[1:] != y[:-1], [True]]))
    return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:]) if b - a > 1]


def _design(n, x, dtype):
    return np.ones((n, 1), dtype=dtype) if x is None else np.hstack([np.ones((n, 1), dtype=dtype),
                                                                    np.asarray(x, dtype=dtype)])


def variance_counts(y, cw, v, nf, mu0):
    d = y - mu0
    m0, m1, m2 = (cw[:, None] * v).sum(0), (cw[:, None] * v * d[:, None]).sum(0), (cw[:, None] * v * (d * d)[:, None]).sum(0)
    m3, m4 = (cw * d ** 3).sum(), (cw * d ** 4).sum()
    dl = m1[0] / nf
    nu = (m2[0] - nf * dl * dl) / nf
    ga = m2 - 2 * dl * m1 + dl * dl * m0
    grr = m4 - 4 * dl * m3 + 6 * dl * dl * m2[0] - 4 * dl ** 3 * m1[0] + dl ** 4 * nf
    return nu, np.concatenate([ga, [grr]]), (float(m2[0] / nf), float(np.abs(m2).max()))


def gini_counts(y, cw, v, nf, runs):
    cin, sin = np.cumsum(cw), np.cumsum(cw * y)
    mu = sin[-1] / nf
    if not mu > 0:
        return np.nan, np.zeros(v.shape[1] + 1), None
    z = y * (1 - cin / nf) + sin / nf
    e = sum((y[a] * (cw[a:b].sum() ** 2 - (cw[a:b] ** 2).sum()) / 2 for a, b in runs), type(mu)(0))
    big_r = ((cw * sin).sum() + e) / (nf * nf)
    al, be = 2 * big_r / (mu * mu), 2 / mu
    m0, ya, za = (cw[:, None] * v).sum(0), (cw[:, None] * v * y[:, None]).sum(0), (cw[:, None] * v * z[:, None]).sum(0)
    grr = (nf + al * al * (cw * y * y).sum() + be * be * (cw * z * z).sum() + 2 * al * ya[0] - 2 * be * za[0]
           - 2 * al * be * (cw * y * z).sum())
    return 1 - 2 * big_r / mu, np.concatenate([m0 + al * ya - be * za, [grr]]), (1.0, float(np.abs(m0).max()))


def range_counts(rq, taus, upper, lower, nf):
    """rq: rifq_ref.restate at `taus` (which hold upper and lower)."""
    h, l = taus.index(upper), taus.index(lower)
    ah, al, bh, bl = rq["A"][h], rq["A"][l], rq["B"][h], rq["B"][l]
    nh, nl = rq["n_le"][h], rq["n_le"][l]
    gh, gl = rq["gy"][h], rq["gy"][l]
    cross = ah * al * nf - ah * bl * nl - al * bh * nh + bh * bl * nl
    ga = gh[:-1] - gl[:-1]
    scale = (float(max(abs(rq["q"][h]), abs(rq["q"][l]))), float(max(np.abs(gh).max(), np.abs(gl).max())))
    return rq["q"][h] - rq["q"][l], np.concatenate([ga, [gh[-1] + gl[-1] - 2 * cross]]), rq["floored"][h] or rq["floored"][l], scale


def range_taus(stats):
    return tuple(sorted({float(p[key]) for name, p in stats if name == "iqr" for key in ("upper", "lower")}))


def restate(y_sorted, c, stats, x=None, dtype=np.float64):
    """-> dict of nu [S], gy [S][k + 1], ok [S], floored [S], scale [S] = (of nu, of gy), rq (the quantile
    restatement of the ranges, or None)."""
    y64 = np.ascontiguousarray(y_sorted, dtype=np.float64)
    c = np.asarray(c, dtype=np.int64)
    n = int(c.sum())
    assert n == len(y64) and n >= 2
    y, cw, nf = y64.astype(dtype), c.astype(dtype), dtype(n)
    v = _design(n, x, dtype)
    mu0 = y.sum() / nf  # the sample's own mean: any centre gives the same values up to rounding
    taus = range_taus(stats)
    rq = R.restate(y64, c, taus, x, dtype) if taus else None
    runs = tie_runs(y64)
    out = {"nu": [], "gy": [], "ok": [], "floored": [], "scale": [], "rq": rq}
    for name, p in stats:
        fl = False
        if name == "variance":
            nu, gy, scale = variance_counts(y, cw, v, nf, mu0)
        elif name == "gini":
            nu, gy, scale = gini_counts(y, cw, v, nf, runs)
        else:
            nu, gy, fl, scale = range_counts(rq, taus, float(p["upper"]), float(p["lower"]), nf)
        out["nu"].append(nu)
        out["gy"].append(gy)
        out["ok"].append(scale is not None)
        out["floored"].append(bool(fl))
        out["scale"].append(scale)
    return out


def expanded(y_sorted, c, stat, params, x=None, dtype=np.float64):
    """nu and the y-pairs from tests/rif_stat_ref.py's RIF column of the expanded resample."""
    ye = np.repeat(np.asarray(y_sorted, dtype=np.float64), c)
    rif, nu = S.rif_statistic(ye, stat, dtype, **params)
    ve = np.repeat(_design(len(y_sorted), x, dtype), c, axis=0)
    return nu, np.concatenate([(ve * rif[:, None]).sum(0), [(rif * rif).sum()]])


def mixed_err(a, b, scale=0.0):
    """max |a - b| relative to the larger of max |b| and `scale`, the size of the sums the formula combines
    (restate's scale: the second moment for the variance, n for the Gini, q and the two quantile pairs for a range).
    Where every draw of a resample is one row the variance pairs are 0 and only the absolute error against that size
    means anything."""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), np.longdouble(scale), np.longdouble(1e-300)))


def bound(E):
    return max(8.0 * E, FLOOR)


# ---- the inputs of tests/test_gpu_rifs.py ---------------------------------------------------------------------------
def straddle(n=513):
    """Tie runs laid across the chunk boundary at row 256 and the sub-tile boundary at row 64."""
    y, x = R.panel(n, 2)
    y = y.copy()
    y[250:262] = y[256]
    y[60:70] = y[64]
    assert np.all(np.diff(y) >= 0)
    return y, x


def straddle_counts(n=513):
    """Counts on both sides of both boundaries, zero elsewhere in the runs; sums to n."""
    c = np.zeros(n, dtype=np.int64)
    c[[254, 255, 256, 257, 261]] = (3, 1, 2, 5, 1)
    c[[62, 63, 64, 69]] = (2, 2, 1, 4)
    c[400] = 200
    rest = n - c.sum()
    c[10], c[500] = rest // 2, rest - rest // 2
    return c


def cases(O, reps=4):
    """(name, y_sorted, x, counts [reps'][n], stats) of the rifs_pass tests. Every y is positive but for the exact
    zeros of `zeros257`."""
    out = []
    for n, p in zip(SIZES, (2, 0, 8, 2, 31)):  # K = 3, 1, 9, 3, 32
        y, x = R.panel(n, p)
        cs = np.vstack([R.stream_counts(O, n, reps), R.hand_counts(n)[None, :]])
        out.append((f"n{n}", y, x if p else None, cs, STATS))
    y, x = R.panel(257, 2, decimals=1)
    out.append(("ties257", y, x, R.stream_counts(O, 257, reps), STATS))
    y, x = straddle()
    out.append(("straddle513", y, x, np.vstack([R.stream_counts(O, 513, reps), straddle_counts()[None, :]]), STATS))
    _, x = R.panel(130, 2)
    out.append(("const130", np.full(130, 3.25), x, R.stream_counts(O, 130, reps), STATS))
    y, x = R.panel(257, 2)
    y = y.copy()
    y[:20] = 0.0
    out.append(("zeros257", y, x, R.stream_counts(O, 257, reps), STATS))
    for _, y, _, cs, _ in out:
        assert np.all(y >= 0) and np.all(cs.sum(1) == len(y))
    return out


def check_ranges(r):
    if r["rq"] is not None:
        R.check_steps(r["rq"])


def restatement_error(O):
    """E per statistic and quantity: the f64 restatement against the longdouble run over every case and replicate,
    and the counts form against rif_stat_ref on the expanded resample (asserted within bound(E))."""
    E = {name: {"nu": 0.0, "gy": 0.0} for name in ("variance", "gini", "iqr")}
    pending = []
    for label, y, x, cs, stats in cases(O):
        for c in cs:
            r64, rld = restate(y, c, stats, x), restate(y, c, stats, x, dtype=np.longdouble)
            check_ranges(r64)
            if r64["rq"] is not None:
                assert r64["rq"]["q"] == rld["rq"]["q"] and r64["rq"]["p"] == rld["rq"]["p"]
            for s, (name, p) in enumerate(stats):
                assert r64["ok"][s] and rld["ok"][s]
                s_nu, s_gy = r64["scale"][s]
                E[name]["nu"] = max(E[name]["nu"], mixed_err(r64["nu"][s], rld["nu"][s], s_nu))
                E[name]["gy"] = max(E[name]["gy"], mixed_err(r64["gy"][s], rld["gy"][s], s_gy))
                nu_e, gy_e = expanded(y, c, name, p, x, np.longdouble)
                pending.append((label, name, mixed_err(r64["nu"][s], nu_e, s_nu), mixed_err(r64["gy"][s], gy_e, s_gy),
                                mixed_err(rld["nu"][s], nu_e, s_nu), mixed_err(rld["gy"][s], gy_e, s_gy)))
    for label, name, e_nu, e_gy, l_nu, l_gy in pending:
        # the identities themselves, in extended precision, then the f64 counts form against the expanded reference
        assert l_nu <= 1e-15 and l_gy <= 1e-15, (label, name, l_nu, l_gy)
        assert e_nu <= bound(E[name]["nu"]) and e_gy <= bound(E[name]["gy"]), (label, name, e_nu, e_gy)
    return E


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "oracle"))
    import oracle

    oracle.build()
    for name, e in restatement_error(oracle).items():
        for key, val in e.items():
            print(f"E[{name}][{key}] = {val:.3e}   bound {bound(val):.3e}")


# ---- the refitted decomposition (ob_builder_prepare_statistics_refit) -----------------------------------------------
def positive_frame(k, n_a=130, n_b=257, seed=5):
    """rifq_ref.frame with the outcome as a wage (exp of the log wage), so that the Gini is defined."""
    f, num, cat = R.frame(k, n_a, n_b, seed)
    f["y"] = np.exp(np.asarray(f["y"]) - 1.0).tolist()
    return f, num, cat


def oracle_row(O, cfg, xa, ya, xb, yb, stat, params, ia=None, ib=None):
    """The refitted row of one (re)sample: rif_stat_ref's RIF of the resampled outcome, O.single_pass on the resampled
    designs, then nu_A, nu_B. xa .. yb are y-sorted; ia / ib index them (None: the sample itself)."""
    xa_, ya_ = (xa, ya) if ia is None else (xa[ia], ya[ia])
    xb_, yb_ = (xb, yb) if ib is None else (xb[ib], yb[ib])
    ra, nua = S.rif_statistic(ya_, stat, **params)
    rb, nub = S.rif_statistic(yb_, stat, **params)
    rc, row = O.single_pass(cfg, xa_, np.ascontiguousarray(ra), None, xb_, np.ascontiguousarray(rb), None)
    return rc, np.concatenate([row, [nua, nub]])


def oracle_boot(O, cfg, xa, ya, xb, yb, stats, seed, first_rep, n_reps):
    """-> rows (S, n_reps, row_len + 2), ok (S, n_reps): OBRS-3 position i of group g is the i-th y-sorted row."""
    rows = np.full((len(stats), n_reps, cfg.row_len + 2), np.nan)
    ok = np.zeros((len(stats), n_reps), dtype=np.uint8)
    for r in range(n_reps):
        ia = O.resample_indices(seed, first_rep + r, 0, len(ya))
        ib = O.resample_indices(seed, first_rep + r, 1, len(yb))
        for t, (stat, params) in enumerate(stats):
            rc, row = oracle_row(O, cfg, xa, ya, xb, yb, stat, params, ia, ib)
            ok[t, r] = 1 if rc == 0 else 0
            rows[t, r] = row
    return rows, ok
