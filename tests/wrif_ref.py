"""References for the weighted RIF pass (ob_rif_stat_weighted), plain numpy.

For a group's outcome y of n rows with weights w >= 0, W = sum w > 0: wt_i = w_i n / W (so sum wt = n). The rows
are ordered by y, stable; W and every sum below run over that order. S_i is the inclusive sum of wt up to the end
of y_i's tie run, F_i = S_i / n, mu = sum wt y / n, and Y(t), 0 < t <= n, is the sorted value at the first position
whose run-end S >= t (the last value when rounding leaves t above the last S).

  variance   RIF_i = (y_i - mu)^2, statistic sum wt (y - mu)^2 / n.
  gini       GL_i = (1/n) sum_{y_j <= y_i} wt_j y_j, R = (1/n) sum wt_i GL_i, G = 1 - 2R/mu,
             RIF_i = 1 + (2R/mu^2) y_i - (2/mu) [y_i (1 - F_i) + GL_i].
  quantile   math/rif.rs:14-88 with every order statistic read through Y: h = (n - 1) tau, lo = floor(h),
             f = h - lo, q = Y(lo + 1) + f (Y(min(lo + 2, n)) - Y(lo + 1)) (Y(lo + 1) itself when f = 0);
             sd = sqrt(sum wt (y - mu)^2 / (n - 1)); quartiles Y(min(max(ceil(p n), 1), n)); the fallbacks
             (iqr <= 1e-8: sd; spread < 1e-8: 1); bandwidth 0.9 spread n^-0.2 with n the row count; density
             sum wt phi((q - y) / bw) / (n bw) with the floor 1e-8; RIF_i = q + (tau - 1[y_i <= q]) / density.
             Statistic q.
  iqr        the difference of two such quantile RIFs on one bandwidth; statistic q_hi - q_lo.

At w = 1 every wt is exactly 1 and these are the unweighted definitions of rif_stat_ref.py.

Every function takes dtype: np.float64 is the reference of the tests, np.longdouble measures it. The index
arithmetic ((n - 1) tau, ceil(p n)) stays in f64 in both, as in the code.

Tolerance. E per statistic = the largest mixed error (rif_stat_ref.mixed_error) of the f64 form against its
longdouble run over inputs() below, measured on x86-64 by `python tests/wrif_ref.py`:
    variance  E = 1.02e-15     gini  E = 4.61e-14     quantile  E = 5.42e-16     iqr  E = 7.84e-16
(gini's is the sequential np.cumsum over 70,001 values), so 8 E = 8.2e-15, 3.7e-13, 4.3e-15 and 6.3e-15, and with
the floor of DESIGN.md §5.10 TOL = 1e-12 for all four.

Y(t) is a step function: a last-bit difference in S can move q to a neighbouring value where some t lies on a
run-end S. step_margins() measures how far the inputs are from that; the seeds below keep every quantile input
clear of it (tests/test_gpu_wrif.py asserts so on the CPU).

The inputs. Weights are lognormal with sigma = 2 (six decades, as psi has), with exact zeros on about 5 % of the
rows and, from n = 64 up, on the rows holding the smallest and the largest y. At n = 3 only the smallest y's
weight is zero and at n = 2 none is, so that W > 0 and the last row carries weight. `constant` has weights that are
small powers of two summing to 2 n: there mu = y exactly, the variance and its RIF are exactly 0, and a comparison
has a meaning; with any other weights (y - mu)^2 is the square of mu's last-bit error in both the reference and the
code. `constant_ln` is the same y under lognormal weights, for every statistic but the variance.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rif_stat_ref as U  # noqa: E402

E_MEASURED = {"variance": 1.02e-15, "gini": 4.61e-14, "quantile": 5.42e-16, "iqr": 7.84e-16}
TOL = {k: max(8 * e, 1e-12) for k, e in E_MEASURED.items()}
SCAN_BLOCK = U.SCAN_BLOCK
TAUS = [0.1, 0.5, 0.9]
IQR_PAIRS = U.IQR_PAIRS
STATS = ([("variance", {}), ("gini", {})] + [("quantile", {"tau": t}) for t in TAUS] +
         [("iqr", {"upper": u, "lower": l}) for u, l in IQR_PAIRS])
mixed_error = U.mixed_error


class Sorted:
    """The sorted view of (y, w) in `dtype` and what every statistic reads from it."""

    def __init__(self, y, w, dtype=np.float64):
        y = np.asarray(y, dtype=np.float64).astype(dtype)
        w = np.asarray(w, dtype=np.float64).astype(dtype)
        self.dtype, self.n = dtype, len(y)
        self.order = np.argsort(y, kind="stable")
        self.y, self.ys, ws = y, y[self.order], w[self.order]
        nf = dtype(self.n)
        self.wt = ws * nf / np.sum(ws)
        self.S = np.cumsum(self.wt)
        self.SY = np.cumsum(self.wt * self.ys)
        self.r = np.searchsorted(self.ys, self.ys, side="right")  # the position after each run's last element
        self.SE = self.S[self.r - 1]  # run-end S per sorted position
        self.mu = np.sum(self.wt * self.ys) / nf
        self.s2 = np.sum(self.wt * (self.ys - self.mu) ** 2)

    def rows(self, v):
        """A vector over the sorted positions -> row order."""
        out = np.empty(self.n, dtype=self.dtype)
        out[self.order] = v
        return out

    def Y(self, t):
        i = int(np.searchsorted(self.SE, self.dtype(t), side="left"))
        return self.ys[min(i, self.n - 1)]


def quantile_ts(n, tau):
    """-> (lo + 1, min(lo + 2, n), f) of h = (n - 1) tau, in f64."""
    h = float(n - 1) * float(tau)
    lo = int(np.floor(h))
    return lo + 1, min(lo + 2, n), h - np.floor(h)


def quartile_ts(n):
    return [min(max(int(np.ceil(p * float(n))), 1), n) for p in (0.75, 0.25)]


def variance(y, w, dtype=np.float64):
    s = Sorted(y, w, dtype)
    return (s.y - s.mu) ** 2, s.s2 / dtype(s.n)


def gini(y, w, dtype=np.float64):
    s = Sorted(y, w, dtype)
    nf = dtype(s.n)
    gl = s.SY[s.r - 1] / nf
    big_r = np.sum(s.wt * gl) / nf
    f = s.SE / nf
    rif = dtype(1) + (dtype(2) * big_r / (s.mu * s.mu)) * s.ys - (dtype(2) / s.mu) * (s.ys * (dtype(1) - f) + gl)
    return s.rows(rif), dtype(1) - dtype(2) * big_r / s.mu


def _bandwidth(s):
    dtype, nf = s.dtype, s.dtype(s.n)
    sd = np.sqrt(s.s2 / (nf - dtype(1)))
    t75, t25 = quartile_ts(s.n)
    iqr = s.Y(t75) - s.Y(t25)
    spread = min(sd, iqr / dtype(1.34)) if iqr > 1e-8 else sd
    if spread < 1e-8:
        spread = dtype(1)
    return dtype(0.9) * spread * nf ** dtype(-0.2)


def _quantile_pieces(s, tau, bw):
    dtype = s.dtype
    t0, t1, f = quantile_ts(s.n, tau)
    q = s.Y(t0)
    if f != 0.0:
        q = q + dtype(f) * (s.Y(t1) - q)
    if dtype is np.float64:
        c = dtype(1.0 / np.sqrt(2.0 * np.pi))
    else:
        c = dtype(1) / np.sqrt(dtype(8) * np.arctan(dtype(1)))
    u = (q - s.ys) / bw
    dens = np.sum(s.wt * (c * np.exp(dtype(-0.5) * (u * u)))) / (dtype(s.n) * bw)
    if dens < 1e-8:
        dens = dtype(1e-8)
    return q, dens


def quantile(y, w, tau, dtype=np.float64):
    s = Sorted(y, w, dtype)
    q, dens = _quantile_pieces(s, tau, _bandwidth(s))
    return q + (dtype(tau) - (s.y <= q).astype(dtype)) / dens, q


def iqr(y, w, upper=0.9, lower=0.1, dtype=np.float64):
    s = Sorted(y, w, dtype)
    bw = _bandwidth(s)
    qh, dh = _quantile_pieces(s, upper, bw)
    ql, dl = _quantile_pieces(s, lower, bw)
    hi = qh + (dtype(upper) - (s.y <= qh).astype(dtype)) / dh
    lo = ql + (dtype(lower) - (s.y <= ql).astype(dtype)) / dl
    return hi - lo, qh - ql


def rif_statistic(y, w, stat, dtype=np.float64, **params):
    if stat == "variance":
        return variance(y, w, dtype)
    if stat == "gini":
        return gini(y, w, dtype)
    if stat == "quantile":
        return quantile(y, w, params["tau"], dtype)
    if stat == "iqr":
        return iqr(y, w, params.get("upper", 0.9), params.get("lower", 0.1), dtype)
    raise ValueError(stat)


def stat_taus(stat, params):
    """The quantiles a statistic reads ([] for the variance and the Gini)."""
    if stat == "quantile":
        return [params["tau"]]
    if stat == "iqr":
        return [params.get("upper", 0.9), params.get("lower", 0.1)]
    return []


def step_margins(y, w, taus):
    """How far a quantile input is from a step of Y -> (m_t, m_q).
    m_t: the least |t - S| / n over the t used (lo + 1, lo + 2 and the two quartile positions) and the run-end
    S, not counting a t that equals S exactly under unit weights (where S is an exact integer) and not counting
    the last run-end at t = n (it is n up to rounding, and Y(n) is the last value on either side of it).
    m_q: the least |q - y_i| / |q| over the y_i that q is not equal to by construction (q is one of the y_i
    exactly when f = 0 or both of its order statistics are one value)."""
    s = Sorted(y, w, np.float64)
    unit = bool(np.all(np.asarray(w) == 1.0))
    se = np.unique(s.SE)
    m_t, m_q = np.inf, np.inf
    ts = set(quartile_ts(s.n))
    for tau in taus:
        t0, t1, f = quantile_ts(s.n, tau)
        ts.add(t0)
        if f != 0.0:
            ts.add(t1)
        q = s.Y(t0) if f == 0.0 else s.Y(t0) + f * (s.Y(t1) - s.Y(t0))
        d = np.abs(s.ys - q)
        if f == 0.0 or s.Y(t0) == s.Y(t1):
            d = d[s.ys != q]
        if len(d):
            m_q = min(m_q, float(np.min(d)) / abs(float(q)) if q != 0 else float(np.min(d)))
    for t in ts:
        d = np.abs(se - float(t))
        keep = np.ones(len(se), dtype=bool)
        if unit:
            keep &= d != 0.0
        if t == s.n:
            keep[-1] = False
        if keep.any():
            m_t = min(m_t, float(np.min(d[keep])) / s.n)
    return m_t, m_q


# ---- the test inputs (shared by tests/test_gpu_wrif.py and the measurement below) ----------------------------
def weights(n, seed, zeros=True):
    rng = np.random.default_rng(seed)
    w = rng.lognormal(0.0, 2.0, n)
    if zeros and n >= 20:
        w[rng.choice(n, max(n // 20, 1), replace=False)] = 0.0
    return w


def inputs(block=SCAN_BLOCK):
    """name -> (y, w)."""
    ys = U.inputs(block)
    out = {}
    for name in ("n2", "n3", "n64", "n257", f"n{block + 1}", "n70001"):
        y = ys[name]
        n = len(y)
        w = weights(n, 900 + n)
        if n >= 64:
            w[np.argmin(y)] = 0.0
            w[np.argmax(y)] = 0.0
        elif n == 3:
            w[np.argmin(y)] = 0.0
        out[name] = (y, w)
    out["ties"] = (ys["ties"], weights(len(ys["ties"]), 31))
    out["straddle"] = (ys["straddle"], weights(block + 1, 32, zeros=False))
    const = ys["constant"]
    out["constant"] = (const, np.tile([1.0, 2.0, 4.0, 1.0], len(const) // 4))  # sum = 2 n
    out["constant_ln"] = (const, weights(len(const), 33))
    out["zeros"] = (ys["zeros"], weights(len(ys["zeros"]), 34))
    return out


def stats_for(name):
    return [(s, kw) for s, kw in STATS if not (name == "constant_ln" and s == "variance")]


def measure(block=SCAN_BLOCK, verbose=True):
    worst = {k: 0.0 for k in E_MEASURED}
    for name, (y, w) in inputs(block).items():
        for stat, params in stats_for(name):
            a = rif_statistic(y, w, stat, np.float64, **params)
            b = rif_statistic(y, w, stat, np.longdouble, **params)
            e = mixed_error(a[0], a[1], b[0], b[1])
            worst[stat] = max(worst[stat], e)
            if verbose:
                print(f"{name:12s} n={len(y):6d} {stat:8s} {params}: E = {e:.3e}")
    return worst


def unit_weight_gap(block=SCAN_BLOCK):
    """The largest mixed difference between this file at w = 1 and rif_stat_ref.py over the latter's inputs."""
    worst = {"variance": 0.0, "gini": 0.0, "iqr": 0.0}
    for name, y in U.inputs(block).items():
        one = np.ones(len(y))
        for stat, params in [("variance", {}), ("gini", {})] + [("iqr", {"upper": u, "lower": l}) for u, l in IQR_PAIRS]:
            a = rif_statistic(y, one, stat, **params)
            b = U.rif_statistic(y, stat, **params)
            worst[stat] = max(worst[stat], mixed_error(a[0], a[1], b[0], b[1]))
    return worst


if __name__ == "__main__":
    w = measure()
    print("E: " + ", ".join(f"{k} = {v:.3e}" for k, v in w.items()))
    print("w = 1 against rif_stat_ref: " + ", ".join(f"{k} = {v:.3e}" for k, v in unit_weight_gap().items()))
    for name, (y, wt) in inputs().items():
        taus = sorted({t for s, kw in STATS for t in stat_taus(s, kw)})
        m_t, m_q = step_margins(y, wt, taus)
        print(f"{name:12s} step margins: t {m_t:.3e} (>= 1e-9), q {m_q:.3e} (>= 1e-9)")
