"""References for the RIF statistics tests, plain numpy.

For a group's outcome y of n rows, all unweighted: mu = sum(y) / n, r(i) = #{j : y_j <= y_i} (tied rows share
the last rank of their run), p_i = r(i) / n.

  variance   RIF_i = (y_i - mu)^2, statistic sigma^2 = sum (y - mu)^2 / n, mean(RIF) = sigma^2.
  gini       GL_i = (1/n) sum_{y_j <= y_i} y_j, R = (1/n) sum_i GL_i, G = 1 - 2R/mu,
             RIF_i = 1 + (2R/mu^2) y_i - (2/mu) [y_i (1 - p_i) + GL_i]   (Firpo, Fortin, Lemieux 2018);
             on n distinct values mean(RIF) = G + 2/n exactly in real arithmetic.
  iqr        RIF = RIF_hi - RIF_lo, each the quantile RIF of math/rif.rs:14-88: R type-7 quantile q, Silverman
             bandwidth 0.9 min(sd, iqr/1.34) n^-0.2 with the sd over n - 1, the quartiles at the sorted indices
             ceil(p n) - 1, the fallbacks (iqr <= 1e-8: sd; spread < 1e-8: 1), Gaussian density at q with the floor
             1e-8, RIF_i = q + (tau - 1[y_i <= q]) / f(q). Statistic q_hi - q_lo.

Every function takes dtype: np.float64 is the reference of the tests, np.longdouble (64 mantissa bits on x86-64)
measures it. The index arithmetic of the quantile ((n - 1) tau, ceil(p n)) stays in f64 in both, as in the code.

Tolerance. E per statistic = the largest mixed error max|f64 - longdouble| / max(|longdouble|, |statistic|) over
inputs() below, RIF values and the statistic itself, measured on x86-64 by `python tests/rif_stat_ref.py`:
    variance  E = 7.44e-16      gini  E = 2.89e-14      iqr  E = 4.47e-16
(gini's is the sequential np.cumsum over 70,001 values). The device sums the same f64 terms in another order, so
the GPU tests allow 8 E with a floor of 1e-12, the rule of DESIGN.md §5.10: 8 E = 5.95e-15, 2.31e-13 and 3.58e-15, so TOL = 1e-12 for all three.

The indicator term. mean(RIF_tau) = q + (tau - #{y <= q} / n) / f(q), and on distinct values the type-7 quantile
has #{y <= q} = floor((n - 1) tau) + 1, so |tau - #{y <= q} / n| < 1/n and
    |mean(iqr RIF) - (q_hi - q_lo)| <= (1 / f(q_hi) + 1 / f(q_lo)) / n = iqr_identity_bound().
The script prints the measured gap beside that bound for every input of distinct values.
"""
import numpy as np

E_MEASURED = {"variance": 7.44e-16, "gini": 2.89e-14, "iqr": 4.47e-16}
TOL = {k: max(8 * e, 1e-12) for k, e in E_MEASURED.items()}
SCAN_BLOCK = 1024  # elements of a scan block of csrc/ob_rif.hip (ob_rif_scan_block(); the GPU tests pass the library's)
IQR_PAIRS = [(0.9, 0.1), (0.75, 0.25)]


def _prep(y, dtype):
    y = np.asarray(y, dtype=np.float64).astype(dtype)
    s = np.sort(y, kind="stable")
    r = np.searchsorted(s, y, side="right")  # #{j : y_j <= y_i}: the last rank of a tie run
    return y, len(y), s, r


def variance(y, dtype=np.float64):
    y, n, _, _ = _prep(y, dtype)
    mu = np.sum(y) / dtype(n)
    rif = (y - mu) ** 2
    return rif, np.sum(rif) / dtype(n)


def gini(y, dtype=np.float64):
    y, n, s, r = _prep(y, dtype)
    nf = dtype(n)
    mu = np.sum(y) / nf
    gl = np.cumsum(s)[r - 1] / nf
    big_r = np.sum(gl) / nf
    p = r.astype(dtype) / nf
    rif = dtype(1) + (dtype(2) * big_r / (mu * mu)) * y - (dtype(2) / mu) * (y * (dtype(1) - p) + gl)
    return rif, dtype(1) - dtype(2) * big_r / mu


def _bandwidth(y, s, n, dtype):
    nf = dtype(n)
    mu = np.sum(y) / nf
    sd = np.sqrt(np.sum((y - mu) ** 2) / (nf - dtype(1)))
    i75 = max(int(np.ceil(0.75 * float(n))) - 1, 0)
    i25 = max(int(np.ceil(0.25 * float(n))) - 1, 0)
    iqr = s[min(i75, n - 1)] - s[min(i25, n - 1)]
    spread = min(sd, iqr / dtype(1.34)) if iqr > 1e-8 else sd
    if spread < 1e-8:
        spread = dtype(1)
    return dtype(0.9) * spread * nf ** dtype(-0.2)


def _quantile_pieces(y, s, n, tau, bw, dtype):
    h = float(n - 1) * float(tau)
    hf, hc = int(np.floor(h)), int(np.ceil(h))
    q = s[hf] if hf == hc else s[hf] + dtype(h - np.floor(h)) * (s[hc] - s[hf])
    if dtype is np.float64:
        c = dtype(1.0 / np.sqrt(2.0 * np.pi))
    else:
        c = dtype(1) / np.sqrt(dtype(8) * np.arctan(dtype(1)))
    u = (q - y) / bw
    dens = np.sum(c * np.exp(dtype(-0.5) * (u * u))) / (dtype(n) * bw)
    if dens < 1e-8:
        dens = dtype(1e-8)
    return q, dens


def quantile_rif(y, tau, dtype=np.float64):
    """math/rif.rs:14-88 for n >= 2 -> (rif, q, density)."""
    y, n, s, _ = _prep(y, dtype)
    bw = _bandwidth(y, s, n, dtype)
    q, dens = _quantile_pieces(y, s, n, tau, bw, dtype)
    return q + (dtype(tau) - (y <= q).astype(dtype)) / dens, q, dens


def iqr(y, upper=0.9, lower=0.1, dtype=np.float64):
    y, n, s, _ = _prep(y, dtype)
    bw = _bandwidth(y, s, n, dtype)  # one sort and one bandwidth serve both quantiles
    qh, dh = _quantile_pieces(y, s, n, upper, bw, dtype)
    ql, dl = _quantile_pieces(y, s, n, lower, bw, dtype)
    hi = qh + (dtype(upper) - (y <= qh).astype(dtype)) / dh
    lo = ql + (dtype(lower) - (y <= ql).astype(dtype)) / dl
    return hi - lo, qh - ql


def iqr_identity_bound(y, upper=0.9, lower=0.1):
    """(1 / f(q_hi) + 1 / f(q_lo)) / n: what the indicator terms leave of mean(RIF) - (q_hi - q_lo), distinct values."""
    _, _, dh = quantile_rif(y, upper)
    _, _, dl = quantile_rif(y, lower)
    return float((1.0 / dh + 1.0 / dl) / len(y))


def rif_statistic(y, stat, dtype=np.float64, **params):
    if stat == "variance":
        return variance(y, dtype)
    if stat == "gini":
        return gini(y, dtype)
    if stat == "iqr":
        return iqr(y, params.get("upper", 0.9), params.get("lower", 0.1), dtype)
    raise ValueError(stat)


def mixed_error(rif, stat, ref_rif, ref_stat):
    """max over the RIF values and the statistic of |got - ref| / max(|ref|, |statistic|); 0 / 0 counts as 0."""
    d = np.abs(np.append(np.asarray(rif, dtype=np.longdouble), stat) - np.append(ref_rif, ref_stat))
    den = np.maximum(np.abs(np.append(ref_rif, ref_stat)), abs(ref_stat)).astype(np.longdouble)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(d == 0, 0, d / den)
    return float(np.max(e))


# ---- the test inputs (shared by tests/test_gpu_rif_stat.py and the measurement below) ------------------------
def wages(n, seed):
    """Positive, distinct with probability one: log-normal wages."""
    return np.random.default_rng(seed).lognormal(3.0, 0.5, n)


def straddle(block, seed=21):
    """n = block + 1 with a tie run over the sorted positions block - 4 .. block: it crosses the scan-block boundary."""
    s = np.sort(wages(block + 1, seed))
    s[block - 4:] = s[block - 4]
    return np.random.default_rng(seed + 1).permutation(s)


def inputs(block=SCAN_BLOCK):
    rng = np.random.default_rng(7)
    z = wages(500, 19)
    z[rng.choice(500, 50, replace=False)] = 0.0
    out = {f"n{n}": wages(n, 100 + n) for n in (2, 3, 64, 257, block + 1, 70001)}
    out["ties"] = np.round(rng.uniform(-0.49, 9.49, 1000)) + 0.0  # integers in [0, 9], -0.0 folded into 0.0
    out["straddle"] = straddle(block)
    out["constant"] = np.full(300, 3.0)
    out["zeros"] = z
    return out


DISTINCT = ("n2", "n3", "n64", "n257", "n70001")


def measure(block=SCAN_BLOCK, verbose=True):
    worst = {"variance": 0.0, "gini": 0.0, "iqr": 0.0}
    for name, y in inputs(block).items():
        for stat, params in [("variance", {}), ("gini", {})] + [("iqr", {"upper": u, "lower": l}) for u, l in IQR_PAIRS]:
            a = rif_statistic(y, stat, np.float64, **params)
            b = rif_statistic(y, stat, np.longdouble, **params)
            e = mixed_error(a[0], a[1], b[0], b[1])
            worst[stat] = max(worst[stat], e)
            if verbose:
                print(f"{name:10s} n={len(y):6d} {stat:8s} {params}: E = {e:.3e}")
    return worst


if __name__ == "__main__":
    w = measure()
    for name in DISTINCT + (f"n{SCAN_BLOCK + 1}",):
        y = inputs()[name]
        n = len(y)
        v, sv = variance(y, np.longdouble)
        g, sg = gini(y, np.longdouble)
        print(f"{name}: |mean(variance RIF) - sigma^2| / sigma^2 = {float(abs(np.sum(v) / n - sv) / sv):.3e}, "
              f"|mean(gini RIF) - (G + 2/n)| / G = {float(abs(np.sum(g) / n - (sg + np.longdouble(2) / n)) / sg):.3e}")
        for u, l in IQR_PAIRS:
            r, s = iqr(y, u, l)
            print(f"    iqr({u}, {l}): |mean(RIF) - (q_hi - q_lo)| = {abs(float(np.mean(r) - s)):.3e}, "
                  f"bound (1/f_hi + 1/f_lo)/n = {iqr_identity_bound(y, u, l):.3e}")
    print("E: " + ", ".join(f"{k} = {v:.3e}" for k, v in w.items()))
