"""numpy f64 restatement of the bootstrapped DFL density decomposition of include/oaxaca_boot.h:
the propensity logit is the reweighted decomposition's (reweight_ref.logit), psi = p / (1 - p) of the clamped p on
B's rows, and the three densities are weighted Gaussian kernel sums on a fixed grid with fixed bandwidths. A replicate
enters through its resample counts (reweight_ref.counts: oracle.resample_indices binned). Shared by
test_density_host.py and test_gpu_density.py."""
import numpy as np

import reweight_ref as R

CURVES = ("density_a", "density_b", "density_counterfactual", "total", "composition", "structure")
MAX_GRID, MAX_K = 256, 32


def row_len(k, G):
    return 6 * G + k + 2


def default_grid(y, G=100):
    """dfl.rs:164-172: g_j = min + j (max - min) / G."""
    lo, hi = float(np.min(y)), float(np.max(y))
    step = (hi - lo) / float(G)
    return np.array([lo + float(j) * step for j in range(G)])


def silverman(y):
    """math/kde.rs:44-59, unweighted."""
    y = np.asarray(y, dtype=np.float64)
    n = float(len(y))
    sd = np.sqrt(np.sum((y - y.sum() / n) ** 2) / (n - 1.0))
    s = np.sort(y)
    iqr = s[int(n * 0.75)] - s[int(n * 0.25)]
    return 0.9 * min(sd, iqr / 1.34) * n ** -0.2


def kernel_sums(y, v, grid, h):
    """sum_i v_i phi((g_j - y_i) / h) per grid point, phi the standard normal density."""
    u = (np.asarray(grid)[None, :] - np.asarray(y)[:, None]) / h
    return (np.asarray(v)[:, None] * (np.exp(-0.5 * u * u) / np.sqrt(2.0 * np.pi))).sum(0)


def decompose(xa, ya, xb, yb, grid, h_a, h_b, wa=None, wb=None, ca=None, cb=None):
    """One pass over (n, K) designs with the intercept as column 0; w the sample weights (None: 1), c the resample
    counts (None: 1) -> (row, norms); row is None for a failed pass."""
    k, G = xa.shape[1], len(grid)
    wa = np.ones(len(ya)) if wa is None else np.asarray(wa, float)
    wb = np.ones(len(yb)) if wb is None else np.asarray(wb, float)
    ca = np.ones(len(ya)) if ca is None else np.asarray(ca, float)
    cb = np.ones(len(yb)) if cb is None else np.asarray(cb, float)
    cwa, cwb = ca * wa, cb * wb
    x = np.vstack([xa, xb])
    d = np.concatenate([np.ones(len(ya)), np.zeros(len(yb))])
    gamma, passes, ok, norms = R.logit(x, d, np.concatenate([cwa, cwb]))
    if not ok or not (cwa.sum() > 0.0 and cwb.sum() > 0.0):
        return None, norms
    p = R.sigmoid_clamped(xb @ gamma)
    psi = p / (1 - p)
    f_a = kernel_sums(ya, cwa, grid, h_a) / (h_a * cwa.sum())
    f_b = kernel_sums(yb, cwb, grid, h_b) / (h_b * cwb.sum())
    f_c = kernel_sums(yb, cwb * psi, grid, h_b) / (h_b * np.sum(cwb * psi))
    ess = np.sum(cwb * psi) ** 2 / np.sum(cb * (wb * psi) ** 2)
    row = np.concatenate([f_a, f_b, f_c, f_a - f_b, f_c - f_b, f_a - f_c, gamma, [ess, float(passes)]])
    assert row.shape == (row_len(k, G),)
    return row, norms


def boot(O, xa, ya, xb, yb, grid, h_a, h_b, wa, wb, seed, first_rep, n_reps):
    """Replicates first_rep .. first_rep + n_reps - 1 -> (rows, ok, step norms per replicate)."""
    rows = np.full((n_reps, row_len(xa.shape[1], len(grid))), np.nan)
    ok = np.zeros(n_reps, dtype=np.uint8)
    all_norms = []
    for r in range(n_reps):
        ca = R.counts(O, seed, first_rep + r, 0, len(ya))
        cb = R.counts(O, seed, first_rep + r, 1, len(yb))
        row, norms = decompose(xa, ya, xb, yb, grid, h_a, h_b, wa, wb, ca, cb)
        all_norms.append(norms)
        if row is not None:
            rows[r], ok[r] = row, 1
    return rows, ok, all_norms


def aggregate(O, point, rows, ok, G):
    """Per curve a dict of (G,) arrays estimate, std_err, p_value, ci_lower, ci_upper, band_lower, band_upper and the
    scalar band_critical, over the replicates kept: O.bootstrap_stats per entry, then the uniform 95 % band from
    t_r = max over the grid points with se > 0 of |v_rj - point_j| / se_j and the ascending-sorted t at index
    min(R - 1, floor(0.95 R))."""
    good = rows[ok.astype(bool)]
    out = {}
    for c, name in enumerate(CURVES):
        pt = np.asarray(point[c * G:(c + 1) * G], dtype=np.float64)
        se, pv, lo, hi = np.empty(G), np.empty(G), np.empty(G), np.empty(G)
        for j in range(G):
            se[j], pv[j], (lo[j], hi[j]) = O.bootstrap_stats(good[:, c * G + j])
        live = se > 0.0
        crit = np.nan
        if len(good) and live.any():
            t = np.sort(np.max(np.abs(good[:, c * G:(c + 1) * G][:, live] - pt[live]) / se[live], axis=1))
            crit = t[min(len(t) - 1, int(np.floor(0.95 * len(t))))]
        band_lo = np.where(live, pt - crit * np.where(live, se, 0.0), pt)
        band_hi = np.where(live, pt + crit * np.where(live, se, 0.0), pt)
        out[name] = {"estimate": pt, "std_err": se, "p_value": pv, "ci_lower": lo, "ci_upper": hi,
                     "band_lower": band_lo, "band_upper": band_hi, "band_critical": float(crit)}
    return out
