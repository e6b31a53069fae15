"""numpy restatement of the distribution-regression decomposition of include/oaxaca_boot.h (Chernozhukov,
Fernandez-Val and Melly 2013): the thresholds, a logit of 1[y <= c_t] per group and threshold by
Newton from 0 with the reweighted decomposition's clamp, Cholesky solve and stopping rule (reweight_ref.logit), the
four distributions, the rearrangement and the interpolated inverse, the effects, the row. A replicate enters
through its resample counts (reweight_ref.counts: oracle.resample_indices binned). The two device pieces have a
restatement in any float type, so that the f64 one can be measured against a longdouble run. Shared by
test_dr_host.py and test_gpu_dr.py."""
import numpy as np

import reweight_ref as R

MAX_T, MAX_Q, MAX_K = 64, 32, 32
EFFECTS = ("total", "composition", "structure")


def row_len(T, nq):
    return 6 * nq + 7 * T + 1


def thresholds(y, n_thresholds=50, lo=0.05, hi=0.95):
    """The sample quantiles of y at evenly spaced levels of [lo, hi] (the interpolation of math/rif.rs), exact
    duplicates removed."""
    s = np.sort(np.asarray(y, dtype=np.float64))
    out = []
    for i in range(n_thresholds):
        level = lo + (hi - lo) * float(i) / float(n_thresholds - 1)
        h = (len(s) - 1.0) * level
        hf, hc = int(np.floor(h)), int(np.ceil(h))
        q = s[hf] if hf == hc else s[hf] + (h - hf) * (s[hc] - s[hf])
        if not out or q != out[-1]:
            out.append(float(q))
    return np.array(out)


def logit_pass(x, y, cw, thr, betas, dtype=np.float64):
    """One pass of the T threshold logits at betas (T, k) -> (info (T, k, k), grad (T, k))."""
    x, y, cw, betas = (np.asarray(a, dtype=dtype) for a in (x, y, cw, betas))
    info, grad = [], []
    for c, b in zip(thr, betas):
        d = (y <= dtype(c)).astype(dtype)
        i, g = R.logit_pass(x, d, cw, b, dtype=dtype)
        info.append(i)
        grad.append(g)
    return np.array(info), np.array(grad)


def cdf_sums(x, cw, betas, dtype=np.float64):
    """-> (sum c w L(x'beta_v) per row of betas, sum c w)."""
    x, cw, betas = (np.asarray(a, dtype=dtype) for a in (x, cw, betas))
    return np.array([np.sum(cw * R.sigmoid_clamped(x @ b)) for b in betas]), np.sum(cw)


def quantiles(f, thr, taus):
    """Rearranges f on the threshold grid and inverts it -> (Q per tau, rearranged f, edge codes 0 / 1 / 2)."""
    s = np.sort(np.asarray(f, dtype=np.float64))
    q, edge = np.empty(len(taus)), np.zeros(len(taus), dtype=np.uint8)
    for i, tau in enumerate(taus):
        at = np.flatnonzero(s >= tau)
        if len(at) == 0:
            q[i], edge[i] = thr[-1], 2
        elif at[0] == 0:
            q[i], edge[i] = thr[0], 1
        else:
            t = at[0]
            q[i] = thr[t - 1] + (tau - s[t - 1]) * (thr[t] - thr[t - 1]) / (s[t] - s[t - 1])
    return q, s, edge


def fit_group(x, y, cw, thr):
    """-> (betas (T, k), passes (T), ok, step norms per threshold)."""
    betas, passes, norms, ok = [], [], [], True
    for c in thr:
        b, p, good, nm = R.logit(x, (y <= c).astype(float), cw)
        betas.append(b)
        passes.append(p)
        norms.append(nm)
        ok = ok and good
    return np.array(betas), np.array(passes), ok, norms


def decompose(xa, ya, xb, yb, thr, taus, wa=None, wb=None, ca=None, cb=None):
    """One pass over (n, K) designs with the intercept as column 0 -> (row, info); row is None for a failed pass.
    info: betas (2, T, K), passes (2, T), step norms of the 2 T fits, the edge codes (3, n_q)."""
    wa = np.ones(len(ya)) if wa is None else np.asarray(wa, float)
    wb = np.ones(len(yb)) if wb is None else np.asarray(wb, float)
    ca = np.ones(len(ya)) if ca is None else np.asarray(ca, float)
    cb = np.ones(len(yb)) if cb is None else np.asarray(cb, float)
    cwa, cwb = ca * wa, cb * wb
    thr, taus = np.asarray(thr, float), np.asarray(taus, float)
    T, nq = len(thr), len(taus)
    ba, pa, oka, na = fit_group(xa, ya, cwa, thr)
    bb, pb, okb, nb = fit_group(xb, yb, cwb, thr)
    info = {"beta": np.array([ba, bb]), "passes": np.array([pa, pb]), "norms": na + nb}
    if not (oka and okb):
        return None, info
    both = np.vstack([ba, bb])
    sa, wsa = cdf_sums(xa, cwa, both)
    sb, wsb = cdf_sums(xb, cwb, both)
    if not (wsa > 0.0 and wsb > 0.0):
        return None, info
    f_aa, f_ab, f_ba, f_bb = sa[:T] / wsa, sa[T:] / wsa, sb[:T] / wsb, sb[T:] / wsb
    (qa, _, ea), (qb, _, eb), (qc, _, ec) = (quantiles(f, thr, taus) for f in (f_aa, f_bb, f_ab))
    info["edge"] = np.array([ea, eb, ec])
    row = np.concatenate([qa - qb, qc - qb, qa - qc, qa, qb, qc, f_aa - f_bb, f_ab - f_bb, f_aa - f_ab,
                          f_aa, f_bb, f_ab, f_ba, [float(max(pa.max(), pb.max()))]])
    assert row.shape == (row_len(T, nq),)
    return row, info


def boot(O, xa, ya, xb, yb, wa, wb, thr, taus, seed, first_rep, n_reps):
    """Replicates first_rep .. first_rep + n_reps - 1 -> (rows, ok, step norms per replicate)."""
    rows = np.full((n_reps, row_len(len(thr), len(taus))), np.nan)
    ok = np.zeros(n_reps, dtype=np.uint8)
    all_norms = []
    for r in range(n_reps):
        ca = R.counts(O, seed, first_rep + r, 0, len(ya))
        cb = R.counts(O, seed, first_rep + r, 1, len(yb))
        row, info = decompose(xa, ya, xb, yb, thr, taus, wa, wb, ca, cb)
        all_norms.append(info["norms"])
        if row is not None:
            rows[r], ok[r] = row, 1
    return rows, ok, all_norms


def aggregate(O, point, rows, ok):
    """(estimate, se, ci_lower, ci_upper) per row entry but the pass count, over the replicates kept."""
    good = rows[ok.astype(bool)]
    out = np.empty((len(point) - 1, 4))
    for j in range(len(point) - 1):
        se, p, (lo, hi) = O.bootstrap_stats(good[:, j])
        out[j] = point[j], se, lo, hi
    return out
