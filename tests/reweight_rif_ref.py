"""numpy f64 restatement of the reweighted decomposition of a statistic, from the pieces of
reweight_ref.py and wrif_ref.py: the point logit, psi-hat, the three weighted RIFs (A under w, B under w, C = B
under w psi-hat), and per replicate reweight_ref's decomposition on the replicate's counts with RIF_A, RIF_B and
RIF_C as the outcomes of the three fits. The RIFs are fixed at the point estimate. Shared by
test_gpu_reweight_rif.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reweight_ref as R  # noqa: E402
import rif_stat_ref as U  # noqa: E402
import wrif_ref as W  # noqa: E402

STATS = [("quantile", {"tau": 0.5}), ("variance", {}), ("gini", {}), ("iqr", {"upper": 0.9, "lower": 0.1})]
GINI_OFFSET = 4.0  # added to reweight_ref.panel's outcome for the Gini: y > 0


def panel(k, weighted, stat):
    xa, ya, xb, yb, wa, wb = R.panel(k, weighted)
    if stat == "gini":
        ya, yb = ya + GINI_OFFSET, yb + GINI_OFFSET
        assert ya.min() > 0 and yb.min() > 0
    return xa, ya, xb, yb, wa, wb


def point_logit(xa, xb, wa, wb):
    """-> (gamma-hat, psi-hat over B's rows, the step norms)."""
    wa = np.ones(len(xa)) if wa is None else wa
    wb = np.ones(len(xb)) if wb is None else wb
    x = np.vstack([xa, xb])
    d = np.concatenate([np.ones(len(xa)), np.zeros(len(xb))])
    gamma, passes, ok, norms = R.logit(x, d, np.concatenate([wa, wb]))
    assert ok
    p = R.sigmoid_clamped(xb @ gamma)
    return gamma, p / (1 - p), norms


def rifs(ya, yb, wa, wb, psi, stat, **kw):
    """-> (RIF_A, RIF_B, RIF_C), (nu_A, nu_B, nu_C)."""
    wa = np.ones(len(ya)) if wa is None else wa
    wb = np.ones(len(yb)) if wb is None else wb
    out = [W.rif_statistic(ya, wa, stat, **kw), W.rif_statistic(yb, wb, stat, **kw),
           W.rif_statistic(yb, wb * psi, stat, **kw)]
    return tuple(np.asarray(r[0], dtype=np.float64) for r in out), tuple(float(r[1]) for r in out)


def decompose(xa, ra, xb, rb, rc, wa=None, wb=None, ca=None, cb=None):
    """reweight_ref.decompose with the outcomes RIF_A (fit A), RIF_B (fit B) and RIF_C (fit C) -> (row, norms)."""
    k = xa.shape[1]
    wa = np.ones(len(ra)) if wa is None else np.asarray(wa, float)
    wb = np.ones(len(rb)) if wb is None else np.asarray(wb, float)
    ca = np.ones(len(ra)) if ca is None else np.asarray(ca, float)
    cb = np.ones(len(rb)) if cb is None else np.asarray(cb, float)
    cwa, cwb = ca * wa, cb * wb
    x = np.vstack([xa, xb])
    d = np.concatenate([np.ones(len(ra)), np.zeros(len(rb))])
    gamma, passes, ok, norms = R.logit(x, d, np.concatenate([cwa, cwb]))
    if not ok:
        return None, norms
    p = R.sigmoid_clamped(xb @ gamma)
    psi = p / (1 - p)
    fits = [R.wls(xa, ra, cwa), R.wls(xb, rb, cwb), R.wls(xb, rc, cwb * psi)]
    if any(f is None for f in fits):
        return None, norms
    (ba, ma, ya_m), (bb, mb, yb_m), (bc, mc, yc_m) = fits
    pe, se, pu, re = (mc - mb) * bb, mc * (bc - bb), ma * (ba - bc), (ma - mc) * bc
    ess = np.sum(cwb * psi) ** 2 / np.sum(cb * (wb * psi) ** 2)
    row = np.concatenate([[ya_m - yb_m, mc @ bc - mb @ bb, ma @ ba - mc @ bc, pe.sum(), se.sum(), pu.sum(), re.sum()],
                          pe, se, pu, re, ba, bb, bc, ma, mb, mc, gamma, [ya_m, yb_m, yc_m, ess, float(passes)]])
    assert row.shape == (R.row_len(k),)
    return row, norms


def run(O, k, weighted, stat, kw, seed, first_rep, n_reps):
    """-> (point row, replicate rows, ok, (nu_A, nu_B, nu_C), the logits' step norms)."""
    xa, ya, xb, yb, wa, wb = panel(k, weighted, stat)
    _, psi, pn = point_logit(xa, xb, wa, wb)
    (ra, rb, rc), nu = rifs(ya, yb, wa, wb, psi, stat, **kw)
    point, _ = decompose(xa, ra, xb, rb, rc, wa, wb)
    assert point is not None
    rows = np.full((n_reps, R.row_len(k)), np.nan)
    ok = np.zeros(n_reps, dtype=np.uint8)
    all_norms = [pn]
    for r in range(n_reps):
        ca = R.counts(O, seed, first_rep + r, 0, len(ya))
        cb = R.counts(O, seed, first_rep + r, 1, len(yb))
        row, norms = decompose(xa, ra, xb, rb, rc, wa, wb, ca, cb)
        all_norms.append(norms)
        if row is not None:
            rows[r], ok[r] = row, 1
    return point, rows, ok, nu, all_norms


def quantile_beta_gap(k, tau=0.5):
    """The largest difference, relative to the largest coefficient, between the group coefficients of the two
    restatements of an unweighted quantile RIF regression: wrif_ref at w = 1 (the reweighted path's A and B fits)
    and rif_stat_ref.quantile_rif (decompose_quantile's host RIF)."""
    xa, ya, xb, yb, _, _ = R.panel(k, False)
    worst = 0.0
    for x, y in ((xa, ya), (xb, yb)):
        one = np.ones(len(y))
        b0 = R.wls(x, W.quantile(y, one, tau)[0], one)[0]
        b1 = R.wls(x, U.quantile_rif(y, tau)[0], one)[0]
        worst = max(worst, float(np.max(np.abs(b0 - b1)) / np.max(np.abs(b1))))
    return worst


if __name__ == "__main__":
    for k in (3, 9):
        g = quantile_beta_gap(k)
        print(f"K = {k}: quantile(0.5) coefficients, wrif_ref at w = 1 against rif_stat_ref: {g:.3e} "
              f"(8x = {8 * g:.3e}, floor 1e-9)")
        for weighted in (False, True):
            for stat, kw in STATS:
                xa, ya, xb, yb, wa, wb = panel(k, weighted, stat)
                _, psi, _ = point_logit(xa, xb, wa, wb)
                w_c = (np.ones(len(yb)) if wb is None else wb) * psi
                taus = W.stat_taus(stat, kw)
                if taus:
                    for name, y, w in (("A", ya, wa), ("B", yb, wb), ("C", yb, w_c)):
                        m = W.step_margins(y, np.ones(len(y)) if w is None else w, taus)
                        print(f"  K = {k} weighted = {weighted} {stat} {kw} sample {name}: step margins t {m[0]:.2e} q {m[1]:.2e}")
