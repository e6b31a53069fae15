"""References for the jackknife / BCa tests, plain numpy plus the oracle.

1. brute(): delete row i and call oracle.single_pass on what is left. This is the reference's own algorithm
   (run_single_pass on a frame without the row) and the yardstick.
2. closed_form(): the Sherman-Morrison formulas of the device pass in numpy f64:
     t = G_g^-1 x_i, h = w x't, e = y - x'beta_g, beta_g(i) = beta_g - t w e / (1 - h),
     means (S_g - w x) / (W_g - w) (w = 1, W_g = n_g without weights), Pooled: the same update of the pooled
     fit on [x, 1[g = A]] with the indicator's coefficient removed, Weighted: s(i) from W_g - w;
   then decomposition.rs:56-122 with the other group at its point estimate. A row is dropped when 1 - h <=
   2^-40 (Pooled: or 1 - h^P <= 2^-40) or W_g - w <= 0. finish(): accel, jack_se, jack_bias; bca(): the
   interval with statistics.NormalDist. closed_form(deviations=True) gives d = theta_(i) - theta_hat formed from
   the changes themselves, which is what the power sums need (jack_bias multiplies d's mean by m_g - 1);
   dtype=np.longdouble runs the plain form at 64 mantissa bits, to measure the f64 forms against.

Tolerance. E = the largest mixed error max|closed - brute| / max(|brute|, |total_gap|) over the panels of
tests/test_gpu_jackknife.py, measured on x86-64 by `python tests/jackknife_ref.py` (every shape, reference
mode and weighting below, the dummy, single-member and zero-weight panels; the widest panel, p = 118, sets it):
    E = 2.92e-13
The device sums the same f64 terms in another order over at most 120-term dot products; the GPU tests allow
8 E with a floor of 1e-12:
    TOL = 2.336e-12
"""
import math
from statistics import NormalDist

import numpy as np

E_MEASURED = 2.92e-13
TOL = max(8 * E_MEASURED, 1e-12)
TINY = 2.0 ** -40
REFS = {"group_a": 0, "group_b": 1, "pooled": 2, "weighted": 3}


def n_components(k):
    return 6 + 2 * k


def brute(O, ref, xa, ya, wa, xb, yb, wb, rows, n_num=None):
    """theta_(i) for the stacked row indices `rows` (A's rows first) by refitting -> (theta, rc)."""
    k = xa.shape[1] + 1
    cfg = O.PassConfig(k, xa.shape[1] if n_num is None else n_num, ref, wa is not None)
    c = n_components(k)
    xa1, xb1 = O.with_intercept(xa), O.with_intercept(xb)
    out = np.full((len(rows), c), np.nan)
    rcs = np.zeros(len(rows), dtype=int)
    na = len(ya)
    for t, i in enumerate(rows):
        if i < na:
            m = np.arange(na) != i
            rc, row = O.single_pass(cfg, xa1[m], ya[m], None if wa is None else wa[m], xb1, yb, wb)
        else:
            m = np.arange(len(yb)) != i - na
            rc, row = O.single_pass(cfg, xa1, ya, wa, xb1[m], yb[m], None if wb is None else wb[m])
        rcs[t] = rc
        if rc == 0:
            out[t] = row[:c]
    return out, rcs


def point(O, ref, xa, ya, wa, xb, yb, wb, n_num=None):
    k = xa.shape[1] + 1
    cfg = O.PassConfig(k, xa.shape[1] if n_num is None else n_num, ref, wa is not None)
    rc, row = O.single_pass(cfg, O.with_intercept(xa), ya, wa, O.with_intercept(xb), yb, wb)
    assert rc == 0
    return row[: n_components(k)]


def _components(xa, xb, ba, bb, bs, gap):
    """decomposition.rs:56-122 for (n, K) arrays -> (n, 6 + 2K)."""
    dx, db = xa - xb, ba - bb
    dex = dx * bs
    dun = xa * (ba - bs) + xb * (bs - bb)
    expl = dex.sum(1)
    six = np.stack([expl, ((xa * ba).sum(1) - (xb * bb).sum(1)) - expl, (dx * bb).sum(1), (xb * db).sum(1),
                    (dx * db).sum(1), gap], axis=1)
    return np.hstack([six, dex, dun])


def _inv(m):
    """m^-1: numpy's for f64; Gauss-Jordan with partial pivoting in m's own dtype otherwise (longdouble)."""
    if m.dtype == np.float64:
        return np.linalg.inv(m)
    k = m.shape[0]
    a = np.hstack([m.copy(), np.eye(k, dtype=m.dtype)])
    for i in range(k):
        p = i + int(np.argmax(np.abs(a[i:, i])))
        a[[i, p]] = a[[p, i]]
        a[i] = a[i] / a[i, i]
        for r in range(k):
            if r != i:
                a[r] = a[r] - a[r, i] * a[i]
    return a[:, k:]


def closed_form(ref, xa, ya, wa, xb, yb, wb, with_point=False, dtype=np.float64, deviations=False):
    """-> (theta (n_a + n_b, C), kept[, theta_hat]). Numpy f64 throughout. theta_hat is this closed form's own
    point estimate: the deviations d = theta_(i) - theta_hat of a reference are taken from ITS point estimate,
    as the engine takes them from its own (jack_bias multiplies any offset between the two by m_g - 1).
    deviations=True returns d = theta_(i) - theta_hat in place of theta, formed from the changes themselves: with
    u' = u + du, u'v' - uv = du v' + u dv for every product of decomposition.rs:56-122, du being xbar_g(i) - xbar_g
    = w (xbar_g - x_i) / (W_g - w), beta_g(i) - beta_g = -t w e / (1 - h) and the like. theta_(i) - theta_hat taken
    as a difference instead carries the rounding of theta_hat (an ulp of the mean outcome for `unexplained`) into
    every row alike, and jack_bias multiplies that by m_g - 1: measured below, 5e-12 at m = 8,001."""
    xs = [np.hstack([np.ones((len(ya), 1)), xa]).astype(dtype), np.hstack([np.ones((len(yb), 1)), xb]).astype(dtype)]
    ys = [np.asarray(ya, dtype), np.asarray(yb, dtype)]
    ws = [np.ones(len(ya), dtype) if wa is None else np.asarray(wa, dtype),
          np.ones(len(yb), dtype) if wb is None else np.asarray(wb, dtype)]
    k = xs[0].shape[1]
    G = [(x * w[:, None]).T @ x for x, w in zip(xs, ws)]
    r = [(x * w[:, None]).T @ y for x, y, w in zip(xs, ys, ws)]
    Gi = [_inv(g) for g in G]
    beta = [np.linalg.solve(g, v) if dtype == np.float64 else gi @ v for g, gi, v in zip(G, Gi, r)]
    S = [(x * w[:, None]).sum(0) for x, w in zip(xs, ws)]
    W = [s[0] for s in S]  # the intercept's entry: (W - w) / (W - w) is then exactly 1, as on the device
    SY = [(w * y).sum() for w, y in zip(ws, ys)]
    xbar = [s / wt for s, wt in zip(S, W)]
    ybar = [s / wt for s, wt in zip(SY, W)]
    if ref == REFS["pooled"]:
        zs = [np.hstack([xs[0], np.ones((len(ya), 1), dtype)]), np.hstack([xs[1], np.zeros((len(yb), 1), dtype)])]
        P = sum((z * w[:, None]).T @ z for z, w in zip(zs, ws))
        rp = sum((z * w[:, None]).T @ y for z, y, w in zip(zs, ys, ws))
        Pi = _inv(P)
        bp = np.linalg.solve(P, rp) if dtype == np.float64 else Pi @ rp
    theta, kept = [], []
    for g in (0, 1):
        x, y, w = xs[g], ys[g], ws[g]
        n = len(y)
        t = x @ Gi[g]
        h = w * (t * x).sum(1)
        e = y - x @ beta[g]
        om = 1.0 - h
        wm = W[g] - w
        keep = (om > TINY) & (wm > 0.0)
        if deviations:
            r_ = w / wm
            d_x = r_[:, None] * (xbar[g][None, :] - x)   # xbar_g(i) - xbar_g, formed directly
            d_b = -t * (w * e / om)[:, None]             # beta_g(i) - beta_g
            d_y = r_ * (ybar[g] - y)
            zero = np.zeros((n, k), dtype)
            pa, pb = np.broadcast_to(beta[0], (n, k)), np.broadcast_to(beta[1], (n, k))
            qa, qb = np.broadcast_to(xbar[0], (n, k)), np.broadcast_to(xbar[1], (n, k))
            dxa, dxb = (d_x, zero) if g == 0 else (zero, d_x)
            dba, dbb = (d_b, zero) if g == 0 else (zero, d_b)
            if ref == REFS["group_a"]:
                ps, dbs = pa, dba
            elif ref == REFS["group_b"]:
                ps, dbs = pb, dbb
            elif ref == REFS["weighted"]:
                tot = W[0] + W[1]
                w_a = W[0] / tot
                ps = pa * w_a + pb * (1.0 - w_a)
                d_wa = (-w * W[1] if g == 0 else w * W[0]) / ((tot - w) * tot)
                w_own = (W[g] - w) / (tot - w)
                dbs = d_b * w_own[:, None] + (pa - pb) * d_wa[:, None]
            else:
                z = zs[g]
                tp = z @ Pi
                hp = w * (tp * z).sum(1)
                omp = 1.0 - hp
                keep &= omp > TINY
                ps = np.broadcast_to(bp[:k], (n, k))
                dbs = (-tp * (w * (y - z @ bp) / omp)[:, None])[:, :k]
            na_, nb_, ns_ = pa + dba, pb + dbb, ps + dbs   # the values without the row
            pdx, ddx, pdb, ddb = qa - qb, dxa - dxb, pa - pb, dba - dbb
            dex = ddx * ns_ + pdx * dbs
            dun = dxa * (na_ - ns_) + qa * (dba - dbs) + dxb * (ns_ - nb_) + qb * (dbs - dbb)
            d_expl = dex.sum(1)
            six = np.stack([d_expl, ((dxa * na_ + qa * dba).sum(1) - (dxb * nb_ + qb * dbb).sum(1)) - d_expl,
                            (ddx * nb_ + pdx * dbb).sum(1), (dxb * (pdb + ddb) + qb * ddb).sum(1),
                            (ddx * (pdb + ddb) + pdx * ddb).sum(1), d_y if g == 0 else -d_y], axis=1)
            th = np.hstack([six, dex, dun])
            th[~keep] = np.nan
            theta.append(th)
            kept.append(keep)
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            bown = beta[g][None, :] - t * (w * e / om)[:, None]
            xown = (S[g][None, :] - w[:, None] * x) / wm[:, None]
            yown = (SY[g] - w * y) / wm
            both = np.broadcast_to(beta[1 - g], (n, k))
            xoth = np.broadcast_to(xbar[1 - g], (n, k))
            b_a, b_b = (bown, both) if g == 0 else (both, bown)
            x_a, x_b = (xown, xoth) if g == 0 else (xoth, xown)
            gap = yown - ybar[1] if g == 0 else ybar[0] - yown
            if ref == REFS["group_a"]:
                bs = b_a
            elif ref == REFS["group_b"]:
                bs = b_b
            elif ref == REFS["weighted"]:
                sa = W[0] - (w if g == 0 else 0.0)
                sb = W[1] - (w if g == 1 else 0.0)
                wa_ = sa / (sa + sb)
                bs = b_a * np.asarray(wa_)[..., None] + b_b * (1.0 - np.asarray(wa_))[..., None]
            else:
                z = zs[g]
                tp = z @ Pi
                hp = w * (tp * z).sum(1)
                ep = y - z @ bp
                omp = 1.0 - hp
                keep &= omp > TINY
                bs = (bp[None, :] - tp * (w * ep / omp)[:, None])[:, :k]
            th = _components(x_a, x_b, b_a, b_b, bs, gap)
        th[~keep] = np.nan
        theta.append(th)
        kept.append(keep)
    if not with_point:
        return np.vstack(theta), np.concatenate(kept)
    if ref == REFS["group_a"]:
        bs = beta[0]
    elif ref == REFS["group_b"]:
        bs = beta[1]
    elif ref == REFS["weighted"]:
        w_a = W[0] / (W[0] + W[1])
        bs = beta[0] * w_a + beta[1] * (1.0 - w_a)
    else:
        bs = bp[:k]
    hat = _components(xbar[0][None, :], xbar[1][None, :], beta[0][None, :], beta[1][None, :], bs[None, :],
                      np.array([ybar[0] - ybar[1]]))[0]
    return np.vstack(theta), np.concatenate(kept), hat


def power_sums(theta, kept, theta_hat, n_a):
    """-> sums (2, C, 3), n_used (2,) over the kept rows of each group."""
    out = np.zeros((2, theta.shape[1], 3))
    used = [0, 0]
    for g, sl in enumerate((slice(0, n_a), slice(n_a, None))):
        d = theta[sl][kept[sl]] - theta_hat[None, :]
        used[g] = len(d)
        out[g, :, 0], out[g, :, 1], out[g, :, 2] = d.sum(0), (d ** 2).sum(0), (d ** 3).sum(0)
    return out, used


def finish(sums, n_used):
    """accel, jack_se, jack_bias per component from the power sums (the issue's formulas) -> (C, 3)."""
    c = sums.shape[1]
    u2 = np.zeros(c)
    u3 = np.zeros(c)
    se2 = np.zeros(c)
    bias = np.zeros(c)
    for g in (0, 1):
        m = float(n_used[g])
        if m <= 0:
            continue
        dbar = sums[g, :, 0] / m
        g2 = sums[g, :, 1] - m * dbar ** 2
        g3 = -(sums[g, :, 2] - 3 * dbar * sums[g, :, 1] + 2 * m * dbar ** 3)
        u2 += g2
        u3 += g3
        se2 += (m - 1) / m * g2
        bias += (m - 1) * dbar
    den = 6 * np.maximum(u2, 0.0) ** 1.5
    accel = np.where(den > 0, u3 / np.where(den > 0, den, 1.0), 0.0)
    return np.stack([accel, np.sqrt(np.maximum(se2, 0.0)), bias], axis=1)


def finish_direct(theta, kept, n_a):
    """The same three statistics from u_gi = thetabar_g - theta_g(i) directly (no power sums of d)."""
    c = theta.shape[1]
    u2 = np.zeros(c)
    u3 = np.zeros(c)
    se2 = np.zeros(c)
    for sl in (slice(0, n_a), slice(n_a, None)):
        t = theta[sl][kept[sl]]
        m = len(t)
        u = t.mean(0)[None, :] - t
        u2 += (u ** 2).sum(0)
        u3 += (u ** 3).sum(0)
        se2 += (m - 1) / m * (u ** 2).sum(0)
    return u3 / (6 * u2 ** 1.5), np.sqrt(se2)


def bca(values, point_estimate, accel, level=0.95):
    """-> dict(ci_lower, ci_upper, z0, alpha_lo, alpha_hi, flag), with statistics.NormalDist."""
    v = np.sort(np.asarray(values, float))
    n = len(v)
    nan = float("nan")
    out = {"ci_lower": nan, "ci_upper": nan, "z0": nan, "alpha_lo": nan, "alpha_hi": nan, "flag": 0}
    if n == 0:
        out["flag"] = 1
        return out
    p0 = ((v < point_estimate).sum() + 0.5 * (v == point_estimate).sum()) / n
    if p0 <= 0.0 or p0 >= 1.0:
        out["flag"] = 2
        return out
    nd = NormalDist()
    z0 = nd.inv_cdf(p0)
    out["z0"] = z0
    if not math.isfinite(accel):
        out["flag"] = 3
        return out
    ap = []
    for alpha in ((1 - level) / 2, 1 - (1 - level) / 2):
        q = z0 + nd.inv_cdf(alpha)
        if 1 - accel * q <= 0:
            out["flag"] = 4
            return out
        ap.append(nd.cdf(z0 + q / (1 - accel * q)))
    out["alpha_lo"], out["alpha_hi"] = ap
    out["ci_lower"] = v[min(int(math.floor(ap[0] * n)), n - 1)]
    out["ci_upper"] = v[min(int(math.floor(ap[1] * n)), n - 1)]
    return out


def mixed_error(got, ref, gap):
    """max |got - ref| / max(|ref|, |total_gap|)."""
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), abs(gap))))


# ---- the test panels (shared by tests/test_gpu_jackknife.py and the measurement below) ---------------------
def panel(O, n_a, n_b, p, weighted, seed):
    d = O.synthetic_panel(2 * max(n_a, n_b), p, weighted, seed=seed)
    pick = lambda a, n: None if a is None else a[:n]
    return (d["xa"][:n_a], d["ya"][:n_a], pick(d["wa"], n_a), d["xb"][:n_b], d["yb"][:n_b], pick(d["wb"], n_b))


def dummy_panel(O, n_a, n_b, weighted, seed, single_member=False):
    """Two numeric predictors and two dummy columns (n_num = 2). single_member: the first dummy is 1 in exactly
    one row of A (row 7), so the fit without that row is singular."""
    xa, ya, wa, xb, yb, wb = panel(O, n_a, n_b, 2, weighted, seed)
    rng = np.random.default_rng(seed + 1)
    da, db = (rng.random((n_a, 2)) < 0.3).astype(float), (rng.random((n_b, 2)) < 0.3).astype(float)
    if single_member:
        da[:, 0] = 0.0
        da[7, 0] = 1.0
    ya = ya + 0.3 * da[:, 0] - 0.2 * da[:, 1]
    yb = yb + 0.1 * db[:, 0]
    return np.hstack([xa, da]), ya, wa, np.hstack([xb, db]), yb, wb


def zero_weight_panel(O):
    """A WLS panel with one zero-weight row in each group (A's row 5, B's row 9)."""
    xa, ya, wa, xb, yb, wb = panel(O, 37, 53, 2, True, 13)
    wa, wb = wa.copy(), wb.copy()
    wa[5] = 0.0
    wb[9] = 0.0
    return xa, ya, wa, xb, yb, wb


SHAPES = [(37, 53, 2), (37, 53, 16), (400, 417, 118)]


def brute_rows(n_a, n_b, p):
    """All rows, or for the widest panel rows 0, 15, 16, n_g - 1 and 60 more at a fixed stride per group."""
    if p < 100:
        return np.arange(n_a + n_b)
    out = []
    for off, n in ((0, n_a), (n_a, n_b)):
        stride = [i for i in range(3, n, 6) if i not in (15, n - 1)][:60]
        out += [off + i for i in sorted({0, 15, 16, n - 1} | set(stride))]
    return np.array(out)


if __name__ == "__main__":  # the measurement of E
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
    import oracle as O

    O.build()
    worst = 0.0
    cases = [("synthetic", s, panel(O, s[0], s[1], s[2], w, 11 + s[2]), None) for s in SHAPES for w in (False, True)]
    cases += [("dummy", (61, 45, 4), dummy_panel(O, 61, 45, w, 5), 2) for w in (False, True)]
    cases += [("single-member dummy", (61, 45, 4), dummy_panel(O, 61, 45, w, 5, single_member=True), 2)
              for w in (False, True)]
    cases += [("zero weight", (37, 53, 2), zero_weight_panel(O), None)]
    for kind, s, (xa, ya, wa, xb, yb, wb), n_num in cases:
        for name, ref in REFS.items():
            rows = brute_rows(len(ya), len(yb), xa.shape[1])
            bt, rcs = brute(O, ref, xa, ya, wa, xb, yb, wb, rows, n_num)
            cf, kept = closed_form(ref, xa, ya, wa, xb, yb, wb)
            assert ((rcs == 0) == kept[rows]).all()
            rows, bt = rows[rcs == 0], bt[rcs == 0]
            gap = point(O, ref, xa, ya, wa, xb, yb, wb, n_num)[5]
            e = mixed_error(cf[rows], bt, gap)
            worst = max(worst, e)
            print(f"{kind} {s} weighted={wa is not None} {name}: E = {e:.3e}")
    print(f"E = {worst:.3e}")
