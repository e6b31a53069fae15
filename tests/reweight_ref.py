"""numpy f64 restatement of the reweighted Oaxaca-Blinder decomposition of include/oaxaca_boot.h (DESIGN.md
§5.14): the propensity logit is math/logit.rs:31-118 with a factor c w on every row's term, the three fits are
(W)LS by the Cholesky factor of the Gram, a replicate enters through its resample counts
(oracle.resample_indices binned). The two device pieces have a restatement in any float type, so that the f64
one can be measured against a longdouble run. Shared by test_reweight_host.py and test_gpu_reweight.py."""
import numpy as np

AGG = ("total_gap", "composition", "structure", "pure_explained", "specification_error", "pure_unexplained",
       "reweighting_error")
MAX_PASSES, TOL = 100, 1e-6
LO, HI = 1e-10, 1.0 - 1e-10


def row_len(k):
    return 7 + 11 * k + 5


def sigmoid_clamped(z):
    with np.errstate(over="ignore"):
        return np.clip(1.0 / (1.0 + np.exp(-z)), z.dtype.type(LO), z.dtype.type(HI))


def logit_pass(x, d, cw, gamma, dtype=np.float64):
    """One pass at gamma -> (information matrix sum c w p (1 - p) x x', gradient sum c w (d - p) x)."""
    x, d, cw, gamma = (np.asarray(a, dtype=dtype) for a in (x, d, cw, gamma))
    p = sigmoid_clamped(x @ gamma)
    return (x * (cw * (p * (1 - p)))[:, None]).T @ x, x.T @ (cw * (d - p))


def psi_gram(x, y, cw, w, c, gamma, dtype=np.float64):
    """The psi-weighted extended Gram of v = [x, y] and sum c (w psi)^2, psi = p / (1 - p) of the clamped p."""
    x, y, cw, w, c, gamma = (np.asarray(a, dtype=dtype) for a in (x, y, cw, w, c, gamma))
    p = sigmoid_clamped(x @ gamma)
    psi = p / (1 - p)
    v = np.column_stack([x, y])
    return (v * (cw * psi)[:, None]).T @ v, np.sum(c * (w * psi) ** 2)


def chol_solve(m, b):
    """(l l')^-1 b, or None when m has no Cholesky factor."""
    if not np.isfinite(m).all():
        return None
    try:
        l = np.linalg.cholesky(m)
    except np.linalg.LinAlgError:
        return None
    return np.linalg.solve(l.T, np.linalg.solve(l, b))


def logit(x, d, cw, gamma0=None):
    """Newton from 0 -> (gamma, passes, ok, step norms). ok is False where the information matrix has no
    Cholesky factor or the step norm stays at or above 1e-6 for 100 passes."""
    gamma = np.zeros(x.shape[1]) if gamma0 is None else np.array(gamma0, dtype=float)
    norms = []
    for it in range(MAX_PASSES):
        info, grad = logit_pass(x, d, cw, gamma)
        step = chol_solve(info, grad)
        if step is None:
            return gamma, it + 1, False, norms
        gamma = gamma + step
        norms.append(float(np.sqrt(np.sum(step * step))))
        if norms[-1] < TOL:
            return gamma, it + 1, True, norms
    return gamma, MAX_PASSES, False, norms


def wls(x, y, w):
    """-> (beta, xbar, ybar) with weights w, or None when the Gram has no Cholesky factor."""
    s = np.sum(w)
    if not s > 0.0:
        return None
    beta = chol_solve((x * w[:, None]).T @ x, x.T @ (w * y))
    return None if beta is None else (beta, (w[:, None] * x).sum(0) / s, np.sum(w * y) / s)


def decompose(xa, ya, xb, yb, wa=None, wb=None, ca=None, cb=None, force_gamma=None):
    """One pass over (n, K) designs with the intercept as column 0; w the sample weights (None: 1), c the
    resample counts (None: 1) -> (row, norms); row is None for a failed pass. force_gamma skips the logit."""
    k = xa.shape[1]
    wa = np.ones(len(ya)) if wa is None else np.asarray(wa, float)
    wb = np.ones(len(yb)) if wb is None else np.asarray(wb, float)
    ca = np.ones(len(ya)) if ca is None else np.asarray(ca, float)
    cb = np.ones(len(yb)) if cb is None else np.asarray(cb, float)
    cwa, cwb = ca * wa, cb * wb
    if force_gamma is None:
        x = np.vstack([xa, xb])
        d = np.concatenate([np.ones(len(ya)), np.zeros(len(yb))])
        gamma, passes, ok, norms = logit(x, d, np.concatenate([cwa, cwb]))
        if not ok:
            return None, norms
    else:
        gamma, passes, norms = np.asarray(force_gamma, float), 0, []
    p = sigmoid_clamped(xb @ gamma)
    psi = p / (1 - p)
    fits = [wls(xa, ya, cwa), wls(xb, yb, cwb), wls(xb, yb, cwb * psi)]
    if any(f is None for f in fits):
        return None, norms
    (ba, ma, ya_m), (bb, mb, yb_m), (bc, mc, yc_m) = fits
    pe, se, pu, re = (mc - mb) * bb, mc * (bc - bb), ma * (ba - bc), (ma - mc) * bc
    ess = np.sum(cwb * psi) ** 2 / np.sum(cb * (wb * psi) ** 2)
    row = np.concatenate([[ya_m - yb_m, mc @ bc - mb @ bb, ma @ ba - mc @ bc, pe.sum(), se.sum(), pu.sum(), re.sum()],
                          pe, se, pu, re, ba, bb, bc, ma, mb, mc, gamma, [ya_m, yb_m, yc_m, ess, float(passes)]])
    assert row.shape == (row_len(k),)
    return row, norms


def counts(O, seed, rep, g, n):
    return np.bincount(O.resample_indices(seed, rep, g, n), minlength=n)


def boot(O, xa, ya, xb, yb, wa, wb, seed, first_rep, n_reps):
    """Replicates first_rep .. first_rep + n_reps - 1 -> (rows, ok, step norms per replicate)."""
    rows = np.full((n_reps, row_len(xa.shape[1])), np.nan)
    ok = np.zeros(n_reps, dtype=np.uint8)
    all_norms = []
    for r in range(n_reps):
        ca = counts(O, seed, first_rep + r, 0, len(ya))
        cb = counts(O, seed, first_rep + r, 1, len(yb))
        row, norms = decompose(xa, ya, xb, yb, wa, wb, ca, cb)
        all_norms.append(norms)
        if row is not None:
            rows[r], ok[r] = row, 1
    return rows, ok, all_norms


def margin_ok(norms, max_passes=25):
    """Whether a logit converged within max_passes with no step norm within a factor 10 of 1e-6, so that rounding
    can decide neither its pass count nor its ok."""
    return (len(norms) <= max_passes and norms[-1] < TOL / 10 and
            all(not (TOL / 10 <= v <= TOL * 10) for v in norms))


def panel(k, weighted=False, n_a=130, n_b=257, seed=0):
    """Two groups with shifted covariates, a linear outcome in A and a mildly curved one in B -> xa, ya, xb, yb,
    wa, wb (intercept in column 0; wa = wb = None when not weighted). The shift of 0.6 / sqrt(K - 1) per column is
    the one of a CPU scan over 0 .. 2.5 that leaves the fewest replicates with a step norm near 1e-6 (margin_ok)."""
    rng = np.random.default_rng(100000 * seed + 10 * k + int(weighted))
    p = max(k - 1, 1)
    beta = 0.5 / np.sqrt(p) * (-1.0) ** np.arange(k - 1)
    out = []
    for n, shift, c0 in ((n_a, 0.6 / np.sqrt(p), 0.4), (n_b, 0.0, 0.0)):
        x = rng.normal(size=(n, k - 1)) + shift
        y = 2.0 + c0 + x @ beta + (0.15 * x[:, 0] ** 2 if c0 == 0.0 and k > 1 else 0.0) + 0.5 * rng.normal(size=n)
        out += [np.column_stack([np.ones(n), x]), y]
    xa, ya, xb, yb = out
    wa = rng.uniform(0.5, 2.0, n_a) if weighted else None
    wb = rng.uniform(0.5, 2.0, n_b) if weighted else None
    return xa, ya, xb, yb, wa, wb
