"""numpy f64 restatement of the Tobit decomposition of include/oaxaca_boot.h: the censored-normal
fit in Olsen's parameters eta = [delta; theta] by the same iteration as the kernels (the least-squares start, the
N_unc terms, the Cholesky step, the halving guard on theta, the stopping rule on the step taken), the conditional
means, the terms of the row. A replicate enters through its resample counts (oracle.resample_indices binned). Only
numpy and the oracle's normal pdf and cdf are used; only the order of the sums differs from the device. Shared by
test_tobit_host.py and test_gpu_tobit.py."""
import numpy as np

MAX_PASSES, TOL, MAX_HALVINGS = 100, 1e-6, 30
GROUP_A, GROUP_B = 0, 1
TAIL = 17
LAMBDA_CUT = -5.0  # below it the restatement's lambda is the continued fraction


def row_len(k):
    return 6 + 7 * k + TAIL


def lam(O, z):
    """phi(z) / Phi(z): the quotient of the oracle's functions down to LAMBDA_CUT, below it Laplace's continued
    fraction of the Mills ratio, Phi(-t) / phi(t) = 1 / (t + 1 / (t + 2 / (t + 3 / ...))), evaluated bottom-up over
    200 terms (at t >= 5 the truncation is far below one ulp)."""
    z = np.asarray(z, dtype=float)
    out = np.empty_like(z)
    hi = z >= LAMBDA_CUT
    out[hi] = O._npdf(z[hi]) / O._ncdf(z[hi])
    t = -z[~hi]
    f = t.copy()
    for j in range(200, 0, -1):
        f = t + j / f
    out[~hi] = f
    return out


def classes(y, lower, upper):
    """0 uncensored, 1 at the lower limit, 2 at the upper limit."""
    cls = np.zeros(len(y), dtype=int)
    if lower is not None:
        cls[y == lower] = 1
    if upper is not None:
        cls[(y == upper) & (cls == 0)] = 2
    return cls


def score_weights(O, x, y, eta, lower, upper):
    """(u, s, h) of every row at eta."""
    k = x.shape[1]
    u = eta[k] * y - x @ eta[:k]
    cls = classes(y, lower, upper)
    s, h = u.copy(), np.ones(len(y))
    le, ri = cls == 1, cls == 2
    ll, lr = lam(O, u[le]), lam(O, -u[ri])
    s[le], h[le] = -ll, ll * (ll + u[le])
    s[ri], h[ri] = lr, lr * (lr - u[ri])
    return u, s, h


def tobit_pass(O, x, y, cw, eta, lower=None, upper=None):
    """One pass at eta -> (-Hessian, gradient, N_unc), the N_unc terms included."""
    k = x.shape[1]
    _, s, h = score_weights(O, x, y, eta, lower, upper)
    v = np.column_stack([x, -y])
    info = (v * (cw * h)[:, None]).T @ v
    grad = v.T @ (cw * s)
    nunc = float(np.sum(cw[classes(y, lower, upper) == 0]))
    info[k, k] += nunc / (eta[k] * eta[k])
    grad[k] += nunc / eta[k]
    return info, grad, nunc


def loglik(O, x, y, cw, eta, lower=None, upper=None):
    k = x.shape[1]
    u = eta[k] * y - x @ eta[:k]
    cls = classes(y, lower, upper)
    ll = np.where(cls == 0, np.log(eta[k]) - 0.5 * u * u - 0.5 * np.log(2 * np.pi), 0.0)
    with np.errstate(divide="ignore"):
        ll = np.where(cls == 1, np.log(O._ncdf(u)), ll)
        ll = np.where(cls == 2, np.log(O._ncdf(-u)), ll)
    return float(np.sum(cw * ll))


def chol_solve(m, b):
    """(l l')^-1 b, or None when m has no Cholesky factor."""
    if not np.isfinite(m).all():
        return None
    try:
        l = np.linalg.cholesky(m)
    except np.linalg.LinAlgError:
        return None
    return np.linalg.solve(l.T, np.linalg.solve(l, b))


def ols_start(x, y, w=None):
    """The point fit's start: (weighted) least squares on all rows, delta = beta / s, theta = 1 / s,
    s^2 = sum w r^2 / sum w."""
    w = np.ones(len(y)) if w is None else np.asarray(w, float)
    beta = chol_solve((x * w[:, None]).T @ x, x.T @ (w * y))
    r = y - x @ beta
    s = np.sqrt(np.sum(w * r * r) / np.sum(w))
    return np.concatenate([beta / s, [1.0 / s]])


def fit(O, x, y, cw, c, eta0, lower=None, upper=None, trace=False):
    """Newton from eta0 -> (eta, passes, ok, norms of the steps taken); with trace also the halvings of every pass
    that reached the guard, as a fifth value. A fit whose uncensored count sum is at most K is dropped before its
    first step (eta0, 0 passes)."""
    k = x.shape[1]
    eta = np.array(eta0, dtype=float)
    norms, halved = [], []

    def result(passes, ok):
        return (eta, passes, ok, norms, halved) if trace else (eta, passes, ok, norms)

    if not np.sum(c[classes(y, lower, upper) == 0]) > k:
        return result(0, False)
    for it in range(MAX_PASSES):
        info, grad, _ = tobit_pass(O, x, y, cw, eta, lower, upper)
        step = chol_solve(info, grad)
        if step is None:
            return result(it + 1, False)
        scale, halvings = 1.0, 0
        while eta[k] + scale * step[k] <= 0.0 and halvings < MAX_HALVINGS:
            scale *= 0.5
            halvings += 1
        halved.append(halvings)
        step = scale * step
        nrm = float(np.sum(step * step))
        if not nrm < np.inf or not eta[k] + step[k] > 0.0:
            return result(it + 1, False)
        eta = eta + step
        norms.append(float(np.sqrt(nrm)))
        if norms[-1] < TOL:
            return result(it + 1, True)
    return result(MAX_PASSES, False)


def score_hp(x, y, cw, eta, lower, upper, digits=40):
    """The relative score of the censored-normal log-likelihood at eta, in mpmath at `digits` digits, written from
    the likelihood in Olsen's parameters and from nothing above: with u = theta y - x'delta a row contributes
    c w (log theta - u^2 / 2) uncensored, c w log Phi(u) at the lower limit and c w log Phi(-u) at the upper one, and
    du / d eta = -v, v = [x, -y]. So g = sum c w s v + (sum of c w over the uncensored rows) / theta e_theta with
    s = u, -phi(u) / Phi(u), phi(u) / Phi(-u). Returns max_j |g_j| / sum c w |s v_j| (the theta component's
    denominator includes its c w / theta terms) as a float: about 1e-16 at a maximiser found in f64, and about the
    relative error of eta elsewhere."""
    import mpmath as mp

    k = x.shape[1]
    with mp.workdps(digits):
        e = [mp.mpf(float(t)) for t in eta]
        theta = e[k]
        g = [mp.mpf(0)] * (k + 1)
        a = [mp.mpf(0)] * (k + 1)
        for i in range(len(y)):
            if cw[i] == 0:
                continue
            c, yi = mp.mpf(float(cw[i])), mp.mpf(float(y[i]))
            v = [mp.mpf(float(t)) for t in x[i]] + [-yi]
            u = -mp.fdot(v, e)
            if lower is not None and y[i] == lower:
                s = -mp.npdf(u) / mp.ncdf(u)
            elif upper is not None and y[i] == upper:
                s = mp.npdf(u) / mp.ncdf(-u)
            else:
                s = u
                g[k] += c / theta
                a[k] += c / theta
            for j in range(k + 1):
                t = c * s * v[j]
                g[j] += t
                a[j] += abs(t)
        return float(max(abs(g[j]) / a[j] for j in range(k + 1) if a[j] != 0))


def cond_mean(O, xb, sg, lower=None, upper=None):
    """E[y | x] of the censored normal at index xb and scale sg, the terms in the kernels' order."""
    pa = Pa = pb = Qb = t = 0.0
    if lower is not None:
        za = (lower - xb) / sg
        pa, Pa = O._npdf(za), O._ncdf(za)
        t = t + lower * Pa
    if upper is not None:
        zb = (upper - xb) / sg
        pb, Qb = O._npdf(zb), O._ncdf(-zb)
        t = t + upper * Qb
    return t + (1.0 - Pa - Qb) * xb + sg * (pa - pb)


def means(O, x, y, cw, etas, lower=None, upper=None):
    """The means pass over one group -> (M under etas[0], M under etas[1], ybar, sum c w, left share, right share,
    xbar)."""
    k = x.shape[1]
    n = np.sum(cw)
    cls = classes(y, lower, upper)
    m = [np.sum(cw * cond_mean(O, x @ (e[:k] / e[k]), 1.0 / e[k], lower, upper)) / n for e in etas]
    return (m[0], m[1], np.sum(cw * y) / n, n, np.sum(cw[cls == 1]) / n, np.sum(cw[cls == 2]) / n,
            (cw[:, None] * x).sum(0) / n)


def decompose(O, xa, ya, xb, yb, wa=None, wb=None, ca=None, cb=None, ref=GROUP_A, lower=None, upper=None, start=None):
    """One pass over (n, K) designs with the intercept as column 0; w the sample weights (None: 1), c the resample
    counts (None: 1), start (2, K + 1) the fits' starts (None: each group's least squares) -> (row, (eta_A, eta_B),
    norms of both fits); row is None for a dropped replicate."""
    k = xa.shape[1]
    wa = np.ones(len(ya)) if wa is None else np.asarray(wa, float)
    wb = np.ones(len(yb)) if wb is None else np.asarray(wb, float)
    ca = np.ones(len(ya)) if ca is None else np.asarray(ca, float)
    cb = np.ones(len(yb)) if cb is None else np.asarray(cb, float)
    cwa, cwb = ca * wa, cb * wb
    if start is None:
        start = (ols_start(xa, ya, wa), ols_start(xb, yb, wb))
    ea, pa, oka, na = fit(O, xa, ya, cwa, ca, start[0], lower, upper)
    eb, pb, okb, nb = fit(O, xb, yb, cwb, cb, start[1], lower, upper)
    if not (oka and okb and np.sum(cwa) > 0.0 and np.sum(cwb) > 0.0):
        return None, (ea, eb), (na, nb)
    maa, mab, ya_m, _, la, ra, xa_m = means(O, xa, ya, cwa, (ea, eb), lower, upper)
    mba, mbb, yb_m, _, lb, rb, xb_m = means(O, xb, yb, cwb, (ea, eb), lower, upper)
    ba, bb, sa, sb = ea[:k] / ea[k], eb[:k] / eb[k], 1.0 / ea[k], 1.0 / eb[k]
    bs = ba if ref == GROUP_A else bb
    mas, mbs = (maa, mba) if ref == GROUP_A else (mab, mbb)
    total, expl = maa - mbb, mas - mbs
    ua, ub = maa - mas, mbs - mbb
    te, ta, tb = (xa_m - xb_m) * bs, xa_m * (ba - bs), xb_m * (bs - bb)
    de, da, db = te.sum(), ta.sum(), tb.sum()
    dex = np.zeros(k) if de == 0.0 else expl * te / de
    dun = (np.zeros(k) if da == 0.0 else ua * ta / da) + (np.zeros(k) if db == 0.0 else ub * tb / db)
    endow, coef = mab - mbb, mba - mbb
    row = np.concatenate([[expl, total - expl, endow, coef, total - endow - coef, total], dex, dun, ba, bb, xa_m, xb_m,
                          bs, [de, da + db, de + (da + db), maa, mab, mba, mbb, ya_m, yb_m, sa, sb, la, ra, lb, rb,
                               float(pa), float(pb)]])
    assert row.shape == (row_len(k),)
    return row, (ea, eb), (na, nb)


def counts(O, seed, rep, g, n):
    return np.bincount(O.resample_indices(seed, rep, g, n), minlength=n)


def boot(O, xa, ya, xb, yb, wa, wb, seed, first_rep, n_reps, start, ref=GROUP_A, lower=None, upper=None):
    """Replicates first_rep .. first_rep + n_reps - 1 from the point fits `start` -> (rows, ok, step norms)."""
    rows = np.full((n_reps, row_len(xa.shape[1])), np.nan)
    ok = np.zeros(n_reps, dtype=np.uint8)
    all_norms = []
    for r in range(n_reps):
        ca = counts(O, seed, first_rep + r, 0, len(ya))
        cb = counts(O, seed, first_rep + r, 1, len(yb))
        row, _, norms = decompose(O, xa, ya, xb, yb, wa, wb, ca, cb, ref, lower, upper, start)
        all_norms.append(norms)
        if row is not None:
            rows[r], ok[r] = row, 1
    return rows, ok, all_norms


def margin_ok(norms):
    """Whether no step norm of a fit lies within a factor 10 of 1e-6, so that rounding cannot decide its pass count."""
    return all(not (TOL / 10 <= v <= TOL * 10) for v in norms)


def panel(k, weighted=False, n_a=130, n_b=257, seed=0):
    """A censored-normal DGP: two groups with shifted covariates and different coefficients and scales, the latent
    outcome moved so that lower = 0 cuts about a quarter of the rows and cut at `upper`, about its ninth decile ->
    xa, ya, xb, yb, wa, wb, lower, upper (intercept in column 0; wa = wb = None when not weighted)."""
    rng = np.random.default_rng(100000 * seed + 10 * k + int(weighted) + 7)
    p = max(k - 1, 1)
    beta = 0.6 / np.sqrt(p) * (-1.0) ** np.arange(k - 1)
    xs, ys = [], []
    for n, shift, c0, sg in ((n_a, 0.3 / np.sqrt(p), 0.25, 1.0), (n_b, 0.0, 0.0, 0.8)):
        x = rng.normal(size=(n, k - 1)) + shift
        ys.append(c0 + x @ (beta * (1.0 + 0.3 * (c0 > 0))) + sg * rng.normal(size=n))
        xs.append(np.column_stack([np.ones(n), x]))
    pooled = np.concatenate(ys)
    off = np.quantile(pooled, 0.25)
    upper = float(np.round(np.quantile(pooled - off, 0.90), 2))
    ya, yb = (np.clip(y - off, 0.0, upper) for y in ys)
    wa = rng.uniform(0.5, 2.0, n_a) if weighted else None
    wb = rng.uniform(0.5, 2.0, n_b) if weighted else None
    return xs[0], ya, xs[1], yb, wa, wb, 0.0, upper
