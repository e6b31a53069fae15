"""numpy f64 restatement of the binary (probit) Oaxaca-Blinder decomposition of include/oaxaca_boot.h
(DESIGN.md §5.13): the probits are oracle.probit, Phi is oracle._ncdf, a replicate's rows are
oracle.resample_indices materialised. Shared by test_binary_host.py and test_gpu_binary.py."""
import numpy as np

GROUP_A, GROUP_B, WEIGHTED, COTTON = 0, 1, 3, 4
REFS = (GROUP_A, GROUP_B, WEIGHTED, COTTON)


def row_len(k):
    return 6 + 7 * k + 8


def pbar(O, x, beta):
    return float(np.mean(O._ncdf(x @ beta)))


def decompose(O, xa, ya, xb, yb, ref):
    """One pass over (n, K) designs with the intercept as column 0 -> (row, converged). row is None when a
    probit cannot solve its Hessian."""
    k = xa.shape[1]
    try:
        fa = O.probit(ya, xa, full=True)
        fb = O.probit(yb, xb, full=True)
    except np.linalg.LinAlgError:
        return None, False
    ba, bb = fa["coefficients"], fb["coefficients"]
    if ref == GROUP_A:
        bs = ba.copy()
    elif ref == GROUP_B:
        bs = bb.copy()
    elif ref in (WEIGHTED, COTTON):
        wa = len(ya) / (len(ya) + len(yb))
        bs = ba * wa + bb * (1.0 - wa)
    else:
        raise ValueError("Pooled / Neumark are outside the binary decomposition's scope")
    paa, pab, pas = pbar(O, xa, ba), pbar(O, xa, bb), pbar(O, xa, bs)
    pba, pbb, pbs = pbar(O, xb, ba), pbar(O, xb, bb), pbar(O, xb, bs)
    total, expl = paa - pbb, pas - pbs
    ua, ub = paa - pas, pbs - pbb
    endow, coef = pab - pbb, pba - pbb
    ma, mb = xa.mean(0), xb.mean(0)

    def share(part, terms):
        den = terms.sum()
        return np.zeros(k) if den == 0.0 else part * terms / den

    dex = share(expl, (ma - mb) * bs)
    dun = share(ua, ma * (ba - bs)) + share(ub, mb * (bs - bb))
    row = np.concatenate([[expl, total - expl, endow, coef, total - endow - coef, total], dex, dun, ba, bb, ma, mb, bs,
                          [paa, pab, pas, pba, pbb, pbs, ya.mean(), yb.mean()]])
    assert row.shape == (row_len(k),)
    return row, bool(fa["converged"] and fb["converged"])


def boot(O, xa, ya, xb, yb, ref, seed, first_rep, n_reps, strict=True):
    """Replicates first_rep .. first_rep + n_reps - 1 -> (rows, ok); asserts that every probit converged. With
    strict=False nothing is asserted and the result is (rows, ok, conv): conv[r] is 1 where both probits of
    replicate r converged; a replicate that ran out of iterations keeps its row and ok = 1, as on the device."""
    rows = np.full((n_reps, row_len(xa.shape[1])), np.nan)
    ok = np.zeros(n_reps, dtype=np.uint8)
    cv = np.zeros(n_reps, dtype=np.uint8)
    for r in range(n_reps):
        ia = O.resample_indices(seed, first_rep + r, 0, len(ya))
        ib = O.resample_indices(seed, first_rep + r, 1, len(yb))
        row, conv = decompose(O, xa[ia], ya[ia], xb[ib], yb[ib], ref)
        if row is not None:
            assert conv or not strict, f"replicate {first_rep + r}: a probit ran out of iterations"
            rows[r], ok[r], cv[r] = row, 1, conv
    return (rows, ok) if strict else (rows, ok, cv)


def counts(O, seed, rep, g, n):
    return np.bincount(O.resample_indices(seed, rep, g, n), minlength=n)


MILD = ((0.3, 0.7), (0.3, 0.7))


def panel(k, n_a=130, n_b=257, seed=7, slope=1.0, x_scale=1.0, c0_shift=(0.0, 0.0), ybar=MILD, planted=()):
    """A probit DGP -> xa, ya, xb, yb (intercept in column 0). By default P(y = 1) lies between 0.3 and 0.7 in both
    groups. slope multiplies the true coefficients and x_scale the covariates (a steep index), c0_shift moves the
    groups' intercepts (lopsided outcomes; ybar holds the band of each group's mean that is asserted), and planted
    rows (x_1, y) overwrite the last rows of each group after that check (their other covariates are 0)."""
    rng = np.random.default_rng(1000 * seed + k)
    p = max(k - 1, 1)
    beta = 0.6 / np.sqrt(p) * (-1.0) ** np.arange(k - 1)
    out = []
    for g, (n, shift, c0, scale) in enumerate(((n_a, 0.25, 0.15, 1.0), (n_b, 0.0, -0.1, 0.8))):
        x = rng.normal(size=(n, k - 1)) + shift * (np.arange(k - 1) % 2 == 0)
        if x_scale != 1.0:
            x = x * x_scale
        y = (c0 + c0_shift[g] + x @ (scale * slope * beta) + rng.normal(size=n) > 0).astype(float)
        assert ybar[g][0] <= y.mean() <= ybar[g][1], (k, n, y.mean())
        for i, (x1, yv) in enumerate(planted):
            x[n - 1 - i] = 0.0
            x[n - 1 - i, 0], y[n - 1 - i] = x1, yv
        out += [np.column_stack([np.ones(n), x]), y]
    return out


# Row counts per width at which every probit of the point fit and of 67 replicates converges (test_binary_host.py).
SIZES = {1: (130, 257), 2: (130, 257), 3: (130, 257), 8: (130, 257), 9: (130, 257), 16: (300, 513), 17: (300, 513),
         32: (600, 1025)}
CLAMP_Z = 6.3613  # |z| beyond which Phi(z) leaves (1e-10, 1 - 1e-10): the probit's clamp
PLANTED = ((40.0, 0.0), (-40.0, 0.0))
LOPSIDED = ((0.02, 0.06), (0.94, 0.98))
STEEP_SLOPE, STEEP_X = 3.0, 2.5  # x_1's true coefficient 1.27 on x ~ 2.5 N(0, 1): 12 and 23 rows beyond the clamp
LOPSIDED_SHIFT, LOPSIDED_SIZES = (-2.4, 2.0), (257, 513)  # 10 ones among A's rows, 13 zeros among B's


def sized_panel(k):
    return panel(k, *SIZES[k])


def steep_panel(k=3):
    """Fitted indices beyond the clamp in both groups at the point fit and in most resamples."""
    return panel(k, slope=STEEP_SLOPE, x_scale=STEEP_X)


def outlier_panel(k=3):
    """(x_1 = 40, y = 0) and (x_1 = -40, y = 0) as the last two rows of each group of the steep panel. On the mild
    panel the two rows hold x_1's coefficient near 0 (they sit at z = -0.1 and 0.7) and lie beyond the clamp at no
    slope or covariate scale below the steep panel's; there the point fit leaves them at z = -+40. A resample that
    draws them unevenly can oscillate for its 100 iterations: OUTLIER_UNCONVERGED lists those replicates."""
    return panel(k, slope=STEEP_SLOPE, x_scale=STEEP_X, planted=PLANTED)


# replicates (seed 0x0B5EED, 0 .. 66) in which a probit of the restatement runs its 100 iterations
OUTLIER_UNCONVERGED = (5, 8, 10, 17, 19, 21, 22, 27, 29, 31, 32, 39, 40, 42, 47, 52, 55, 58, 59, 65, 66)
K16_SMALL_UNCONVERGED = (33, 59)  # K = 16 at 130 / 257 rows


def lopsided_panel(k=3):
    """P(y = 1) within 0.02 .. 0.06 in group A and 0.94 .. 0.98 in group B."""
    return panel(k, *LOPSIDED_SIZES, c0_shift=LOPSIDED_SHIFT, ybar=LOPSIDED)


def clamped_rows(x, beta, w=None):
    """Counted rows of x whose index under beta lies beyond the probit's clamp."""
    z = np.abs(x @ beta) > CLAMP_Z
    return int(z.sum() if w is None else (z & (w > 0)).sum())


def phi_hp(x, betas, digits=50):
    """Phi(x_i'beta) for every row and every beta in mpmath at `digits` digits (the index in mpmath too, from the
    f64 inputs taken exactly) -> n lists of len(betas) mpf values. Compute it once per design; means_hp weights it."""
    import mpmath as mp

    with mp.workdps(digits):
        bs = [[mp.mpf(float(t)) for t in b] for b in betas]
        return [[mp.ncdf(mp.fdot([mp.mpf(float(t)) for t in xi], b)) for b in bs] for xi in x]


def means_hp(phis, w=None, digits=50):
    """The count-weighted means of phi_hp's values, summed in mpmath, rounded to f64 once at the end."""
    import mpmath as mp

    w = np.ones(len(phis), dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64)
    with mp.workdps(digits):
        acc = [mp.mpf(0)] * len(phis[0])
        for i in np.flatnonzero(w):
            for v, ph in enumerate(phis[i]):
                acc[v] += int(w[i]) * ph
        return np.array([float(a / int(w.sum())) for a in acc])


def phi_fsum(x, betas):
    """phi_hp's values from math.erfc over math.fsum of the index's f64 products: n lists of floats within a few ulp
    of phi_hp's (test_binary_host.py measures it). For designs of tens of thousands of rows, where 10^5 mpmath
    cdfs would take ten seconds; means_fsum adds them without rounding."""
    import math

    r2 = math.sqrt(2.0)
    return [[0.5 * math.erfc(-math.fsum(float(a) * float(c) for a, c in zip(xi, b)) / r2) for b in betas] for xi in x]


def means_fsum(phis, w=None):
    import math

    w = np.ones(len(phis), dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64)
    idx = np.flatnonzero(w)
    return np.array([math.fsum(float(w[i]) * phis[i][v] for i in idx) / float(w.sum()) for v in range(len(phis[0]))])


def case_panel(case):
    """A width (its SIZES panel) or the name of a hard panel -> xa, ya, xb, yb."""
    if isinstance(case, int):
        return sized_panel(case)
    return {"steep": steep_panel, "outliers": outlier_panel, "lopsided": lopsided_panel,
            "k16_small": lambda: panel(16)}[case]()


_case_rows = {}


def case_rows(O, case, ref, seed, reps):
    """The restatement's (point row, point converged, replicate rows, ok, conv) of a case, computed once and shared
    by the host and the GPU tests (read-only). Nothing is asserted here: the tests state what each case must show."""
    key = (case, ref, seed, reps)
    if key not in _case_rows:
        p = case_panel(case)
        point, conv = decompose(O, *p, ref)
        rows, ok, cv = boot(O, *p, ref, seed, 0, reps, strict=False)
        for a in (point, rows, ok, cv):
            a.setflags(write=False)
        _case_rows[key] = (point, conv, rows, ok, cv)
    return _case_rows[key]
