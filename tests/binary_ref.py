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


def boot(O, xa, ya, xb, yb, ref, seed, first_rep, n_reps):
    """Replicates first_rep .. first_rep + n_reps - 1 -> (rows, ok); asserts that every probit converged."""
    rows = np.full((n_reps, row_len(xa.shape[1])), np.nan)
    ok = np.zeros(n_reps, dtype=np.uint8)
    for r in range(n_reps):
        ia = O.resample_indices(seed, first_rep + r, 0, len(ya))
        ib = O.resample_indices(seed, first_rep + r, 1, len(yb))
        row, conv = decompose(O, xa[ia], ya[ia], xb[ib], yb[ib], ref)
        if row is not None:
            assert conv, f"replicate {first_rep + r}: a probit ran out of iterations"
            rows[r], ok[r] = row, 1
    return rows, ok


def counts(O, seed, rep, g, n):
    return np.bincount(O.resample_indices(seed, rep, g, n), minlength=n)


def panel(k, n_a=130, n_b=257, seed=7):
    """A probit DGP with P(y = 1) between 0.3 and 0.7 in both groups -> xa, ya, xb, yb (intercept in column 0)."""
    rng = np.random.default_rng(1000 * seed + k)
    p = max(k - 1, 1)
    beta = 0.6 / np.sqrt(p) * (-1.0) ** np.arange(k - 1)
    out = []
    for n, shift, c0, scale in ((n_a, 0.25, 0.15, 1.0), (n_b, 0.0, -0.1, 0.8)):
        x = rng.normal(size=(n, k - 1)) + shift * (np.arange(k - 1) % 2 == 0)
        y = (c0 + x @ (scale * beta) + rng.normal(size=n) > 0).astype(float)
        assert 0.3 <= y.mean() <= 0.7, (k, n, y.mean())
        out += [np.column_stack([np.ones(n), x]), y]
    return out
