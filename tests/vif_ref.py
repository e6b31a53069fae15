"""NumPy restatement of the reference's calculate_vif (math/diagnostics.rs:29-109 over math/ols.rs:44-144),
for the VIF tests. `dtype` is float64 or longdouble; the f64 solve is oracle._chol_solve_nalgebra.

For predictors x_0..x_{K-1}, in the order given: fewer than two is a DiagnosticError; for each j the
regressand is x_j and the design Z = [x_c for c != j, then the intercept LAST]; n <= K is
InsufficientData; a failed Cholesky of Z'Z is a NalgebraError that ends the whole call; residuals are
formed row by row; ss_tot == 0 scores +inf; else r2 = 1 - ss_res / ss_tot and the score is +inf when
|1 - r2| < 1e-9, else 1 / (1 - r2).

All K fits read one extended Gram G = Xe'Xe, Xe = [x_0..x_{K-1}, 1]: Z'Z and Z'y of fit j are its rows
and columns in Z's order, which is what the engine does, and algebraically what ols() forms per fit.

Rounding bars of tests/test_gpu_vif.py, u = 2^-53, first order, valid for any summation order (a sum of m
products carries at most m u times the sum of the magnitudes):
  gram   |G - G*|_ab          <= n u (|Xe|'|Xe|)_ab
  sums   |ss_res - ss_res*|_j <= 2 (K + 2) u sum_i |r_ij| rho_ij + (n + 1) u sum_i r_ij^2,
                                 rho_ij = |x_ij| + sum_c |xe_ic| |B_cj|  (the residual's own dot product)
         |ss_tot - ss_tot*|_j <= (n + 3) u ss_tot_j
  vif    relative             <= [(2 n + 4) + 2 (K + 2) S_j + 4 + 2 vif_j] u + cond^3 ((n + K + 2) u)^2
         with S_j = sum_i |r_ij| rho_ij / sum_i r_ij^2 at the exact coefficients. The sums are stationary
         in the coefficients and in the mean (the residual is orthogonal to Z, the deviations sum to 0), so
         the Gram's and the solve's rounding enters at second order only: ||Z db||^2 / ss_res <= cond
         (cond e)^2 with e = (n + K + 2) u the relative perturbation of the normal equations. The last
         term of the bracket is the final 1 - ss_res / ss_tot and 1 / (1 - r2).
  From n, K and cond alone: S_j <= sqrt((K + 1) cond) (Cauchy-Schwarz, ||r||^2 >= lambda_min ||b||^2,
  sum rho^2 <= trace(G) ||b||^2) and vif_j <= cond, which is vif_bar_bound()."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
from oracle import _chol_solve_nalgebra  # noqa: E402

U = 2.0 ** -53
LD = np.longdouble

MSG_TOO_FEW = "VIF calculation requires at least two predictors."
MSG_CHOLESKY = ("Failed to perform Cholesky decomposition. Matrix may be singular or not positive definite due to "
                "multicollinearity.")


class VifRefError(Exception):
    def __init__(self, kind, msg, partial=None):
        super().__init__(msg)
        self.kind = kind          # "diagnostic" | "insufficient" | "linalg"
        self.partial = partial    # the scores of the fits before the failing one


def fixture(n, k, seed):
    """The correlated design of the GPU tests: VIFs between 1.2 and 16, cond(G) <= 4e4."""
    rng = np.random.default_rng(seed)
    f = rng.normal(size=(n, 4))
    return rng.normal(size=(n, k)) + f @ rng.normal(size=(4, k)) + rng.uniform(-2, 2, k)


def threshold_case(n=1000):
    """K = 2 with x2 = x1 + 1e-6 e: 1 - r2 is about 1e-12, two orders under the 1e-9 rule."""
    rng = np.random.default_rng(29)
    x1, e = rng.normal(size=n), rng.normal(size=n)
    return np.stack([x1, x1 + 1e-6 * e], axis=1)


def extended(x, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    return np.concatenate([x, np.ones((x.shape[0], 1), dtype=dtype)], axis=1)


def gram(x, dtype=np.float64):
    xe = extended(x, dtype)
    return xe.T @ xe


def _chol_solve(m, b, dtype):
    """nalgebra's Cholesky::new + solve: oracle._chol_solve_nalgebra in f64; in a wider dtype the same
    factorisation with each column's updates as one product (the order of a 64-bit-mantissa run is
    immaterial at the bars' scale)."""
    if dtype == np.float64:
        return _chol_solve_nalgebra(m, b)
    k = m.shape[0]
    a = np.array(m, dtype=dtype, order="F")
    for j in range(k):
        a[j:, j] -= a[j:, :j] @ a[j, :j]
        d = a[j, j]
        if not (d != 0.0 and d >= 0.0):
            return None
        a[j, j] = np.sqrt(d)
        a[j + 1:, j] /= a[j, j]
    x = np.array(b, dtype=dtype)
    for i in range(k):
        x[i] = x[i] / a[i, i]
        x[i + 1:] -= x[i] * a[i + 1:, i]
    for i in range(k - 1, -1, -1):
        x[i] = (x[i] - a[i + 1:, i] @ x[i + 1:]) / a[i, i]
    return x


def order(j, k):
    """Z's columns as positions of Xe: the other predictors in the given order, the intercept last."""
    return [c for c in range(k) if c != j] + [k]


def solve(g, n, k, dtype=np.float64):
    """The (K + 1) x K coefficient matrix: column j is fit j's beta scattered to Xe's positions, B[j][j] = 0."""
    if k < 2:
        raise VifRefError("diagnostic", MSG_TOO_FEW)
    if n <= k:
        raise VifRefError("insufficient", f"n_obs ({n}) must be strictly greater than k ({k})")
    g = np.asarray(g, dtype=dtype)
    b = np.zeros((k + 1, k), dtype=dtype)
    for j in range(k):
        idx = order(j, k)
        beta = _chol_solve(g[np.ix_(idx, idx)], g[idx, j], dtype)
        if beta is None:
            raise VifRefError("linalg", MSG_CHOLESKY, partial=j)
        b[idx, j] = beta
    return b


def sums(x, b, means, dtype=np.float64):
    """(ss_res, ss_tot) of every fit from explicit residuals, row by row as ols.rs does."""
    xe = extended(x, dtype)
    k = xe.shape[1] - 1
    r = xe[:, :k] - xe @ np.asarray(b, dtype=dtype)
    d = xe[:, :k] - np.asarray(means, dtype=dtype)[None, :]
    return np.sum(r * r, axis=0), np.sum(d * d, axis=0)


def scores(ss_res, ss_tot):
    out = np.empty(len(ss_res))
    for j, (a, t) in enumerate(zip(ss_res, ss_tot)):
        if t == 0.0:
            out[j] = np.inf
            continue
        one_minus = 1.0 - (1.0 - a / t)
        out[j] = np.inf if abs(one_minus) < 1e-9 else float(1.0 / one_minus)
    return out


def vif(x, dtype=np.float64, parts=False):
    """The scores of every predictor; raises VifRefError as the reference returns its errors. On a
    Cholesky failure the error's `partial` holds the scores of the fits before it."""
    x = np.asarray(x, dtype=dtype)
    n, k = x.shape
    if k < 2:
        raise VifRefError("diagnostic", MSG_TOO_FEW)
    g = gram(x, dtype)
    means = g[:k, k] / dtype(n) if n else np.zeros(k, dtype=dtype)
    try:
        b = solve(g, n, k, dtype)
    except VifRefError as e:
        if e.kind == "linalg":  # the fits before the failing one, as the reference would have pushed them
            jf = e.partial
            bp = np.zeros((k + 1, k), dtype=dtype)
            for j in range(jf):
                idx = order(j, k)
                bp[idx, j] = _chol_solve(g[np.ix_(idx, idx)], g[idx, j], dtype)
            a, t = sums(x, bp, means, dtype)
            e.partial = scores(a[:jf], t[:jf])
        raise
    a, t = sums(x, b, means, dtype)
    s = scores(a, t)
    return (s, g, b, means, a, t) if parts else s


def one_minus_r2(x, dtype=LD):
    """1 - r2 of every fit (no threshold), for the test that pins the 1e-9 rule away from rounding."""
    _, _, _, _, a, t = vif(x, dtype, parts=True)
    return a / t


# ---- bars ------------------------------------------------------------------------------------------------

def gram_bar(x):
    xe = np.abs(extended(x, LD))
    return x.shape[0] * U * (xe.T @ xe)


def sums_bar(x, b, ss_res, ss_tot):
    """The two sums' bars at coefficients b (held in longdouble)."""
    xe = extended(x, LD)
    n, k = x.shape
    b = np.asarray(b, dtype=LD)
    r = xe[:, :k] - xe @ b
    rho = np.abs(xe[:, :k]) + np.abs(xe) @ np.abs(b)
    res = 2 * (k + 2) * U * np.sum(np.abs(r) * rho, axis=0) + (n + 1) * U * np.sum(r * r, axis=0)
    return res, (n + 3) * U * np.asarray(ss_tot, dtype=LD)


def vif_bar(x, cond, s, b, a):
    """Relative bar of every score, from the longdouble run's scores, coefficients and ss_res."""
    n, k = x.shape
    xe = extended(x, LD)
    r = xe[:, :k] - xe @ b
    rho = np.abs(xe[:, :k]) + np.abs(xe) @ np.abs(b)
    big_s = np.sum(np.abs(r) * rho, axis=0) / a
    return ((2 * n + 4) + 2 * (k + 2) * big_s + 4 + 2 * s) * U + cond ** 3 * ((n + k + 2) * U) ** 2


def vif_bar_bound(n, k, cond):
    """An upper bound of vif_bar from the shape and the Gram's condition number alone."""
    return ((2 * n + 8) + 2 * (k + 2) * np.sqrt((k + 1) * cond) + 2 * cond) * U + cond ** 3 * ((n + k + 2) * U) ** 2


def solve_sequential(g, n, k):
    """solve() in f64 with every sum written out term by term: the operation order of ob_linalg.hpp's
    chol_factor_solve(.., BackSub::Dot), with no BLAS dot product in it (NumPy's fuses each product into
    the running sum and regroups the terms of a long one), so its bytes are the engine's at any K."""
    g = np.asarray(g, dtype=np.float64)
    b = np.zeros((k + 1, k))
    for j in range(k):
        idx = order(j, k)
        a = [[float(g[r, c]) for c in idx] for r in idx]  # a[row][col]; the lower triangle is used
        x = [float(g[r, j]) for r in idx]
        for c in range(k):
            for r in range(c, k):
                v = a[r][c]
                for t in range(c):
                    v = -a[c][t] * a[r][t] + v
                a[r][c] = v
            d = a[c][c]
            if not (d != 0.0 and d >= 0.0):
                raise VifRefError("linalg", MSG_CHOLESKY, partial=j)
            den = float(np.sqrt(d))
            for r in range(c, k):
                a[r][c] = den if r == c else a[r][c] / den
        for i in range(k):
            co = x[i] / a[i][i]
            for r in range(i + 1, k):
                x[r] -= co * a[r][i]
            x[i] = co
        for i in range(k - 1, -1, -1):
            part = 0.0
            for r in range(i + 1, k):
                part += a[r][i] * x[r]
            x[i] = (x[i] - part) / a[i][i]
        b[idx, j] = x
    return b


_REFS = {}


def reference(n, k, seed):
    """One shape's fixture with its f64 and longdouble runs, the Gram's condition number and the
    bars; computed once per process and shared (treat it as read-only)."""
    key = (n, k, seed)
    if key not in _REFS:
        x = fixture(n, k, seed)
        s, g, b, m, a, t = vif(x, np.float64, parts=True)
        sl, gl, bl, ml, al, tl = vif(x, LD, parts=True)
        cond = float(np.linalg.cond(g))
        _REFS[key] = {"x": x, "f64": (s, g, b, m, a, t), "ld": (sl, gl, bl, ml, al, tl), "cond": cond,
                      "gram_bar": gram_bar(x), "vif_bar": vif_bar(x, cond, sl, bl, al),
                      "vif_bar_bound": vif_bar_bound(n, k, cond)}
    return _REFS[key]


def sums_reference(x, b, means):
    """The two sums at given f64 coefficients and means, in longdouble, with their bars."""
    a, t = sums(x, b, means, LD)
    rb, tb = sums_bar(x, b, a, t)
    return a, t, rb, tb


# The shapes of tests/test_gpu_vif.py (n, K, seed) and why each can break the kernels.
SHAPES = (
    [(n, 3, 10 + n) for n in (5, 63, 64, 65)]                          # the 64-row sub-tile's edges
    + [(4099, k, 100 + k) for k in (2, 3, 15, 16, 17, 33, 64, 65, 120)]  # K + 1 around each 16-column block
    + [(2051, 120, 7)]
)
