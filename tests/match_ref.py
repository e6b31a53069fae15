"""NumPy f64 restatement of the reference's matching module, used only as the checker of the
engine's matching path (tests/test_match_host.py, tests/test_gpu_match.py, tools/match_time.py),
and the data generators those share. Paths are relative to oaxaca_blinder/src/ of
dot-comma-hyphen/oaxaca-blinder-rs.

    run_matching         matching/engine.rs:113-229
    match_psm            matching/engine.rs:232-283 (prepare_data: engine.rs:38-95)
    MahalanobisDistance  matching/distance.rs:30-53 (covariance and its inverse)
    LogisticRegression   matching/logistic.rs:31-113
    squared_euclidean    the kdtree crate: fold(0, +) over (x - y) * (x - y)

The one deliberate difference: among exactly equidistant controls the reference's choice depends on
the shape of its k-d tree; here (and in the engine) the k nearest are the k smallest by the key
(squared distance, control position).

A frame is a dict of columns: lists of float / int / str, ``None`` for a null.
"""
from __future__ import annotations

import math

import numpy as np

EMPTY_GROUP = "One group is empty"  # engine.rs:57-59
NULL_OUTCOME = "Null values in outcomes"  # engine.rs:84
COV_TOO_FEW = "Not enough data points to calculate covariance"  # distance.rs:33
COV_SINGULAR = "Covariance matrix is singular and cannot be inverted"  # distance.rs:50
CHOLESKY_FAILED = "Cholesky decomposition failed"  # engine.rs:165
HESSIAN_SINGULAR = "Hessian is singular"  # logistic.rs:95
NON_FINITE = "non-finite covariate"  # the engine's stricter rule (include/oaxaca_boot.h)


class MatchError(Exception):
    """An OaxacaError of the matching module; ``kind`` is "polars", "group" or "diag"."""

    def __init__(self, kind, message):
        super().__init__(message)
        self.kind = kind


# ---- nearest neighbours ------------------------------------------------------------------------

def dist2(queries, controls):
    """squared_euclidean of every (query, control) pair: 0 + t_0 t_0 + t_1 t_1 + ... in covariate
    order, each product and each sum rounded on its own (no FMA)."""
    q = np.asarray(queries, dtype=np.float64)
    c = np.asarray(controls, dtype=np.float64)
    d = np.zeros((q.shape[0], c.shape[0]))
    for j in range(q.shape[1]):
        t = q[:, j][:, None] - c[:, j][None, :]
        t *= t
        d += t
    return d


def knn(queries, controls, k, block=256, extra=0):
    """The min(k, n_c) controls of each query by the key (dist2, position) -> (idx int64 [n_q, k],
    dist2 [n_q, k]) with -1 / +inf past min(k, n_c). ``extra`` more columns (k + extra in all) let a
    caller look at the distance after the k-th."""
    q = np.asarray(queries, dtype=np.float64)
    c = np.asarray(controls, dtype=np.float64)
    n_q, n_c, kk = q.shape[0], c.shape[0], k + extra
    idx = np.full((n_q, kk), -1, dtype=np.int64)
    dd = np.full((n_q, kk), np.inf)
    m = min(kk, n_c)
    for s in range(0, n_q, block):
        d = dist2(q[s:s + block], c)
        order = np.argsort(d, axis=1, kind="stable")[:, :m]  # stable: ties by position
        idx[s:s + block, :m] = order
        dd[s:s + block, :m] = np.take_along_axis(d, order, axis=1)
    return idx, dd


def kth_gap(queries, controls, k):
    """Per query, (d_{k+1} - d_k) / d_{k+1} of its sorted squared distances (inf where fewer than
    k + 1 controls exist): how far rounding must move a distance to change the chosen set."""
    _, dd = knn(queries, controls, k, extra=1)
    a, b = dd[:, k - 1], dd[:, k]
    with np.errstate(invalid="ignore", divide="ignore"):
        g = (b - a) / b
    return np.where(np.isfinite(b), g, np.inf)


def weight_table(k, m_max):
    """table[m] = 0.0 with the f64 value 1.0 / k added m times in sequence (engine.rs:206-208)."""
    t = np.zeros(m_max + 1)
    step = 1.0 / float(k) if k else 0.0
    w = 0.0
    for m in range(1, m_max + 1):
        w += step
        t[m] = w
    return t


# ---- Mahalanobis transform ---------------------------------------------------------------------

def covariance(x):
    """distance.rs:36-44: centred on the row mean, the n - 1 divisor."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    if n < 2:
        raise MatchError("diag", COV_TOO_FEW)  # distance.rs:32-34
    xc = x - x.sum(axis=0) / n
    return (xc.T @ xc) / float(n - 1)


def _lu_solve(a, b):
    """nalgebra LU::new (partial pivoting by the largest |entry|, a zero pivot column skipped) and
    solve: None when a diagonal entry of U is zero."""
    a = np.array(a, dtype=np.float64)
    b = np.array(b, dtype=np.float64)
    n = a.shape[0]
    for i in range(n):
        p = i + int(np.argmax(np.abs(a[i:, i])))
        if a[p, i] == 0.0:
            continue
        if p != i:
            a[[i, p]] = a[[p, i]]
            b[[i, p]] = b[[p, i]]
        f = a[i + 1:, i] / a[i, i]
        a[i + 1:, i + 1:] -= np.outer(f, a[i, i + 1:])
        a[i + 1:, i] = 0.0
        b[i + 1:] -= np.multiply.outer(f, b[i]) if b.ndim > 1 else f * b[i]
    for i in range(n - 1, -1, -1):
        if a[i, i] == 0.0:
            return None
        b[i] = (b[i] - a[i, i + 1:] @ b[i + 1:]) / a[i, i]
    return b


def try_inverse(m):
    """nalgebra's try_inverse: the adjugate over the determinant up to dimension 4 (None when the
    determinant is exactly zero), LU with partial pivoting beyond (None on a zero pivot). In
    dimension 4 nalgebra expands the cofactors into products; here they are 3 x 3 determinants, which
    rounds differently in the last bits."""
    m = np.array(m, dtype=np.float64)
    d = m.shape[0]
    if d == 0:
        return m
    if d <= 4:
        cof = np.empty_like(m)
        for i in range(d):
            for j in range(d):
                minor = np.delete(np.delete(m, i, 0), j, 1)
                cof[i, j] = (-1.0) ** (i + j) * (_det(minor) if d > 1 else 1.0)
        det = float(m[0] @ cof[0])
        if det == 0.0:
            return None
        return cof.T / det
    return _lu_solve(m, np.eye(d))


def _det(a):
    n = a.shape[0]
    if n == 1:
        return float(a[0, 0])
    if n == 2:
        return float(a[0, 0] * a[1, 1] - a[1, 0] * a[0, 1])
    return float(sum((-1.0) ** j * a[0, j] * _det(np.delete(a[1:], j, 1)) for j in range(n)))


def cholesky_lower(m):
    """nalgebra Cholesky::new -> l(): None when a pivot is zero, negative or NaN."""
    k = m.shape[0]
    l = np.array(m, dtype=np.float64)
    for j in range(k):
        for c in range(j):
            l[j:, j] -= l[j, c] * l[j:, c]
        d = l[j, j]
        if not (d != 0.0 and d >= 0.0):
            return None
        d = math.sqrt(d)
        l[j, j] = d
        l[j + 1:, j] /= d
    return np.tril(l)


def mahalanobis_factor(controls):
    """engine.rs:148-167: L with L L^T = S^-1, S the controls' covariance."""
    inv = try_inverse(covariance(controls))
    if inv is None:
        raise MatchError("diag", COV_SINGULAR)
    l = cholesky_lower(inv)
    if l is None:
        raise MatchError("diag", CHOLESKY_FAILED)
    return l


# ---- logistic regression (matching/logistic.rs, not math/logit.rs) -------------------------------

def _sigmoid(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.power(math.e, -z))  # logistic.rs:51,111: E.powf(-val), no clamp


def logistic(x, y, max_iter=100, tol=1e-6):
    """logistic.rs:31-113 -> dict(coefficients, scores, iterations, step_norms). ``iterations``
    counts the Newton steps taken; running out of them is not an error (logistic.rs:48,104)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    k = x.shape[1]
    beta = np.zeros(k)  # logistic.rs:46
    norms = []
    for _ in range(max_iter):
        p = _sigmoid(x @ beta)  # logistic.rs:50-51
        gradient = x.T @ (y - p)  # logistic.rs:55-56
        w = p * (1.0 - p)  # logistic.rs:68
        hessian = x.T @ (x * w[:, None])  # logistic.rs:81-85
        hessian[np.diag_indices(k)] += 1e-6  # logistic.rs:89-91
        delta = _lu_solve(hessian, gradient)  # logistic.rs:95
        if delta is None:
            raise MatchError("diag", HESSIAN_SINGULAR)
        beta = beta + delta  # logistic.rs:97
        norms.append(float(np.sqrt(delta @ delta)))
        if norms[-1] < tol:  # logistic.rs:99-101
            break
    return dict(coefficients=beta, scores=_sigmoid(x @ beta), iterations=len(norms), step_norms=norms)


# ---- frame rules ---------------------------------------------------------------------------------

def _is_str_col(col):
    return any(isinstance(v, str) for v in col)


def _groups(frame, treatment):
    if treatment not in frame:
        raise MatchError("polars", f"not found: {treatment}")
    col = list(frame[treatment])
    if _is_str_col(col):  # Series::equal(1) on a string column
        raise MatchError("polars", "cannot compare a string column with a number")
    t = [i for i, v in enumerate(col) if v is not None and v == 1]  # engine.rs:120-123
    c = [i for i, v in enumerate(col) if v is not None and v == 0]  # engine.rs:124-127
    return col, t, c


def _covariates(frame, covariates, rows=None):
    cols = []
    for name in covariates:
        if name not in frame:
            raise MatchError("polars", f"not found: {name}")
        col = list(frame[name])
        if _is_str_col(col):
            raise MatchError("polars", f"string covariate column `{name}`")
        if any(v is None for v in col):  # the engine's stricter rule (include/oaxaca_boot.h)
            raise MatchError("polars", f"null value in covariate column `{name}`")
        cols.append(np.array(col, dtype=np.float64))  # to_ndarray::<Float64Type> (engine.rs:133-142)
    n = len(next(iter(frame.values()))) if frame else 0
    x = np.column_stack(cols) if cols else np.zeros((n, 0))
    return x if rows is None else x[rows]


def match_arrays(xt, xc, k, use_mahalanobis):
    """engine.rs:147-209 on the two groups' covariates -> dict(counts per control, idx, dist2,
    xt, xc as matched on)."""
    if use_mahalanobis:
        l = mahalanobis_factor(xc)
        xt, xc = xt @ l, xc @ l  # engine.rs:174-175
    if not (np.all(np.isfinite(xt)) and np.all(np.isfinite(xc))):
        raise MatchError("diag", NON_FINITE)
    idx, dd = knn(xt, xc, k) if k > 0 else (np.zeros((len(xt), 0), np.int64), np.zeros((len(xt), 0)))
    counts = np.bincount(idx[idx >= 0].ravel(), minlength=len(xc)) if len(xc) else np.zeros(0, np.int64)
    return dict(counts=counts, idx=idx, dist2=dd, xt=xt, xc=xc)


def run_matching(frame, treatment, covariates, k, use_mahalanobis=False, detail=False):
    """engine.rs:113-229 -> the weight of every row (the outcome column is never read)."""
    col, t, c = _groups(frame, treatment)
    x = _covariates(frame, covariates)
    m = match_arrays(x[t], x[c], k, use_mahalanobis)
    table = weight_table(k, int(m["counts"].max()) if len(c) else 0)
    w = np.zeros(len(col))
    w[t] = 1.0  # engine.rs:215-218
    w[c] = table[m["counts"]]  # engine.rs:221-226
    if detail:
        m.update(weights=w, treated=np.array(t, np.int64), control=np.array(c, np.int64))
        return m
    return w


def match_psm(frame, treatment, outcome, covariates, k, detail=False):
    """engine.rs:232-283."""
    col, t, c = _groups(frame, treatment)
    if not t or not c:  # engine.rs:56-60
        raise MatchError("group", EMPTY_GROUP)
    x = _covariates(frame, covariates)
    if outcome not in frame:  # engine.rs:79
        raise MatchError("polars", f"not found: {outcome}")
    ocol = list(frame[outcome])
    if any(v is not None and not isinstance(v, float) for v in ocol):
        raise MatchError("polars", "invalid series dtype: expected `Float64`")
    if any(ocol[i] is None for i in t + c):  # engine.rs:82-86
        raise MatchError("group", NULL_OUTCOME)
    if any(v is not None and not isinstance(v, float) for v in col):  # `.f64()?` engine.rs:255
        raise MatchError("polars", "invalid series dtype: expected `Float64`")
    y = np.array([0.0 if v is None else v for v in col], dtype=np.float64)  # engine.rs:256-259
    design = np.column_stack([np.ones(len(col)), x])  # engine.rs:250-253
    fit = logistic(design, y, 100, 1e-6)  # engine.rs:262-265
    scored = dict(frame)
    scored["propensity_score"] = [float(v) for v in fit["scores"]]  # engine.rs:272-274
    res = run_matching(scored, treatment, ["propensity_score"], k, False, detail=detail)  # engine.rs:276-282
    if detail:
        res.update(fit=fit, design=design, target=y)
    return res


# ---- data generators shared by the tests and tools/match_time.py -----------------------------------

def knn_data(n_q, n_c, d, seed, mix=False):
    """rng.normal queries, controls shifted by 0.3; ``mix``: both multiplied by one random d x d
    matrix, so the covariates are correlated (the Mahalanobis cases)."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n_q, d))
    c = rng.normal(size=(n_c, d)) + 0.3
    if mix:
        a = rng.normal(size=(d, d))
        q, c = q @ a, c @ a
    return q, c


def frame_of(n_q, n_c, d, seed, mix=False, int_treatment=False, extras=True):
    """A frame whose treated rows are knn_data's queries and whose controls are its controls, in a
    seeded random row order, plus (``extras``) six rows in neither group: treatment 2 and null. The
    covariates are x0 .. x{d-1}; "y" is an f64 outcome. An int treatment column holds ints."""
    q, c = knn_data(n_q, n_c, d, seed, mix)
    rng = np.random.default_rng(seed + 1000)
    n_x = 6 if extras else 0
    x = np.vstack([q, c, rng.normal(size=(n_x, d))])
    tr = [1] * n_q + [0] * n_c + [2, None, 2, None, 2, 2][:n_x]
    perm = rng.permutation(len(tr))
    rows = np.empty(len(tr), dtype=np.int64)  # rows[p]: the source row at frame position p
    for lo, hi in ((0, n_q), (n_q, n_q + n_c), (n_q + n_c, len(tr))):
        rows[np.sort(perm[lo:hi])] = np.arange(lo, hi)  # each group keeps knn_data's order
    frame = {"treat": [None if tr[r] is None else (int(tr[r]) if int_treatment else float(tr[r])) for r in rows]}
    for j in range(d):
        frame[f"x{j}"] = [float(v) for v in x[rows, j]]
    frame["y"] = [float(v) for v in rng.normal(size=len(tr))]
    return frame, [f"x{j}" for j in range(d)]
