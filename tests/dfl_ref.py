"""NumPy f64 restatement of the reference's DFL reweighting, used only as the checker of the
engine's DFL path (tests/test_dfl_host.py, tests/test_gpu_dfl.py, tests/test_gpu_dfl_passes.py,
tools/dfl_time.py), and the case table and extended-precision trajectory of the latter. Paths are
relative to oaxaca_blinder/src/ of dot-comma-hyphen/oaxaca-blinder-rs.

    logit                math/logit.rs:31-118
    kde                  math/kde.rs:20-41
    silverman_bandwidth  math/kde.rs:44-59
    run_dfl              dfl.rs:34-195

A frame is a dict of columns: lists of float / int / str, ``None`` for a null.
"""
from __future__ import annotations

import math

import numpy as np

LINALG_MESSAGE = "Failed to solve Information Matrix in Logit. Perfect separation?"  # logit.rs:92
NULL_OUTCOME_MESSAGE = "Null outcome encountered in DFL"  # dfl.rs:146


class LinalgError(Exception):
    """OaxacaError::NalgebraError (logit.rs:90-94)."""


class DflError(Exception):
    """Any other OaxacaError of run_dfl; ``kind`` is "polars" or "group"."""

    def __init__(self, kind, message):
        super().__init__(message)
        self.kind = kind


def _cholesky_solve(m, b):
    """nalgebra Cholesky::new + solve: None when a pivot is zero, negative or NaN."""
    k = len(b)
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
    z = np.array(b, dtype=np.float64)
    for i in range(k):
        z[i] /= l[i, i]
        z[i + 1:] -= z[i] * l[i + 1:, i]
    for i in range(k - 1, -1, -1):
        z[i] = (z[i] - l[i + 1:, i] @ z[i + 1:]) / l[i, i]
    return z


def _probs(x, beta):
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-(x @ beta)))  # logit.rs:15-17
    return np.clip(p, 1e-10, 1.0 - 1e-10)  # logit.rs:45


def logit(y, x, max_iter=100, tol=1e-6):
    """logit.rs:31-118 -> dict(coefficients, predicted_probs, converged, iterations, step_norms).
    ``step_norms`` (one per iteration) is not in the reference: tests use it to show that the
    iteration count of a case cannot hinge on rounding."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    k = x.shape[1]
    beta = np.zeros(k)  # logit.rs:41
    norms = []
    for it in range(max_iter):  # logit.rs:43
        probs = _probs(x, beta)  # logit.rs:44-45
        gradient = x.T @ (y - probs)  # logit.rs:48-49
        w = probs * (1.0 - probs)  # logit.rs:57
        xt = x * np.sqrt(w)[:, None]  # logit.rs:64-68
        info = xt.T @ xt  # logit.rs:70,82
        step = _cholesky_solve(info, gradient)  # logit.rs:88-95
        if step is None:
            raise LinalgError(LINALG_MESSAGE)
        beta = beta + step  # logit.rs:96
        norms.append(float(np.sqrt(step @ step)))
        if norms[-1] < tol:  # logit.rs:98-105: probs are those of this iteration's start
            return dict(coefficients=beta, predicted_probs=probs, converged=True, iterations=it + 1,
                        step_norms=norms)
    return dict(coefficients=beta, predicted_probs=_probs(x, beta), converged=False,  # logit.rs:108-117
                iterations=max_iter, step_norms=norms)


# ---- extended-precision Newton trajectory (tests/test_dfl_host.py, tests/test_gpu_dfl_passes.py) ----

EXTENDED = bool(np.finfo(np.longdouble).eps < 1e-18)  # x87 80-bit: eps 1.08e-19
EPS = 2.0 ** -52


def _solve_spd(m, b, dtype):
    """_cholesky_solve with every operation in ``dtype``."""
    k = len(b)
    l = np.array(m, dtype=dtype)
    for j in range(k):
        for c in range(j):
            l[j:, j] -= l[j, c] * l[j:, c]
        if not l[j, j] > 0:
            raise LinalgError(LINALG_MESSAGE)
        l[j, j] = np.sqrt(l[j, j])
        l[j + 1:, j] /= l[j, j]
    z = np.array(b, dtype=dtype)
    for i in range(k):
        z[i] /= l[i, i]
        z[i + 1:] -= z[i] * l[i + 1:, i]
    for i in range(k - 1, -1, -1):
        z[i] = (z[i] - l[i + 1:, i] @ z[i + 1:]) / l[i, i]
    return z


def _fsum_tn(a, b):
    """a^T b with every entry an exact sum of the f64 products (the 64-bit longdouble fallback)."""
    a2, b2 = a.reshape(len(a), -1), b.reshape(len(b), -1)
    out = np.array([[math.fsum((a2[:, i] * b2[:, j]).tolist()) for j in range(b2.shape[1])]
                    for i in range(a2.shape[1])])
    return out.reshape(a.shape[1:] + b.shape[1:])


def logit_trajectory(y, x, iters, dtype=np.longdouble):
    """The Newton recursion of ``logit`` (clamp included), exactly ``iters`` iterations from beta = 0,
    with the sums, the probabilities and the solve carried in ``dtype``. Returns dict(betas: beta_t
    for t = 1 .. iters, probs_start: the probabilities at each iteration's start, conds: the 2-norm
    condition number of each iteration's information matrix, final_probs: the probabilities at the
    last beta, step_norms). The probabilities at beta_t are probs_start[t] (final_probs for
    t = iters). Where longdouble is 64 bits wide the sums are exact (fsum) sums of f64 products."""
    dtype = np.dtype(dtype)
    wide = EXTENDED or dtype != np.dtype(np.longdouble)
    xe, ye = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
    lo, hi = dtype.type(1e-10), dtype.type(1.0 - 1e-10)  # the f64 constants of logit.rs:45
    # a^T b with the long axis contiguous in both operands (numpy's longdouble matmul is a plain loop)
    tn = (lambda a, b: np.ascontiguousarray(a.T) @ np.ascontiguousarray(b.T).T) if wide else _fsum_tn

    def probs_at(beta):
        eta = xe @ beta if wide else _fsum_tn(xe.T, beta)
        with np.errstate(over="ignore"):
            return np.clip(1 / (1 + np.exp(-eta)), lo, hi)

    beta = np.zeros(xe.shape[1], dtype=dtype)
    betas, starts, conds, norms = [], [], [], []
    for _ in range(iters):
        p = probs_at(beta)
        info = tn(xe, xe * (p * (1 - p))[:, None])
        step = _solve_spd(info, tn(xe, ye - p), dtype)
        beta = beta + step
        betas.append(beta)
        starts.append(p)
        conds.append(float(np.linalg.cond(info.astype(np.float64))))
        norms.append(float(np.sqrt(step @ step)))
    return dict(betas=betas, probs_start=starts, conds=conds, final_probs=probs_at(beta), step_norms=norms)


def beta_bar(cond):
    """The bar on max|beta_t - ref_t| / max|ref_t| of one Newton iterate: 512 cond(H_t) 2^-52. The
    f64 restatement sits within 6.4 cond eps of the extended recursion, the device's fixed-order sum
    of up to 4096 per-wave partials adds the same order, and about 64x is margin."""
    return 512.0 * cond * EPS


def panel(n, k, seed):
    """Random normal design with an intercept, beta ~ 0.5 / sqrt(K) (test_gpu_dfl.py's _panel)."""
    rng = np.random.default_rng(seed)
    x = np.column_stack([np.ones(n), rng.normal(size=(n, k - 1))])
    beta = rng.normal(size=k) * 0.5 / np.sqrt(k)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-(x @ beta)))).astype(np.float64)
    return x, y


def saturated_panel(n, k, seed):
    """``panel`` with eight rows of column 1 at +-55 .. +-70 and that column's true coefficient 0.6,
    y drawn from the model: from the third iteration on, those rows' probabilities sit on both
    clamps of logit.rs:45 at the iteration's start, and |x beta| stays under 45."""
    rng = np.random.default_rng(seed)
    x = np.column_stack([np.ones(n), rng.normal(size=(n, k - 1))])
    x[:8, 1] = [55.0, -55.0, 60.0, -60.0, 65.0, -65.0, 70.0, -70.0]
    beta = rng.normal(size=k) * 0.5 / np.sqrt(k)
    beta[1] = 0.6
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-(x @ beta)))).astype(np.float64)
    return x, y


class PassCase:
    """One row of the Newton-pass case table, with its data and references computed once."""

    def __init__(self, n, k, seed, ldx=None, saturated=False, max_t=4, converges=True, note=""):
        self.n, self.k, self.seed, self.ldx, self.saturated = n, k, seed, ldx, saturated
        self.max_t, self.converges, self.note = max_t, converges, note
        self.big = n > 100000
        self.id = f"{n}x{k}"
        self._data = self._conv = self._traj = None

    def data(self):
        if self._data is None:
            self._data = (saturated_panel if self.saturated else panel)(self.n, self.k, self.seed)
        return self._data

    def converged(self):
        """``logit`` at the reference's own tol = 1e-6, max_iter = 100 (None for the one-row case)."""
        if self._conv is None and self.converges:
            x, y = self.data()
            self._conv = logit(y, x, 100, 1e-6)
        return self._conv

    def steps(self):
        """The iterations t = 1 .. steps() held to the bar: min(iterations to converge, 4)."""
        return min(self.converged()["iterations"], self.max_t) if self.converges else self.max_t

    def trajectory(self):
        """The extended trajectory over every iteration of the converged run (at least steps())."""
        if self._traj is None:
            x, y = self.data()
            iters = max(self.steps(), self.converged()["iterations"] if self.converges else 0)
            self._traj = logit_trajectory(y, x, iters)
        return self._traj


PASS_CASES = [
    PassCase(64, 1, 44, note="intercept only, one exactly full sub-tile"),
    PassCase(1, 1, 32, max_t=2, converges=False, note="one row, max_iter = 2 only"),
    PassCase(128, 16, 33, note="one full column block, two full sub-tiles"),
    PassCase(1000, 17, 45, note="first NCB = 2"),
    PassCase(2000, 32, 35),
    PassCase(3000, 48, 36),
    PassCase(3000, 49, 37, note="first NCB = 4"),
    PassCase(3000, 64, 38, note="K_max"),
    PassCase(1000, 5, 39, ldx=1037, note="ldx = 1037"),
    PassCase(4099, 9, 40, saturated=True, note="both clamps bind"),
    PassCase(262145, 3, 41, note="spu = 2, units = 2049, the last unit has one sub-tile with one live row"),
    PassCase(262145, 17, 42, note="spu = 2 with NCB = 2"),
    PassCase(600001, 2, 43, note="spu = 3, units = 3126, short last unit"),
]
BIG_SKIP = "longdouble is 64 bits wide here: the fsum fallback is too slow for the n > 100000 cases"


def gaussian_kernel(u):
    return (1.0 / math.sqrt(2.0 * math.pi)) * np.exp(-0.5 * u * u)  # kde.rs:4-6


def kde(data, weights, grid, bandwidth):
    """kde.rs:20-41."""
    data = np.asarray(data, dtype=np.float64)
    grid = np.asarray(grid, dtype=np.float64)
    n = len(data)
    if weights is not None:  # kde.rs:24-29
        ws = np.asarray(weights, dtype=np.float64)
        sum_w = 0.0
        for v in ws.tolist():
            sum_w += v
        w = ws / sum_w
    else:
        w = np.full(n, 1.0 / n) if n else np.zeros(0)
    out = np.empty(len(grid))
    for g, xg in enumerate(grid.tolist()):  # kde.rs:31-38
        u = (xg - data) / bandwidth
        out[g] = math.fsum(w * gaussian_kernel(u)) / bandwidth
    return out


def silverman_bandwidth(data):
    """kde.rs:44-59 (the (n - 1) variance; quartiles by truncated index; not math/rif.rs)."""
    data = np.asarray(data, dtype=np.float64)
    n = float(len(data))
    mean = math.fsum(data) / n  # kde.rs:46
    with np.errstate(invalid="ignore", divide="ignore"):
        variance = np.float64(math.fsum((data - mean) ** 2)) / np.float64(n - 1.0)  # kde.rs:47
        std_dev = float(np.sqrt(variance))
    s = np.sort(data)  # kde.rs:51-52
    iqr = float(s[int(n * 0.75)] - s[int(n * 0.25)])  # kde.rs:53-55
    a = iqr / 1.34 if math.isnan(std_dev) else min(std_dev, iqr / 1.34)  # f64::min ignores a NaN
    return 0.9 * a * n ** (-0.2)  # kde.rs:58


def _sorted_unique(col):
    """polars unique() + sort(nulls_last = false): the null (if any) first, then byte order."""
    vals = sorted({v for v in col if v is not None}, key=lambda s: s.encode())
    return ([None] if any(v is None for v in col) else []) + vals


def design(frame, predictors):
    """dfl.rs:75-108 -> (X with the intercept column, column names)."""
    n = len(next(iter(frame.values()))) if frame else 0
    cols, names = [np.ones(n)], ["__ob_intercept__"]
    for pred in predictors:
        if pred not in frame:
            raise DflError("polars", f"not found: {pred}")
        col = list(frame[pred])
        if any(v is None for v in col):  # the engine's stricter rule (include/oaxaca_boot.h)
            raise DflError("polars", f"null value in predictor column `{pred}`")
        if col and isinstance(col[0], str):  # dfl.rs:82-98
            for val in _sorted_unique(col)[1:]:
                cols.append(np.array([1.0 if v == val else 0.0 for v in col]))
                names.append(f"{pred}_{val}")
        else:  # dfl.rs:100-101
            cols.append(np.array(col, dtype=np.float64))
            names.append(pred)
    return np.column_stack(cols), names


def run_dfl(frame, outcome, group, reference_group, predictors, grid_size=100):
    """dfl.rs:34-195 -> dict(grid, density_a, density_b, density_b_counterfactual, n_a, n_b,
    group_a, iterations, converged, bandwidth_a, bandwidth_b). ``grid_size`` is the engine's
    extension (the reference fixes 100, dfl.rs:170)."""
    if group not in frame:
        raise DflError("polars", f"not found: {group}")
    gcol = list(frame[group])
    if any(v is not None and not isinstance(v, str) for v in gcol):
        raise DflError("polars", "invalid series dtype: expected `String`")  # `.str()?` dfl.rs:49
    uniq = _sorted_unique(gcol)  # dfl.rs:43-47

    def get(i, default):
        return uniq[i] if i < len(uniq) and uniq[i] is not None else default

    a_name = get(0, reference_group)  # dfl.rs:49
    if a_name == reference_group:  # dfl.rs:50-54
        a_name = get(1, "")
    y = np.array([1.0 if (v if v is not None else "") == a_name else 0.0 for v in gcol])  # dfl.rs:57-67
    x, _ = design(frame, predictors)
    n = len(gcol)
    n_a = sum(1 for v in gcol if v is not None and v == a_name)  # dfl.rs:119-125
    n_b = sum(1 for v in gcol if v is not None and v == reference_group)  # dfl.rs:126-132
    if n_a == 0 or n_b == 0:  # the engine's stricter rule (include/oaxaca_boot.h)
        raise DflError("group", "DFL needs rows in both groups")
    res = logit(y, x, 100, 1e-6)  # dfl.rs:111
    probs = res["predicted_probs"]
    ratio_marginal = (n_b / n) / (n_a / n)  # dfl.rs:134-136
    if outcome not in frame:
        raise DflError("polars", f"not found: {outcome}")
    ocol = list(frame[outcome])
    if any(v is not None and not isinstance(v, float) for v in ocol):
        raise DflError("polars", "invalid series dtype: expected `Float64`")  # `.f64()?` dfl.rs:139
    weights, out_a, out_b = [], [], []
    for i in range(n):  # dfl.rs:143-160
        if ocol[i] is None:
            raise DflError("group", NULL_OUTCOME_MESSAGE)
        if y[i] == 0.0:
            p = min(max(float(probs[i]), 0.0001), 0.9999)
            weights.append((p / (1.0 - p)) * ratio_marginal)
            out_b.append(ocol[i])
        else:
            out_a.append(ocol[i])
    lo, hi = min(ocol), max(ocol)  # dfl.rs:164-168
    step = (hi - lo) / float(grid_size)  # dfl.rs:169-171
    grid = np.array([lo + float(i) * step for i in range(grid_size)])  # dfl.rs:172
    bw_a, bw_b = silverman_bandwidth(out_a), silverman_bandwidth(out_b)  # dfl.rs:174-175
    return dict(grid=grid, density_a=kde(out_a, None, grid, bw_a), density_b=kde(out_b, None, grid, bw_b),
                density_b_counterfactual=kde(out_b, weights, grid, bw_b),  # dfl.rs:180-187
                n_a=n_a, n_b=n_b, group_a=a_name, iterations=res["iterations"], converged=res["converged"],
                bandwidth_a=bw_a, bandwidth_b=bw_b, weights=np.array(weights), step_norms=res["step_norms"])
