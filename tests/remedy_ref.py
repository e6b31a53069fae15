"""NumPy restatement of the reference's optimize_inner (engine/src/analysis.rs:309-869) for the remediation
tests, with the project's deliberate differences. `dtype` is float64 or longdouble.

The engine's A is the reference group, B the target. Design xe = [1, features]. beta solves the normal
equations of the fit rows (A, or A stacked over B) by nalgebra's Cholesky (the deliberate difference from
the reference's SVD solve); cov = (X_A'X_A)^-1 by nalgebra's try_inverse; sigma2 = rss_A / (n_A - K) or 0;
z = Phi^-1(1 - alpha / 2) for the confidence clamped to [0.50, 0.999]; interval fair -+ z sqrt(sigma2 (1 +
h)), degenerate when sigma2 <= 1e-9; B's target by RangeTarget, A's always the midpoint; a gap is positive
when diff > 1e-6, eligible when diff / actual >= min_gap_pct; the stable descending order of the diffs
(push order: all of B, then all of A); greedy pay min(diff, remaining) or equitable diff * min(budget /
need, 1); output by original index. optimize() runs the reference's SEQUENTIAL loop with its running
current_spend; closed_form() is the engine's clamp(budget - P_c, 0, diff_c).

Rounding bars, u = 2^-53, first order, valid for any summation order (a sum of m products carries at most
m u times the sum of the magnitudes); each compares the device with the longdouble run on the SAME f64
inputs (beta and cov for the score; y, fair, leverage and sigma2 for the allocation):
  fair      |f - f*|_i   <= (K + 1) u sum_j |xe_ij| |beta_j|                     (K-term dot)
  leverage  |h - h*|_i   <= (2 K + 2) u sum_ab |xe_ia| |C_ab| |xe_ib|            (K^2 terms in two K-term stages;
                            the magnitudes of C carry its condition number)
  rss       |rss - rss*| <= 2 sum_i |e_i| (fbar_i + 2 u (|y_i| + |f_i|)) + (n + 2) u sum_i e_i^2
  interval  |lo - lo*|   <= 6 u (|f| + margin)  (z, the product, 1 + h, the square root, z * se, f - margin)
  diff      |d - d*|     <= interval bar (0 at the midpoint) + u |d|
  sums      |S - S*|     <= sum_i dbar_i + (m + 1) u sum_i |d_i|                 (m terms)
  prefix    |P_c - P_c*| <= sum_{j<c} dbar_j + (c + 1) u sum_{j<c} |d_j|
  pay       |pay - pay*| <= prefix bar + dbar_c + 2 u budget, budget's own bar included when it is the auto
                            budget need * 1.00001; the same bar bounds closed form against sequential loop
  cost      as sums over the pays' bars.
normal_inverse_cdf: the restatement of statrs's rational approximations against a longdouble Newton root of
Phi(z) = p (erf by its all-positive series, so no cancellation): measured on x86-64 at p = 0.75, 0.975 and
0.9995 the error is 0.98 u, 0.12 u and 0.66 u of z; Z_BAR = 2 u relative is that measured 1 u and one more for
another libm's log and sqrt.
End to end (OaxacaBuilder.optimize against the longdouble run from the same design), beta itself differs:
the normal equations carry a relative perturbation e = (n + K + 2) u, so ||d beta|| <= cond e ||beta|| and
  fair      adds ||xe_i|| ||beta|| cond e
  interval  adds that and 2 cond e margin (the leverage is linear in C, whose relative error is cond e; rss is
            stationary in beta, so sigma2 moves at second order and by its own (n + 2) u)
  pay, sums take the fair term as one more part of every diff's bar.
Greedy pay end to end depends on the ORDER of the gaps. Two gaps whose exact values differ by less than the sum
of their bars can be ordered either way by a correct evaluation; each gap's bar is its fair-wage bar (plus the
interval's), so two gaps within 2 bars of each other are unordered, and a candidate within 2 bars of the last
paid gap on either side may swap with it: 4 fair-wage bars is the width of that window. Inside it the end-to-end
test compares the group's summed pay; the stable order itself is held bitwise on the array path.
The solve tests hold ob_remedy_solve to the same cond e against the longdouble solve, with e's constant
written out: SOLVE_E(n, K) = (n + K + 2) u."""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
Z_BAR = 2 * U
MSG_SINGULAR = "Covariance matrix is singular, likely due to perfect multicollinearity."


def mock_frame():
    """analysis.rs create_mock_csv: 20 repeats of 4 Male and 4 Female rows."""
    rows = [(50000, 12, 5, "Male", "Sales"), (55000, 16, 2, "Male", "Engineering"), (60000, 14, 8, "Male", "Sales"),
            (80000, 18, 10, "Male", "Engineering"), (40000, 12, 5, "Female", "Sales"),
            (42000, 14, 3, "Female", "Engineering"), (45000, 12, 6, "Female", "Sales"),
            (50000, 16, 5, "Female", "Engineering")] * 20
    return {"wage": [float(r[0]) for r in rows], "education": [float(r[1]) for r in rows],
            "experience": [float(r[2]) for r in rows], "gender": [r[3] for r in rows],
            "department": [r[4] for r in rows]}


def fixture(n_a, n_b, k, seed, noise=1.0, dup=False):
    """Wages with a pay gap: K - 1 features (design column 0 is the intercept), B paid about 2 less.
    Returns (x, y) stacked, A's rows first. dup: B's rows in identical pairs, so ties test the stable order."""
    rng = np.random.default_rng(seed)
    n = n_a + n_b
    x = rng.normal(size=(n, k - 1)) + rng.uniform(-1, 1, k - 1)
    beta = rng.uniform(0.5, 2.0, k)
    y = 30.0 + x @ beta[1:] + noise * rng.normal(size=n)
    y[n_a:] -= 2.0
    if dup:
        half = n_b // 2
        x[n_a + half:n_a + 2 * half] = x[n_a:n_a + half]
        y[n_a + half:n_a + 2 * half] = y[n_a:n_a + half]
    return x, y


def design(x, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    return np.concatenate([np.ones((x.shape[0], 1), dtype=dtype), x], axis=1)


def gram(x, y, dtype=np.float64):
    """ob_vif_gram's layout over [features, y]: columns features, y, ones."""
    z = np.concatenate([np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)[:, None],
                        np.ones((len(y), 1), dtype=dtype)], axis=1)
    return z.T @ z


def _normal(g, k):
    """The design-order normal matrix and right-hand side out of a Gram in gram()'s layout."""
    idx = [k] + list(range(k - 1))
    return g[np.ix_(idx, idx)], g[idx, k - 1]


def _chol_solve_sequential(m, b):
    """nalgebra's Cholesky::new + solve term by term (ob_linalg.hpp chol_factor_solve, BackSub::Dot)."""
    k = len(b)
    a = [[float(m[r, c]) for c in range(k)] for r in range(k)]
    x = [float(v) for v in b]
    for c in range(k):
        for r in range(c, k):
            v = a[r][c]
            for t in range(c):
                v = -a[c][t] * a[r][t] + v
            a[r][c] = v
        d = a[c][c]
        if not (d != 0.0 and d >= 0.0):
            return None
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
    return np.array(x)


def _try_inverse_sequential(m):
    """nalgebra's try_inverse term by term (ob_linalg.hpp): the adjugate at d = 2, LU with partial pivoting
    beyond 4. (d = 3, 4 are not restated; the tests use K in {2, 5, 17, 33}.)"""
    d = m.shape[0]
    if d == 2:
        cof = [[float(m[1, 1]), -float(m[1, 0])], [-float(m[0, 1]), float(m[0, 0])]]  # cof[r][c]
        det = 0.0
        for c in range(2):
            det += float(m[0, c]) * cof[0][c]
        if det == 0.0:
            return None
        return np.array([[cof[c][r] / det for c in range(2)] for r in range(2)])
    assert d > 4
    a = [[float(m[r, c]) for c in range(d)] for r in range(d)]
    inv = [[1.0 if r == c else 0.0 for c in range(d)] for r in range(d)]
    for i in range(d):
        piv = i
        for r in range(i + 1, d):
            if abs(a[r][i]) > abs(a[piv][i]):
                piv = r
        if a[piv][i] == 0.0:
            continue
        if piv != i:
            a[i], a[piv] = a[piv], a[i]
            inv[i], inv[piv] = inv[piv], inv[i]
        for r in range(i + 1, d):
            f = a[r][i] / a[i][i]
            for c in range(i + 1, d):
                a[r][c] -= f * a[i][c]
            for c in range(d):
                inv[r][c] -= f * inv[i][c]
    for i in range(d - 1, -1, -1):
        if a[i][i] == 0.0:
            return None
        for c in range(d):
            part = inv[i][c]
            for j in range(i + 1, d):
                part -= a[i][j] * inv[j][c]
            inv[i][c] = part / a[i][i]
    return np.array(inv)


class RemedyRefError(Exception):
    pass


def solve(gram_a, gram_fit=None, dtype=np.float64, sequential=False):
    """(beta, cov) in design order. sequential (f64 only): every operation in the engine's order."""
    k = gram_a.shape[0] - 1
    ma, _ = _normal(np.asarray(gram_a, dtype=dtype), k)
    mf, rhs = _normal(np.asarray(gram_a if gram_fit is None else gram_fit, dtype=dtype), k)
    if sequential:
        cov = _try_inverse_sequential(ma)
        beta = None if cov is None else _chol_solve_sequential(mf, rhs)
        if beta is None:
            raise RemedyRefError(MSG_SINGULAR)
        return beta, cov
    if np.linalg.matrix_rank(ma.astype(np.float64)) < k:
        raise RemedyRefError(MSG_SINGULAR)
    eye = np.eye(k, dtype=dtype)
    return _gauss(mf, rhs[:, None], dtype)[:, 0], _gauss(ma, eye, dtype)


def _gauss(m, b, dtype):
    """Gaussian elimination with partial pivoting in `dtype` (np.linalg has no longdouble)."""
    a = np.array(m, dtype=dtype)
    x = np.array(b, dtype=dtype)
    d = a.shape[0]
    for i in range(d):
        p = i + int(np.argmax(np.abs(a[i:, i])))
        if p != i:
            a[[i, p]], x[[i, p]] = a[[p, i]], x[[p, i]]
        f = a[i + 1:, i] / a[i, i]
        a[i + 1:] -= f[:, None] * a[i]
        x[i + 1:] -= f[:, None] * x[i]
    for i in range(d - 1, -1, -1):
        x[i] = (x[i] - a[i, i + 1:] @ x[i + 1:]) / a[i, i]
    return x


def score(x, beta, cov, y_a=None, dtype=np.float64):
    """(fair, leverage, rss over the first len(y_a) rows, contributions)."""
    xe = design(x, dtype)
    b, c = np.asarray(beta, dtype=dtype), np.asarray(cov, dtype=dtype)
    fair = xe @ b
    lev = np.sum((xe @ c) * xe, axis=1)
    rss = dtype(0.0)
    if y_a is not None:
        e = np.asarray(y_a, dtype=dtype) - fair[:len(y_a)]
        rss = e @ e
    return fair, lev, rss, xe * b[None, :]


def score_bars(x, beta, cov, y_a):
    xe = np.abs(design(x, LD))
    k = xe.shape[1]
    fbar = (k + 1) * U * (xe @ np.abs(np.asarray(beta, dtype=LD)))
    hbar = (2 * k + 2) * U * np.sum((xe @ np.abs(np.asarray(cov, dtype=LD))) * xe, axis=1)
    fair = design(x, LD) @ np.asarray(beta, dtype=LD)
    n = len(y_a)
    y = np.asarray(y_a, dtype=LD)
    e = y - fair[:n]
    rbar = 2 * np.sum(np.abs(e) * (fbar[:n] + 2 * U * (np.abs(y) + np.abs(fair[:n])))) + (n + 2) * U * (e @ e)
    return fbar, hbar, rbar


# ---- Phi^-1 ------------------------------------------------------------------------------------------------

PI_LD = LD("3.14159265358979323846264338327950288")


def inverse_cdf_root(p):
    """The longdouble root z >= 0 of Phi(z) = p for p in (0.5, 1), by Newton."""
    p = LD(p)
    z = LD(1.0)
    for _ in range(60):
        x = z / np.sqrt(LD(2))
        term, s, n = x, x, 0
        while term > s * LD(1e-22):
            n += 1
            term = term * 2 * x * x / (2 * n + 1)
            s += term
        phi = (1 + 2 / np.sqrt(PI_LD) * np.exp(-x * x) * s) / 2
        pdf = np.exp(-z * z / 2) / np.sqrt(2 * PI_LD)
        step = (phi - p) / pdf
        z = z - step
        if abs(step) < LD(1e-19) * abs(z):
            break
    return z


def z_p(confidence):
    c = min(max(0.95 if confidence is None else confidence, 0.50), 0.999)
    alpha = 1.0 - c
    return 1.0 - (alpha / 2.0)  # the p handed to inverse_cdf


# ---- classification and allocation ---------------------------------------------------------------------------

def classify(y, fair, lev, n_a, sigma2, z, dtype=np.float64, min_gap_pct=0.0, forensic_mode=False,
             adjust_both_groups=False, range_target="midpoint"):
    """analysis.rs:516-684: the candidates in push order as dicts, with net_residual_sum_b."""
    y, fair, lev = (np.asarray(a, dtype=dtype) for a in (y, fair, lev))
    n = len(y)
    sigma2, z = dtype(sigma2), dtype(z)
    if sigma2 <= 1e-9:
        lo, up = fair.copy(), fair.copy()
    else:
        margin = z * np.sqrt(sigma2 * (1 + lev))
        lo, up = fair - margin, fair + margin
    cands, net = [], dtype(0.0)
    rows = list(range(n_a, n)) + (list(range(n_a)) if adjust_both_groups or forensic_mode else [])
    for row in rows:
        is_b = row >= n_a
        target = fair[row] if not is_b or range_target == "midpoint" else (lo[row] if range_target == "lower" else up[row])
        diff = target - y[row]
        if is_b:
            net += diff
        elig = False
        if diff > 1e-6:
            pct = diff / y[row] if abs(y[row]) > 1e-6 else dtype(0.0)
            elig = (is_b or adjust_both_groups) and pct >= min_gap_pct
        if elig or forensic_mode:
            cands.append({"row": row, "diff": diff, "elig": elig, "fair": fair[row], "lower": lo[row], "upper": up[row],
                          "current": y[row]})
    return cands, net, lo, up


def allocate(cands, budget, strategy="greedy", dtype=np.float64, closed_form=False):
    """analysis.rs:686-834. closed_form: pay = clamp(budget - P_c, 0, diff_c) instead of the running spend."""
    need = dtype(0.0)
    for p in cands:
        if p["diff"] > 0.0 and p["elig"]:
            need += p["diff"]
    eff = dtype(budget) if budget > 0.0 else need * dtype(1.00001)
    order = sorted(cands, key=lambda p: -p["diff"])  # stable
    spend, prefix, out = dtype(0.0), dtype(0.0), []
    ratio = min(eff / need, dtype(1.0)) if need > 0.0 else dtype(0.0)
    for p in order:
        pay = dtype(0.0)
        if p["diff"] > 0.0 and p["elig"]:
            if strategy == "equitable":
                pay = p["diff"] * ratio
            elif closed_form:
                pay = min(max(eff - prefix, dtype(0.0)), p["diff"])
                prefix += p["diff"]
            else:
                remaining = eff - spend
                pay = min(p["diff"], remaining) if remaining > 0.0 else dtype(0.0)
        if pay > 0.0 or strategy == "equitable":
            spend += pay
        out.append(dict(p, pay=pay, new=p["current"] + pay))
    return out, need, eff, spend


def optimize_arrays(y, fair, lev, n_a, sigma2, z, index=None, dtype=np.float64, budget=0.0, strategy="greedy",
                    closed_form=False, **kw):
    """The whole of analysis.rs:516-857 over stacked arrays; the result sorted by original index."""
    cands, net, lo, up = classify(y, fair, lev, n_a, sigma2, z, dtype, **kw)
    out, need, eff, spend = allocate(cands, budget, strategy, dtype, closed_form)
    idx = np.arange(len(y)) if index is None else np.asarray(index)
    out.sort(key=lambda p: idx[p["row"]])
    n_b = len(y) - n_a
    return {"index": np.array([idx[p["row"]] for p in out], dtype=np.int64),
            "row": np.array([p["row"] for p in out], dtype=np.int64),
            "adjustment": np.array([p["pay"] for p in out], dtype=dtype),
            "current_wage": np.array([p["current"] for p in out], dtype=dtype),
            "new_wage": np.array([p["new"] for p in out], dtype=dtype),
            "fair_wage": np.array([p["fair"] for p in out], dtype=dtype),
            "lower": np.array([p["lower"] for p in out], dtype=dtype),
            "upper": np.array([p["upper"] for p in out], dtype=dtype),
            "diff": np.array([p["diff"] for p in out], dtype=dtype),
            "elig": np.array([p["elig"] for p in out], dtype=bool),
            "total_cost": spend, "required_budget": need, "effective_budget": eff, "net_residual_sum_b": net,
            "original_unexplained_gap": -net / n_b if n_b else dtype(0.0),
            "new_unexplained_gap": -(net - spend) / n_b if n_b else dtype(0.0)}


def solve_e(n, k):
    return (n + k + 2) * U


def e2e_extra(x_rows, beta, cond, n):
    """The end-to-end additions per row: (fair term, relative margin term)."""
    xe = design(x_rows, LD)
    k = xe.shape[1]
    ce = LD(cond) * solve_e(n, k)
    return np.sqrt(np.sum(xe * xe, axis=1)) * np.sqrt(np.sum(np.asarray(beta, dtype=LD) ** 2)) * ce, 2 * ce


def allocation_bars(ref, n_push, budget, range_target="midpoint", sigma2=1.0, extra_fair=0.0, extra_margin=0.0):
    """Bars of the allocation from its longdouble run `ref` (optimize_arrays(.., dtype=LD)): per-entry interval
    and pay bars, and the bars of the sums. n_push: the rows visited."""
    f = np.abs(ref["fair_wage"])
    margin = np.abs(ref["upper"] - ref["fair_wage"])
    ibar = 6 * U * (f + margin) + extra_fair + extra_margin * margin
    dbar = (ibar if range_target != "midpoint" and sigma2 > 1e-9 else extra_fair) + U * np.abs(ref["diff"]) + U * f
    d = np.where(ref["elig"], np.abs(ref["diff"]), 0.0)
    db = np.where(ref["elig"], dbar, 0.0)
    m = len(d)
    total_d, total_db = d.sum() if m else LD(0), (db.sum() if m else LD(0))
    sum_bar = total_db + (n_push + 1) * U * total_d
    budget_bar = 2 * U * abs(ref["effective_budget"]) + (sum_bar * 1.00001 if budget <= 0.0 else 0.0)
    pay_bar = sum_bar + dbar + budget_bar  # the prefix bar at its largest, c = m
    return {"interval": ibar, "pay": pay_bar, "need": sum_bar, "cost": m * np.max(pay_bar) if m else LD(0),
            "fair": extra_fair + U * f}


# The shapes of tests/test_gpu_remedy.py's score tests: (n_a, n_b) and K, and why each can break the kernel.
SCORE_ROWS = [(5, 1), (37, 5), (257, 63), (4099, 1031)]  # below one 16-row block, ragged blocks, several units
SCORE_KS = [2, 4, 16, 17, 33]                             # K + 1 at, below and above a 16-column block edge

# The shapes of the allocation tests (n_a, n_b, K).
ALLOC_SHAPES = [(257, 63, 4), (4099, 1031, 17)]


def frame_design(kat):
    """A KAT frame as the builder lays it out: stacked features (predictors, then one dummy per categorical
    level but the first in sorted order), wages, n_a and the original indices, the reference group first."""
    rows = kat["rows"] * kat.get("repeats", 1)
    cols = kat["columns"]
    feats = [[float(r[cols.index(p)]) for r in rows] for p in kat["predictors"]]
    names = list(kat["predictors"])
    for c in kat.get("categorical", []):
        vals = [r[cols.index(c)] for r in rows]
        for lev in sorted(set(vals))[1:]:
            feats.append([1.0 if v == lev else 0.0 for v in vals])
            names.append(f"{c}_{lev}")
    x = np.array(feats, dtype=np.float64).T
    y = np.array([r[cols.index(kat["outcome"])] for r in rows], dtype=np.float64)
    ref = np.array([r[cols.index(kat["group"])] == kat["reference_group"] for r in rows])
    order = np.concatenate([np.flatnonzero(ref), np.flatnonzero(~ref)])
    frame = {c: [r[i] if isinstance(r[i], str) else float(r[i]) for r in rows] for i, c in enumerate(cols)}
    return x[order], y[order], int(ref.sum()), order, names, frame


def optimize_frame(kat, dtype=LD, target="reference", confidence_level=0.95, **kw):
    """optimize_inner on a KAT frame in `dtype`: (result, beta, extras for the end-to-end bars)."""
    x, y, n_a, index, names, _ = frame_design(kat)
    ga = gram(x[:n_a], y[:n_a], dtype)
    gf = ga + gram(x[n_a:], y[n_a:], dtype) if target == "pooled" else None
    beta, cov = solve(ga, gf, dtype)
    fair, lev, rss, _ = score(x, beta, cov, y[:n_a], dtype)
    k = x.shape[1] + 1
    sigma2 = rss / (n_a - k) if n_a - k > 0 else dtype(0.0)
    z = inverse_cdf_root(z_p(confidence_level))
    res = optimize_arrays(y, fair, lev, n_a, sigma2, z, index=index, dtype=dtype, closed_form=True, **kw)
    # the condition number of the normal matrices the two solves see (the design's, not the Gram's with y)
    cond = max(float(np.linalg.cond(np.asarray(_normal(g, k)[0], dtype=np.float64))) for g in (ga, ga if gf is None else gf))
    return res, beta, sigma2, (x, cond, len(y))


# ---- efficient frontier (analysis.rs:871-1153) ---------------------------------------------------------------
# Bar of each t, first order, as the VIF bar: t = b_g / sqrt(rss / dof * c11) for the pooled fit of y + pay_s.
#   b_g   |d b_g| <= cond e ||beta_s||, e = (n + K + 3) u the relative perturbation of the normal equations (the
#         X_p'Y column is an n-term sum like the Gram's entries)
#   c11   relative cond e
#   rss   stationary in beta_s (the residual is orthogonal to X_p), so beta's error enters at second order,
#         cond (cond e)^2; its own n-term sum and each residual's K-term dot give (n + 2 K + 6) u relative with
#         sum |e| rho / rss folded in as in vif_ref (rho <= |y| + |x_p| |beta|): S_s below
#   pay   the closed form against the sequential carry-over: each wage moves by at most the prefix bar
#         (m + 1) u sum gap, which moves t through b_g and rss by the same first-order terms (folded into e
#         by adding (m + 1) u sum gap / ||y|| to it)
# |dt| <= |t| (cond e + ((n + 2 K + 6) + 2 (K + 3) S_s) u / 2 + cond (cond e)^2 / 2 + 2 u) + cond e ||beta_s|| / se_s.

def frontier(kat, steps=50, max_budget=None, dtype=LD, opt=None):
    """The reference's loop, sequential carry-over included: (budgets, t, p, significant, extras for the bar).
    opt: the optimize step's result (row, adjustment, required_budget) to start from, default this module's own
    in `dtype`. The GPU tests hand in the engine's f64 gaps: frames that repeat their rows have gaps that are
    equal in exact arithmetic, rounding decides their order, and at a budget that ends inside such a group the
    t statistic depends on which member was paid; the frontier is then compared on the same gaps, and the gaps
    themselves are the optimize tests' business."""
    import math

    x, y, n_a, index, names, _ = frame_design(kat)
    if opt is None:
        opt, *_ = optimize_frame(kat, dtype)
    need = opt["required_budget"]
    mb = need * dtype(1.1) if max_budget is None else dtype(max_budget)
    if mb < 1e-9:
        mb = dtype(1000.0)
    step = mb / dtype(steps)
    n = len(y)
    xp = np.concatenate([np.ones((n, 1)), (np.arange(n) >= n_a).astype(np.float64)[:, None], x], axis=1).astype(dtype)
    pending = sorted(zip(opt["row"].tolist(), [dtype(v) for v in opt["adjustment"]]), key=lambda p: -p[1])
    pending = [[r, g] for r, g in pending]
    xtx = xp.T @ xp
    inv = _gauss(xtx, np.eye(xp.shape[1], dtype=dtype), dtype)
    dof = n - xp.shape[1]
    cur = np.asarray(y, dtype=dtype).copy()
    out, extras = [], []

    def point(b):
        beta = inv @ (xp.T @ cur)
        r = cur - xp @ beta
        rss = r @ r
        if dof <= 0:
            return (b, dtype(0), 1.0, False), None
        se = np.sqrt(rss / dof * inv[1, 1])
        t = beta[1] / se
        p = math.erfc(abs(float(t)) / math.sqrt(2.0))
        rho = np.abs(cur) + np.abs(xp) @ np.abs(beta)
        return (b, t, p, p < 0.05), (np.sqrt(beta @ beta), se, np.sum(np.abs(r) * rho) / rss)

    pt, ex = point(dtype(0.0))
    out.append(pt), extras.append(ex)
    pay_idx, cursor = 0, dtype(0.0)
    for sidx in range(1, steps + 1):
        target = dtype(sidx) * step
        avail = target - cursor
        if avail > 0:
            rem = avail
            while rem > 0 and pay_idx < len(pending):
                pp = pending[pay_idx]
                if pp[1] <= rem:
                    cur[pp[0]] += pp[1]
                    rem -= pp[1]
                    pp[1] = dtype(0.0)
                    pay_idx += 1
                else:
                    cur[pp[0]] += rem
                    pp[1] -= rem
                    rem = dtype(0.0)
            cursor = target
        pt, ex = point(target)
        out.append(pt), extras.append(ex)
    cond = float(np.linalg.cond(np.asarray(xtx, dtype=np.float64)))
    gaps = float(np.sum(np.asarray(opt["adjustment"], dtype=np.float64)))
    return out, extras, {"cond": cond, "n": n, "k1": xp.shape[1], "m": len(pending), "gaps": gaps,
                         "ynorm": float(np.sqrt(np.sum(np.asarray(y, dtype=np.float64) ** 2))), "need": float(need)}


def frontier_t_bar(t, extra, info):
    """The bar of one t from frontier()'s extras."""
    bnorm, se, big_s = (float(v) for v in extra)
    n, k1, cond = info["n"], info["k1"], info["cond"]
    e = (n + k1 + 2) * U + (info["m"] + 1) * U * info["gaps"] / info["ynorm"]
    ce = cond * e
    rel = ce + ((n + 2 * k1 + 4) + 2 * (k1 + 2) * big_s) * U / 2 + cond * ce * ce / 2 + 2 * U
    return abs(float(t)) * rel + ce * bnorm / se


def frontier_closed_form(y, rows, gaps, budgets, dtype=np.float64):
    """y + clamp(b - P_i, 0, gap_i) for every budget: what the engine's kernels recompute per tile."""
    order = sorted(range(len(rows)), key=lambda i: -gaps[i])
    out = []
    for b in budgets:
        cur = np.asarray(y, dtype=dtype).copy()
        pre = dtype(0.0)
        for i in order:
            rem = dtype(b) - pre
            cur[rows[i]] += min(rem, dtype(gaps[i])) if rem > 0 else dtype(0.0)
            pre += dtype(gaps[i])
        out.append(cur)
    return out
