"""NumPy restatement of the reference's check_defensibility_inner (engine/src/defensibility.rs) and verify_inner
(engine/src/analysis.rs:40-96) for the defensibility tests. `dtype` is float64 or longdouble. The fair-wage model
itself (design, Gram, solve, score, z) is tests/remedy_ref.py's; this module starts from y, fair, leverage and
sigma2 over the stacked rows (the reference group's n_a first) and a request list of (stacked row, value).

Per adjustment, in request order: current = y[row]; new = current + value; lower / upper = fair -+ z sqrt(sigma2
(1 + h)), both fair when sigma2 <= 1e-9; is_defensible = new >= lower - 1.0. Per row, for the sums: the wage after
the FIRST adjustment of the request list that names it (`for adj in &results { if adj.index == idx { ..; break } }`,
defensibility.rs:296-301 and :343-349). `literal=True` runs that search as written, O(n m); the default goes through
a first-position map, which is what the engine's atomicMin builds. The eight sums: sum_A y, sum_A new, sum_B y,
sum_B new, sum_B (fair - y), sum_B (fair - new), sum_B (fair - y) over fair > y (required_budget), and the values in
request order (total_cost). The reference adds B's terms in HashMap iteration order: there is no order to copy, and
the bars below hold for any.

Rounding bars, u = 2^-53, first order, in remedy_ref's manner; each compares the device with the longdouble run
on the SAME f64 inputs:
  new_wage  none: one IEEE add of two f64 inputs, compared bitwise with NumPy's f64 add (so is current_wage)
  interval  |lo - lo*| <= 6 u (|f| + margin)   (z's product, 1 + h, the product with sigma2, the square root,
                                                z * se, f - margin; a contracted multiply-add only removes one)
  a sum of c terms t_i, each carrying its own bar b_i:  |S - S*| <= sum_i b_i + (c + 1) u sum_i |t_i|
      sum y           b_i = 0 (the inputs themselves)
      sum new         b_i = u |new_i|                         (the add)
      sum (fair - y)  b_i = u |fair_i - y_i|                  (the subtraction); the same for its positive part:
                      fair > y is an exact comparison of the same two f64 values on both sides
      sum (fair-new)  b_i = u |new_i| + u |fair_i - new_i|
      total_cost      b_i = 0
  is_defensible  compares new with lower - 1: it can differ from the longdouble run only where the longdouble
      new - (lower - 1) lies within the interval bar (plus u |lower - 1| for the subtraction of 1) of zero; the GPU
      tests assert that no row of their fixtures is that close (DEFENSIBLE_MARGIN of the bar).
End to end (OaxacaBuilder.check_defensibility against the longdouble run from the same design) the fair wage
itself differs: remedy_ref.e2e_extra's cond e terms and the score's (K + 1) u sum |xe_ij| |beta_j| are added to
every term's bar that holds a fair wage, and 2 cond e margin to the interval's."""
import numpy as np

import remedy_ref as R

U = R.U
LD = R.LD
MSG_OK = "Wage is within or above the calculated fair range."
SUM_NAMES = ("sum_a_y", "sum_a_new", "sum_b_y", "sum_b_new", "sum_b_fair_y", "sum_b_fair_new", "required_budget",
             "total_cost")


def message(is_defensible, new_wage, lower):
    """defensibility.rs:227-235 with Rust's {:.2}."""
    if is_defensible:
        return MSG_OK
    return "Wage is %.2f below the defensible lower bound (%.2f)." % (float(lower - new_wage), float(lower))


def rust_parse_f64(s):
    """core::num::dec2flt's grammar, character by character: [+-] then inf | infinity | nan (any case), or digits
    with at most one point and at least one digit, then an optional exponent [eE][+-]digits. None for Err."""
    t = s
    if t[:1] in ("+", "-"):
        t = t[1:]
    if t.lower() in ("inf", "infinity", "nan"):
        return float(s)
    i, digits = 0, 0
    while i < len(t) and t[i] in "0123456789":
        i, digits = i + 1, digits + 1
    if i < len(t) and t[i] == ".":
        i += 1
        while i < len(t) and t[i] in "0123456789":
            i, digits = i + 1, digits + 1
    if digits == 0:
        return None
    if i < len(t) and t[i] in "eE":
        i += 1
        if i < len(t) and t[i] in "+-":
            i += 1
        j = i
        while i < len(t) and t[i] in "0123456789":
            i += 1
        if i == j:
            return None
    return float(s) if i == len(t) else None


def resolve_overrides(adjustments, predictors, n_rows):
    """defensibility.rs:32-73. adjustments: (index, value, overrides dict or None) with values already numbers.
    Returns {(row, predictor): value}."""
    by_index = {}
    for idx, _, ovr in adjustments:
        if ovr:
            by_index[idx] = dict(ovr)  # HashMap::insert: the row's whole map is replaced
    cells = {}
    for p in predictors:
        for idx, ovr in by_index.items():
            if p in ovr and 0 <= idx < n_rows:
                cells[(idx, p)] = ovr[p]
    return cells


def verify_wages(wage, index, value, dtype=np.float64):
    """analysis.rs:76-88: one by one, in request order."""
    w = np.array(wage, dtype=dtype)
    for i, v in zip(index, value):
        if not 0 <= i < len(w):
            raise IndexError(f"Adjustment index {i} is out of bounds (dataset has {len(w)} rows)")
        w[i] = w[i] + dtype(v)
    return w


def interval(fair, lev, sigma2, z, dtype):
    fair, lev = np.asarray(fair, dtype=dtype), np.asarray(lev, dtype=dtype)
    if dtype(sigma2) <= 1e-9:
        return fair.copy(), fair.copy()
    margin = dtype(z) * np.sqrt(dtype(sigma2) * (1 + lev))
    return fair - margin, fair + margin


def defend_arrays(y, fair, lev, n_a, sigma2, z, rows, values, dtype=np.float64, literal=False):
    y, fair, lev = (np.asarray(a, dtype=dtype) for a in (y, fair, lev))
    rows = np.asarray(rows, dtype=np.int64)
    vals = np.asarray(values, dtype=dtype)
    n, m = len(y), len(rows)
    lo, up = interval(fair, lev, sigma2, z, dtype)
    cur = y[rows] if m else np.zeros(0, dtype=dtype)
    new = cur + vals
    lower, upper = (lo[rows], up[rows]) if m else (cur.copy(), cur.copy())
    after = y.copy()
    if literal:
        for i in range(n):
            for j in range(m):  # for adj in &results { if adj.index == idx { ...; break } }
                if rows[j] == i:
                    after[i] = new[j]
                    break
    else:
        first = {}
        for j in range(m):
            first.setdefault(int(rows[j]), j)
        for i, j in first.items():
            after[i] = new[j]
    a, b = slice(0, n_a), slice(n_a, n)
    gap, gap_new = fair[b] - y[b], fair[b] - after[b]
    pos = fair[b] > y[b]
    zero = dtype(0.0)

    def tot(v):
        s = zero
        for t in v:  # one by one, as the reference's loops
            s = s + t
        return s

    sums = [tot(y[a]), tot(after[a]), tot(y[b]), tot(after[b]), tot(gap), tot(gap_new), tot(gap[pos]), tot(vals)]
    terms = [y[a], after[a], y[b], after[b], gap, gap_new, gap[pos], vals]
    own = [0 * y[a], U * np.abs(after[a]), 0 * y[b], U * np.abs(after[b]), U * np.abs(gap),
           U * (np.abs(after[b]) + np.abs(gap_new)), U * np.abs(gap[pos]), 0 * vals]
    bars = [float(np.sum(o) + (len(t) + 1) * U * np.sum(np.abs(t))) if len(t) else 0.0 for t, o in zip(terms, own)]
    ca, cb = n_a, n - n_a
    mean = lambda s, c: s / c if c > 0 else zero  # noqa: E731
    margin = np.abs(upper - fair[rows]) if m else cur
    return {"row": rows, "adjustment": vals, "current_wage": cur, "new_wage": new, "fair_wage": fair[rows] if m else cur,
            "lower": lower, "upper": upper, "is_defensible": new >= lower - 1,
            "slack": new - (lower - 1),
            "interval_bar": 6 * U * (np.abs(fair[rows]) + margin) if m else cur,
            "sums": sums, "sum_bars": bars, "sum_terms": terms,
            "total_cost": sums[7], "required_budget": sums[6],
            "original_gap": mean(sums[0], ca) - mean(sums[2], cb), "new_gap": mean(sums[1], ca) - mean(sums[3], cb),
            "original_unexplained_gap": mean(sums[4], cb), "new_unexplained_gap": mean(sums[5], cb)}


DEFENSIBLE_MARGIN = 4.0  # no fixture row may have |new - (lower - 1)| under this many bars


def too_close(ref):
    """The adjustments whose defensibility the bars do not decide (longdouble run `ref`)."""
    bar = ref["interval_bar"] + U * np.abs(ref["lower"] - 1)
    return np.abs(ref["slack"]) <= DEFENSIBLE_MARGIN * bar


def adjustment_lists(n_a, n_b, seed):
    """The request lists of tests/test_gpu_defend.py as (name, rows, values)."""
    rng = np.random.default_rng(seed)
    n = n_a + n_b
    out = [("none", np.zeros(0, np.int64), np.zeros(0)),
           ("one_a_row", np.array([n_a // 2], np.int64), np.array([1.25])),
           ("every_b_once", n_a + rng.permutation(n_b), rng.uniform(0.1, 4.0, n_b))]
    reps = np.concatenate([np.repeat(np.arange(n), 2), rng.choice(n, 3, replace=False)])  # m = 2 n + 3: two or three hits a row
    rows = rng.permutation(reps)
    out.append(("twice_or_thrice", rows, rng.uniform(-3.0, 3.0, len(rows))))
    out.append(("all_on_one_row", np.full(9, n - 1, np.int64), rng.uniform(-2.0, 2.0, 9)))
    return out


def defend_frame(kat, adjustments, dtype=LD, frame_edit=None, confidence_level=0.95):
    """check_defensibility_inner on a KAT frame in `dtype`. adjustments: (original index, value).
    frame_edit: {(original row, predictor name): value}, applied before the design is built.
    Returns (result of defend_arrays with `index` and `n_skipped`, beta, extras for the end-to-end bars)."""
    x, y, n_a, order, names, _ = R.frame_design(kat)
    for (row, name), v in (frame_edit or {}).items():
        x[int(np.flatnonzero(order == row)[0]), names.index(name)] = v
    ga = R.gram(x[:n_a], y[:n_a], dtype)
    beta, cov = R.solve(ga, None, dtype)
    fair, lev, rss, _ = R.score(x, beta, cov, y[:n_a], dtype)
    k = x.shape[1] + 1
    sigma2 = rss / (n_a - k) if n_a - k > 0 else dtype(0.0)
    z = R.inverse_cdf_root(R.z_p(confidence_level))
    inverse = {int(o): s for s, o in enumerate(order)}
    kept = [(inverse[i], v, i) for i, v in adjustments if i in inverse]
    res = defend_arrays(y, fair, lev, n_a, sigma2, z, [t[0] for t in kept], [t[1] for t in kept], dtype)
    res["index"] = np.array([t[2] for t in kept], dtype=np.int64)
    res["n_skipped"] = len(adjustments) - len(kept)
    cond = float(np.linalg.cond(np.asarray(R._normal(ga, k)[0], dtype=np.float64)))
    xf, xm = R.e2e_extra(x, beta, cond, len(y))
    fbar = xf + (k + 1) * U * (np.abs(R.design(x, LD)) @ np.abs(np.asarray(beta, dtype=LD)))  # per stacked row
    return res, beta, {"fair_bar": fbar, "margin_rel": xm, "n_a": n_a, "sigma2": sigma2, "cond": cond}


def e2e_sum_bars(ref, extras):
    """The bars of required_budget, the two unexplained sums and total_cost end to end: every B term's fair wage
    carries extras["fair_bar"] on top of defend_arrays' own bars."""
    fb = float(np.sum(extras["fair_bar"][extras["n_a"]:]))
    t6 = ref["sum_terms"][6]
    pos_fb = fb  # a row whose fair - y changes sign contributes at most its own bar: |max(a, 0) - max(b, 0)| <= |a - b|
    return {"original_unexplained": ref["sum_bars"][4] + fb, "new_unexplained": ref["sum_bars"][5] + fb,
            "required_budget": ref["sum_bars"][6] + pos_fb + (len(t6) + 1) * U * float(np.sum(np.abs(t6))),
            "total_cost": ref["sum_bars"][7]}
