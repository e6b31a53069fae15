"""Remediation without a GPU: the NumPy restatement (tests/remedy_ref.py) against the properties the
reference's own unit cases assert (tests/golden/remedy_kat.json), ob_remedy_solve against the restatement's
sequential-order solve bit for bit, ob_normal_inverse_cdf against a longdouble root, the closed-form running
budget against the reference's sequential loop, and the argument errors raised before any device work."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import remedy_ref as R  # noqa: E402

KAT = json.load(open(os.path.join(HERE, "golden", "remedy_kat.json")))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _kat_arrays(name):
    """A KAT frame as stacked arrays, the reference group first: features, wages, n_a, original indices."""
    m = KAT[name]
    rows = m["rows"] * m.get("repeats", 1)
    cols = m["columns"]
    x = np.array([[r[cols.index(p)] for p in m["predictors"]] for r in rows], dtype=np.float64)
    y = np.array([r[cols.index(m["outcome"])] for r in rows], dtype=np.float64)
    ref = np.array([r[cols.index(m["group"])] == m["reference_group"] for r in rows])
    order = np.concatenate([np.flatnonzero(ref), np.flatnonzero(~ref)])
    return x[order], y[order], int(ref.sum()), order


def _ref_optimize(name, dtype, **kw):
    x, y, n_a, index = _kat_arrays(name)
    beta, cov = R.solve(R.gram(x[:n_a], y[:n_a], dtype), None, dtype)
    fair, lev, rss, _ = R.score(x, beta, cov, y[:n_a], dtype)
    sigma2 = rss / (n_a - x.shape[1] - 1)
    z = R.inverse_cdf_root(R.z_p(kw.pop("confidence_level", None)))
    return R.optimize_arrays(y, fair, lev, n_a, sigma2, z, index=index, dtype=dtype, **kw)


@pytest.mark.parametrize("dtype", [np.float64, R.LD], ids=["f64", "longdouble"])
def test_restatement_satisfies_the_reference_properties(dtype):
    x, y, n_a, index = _kat_arrays("mock_csv")
    c = KAT["counts"]
    assert (len(y), n_a, len(y) - n_a) == (c["rows"], c["reference"], c["target"])
    for rq in KAT["requests"]:
        res = _ref_optimize("mock_csv", dtype, **{k: v for k, v in rq.items() if k != "name"})
        assert np.all(np.diff(res["index"]) > 0), rq["name"]
        assert np.all(res["index"] < KAT["properties"]["max_index"])
        assert np.all(res["new_wage"] >= res["current_wage"])
    k = KAT["prediction_interval"]
    res = _ref_optimize("prediction_interval", dtype, **k["request"])
    assert len(res["index"]) > 0 and np.all(res["fair_wage"] > k["min_fair_wage"])
    assert np.all(res["lower"] < res["fair_wage"]) and np.all(res["fair_wage"] < res["upper"])
    assert np.all(res["upper"] - res["lower"] > KAT["properties"]["min_interval_width"])
    # the auto budget pays every eligible gap in full
    assert np.array_equal(res["adjustment"], res["diff"])  # need * 1.00001 is far above every prefix: min(diff, remaining) = diff


@pytest.mark.parametrize("p", [0.75, 0.975, 0.9995])
def test_normal_inverse_cdf_against_longdouble_root(ob, p):
    z = ob.normal_inverse_cdf(p)
    root = R.inverse_cdf_root(p)
    err = float(abs(R.LD(z) - root) / root)
    print(f"inverse_cdf({p}) = {z!r}, root {root!r}, relative error {err:.3g} ({err / R.U:.2f} u, bar {R.Z_BAR / R.U:.0f} u)")
    assert err <= R.Z_BAR


def test_normal_inverse_cdf_ranges(ob):
    """Every range of erf_inv_impl, the symmetry and the ends."""
    for p in (0.5 + 1e-3, 0.6, 0.74, 0.9, 0.999, 1 - 1e-9, 1 - 1e-15):
        z = ob.normal_inverse_cdf(p)
        if p <= 1 - 1e-9:  # beyond, 1 - p itself is not exact in f64
            root = R.inverse_cdf_root(p)
            assert abs(R.LD(z) - root) <= 8 * R.U * root + 4 * R.U / (np.exp(-root * root / 2) / np.sqrt(2 * R.PI_LD)), p
        # the lower tail is the same approximation with the sign turned: only 1 - p rounds (u / pdf in z)
        root = R.inverse_cdf_root(p)
        assert abs(ob.normal_inverse_cdf(1 - p) + z) <= 4 * R.U / float(np.exp(-root * root / 2) / np.sqrt(2 * R.PI_LD)) + R.Z_BAR * z
    for q in (1e-20, 1e-100, 1e-300):  # the deep-tail ranges, by the Mills-ratio bounds pdf z / (z^2 + 1) < Q(z) < pdf / z
        z = -ob.normal_inverse_cdf(q)
        pdf = np.exp(-R.LD(z) ** 2 / 2) / np.sqrt(2 * R.PI_LD)
        tol = (z * z + 2) * R.Z_BAR + 8 * R.U  # d ln Q = -(pdf / Q) dz, and pdf / Q < z + 1 / z
        assert pdf * z / (z * z + 1) * (1 - tol) <= q <= pdf / z * (1 + tol)
    assert ob.normal_inverse_cdf(0.5) == 0.0
    assert ob.normal_inverse_cdf(0.0) == -np.inf and ob.normal_inverse_cdf(1.0) == np.inf
    assert np.isnan(ob.normal_inverse_cdf(1.5)) and np.isnan(ob.normal_inverse_cdf(-0.1))


@pytest.mark.parametrize("k", [2, 5, 17, 33])
@pytest.mark.parametrize("pooled", [False, True], ids=["reference", "pooled"])
def test_solve_is_the_restatement_bit_for_bit(ob, k, pooled):
    n_a, n_b = 300, 120
    x, y = R.fixture(n_a, n_b, k, 40 + k)
    ga = R.gram(x[:n_a], y[:n_a])
    gf = R.gram(x, y) if pooled else None
    beta, cov = ob.remedy_solve(ga, gf)
    want_b, want_c = R.solve(ga, gf, sequential=True)
    assert np.array_equal(_bits(beta), _bits(want_b))
    assert np.array_equal(_bits(cov), _bits(want_c))
    ld_b, ld_c = R.solve(ga, gf, R.LD)
    cond = max(np.linalg.cond(ga), np.linalg.cond(ga if gf is None else gf))
    e = cond * R.solve_e(n_a + n_b, k)  # remedy_ref.py: ||d beta|| <= cond e ||beta||, and so for C
    assert np.linalg.norm(np.asarray(beta - ld_b, dtype=np.float64)) <= e * np.linalg.norm(np.asarray(ld_b, dtype=np.float64))
    assert np.linalg.norm(np.asarray(cov - ld_c, dtype=np.float64)) <= e * np.linalg.norm(np.asarray(ld_c, dtype=np.float64))


def test_solve_errors(ob, N):
    x = np.array([[1.0, 2.0], [2.0, 4.0], [3.0, 6.0], [4.0, 8.0]])  # the second feature is twice the first
    with pytest.raises(N.OaxacaError) as e:
        ob.remedy_solve(R.gram(x, np.array([1.0, 2.0, 2.0, 5.0])))
    assert e.value.code == N.OB_E_LINALG and str(e.value) == R.MSG_SINGULAR
    with pytest.raises(N.OaxacaError) as e:
        ob.remedy_solve(np.eye(N.OB_REMEDY_MAX_K + 2))
    assert e.value.code == N.OB_E_UNSUPPORTED and "at most 119" in str(e.value)
    ob.remedy_solve(np.eye(N.OB_REMEDY_MAX_K + 1))  # 119 columns beside the intercept are taken
    g = R.gram(*R.fixture(50, 0, 4, 3))
    g[1, 1] = np.nan
    with pytest.raises(N.OaxacaError) as e:
        ob.remedy_solve(g)
    assert e.value.code == N.OB_E_LINALG


@pytest.mark.parametrize("strategy", ["greedy", "equitable"])
@pytest.mark.parametrize("budget", [0.0, 3.0, 40.0, 1e6])
def test_closed_form_equals_the_sequential_loop(strategy, budget):
    n_a, n_b, k = 257, 63, 4
    x, y = R.fixture(n_a, n_b, k, 9, dup=True)
    beta, cov = R.solve(R.gram(x[:n_a], y[:n_a]))
    fair, lev, rss, _ = R.score(x, beta, cov, y[:n_a])
    z = float(R.inverse_cdf_root(0.975))
    kw = dict(budget=budget, strategy=strategy, adjust_both_groups=True)
    seq = R.optimize_arrays(y, fair, lev, n_a, rss / (n_a - k), z, **kw)
    clo = R.optimize_arrays(y, fair, lev, n_a, rss / (n_a - k), z, closed_form=True, **kw)
    ld = R.optimize_arrays(y, fair, lev, n_a, rss / (n_a - k), z, dtype=R.LD, **kw)
    bars = R.allocation_bars(ld, len(y), budget)
    assert np.array_equal(seq["index"], clo["index"]) and len(seq["index"]) > 40
    worst = float(np.max(np.abs(seq["adjustment"] - clo["adjustment"]) / bars["pay"]))
    print(f"{strategy} budget {budget}: closed form vs sequential, worst fraction of the pay bar {worst:.3g}")
    assert worst <= 1.0
    assert float(np.max(np.abs(clo["adjustment"] - ld["adjustment"]) / bars["pay"])) <= 0.125


def _frame(**over):
    f = R.mock_frame()
    f.update(over)
    return f


def test_builder_errors_come_before_any_device_work(ob, N):
    def opt(frame, preds=("education", "experience")):
        return ob.OaxacaBuilder(frame, "wage", "gender", "Male").predictors(list(preds)).optimize()

    g3 = R.mock_frame()["gender"]
    g3[7] = "Other"
    with pytest.raises(N.OaxacaError) as e:
        opt(_frame(gender=g3))
    assert e.value.code == N.OB_E_UNSUPPORTED and "two groups" in str(e.value)
    edu = R.mock_frame()["education"]
    edu[3] = None
    with pytest.raises(N.OaxacaError) as e:
        opt(_frame(education=edu))
    assert e.value.code == N.OB_E_INVALID and "null value" in str(e.value) and "`education`" in str(e.value)
    with pytest.raises(N.OaxacaError) as e:
        opt(R.mock_frame(), preds=("education", "nope"))
    assert e.value.code == N.OB_E_COLUMN and str(e.value) == "Column 'nope' not found in dataset."
    wide = R.mock_frame()
    rng = np.random.default_rng(0)
    for j in range(120):
        wide[f"c{j}"] = rng.normal(size=160)
    with pytest.raises(N.OaxacaError) as e:
        opt(wide, preds=[f"c{j}" for j in range(120)])
    assert e.value.code == N.OB_E_UNSUPPORTED and "at most 119" in str(e.value)
    with pytest.raises(ValueError):
        ob.OaxacaBuilder(R.mock_frame(), "wage", "gender", "Male").predictors(["education"]).optimize(strategy="x")


def test_score_and_allocate_check_arguments_first(N):
    import ctypes as C

    lib = N.lib()
    d = np.zeros(8)
    dp = d.ctypes.data_as(C.POINTER(C.c_double))
    rc = lib.ob_remedy_score(None, dp, 1, dp, 1, 1, 121, dp, dp, dp, dp, None, None)
    assert rc == N.OB_E_UNSUPPORTED
    rc = lib.ob_remedy_score(None, dp, 1, dp, 1, 1, 2, dp, dp, dp, dp, None, None)
    assert rc == N.OB_E_INVALID and b"null pointer" in lib.ob_last_error()
    rq = N.ob_remedy_request(0.0, 0.0, 0.95, 7, 0, 0, 0)
    h = C.c_void_p()
    rc = lib.ob_remedy_allocate(None, dp, dp, dp, 1, 1, None, 1.0, C.byref(rq), C.byref(h))
    assert rc == N.OB_E_INVALID and b"strategy" in lib.ob_last_error()


@pytest.mark.parametrize("n_a,n_b", R.SCORE_ROWS)
@pytest.mark.parametrize("k", R.SCORE_KS)
def test_score_inputs_leave_the_device_seven_eighths(n_a, n_b, k):
    """The f64 restatement sits within 1/8 of each score bar of its longdouble run, on every GPU shape."""
    import test_gpu_remedy as G

    x, y, beta, cov = G.model(n_a, n_b, k)
    f, h, r, _ = R.score(x, beta, cov, y[:n_a])
    fl, hl, rl, _ = R.score(x, beta, cov, y[:n_a], R.LD)
    fbar, hbar, rbar = R.score_bars(x, beta, cov, y[:n_a])
    ff, fh, fr = float(np.max(np.abs(f - fl) / fbar)), float(np.max(np.abs(h - hl) / hbar)), float(abs(r - rl) / rbar)
    print(f"n_a {n_a} n_b {n_b} K {k}: f64 vs longdouble, fractions of the bars fair {ff:.3g} leverage {fh:.3g} rss {fr:.3g}")
    # fair ((K + 1) roundings) and leverage (2 K + 2) are bars of fewer than 64 roundings at these K: the worst of
    # n rows of a sum of m roundings is about 3.5 / sqrt(m) of m u / 2, which no f64 evaluation keeps under an
    # eighth, so they are held to a half; rss is an n-term bar and keeps the eighth
    assert ff <= (0.5 if k + 1 < 64 else 0.125) and fh <= (0.5 if 2 * k + 2 < 64 else 0.125) and fr <= 0.125


@pytest.mark.parametrize("n_a,n_b,k", R.ALLOC_SHAPES)
@pytest.mark.parametrize("range_target", ["midpoint", "upper"])
def test_allocation_inputs_leave_the_device_seven_eighths(n_a, n_b, k, range_target):
    import test_gpu_remedy as G

    x, y, beta, cov = G.model(n_a, n_b, k)
    fair, lev, rss, _ = R.score(x, beta, cov, y[:n_a])
    z = float(R.inverse_cdf_root(0.975))
    kw = dict(budget=25.0, adjust_both_groups=True, range_target=range_target, closed_form=True)
    a = R.optimize_arrays(y, fair, lev, n_a, rss / (n_a - k), z, **kw)
    b = R.optimize_arrays(y, fair, lev, n_a, rss / (n_a - k), z, dtype=R.LD, **kw)
    bars = R.allocation_bars(b, len(y), 25.0, range_target, rss / (n_a - k))
    assert np.array_equal(a["index"], b["index"])
    fr = {"pay": float(np.max(np.abs(a["adjustment"] - b["adjustment"]) / bars["pay"])),
          "interval": float(np.max(np.abs(a["upper"] - b["upper"]) / bars["interval"])),
          "need": float(abs(a["required_budget"] - b["required_budget"]) / bars["need"]),
          "cost": float(abs(a["total_cost"] - b["total_cost"]) / bars["cost"])}
    print(f"n_a {n_a} n_b {n_b} K {k} {range_target}: f64 vs longdouble, fractions of the bars {fr}")
    # the interval's bar is six roundings wide (see above): a half; the pays and the sums keep the eighth
    assert fr.pop("interval") <= 0.5 and all(v <= 0.125 for v in fr.values())


@pytest.mark.parametrize("dtype", [np.float64, R.LD], ids=["f64", "longdouble"])
def test_restatement_satisfies_the_verification_cases(dtype):
    k = KAT["verification"]
    for rq in k["requests"]:
        res, *_ = R.optimize_frame(k, dtype, **{a: b for a, b in rq.items() if a != "name"})
        assert len(res["index"]) > 0 and np.all(res["new_wage"] - res["lower"] >= k["properties"]["min_new_minus_lower"])
        if rq["budget"] == 0.0:
            assert res["total_cost"] > 0
            assert abs(res["total_cost"] - res["required_budget"]) < k["properties"]["max_cost_minus_required"]


def test_allocate_rejects_non_finite_inputs(N):
    import ctypes as C

    lib = N.lib()
    good, bad = np.ones(4), np.array([1.0, np.nan, 1.0, 1.0])
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    rq = N.ob_remedy_request(0.0, 0.0, 0.95, 0, 0, 0, 0)
    h = C.c_void_p()
    for y, f, l in ((bad, good, good), (good, bad, good), (good, good, bad)):
        rc = lib.ob_remedy_allocate(None, dp(y), dp(f), dp(l), 2, 2, None, 1.0, C.byref(rq), C.byref(h))
        assert rc == N.OB_E_INVALID and b"non-finite" in lib.ob_last_error()


def test_frontier_closed_form_equals_the_carry_over_loop():
    """The wages y + clamp(b_s - P_i, 0, gap_i) against the reference's sequential carry-over (remedy_ref.frontier
    pays slice by slice), to the prefix bar (m + 1) u sum gap per wage; and the restatement meets the
    reference's own frontier properties."""
    kat = KAT["verification"]
    x, y, n_a, *_ = R.frame_design(kat)
    opt, *_ = R.optimize_frame(kat, np.float64)
    rows, gaps = opt["row"].tolist(), [float(v) for v in opt["adjustment"]]
    need = float(opt["required_budget"])
    budgets = [s * (need * 1.1 / 50) for s in range(51)]
    closed = R.frontier_closed_form(y, rows, gaps, budgets)
    # the sequential loop, wages only
    pend = sorted(([r, g] for r, g in zip(rows, gaps)), key=lambda p: -p[1])
    cur, idx, cursor = np.array(y, dtype=np.float64), 0, 0.0
    bar = (len(gaps) + 1) * R.U * sum(gaps)
    for s in range(1, 51):
        rem = budgets[s] - cursor
        while rem > 0 and idx < len(pend):
            if pend[idx][1] <= rem:
                cur[pend[idx][0]] += pend[idx][1]
                rem -= pend[idx][1]
                pend[idx][1] = 0.0
                idx += 1
            else:
                cur[pend[idx][0]] += rem
                pend[idx][1] -= rem
                rem = 0.0
        cursor = budgets[s]
        assert np.max(np.abs(cur - closed[s])) <= bar + 2 * R.U * np.max(np.abs(cur)), s
    f = KAT["frontier"]
    for dtype in (np.float64, R.LD):
        pts, _, _ = R.frontier(KAT[f["frame"]], f["steps"], f["max_budget"], dtype)
        assert len(pts) == f["steps"] + 1 and pts[0][0] == 0.0 and all(a[0] < b[0] for a, b in zip(pts, pts[1:]))
