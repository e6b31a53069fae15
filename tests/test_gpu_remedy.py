"""Remediation on the GPU: ob_remedy_score and ob_remedy_allocate against the NumPy restatement
(tests/remedy_ref.py, run in longdouble on the SAME f64 inputs), and OaxacaBuilder.optimize() on the
reference's own unit frames (tests/golden/remedy_kat.json). The bars are the first-order bounds derived in
remedy_ref.py's docstring; each test prints its worst fraction of the bar before it asserts.

Shapes: (n_A, n_B) in {(5, 1), (37, 5), (257, 63), (4099, 1031)} are below one 16-row block, ragged blocks,
more than one wave and several units; K in {2, 4, 16, 17, 33} puts the K + 1 columns of [C | beta] at, below
and above a 16-column block edge."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import remedy_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

KAT = json.load(open(os.path.join(HERE, "golden", "remedy_kat.json")))
_MODEL = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def model(n_a, n_b, k, seed=None, **kw):
    """A fixture with its f64 model (beta, cov from the restatement; any well-conditioned pair serves the
    score test, which compares at the same beta and cov). Shared and read-only."""
    key = (n_a, n_b, k, seed, tuple(sorted(kw.items())))
    if key not in _MODEL:
        x, y = R.fixture(n_a, n_b, k, 1000 * k + n_a if seed is None else seed, **kw)
        if n_a > k:
            beta, cov = R.solve(R.gram(x[:n_a], y[:n_a]))
        else:  # too few rows for a fit: the kernel is indifferent to where beta and cov come from
            rng = np.random.default_rng(k)
            beta = rng.uniform(0.5, 2.0, k)
            m = rng.normal(size=(k + 3, k))
            cov = np.linalg.inv(m.T @ m)
        _MODEL[key] = (x, y, beta, cov)
    return _MODEL[key]


@pytest.mark.parametrize("k", R.SCORE_KS)
@pytest.mark.parametrize("n_a,n_b", R.SCORE_ROWS)
def test_score_against_restatement(ob, n_a, n_b, k):
    x, y, beta, cov = model(n_a, n_b, k)
    fair, lev, rss, con = ob.remedy_score(x, beta, cov, y=y[:n_a], contributions=True)
    f, h, r, c = R.score(x, beta, cov, y[:n_a], R.LD)
    fbar, hbar, rbar = R.score_bars(x, beta, cov, y[:n_a])
    ff, fh, fr = float(np.max(np.abs(fair - f) / fbar)), float(np.max(np.abs(lev - h) / hbar)), float(abs(rss - r) / rbar)
    print(f"score n_a {n_a} n_b {n_b} K {k}: worst fraction of the bar fair {ff:.3g}, leverage {fh:.3g}, rss {fr:.3g}")
    assert ff <= 1.0 and fh <= 1.0 and fr <= 1.0
    assert np.array_equal(_bits(con), _bits(R.design(x) * beta[None, :]))  # one product each
    again = ob.remedy_score(x, beta, cov, y=y[:n_a])
    assert np.array_equal(_bits(again[0]), _bits(fair)) and np.array_equal(_bits(again[1]), _bits(lev)) and again[2] == rss
    assert ob.remedy_score(x, beta, cov)[2] == 0.0


def _compare(ob, y, fair, lev, n_a, sigma2, **kw):
    conf = kw.get("confidence_level", 0.95)
    got = ob.remedy_allocate(y, fair, lev, n_a, sigma2, **kw)
    z = ob.normal_inverse_cdf(R.z_p(conf))
    rk = {a: b for a, b in kw.items() if a not in ("confidence_level", "index")}
    ref = R.optimize_arrays(y, fair, lev, n_a, sigma2, z, index=kw.get("index"), dtype=R.LD, closed_form=True, **rk)
    assert got["z_score"] == z and got["n_adjustments"] == len(got["index"])
    assert np.array_equal(got["index"], ref["index"]) and np.array_equal(got["row"], ref["row"])
    n_push = len(y) if kw.get("forensic_mode") or kw.get("adjust_both_groups") else len(y) - n_a
    bars = R.allocation_bars(ref, n_push, kw.get("budget", 0.0), kw.get("range_target", "midpoint"), sigma2)
    worst = {}
    if len(ref["index"]):
        worst["pay"] = float(np.max(np.abs(got["adjustment"] - ref["adjustment"]) / bars["pay"]))
        worst["lower"] = float(np.max(np.abs(got["lower"] - ref["lower"]) / np.maximum(bars["interval"], 1e-300)))
        worst["upper"] = float(np.max(np.abs(got["upper"] - ref["upper"]) / np.maximum(bars["interval"], 1e-300)))
        assert np.array_equal(_bits(got["new_wage"]), _bits(got["current_wage"] + got["adjustment"]))
        assert np.array_equal(_bits(got["fair_wage"]), _bits(np.asarray(fair)[got["row"]]))
        assert np.array_equal(got["group"], (got["row"] >= n_a).astype(np.int32))
    tiny = 1e-300
    worst["need"] = float(abs(got["required_budget"] - ref["required_budget"]) / max(bars["need"], tiny))
    worst["cost"] = float(abs(got["total_cost"] - ref["total_cost"]) / max(bars["cost"], tiny))
    fb, yb = np.abs(np.asarray(fair[n_a:], dtype=R.LD)), np.abs(np.asarray(y[n_a:], dtype=R.LD))
    mg = z * np.sqrt(R.LD(sigma2) * (1 + np.asarray(lev[n_a:], dtype=R.LD))) if sigma2 > 1e-9 else 0 * fb
    # every diff's own bar (the interval's six roundings and the subtraction), then the m-term sum
    net_bar = float(np.sum(6 * R.U * (fb + mg) + R.U * (fb + mg + yb)) + (n_push + 1) * R.U * np.sum(fb + mg + yb)) + tiny
    worst["net"] = float(abs(got["net_residual_sum_b"] - ref["net_residual_sum_b"]) / net_bar)
    print(f"allocate {kw}: {len(ref['index'])} adjustments, worst fractions of the bars "
          + ", ".join(f"{a} {b:.3g}" for a, b in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    return got, ref


def _scored(ob, n_a=257, n_b=63, k=4, **kw):
    x, y, beta, cov = model(n_a, n_b, k, **kw)
    fair, lev, rss = ob.remedy_score(x, beta, cov, y=y[:n_a])
    return y, fair, lev, n_a, rss / (n_a - k)


@pytest.mark.parametrize("strategy", ["greedy", "equitable"])
@pytest.mark.parametrize("range_target", ["midpoint", "lower", "upper"])
def test_allocate_strategies_and_range_targets(ob, strategy, range_target):
    args = _scored(ob)
    for budget in (0.0, 25.0):
        got, ref = _compare(ob, *args, budget=budget, strategy=strategy, range_target=range_target)
        if range_target != "lower":
            assert len(got["index"]) > 20
        if budget == 0.0 and len(got["index"]):
            # the auto budget need * 1.00001 leaves 1e-5 need over every prefix, far above the prefix bar (m + 1) u
            # need: min(diff, remaining) is diff itself, the f64 target - current, bit for bit
            tgt = {"midpoint": got["fair_wage"], "lower": got["lower"], "upper": got["upper"]}[range_target]
            assert np.array_equal(_bits(got["adjustment"]), _bits(tgt - got["current_wage"]))


def test_allocate_min_gap_forensic_and_both_groups(ob):
    args = _scored(ob)
    base, _ = _compare(ob, *args)
    pct = np.sort((base["fair_wage"] - base["current_wage"]) / base["current_wage"])
    mid = float((pct[len(pct) // 2 - 1] + pct[len(pct) // 2]) / 2)  # between two candidates, away from both
    split, _ = _compare(ob, *args, min_gap_pct=mid)
    assert 0 < len(split["index"]) < len(base["index"])
    fo, _ = _compare(ob, *args, min_gap_pct=mid, forensic_mode=True)
    assert len(fo["index"]) == len(args[0]) and np.count_nonzero(fo["adjustment"]) == len(split["index"])
    both, _ = _compare(ob, *args, adjust_both_groups=True)
    assert len(both["index"]) > len(base["index"]) and (both["group"] == 0).any()
    fb, _ = _compare(ob, *args, forensic_mode=True, adjust_both_groups=True, budget=30.0)
    assert len(fb["index"]) == len(args[0])
    idx = np.arange(len(args[0]))[::-1] * 3 + 5  # any original indices: the output follows them
    _compare(ob, *args, adjust_both_groups=True, index=idx.copy())


def test_allocate_budget_boundaries_and_ties(ob):
    y, fair, lev, n_a, s2 = _scored(ob, dup=True, seed=77)
    base, ref = _compare(ob, y, fair, lev, n_a, s2)
    d = np.sort(np.asarray(ref["diff"], dtype=np.float64))[::-1]
    assert len(np.unique(d)) < len(d)  # the duplicated rows tie
    for budget in (float(np.sum(d[:7])), float(d[-1]) * 0.5, float(np.sum(d)) * 2.0, float(d[0])):
        got, r2 = _compare(ob, y, fair, lev, n_a, s2, budget=budget)
        assert got["total_cost"] - budget <= float(R.allocation_bars(r2, len(y) - n_a, budget)["cost"])
    over, _ = _compare(ob, y, fair, lev, n_a, s2, budget=float(np.sum(d)) * 2.0)
    assert np.array_equal(_bits(over["adjustment"]), _bits(base["adjustment"]))


def test_allocate_zero_candidates_and_degenerate_variance(ob):
    y, fair, lev, n_a, s2 = _scored(ob)
    rich = y.copy()
    rich[n_a:] += 100.0  # nobody in B is underpaid
    got, _ = _compare(ob, rich, fair, lev, n_a, s2)
    assert len(got["index"]) == 0 and got["required_budget"] == 0.0 and got["total_cost"] == 0.0
    # sigma2 = 0 exactly (A on an exact line, or n_A = K: dof <= 0): lower = upper = fair
    for rt in ("midpoint", "lower", "upper"):
        got, _ = _compare(ob, y, fair, lev, n_a, 0.0, range_target=rt, forensic_mode=True)
        assert np.array_equal(_bits(got["lower"]), _bits(got["fair_wage"]))
        assert np.array_equal(_bits(got["upper"]), _bits(got["fair_wage"]))
    x = np.arange(12.0)[:, None]
    line = 3.0 + 2.0 * x[:, 0]
    beta, cov = ob.remedy_solve(ob.vif_gram(np.column_stack([x[:8], line[:8]])))
    f, h, rss = ob.remedy_score(x, beta, cov, y=line[:8])
    # the fit is exact up to the solve's cond e (remedy_ref.py, end to end) and the K-term dot: so is every
    # residual, and rss is at most the eight squared
    cond = np.linalg.cond(R.gram(x[:8], line[:8]))
    fbar = R.e2e_extra(x, beta, cond, 8)[0] + R.score_bars(x, beta, cov, line[:8])[0]
    assert np.all(np.abs(f - line) <= fbar) and rss <= float(np.sum(fbar[:8] ** 2))


def test_repeat_and_large_shape_return_the_same_bytes(ob):
    y, fair, lev, n_a, s2 = _scored(ob, 4099, 1031, 17)
    a = ob.remedy_allocate(y, fair, lev, n_a, s2, budget=300.0, adjust_both_groups=True, forensic_mode=True)
    b = ob.remedy_allocate(y, fair, lev, n_a, s2, budget=300.0, adjust_both_groups=True, forensic_mode=True)
    for key in ("index", "row", "group"):
        assert np.array_equal(a[key], b[key])
    for key in ("adjustment", "new_wage", "lower", "upper"):
        assert np.array_equal(_bits(a[key]), _bits(b[key]))
    assert a["total_cost"] == b["total_cost"] and a["required_budget"] == b["required_budget"]
    _compare(ob, y, fair, lev, n_a, s2, budget=300.0, adjust_both_groups=True)


def _kat_frame(name):
    m = KAT[name]
    rows = m["rows"] * m.get("repeats", 1)
    return {c: [r[i] if isinstance(r[i], str) else float(r[i]) for r in rows] for i, c in enumerate(m["columns"])}, m


def test_builder_optimize_on_the_reference_frames(ob):
    frame, m = _kat_frame("mock_csv")
    b = ob.OaxacaBuilder(frame, m["outcome"], m["group"], m["reference_group"]).predictors(m["predictors"])
    res = b.optimize(budget=KAT["requests"][0]["budget"], contributions=True)
    assert abs(res.original_gap) > 0.0 and [c.name for c in res.model_coefficients][1:] == m["predictors"]
    for adj in res.adjustments:
        assert adj.new_wage >= adj.current_wage and adj.index < KAT["properties"]["max_index"]
        assert frame[m["group"]][adj.index] != m["reference_group"] and frame[m["outcome"]][adj.index] == adj.current_wage
        terms = [c.value for c in adj.contributions]  # two K-term sums of the same products: 2 (K + 1) u sum |terms|
        assert abs(sum(terms) - adj.fair_wage) <= 2 * (len(terms) + 1) * R.U * sum(abs(v) for v in terms)
    assert res.new_gap == res.original_gap + res.total_cost / 80  # the same expression (analysis.rs:841-845)
    # the pieces chained by hand give the same bytes
    x_t, y_t, x_r, y_r, names = b.get_data_matrices()
    x, y = np.vstack([x_r, x_t])[:, 1:], np.concatenate([y_r, y_t])
    beta, cov = ob.remedy_solve(ob.vif_gram(np.column_stack([x_r[:, 1:], y_r])))
    fair, lev, rss = ob.remedy_score(x, beta, cov, y=y_r)
    grp = np.array(frame[m["group"]]) == m["reference_group"]
    hand = ob.remedy_allocate(y, fair, lev, len(y_r), rss / (len(y_r) - x_r.shape[1]), budget=10000.0,
                              index=np.concatenate([np.flatnonzero(grp), np.flatnonzero(~grp)]))
    assert np.array_equal(hand["index"], [a.index for a in res.adjustments])
    assert np.array_equal(_bits(hand["adjustment"]), _bits([a.adjustment for a in res.adjustments]))
    assert np.array_equal(_bits(beta), _bits([c.value for c in res.model_coefficients]))
    pooled = b.optimize(target="pooled", strategy="equitable", range_target="upper", confidence_level=0.5)
    assert pooled.required_budget > 0 and b._bootstrap_reps == 20
    # test_prediction_interval
    frame, m = _kat_frame("prediction_interval")
    res = ob.OaxacaBuilder(frame, m["outcome"], m["group"], m["reference_group"]).predictors(m["predictors"]).optimize()
    assert len(res.adjustments) == 10
    for adj in res.adjustments:
        assert adj.fair_wage > m["min_fair_wage"]
        assert adj.fair_wage_lower_bound < adj.fair_wage < adj.fair_wage_upper_bound
        assert adj.fair_wage_upper_bound - adj.fair_wage_lower_bound > KAT["properties"]["min_interval_width"]
