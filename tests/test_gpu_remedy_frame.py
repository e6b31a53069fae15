"""OaxacaBuilder.optimize (ob_remedy_run) on the GPU, end to end: every target x strategy x range_target on the
reference's verification frame (1000 rows, a categorical predictor) against the longdouble restatement within
the end-to-end bars of tests/remedy_ref.py, the same bytes as the array pieces chained by hand for both
targets, and the degenerate variances (n_A = K: dof <= 0; A on an exact line) through the whole path."""
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
_REF = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _builder(ob, kat, frame):
    b = ob.OaxacaBuilder(frame, kat["outcome"], kat["group"], kat["reference_group"]).predictors(kat["predictors"])
    return b.categorical_predictors(kat["categorical"]) if kat.get("categorical") else b


def _ref(target, strategy, range_target, budget):
    key = (target, strategy, range_target, budget)
    if key not in _REF:
        _REF[key] = R.optimize_frame(KAT["verification"], R.LD, target=target, strategy=strategy,
                                     range_target=range_target, budget=budget)
    return _REF[key]


def _pay_fraction(pay, ref, bars, strategy):
    """The worst pay error as a fraction of its bar. Greedy pay depends on the ORDER of the gaps, and this frame
    repeats its rows' features, so many gaps are equal in exact arithmetic and differ only by rounding: where the
    budget runs out inside such a group, which member is paid is not determined within the bars (nor in the
    reference). Candidates whose gap is within four fair-wage bars of the last paid gap are compared as a group,
    by the sum of their pays; everyone else one by one."""
    err = np.abs(pay - ref["adjustment"])
    tie = np.zeros(len(err), dtype=bool)
    paid = ref["adjustment"] > 0
    if strategy == "greedy" and paid.any() and not paid.all():
        last = np.min(ref["diff"][paid])
        tie = np.abs(ref["diff"] - last) <= 4 * np.max(bars["fair"])
    worst = float(np.max(err[~tie] / bars["pay"][~tie])) if (~tie).any() else 0.0
    if tie.any():
        group = abs(np.sum(pay[tie]) - np.sum(ref["adjustment"][tie])) / np.sum(bars["pay"][tie])
        worst = max(worst, float(group))
    return worst


@pytest.mark.parametrize("target", ["reference", "pooled"])
@pytest.mark.parametrize("strategy", ["greedy", "equitable"])
@pytest.mark.parametrize("range_target", ["midpoint", "lower", "upper"])
def test_optimize_against_restatement(ob, target, strategy, range_target):
    kat = KAT["verification"]
    x, y, n_a, index, names, frame = R.frame_design(kat)
    budget = 400000.0
    res = _builder(ob, kat, frame).optimize(budget=budget, target=target, strategy=strategy, range_target=range_target)
    ref, beta, sigma2, (xs, cond, n) = _ref(target, strategy, range_target, budget)
    assert [c.name for c in res.model_coefficients] == ["__ob_intercept__"] + names
    got_b = np.array([c.value for c in res.model_coefficients])
    e = cond * R.solve_e(n, len(got_b))
    fb = float(np.linalg.norm(np.asarray(got_b - beta, dtype=np.float64)) / (e * np.linalg.norm(np.asarray(beta, dtype=np.float64))))
    assert [a.index for a in res.adjustments] == ref["index"].tolist()
    if not len(ref["index"]):  # the pooled lower bound lies under every wage of the target group: nobody is a candidate
        assert (target, range_target) == ("pooled", "lower") and res.required_budget == 0.0 and res.total_cost == 0.0
        return
    xf, xm = R.e2e_extra(xs[ref["row"]], beta, cond, n)
    bars = R.allocation_bars(ref, len(y) - n_a, budget, range_target, float(sigma2), xf, xm)
    got = {f: np.array([getattr(a, g) for a in res.adjustments]) for f, g in
           (("adjustment", "adjustment"), ("fair_wage", "fair_wage"), ("lower", "fair_wage_lower_bound"),
            ("upper", "fair_wage_upper_bound"))}
    worst = {"beta": fb,
             "fair": float(np.max(np.abs(got["fair_wage"] - ref["fair_wage"]) / bars["fair"])),
             "lower": float(np.max(np.abs(got["lower"] - ref["lower"]) / bars["interval"])),
             "upper": float(np.max(np.abs(got["upper"] - ref["upper"]) / bars["interval"])),
             "pay": _pay_fraction(got["adjustment"], ref, bars, strategy),
             "need": float(abs(res.required_budget - ref["required_budget"]) / bars["need"]),
             "cost": float(abs(res.total_cost - ref["total_cost"]) / bars["cost"])}
    print(f"optimize {target} {strategy} {range_target}: {len(res.adjustments)} adjustments, cond {cond:.3g}, "
          f"worst fractions of the bars " + ", ".join(f"{a} {b:.3g}" for a, b in worst.items()))
    assert len(res.adjustments) > 100 and all(v <= 1.0 for v in worst.values()), worst
    assert res.new_gap == res.original_gap + res.total_cost / (len(y) - n_a)


@pytest.mark.parametrize("target", ["reference", "pooled"])
def test_optimize_is_the_pieces_chained_by_hand(ob, target):
    kat = KAT["verification"]
    x, y, n_a, index, names, frame = R.frame_design(kat)
    b = _builder(ob, kat, frame)
    res = b.optimize(budget=400000.0, target=target, range_target="upper", contributions=True)
    again = b.optimize(budget=400000.0, target=target, range_target="upper", contributions=True)
    assert res == again  # two calls, the same bytes
    ga = ob.vif_gram(np.column_stack([x[:n_a], y[:n_a]]))
    gf = ga + ob.vif_gram(np.column_stack([x[n_a:], y[n_a:]])) if target == "pooled" else None
    beta, cov = ob.remedy_solve(ga, gf)
    fair, lev, rss, con = ob.remedy_score(x, beta, cov, y=y[:n_a], contributions=True)
    hand = ob.remedy_allocate(y, fair, lev, n_a, rss / (n_a - x.shape[1] - 1), budget=400000.0, range_target="upper",
                              index=index)
    assert np.array_equal(_bits(beta), _bits([c.value for c in res.model_coefficients]))
    assert np.array_equal(hand["index"], [a.index for a in res.adjustments])
    for f, g in (("adjustment", "adjustment"), ("new_wage", "new_wage"), ("fair_wage", "fair_wage"),
                 ("lower", "fair_wage_lower_bound"), ("upper", "fair_wage_upper_bound")):
        assert np.array_equal(_bits(hand[f]), _bits([getattr(a, g) for a in res.adjustments])), f
    assert hand["total_cost"] == res.total_cost and hand["required_budget"] == res.required_budget
    want = con[hand["row"]]
    assert np.array_equal(_bits(want), _bits([[c.value for c in a.contributions] for a in res.adjustments]))
    assert b.last_remedy_info["sigma_squared"] == rss / (n_a - x.shape[1] - 1)


def test_verification_cases(ob):
    kat = KAT["verification"]
    frame = R.frame_design(kat)[5]
    for rq in kat["requests"]:
        res = _builder(ob, kat, frame).optimize(**{a: b for a, b in rq.items() if a != "name"})
        assert len(res.adjustments) > 0
        assert all(a.new_wage - a.fair_wage_lower_bound >= kat["properties"]["min_new_minus_lower"] for a in res.adjustments)
        if rq["budget"] == 0.0:
            assert res.total_cost > 0 and abs(res.total_cost - res.required_budget) < kat["properties"]["max_cost_minus_required"]


def test_degenerate_variance_end_to_end(ob, N):
    # n_A = K = 3: the reference's optimize_inner calls run() first, which refuses it; so does ob_remedy_run
    f = {"wage": [10.0, 13.0, 19.0, 9.0, 8.0, 12.0, 30.0], "a": [1.0, 2.0, 4.0, 1.5, 2.5, 3.0, 3.5],
         "b": [0.0, 1.0, 0.5, 2.0, 1.0, 0.0, 1.0], "g": ["r", "r", "r", "t", "t", "t", "t"]}
    with pytest.raises(N.OaxacaError) as e:
        ob.OaxacaBuilder(f, "wage", "g", "r").predictors(["a", "b"]).optimize()
    assert e.value.code == N.OB_E_INSUFFICIENT and "n_obs (3) must be strictly greater than k (3)" in str(e.value)
    # A on an exact line: rss is rounding, far under the 1e-9 rule, and every interval collapses onto the fair wage
    x = np.arange(12.0)
    f = {"wage": list(3.0 + 2.0 * x[:8]) + [5.0, 9.0, 30.0, 2.0], "x": list(x), "g": ["r"] * 8 + ["t"] * 4}
    b = ob.OaxacaBuilder(f, "wage", "g", "r").predictors(["x"])
    for rt in ("midpoint", "lower", "upper"):
        res = b.optimize(range_target=rt)
        # 1e-9 is no tolerance: it is analysis.rs:517's own rule for a degenerate interval
        assert b.last_remedy_info["sigma_squared"] <= 1e-9 and len(res.adjustments) == 3
        assert all(a.fair_wage_lower_bound == a.fair_wage == a.fair_wage_upper_bound for a in res.adjustments)
