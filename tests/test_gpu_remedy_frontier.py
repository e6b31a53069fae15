"""OaxacaBuilder.efficient_frontier (ob_remedy_frontier) on the GPU against the longdouble restatement of the
reference's loop (tests/remedy_ref.py frontier(), sequential carry-over included), each t within the bar derived
there: steps 1 and 50; max_budget below, at and above the total need; above it the tail steps' t bitwise equal;
one candidate; points[0] equal to the unadjusted pooled regression's t; the reference's own unit case."""
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


def _builder(ob, kat):
    frame = R.frame_design(kat)[5]
    b = ob.OaxacaBuilder(frame, kat["outcome"], kat["group"], kat["reference_group"]).predictors(kat["predictors"])
    return b.categorical_predictors(kat["categorical"]) if kat.get("categorical") else b


def _check(ob, name, steps, mb, kat=None):
    import math

    kat = kat or KAT[name]
    b = _builder(ob, kat)
    pts = b.efficient_frontier(steps=steps, max_budget=mb)
    if (name, steps, mb) not in _REF:  # the restatement from the engine's own f64 gaps (see remedy_ref.frontier)
        res = b.optimize()
        where = {int(v): i for i, v in enumerate(R.frame_design(kat)[3])}
        opt = {"row": np.array([where[a.index] for a in res.adjustments], dtype=np.int64),
               "adjustment": np.array([a.adjustment for a in res.adjustments]), "required_budget": R.LD(res.required_budget)}
        _REF[(name, steps, mb)] = R.frontier(kat, steps, mb, R.LD, opt=opt)
    ref, extras, info = _REF[(name, steps, mb)]
    assert len(pts) == steps + 1 and pts[0].budget == 0.0
    assert all(a.budget < b.budget for a, b in zip(pts, pts[1:]))
    worst = 0.0
    for p, (b, t, pv, sig), ex in zip(pts, ref, extras):
        bar = R.frontier_t_bar(t, ex, info)
        worst = max(worst, abs(p.t_statistic - float(t)) / bar)
        # the budgets come from the total need, an m-term sum ((m + 1) u), times 1.1, over steps, times s
        assert abs(p.budget - float(b)) <= (info["m"] + 5) * R.U * float(b)
        # p = erfc(|t| / sqrt 2): its slope in t is 2 pdf(t), plus erfc's own rounding
        assert abs(p.p_value - pv) <= 2 * math.exp(-float(t) ** 2 / 2) / math.sqrt(2 * math.pi) * bar + 8 * R.U * pv
        assert p.is_significant == (p.p_value < 0.05)
    print(f"frontier {name} steps {steps} max_budget {mb}: cond {info['cond']:.3g}, need {info['need']:.6g}, "
          f"t {pts[0].t_statistic:.6g} .. {pts[-1].t_statistic:.6g}, worst fraction of the t bar {worst:.3g}")
    assert worst <= 1.0
    return pts, info


@pytest.mark.parametrize("steps", [1, 50])
def test_frontier_steps(ob, steps):
    pts, _ = _check(ob, "verification", steps, None)
    again = _builder(ob, KAT["verification"]).efficient_frontier(steps=steps)
    assert pts == again  # the same bytes
    one = _builder(ob, KAT["verification"]).efficient_frontier(steps=1)
    assert pts[0] == one[0]  # points[0] is the unadjusted pooled regression whatever the steps


def test_frontier_max_budget_below_at_and_above_need(ob):
    need = _check(ob, "verification", 1, None)[1]["need"]
    _check(ob, "verification", 50, 0.4 * need)
    _check(ob, "verification", 50, need)
    pts, _ = _check(ob, "verification", 50, 2.0 * need)
    tail = [p for p in pts if p.budget > need * (1 + 1e3 * 1000 * R.U)]  # past every gap: the prefix bar of 500 gaps
    assert len(tail) >= 20
    bits = {np.float64(p.t_statistic).view(np.uint64) for p in tail}
    assert len(bits) == 1 and len({p.p_value for p in tail}) == 1
    assert abs(pts[-1].t_statistic) < abs(pts[0].t_statistic)


def test_frontier_one_candidate_and_reference_case(ob):
    k = dict(KAT["prediction_interval"])
    rows = [list(r) for r in k["rows"]]
    for r in rows[50:59]:
        r[0] = 400000.0  # nine of the ten target rows are paid far above the line: one candidate is left
    k["rows"] = rows
    pts, info = _check(ob, "one", 7, None, kat=k)
    assert info["m"] == 1
    f = KAT["frontier"]
    pts, _ = _check(ob, f["frame"], f["steps"], f["max_budget"])
    assert len(pts) == f["steps"] + 1 and pts[0].budget == 0.0


def test_frontier_limits(ob, N):
    b = _builder(ob, KAT["mock_csv"])
    with pytest.raises(N.OaxacaError) as e:
        b.efficient_frontier(steps=0)
    assert e.value.code == N.OB_E_INVALID
    with pytest.raises(N.OaxacaError) as e:
        b.efficient_frontier(steps=N.OB_REMEDY_MAX_STEPS + 1)
    assert e.value.code == N.OB_E_UNSUPPORTED
