"""OaxacaBuilder.check_defensibility (ob_remedy_defend) and verify_adjustments / decompose (ob_remedy_verify) on the
GPU, end to end, on the reference's verification frame (1000 rows, one categorical predictor) and its mock frame:
the round trip of optimize()'s own adjustments, predictor overrides against a frame edited by hand, the skipped
index, and verification against a fresh builder on the hand-adjusted frame. The end-to-end bars are derived in
tests/defend_ref.py and tests/remedy_ref.py."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import defend_ref as D  # noqa: E402
import remedy_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

KAT = json.load(open(os.path.join(HERE, "golden", "remedy_kat.json")))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _builder(ob, kat, frame):
    b = ob.OaxacaBuilder(frame, kat["outcome"], kat["group"], kat["reference_group"]).predictors(kat["predictors"])
    return b.categorical_predictors(kat["categorical"]) if kat.get("categorical") else b


def _mock_kat():
    return {"outcome": "wage", "group": "gender", "reference_group": "Male", "predictors": ["education", "experience"]}


def _same(a, b):
    """Two OptimizationResults, bit for bit."""
    assert len(a.adjustments) == len(b.adjustments)
    for f in ("adjustment", "current_wage", "new_wage", "fair_wage", "fair_wage_lower_bound", "fair_wage_upper_bound"):
        assert np.array_equal(_bits([getattr(x, f) for x in a.adjustments]), _bits([getattr(x, f) for x in b.adjustments])), f
    assert [(x.index, x.is_defensible, x.defensibility_message) for x in a.adjustments] == \
           [(x.index, x.is_defensible, x.defensibility_message) for x in b.adjustments]
    assert np.array_equal(_bits([[c.value for c in x.contributions] for x in a.adjustments]),
                          _bits([[c.value for c in x.contributions] for x in b.adjustments]))
    assert a.model_coefficients == b.model_coefficients
    for f in ("total_cost", "original_gap", "new_gap", "original_unexplained_gap", "new_unexplained_gap", "required_budget"):
        assert _bits([getattr(a, f)])[0] == _bits([getattr(b, f)])[0], f


def test_round_trip_of_optimize(ob):
    kat = KAT["verification"]
    x, y, n_a, order, names, frame = R.frame_design(kat)
    b = _builder(ob, kat, frame)
    opt = b.optimize(budget=0.0, contributions=True)
    res = b.check_defensibility(opt.adjustments)
    info = b.last_defend_info
    assert len(res.adjustments) == len(opt.adjustments) > 100 and info["n_skipped"] == 0
    assert all(a.is_defensible and a.defensibility_message == D.MSG_OK for a in res.adjustments)
    assert [a.index for a in res.adjustments] == [a.index for a in opt.adjustments]
    assert res.model_coefficients == opt.model_coefficients and info["sigma_squared"] == b.last_remedy_info["sigma_squared"]
    ref, beta, ex = D.defend_frame(kat, [(a.index, a.adjustment) for a in opt.adjustments])
    rows = ref["row"]
    margin = np.abs(ref["upper"] - ref["fair_wage"])
    ibar = ref["interval_bar"]  # the array bar: optimize() and this pass read the same fair, leverage and sigma2
    got = {f: np.array([getattr(a, f) for a in res.adjustments]) for f in
           ("fair_wage", "fair_wage_lower_bound", "fair_wage_upper_bound", "new_wage", "current_wage")}
    was = {f: np.array([getattr(a, f) for a in opt.adjustments]) for f in got}
    worst = {"fair vs optimize": float(np.max(np.abs(got["fair_wage"] - was["fair_wage"]) / ibar)),
             "lower vs optimize": float(np.max(np.abs(got["fair_wage_lower_bound"] - was["fair_wage_lower_bound"]) / ibar)),
             "upper vs optimize": float(np.max(np.abs(got["fair_wage_upper_bound"] - was["fair_wage_upper_bound"]) / ibar))}
    assert np.array_equal(_bits(got["new_wage"]), _bits(was["new_wage"])) and np.array_equal(_bits(got["current_wage"]), _bits(y[rows]))
    e2e = ibar + ex["fair_bar"][rows] + ex["margin_rel"] * margin
    worst["lower"] = float(np.max(np.abs(got["fair_wage_lower_bound"] - ref["lower"]) / e2e))
    worst["upper"] = float(np.max(np.abs(got["fair_wage_upper_bound"] - ref["upper"]) / e2e))
    bars = D.e2e_sum_bars(ref, ex)
    n_b = len(y) - n_a
    worst["required_budget"] = float(abs(res.required_budget - ref["required_budget"]) / bars["required_budget"])
    worst["original_unexplained"] = float(abs(res.original_unexplained_gap - ref["original_unexplained_gap"]) * n_b
                                          / bars["original_unexplained"])
    worst["new_unexplained"] = float(abs(res.new_unexplained_gap - ref["new_unexplained_gap"]) * n_b / bars["new_unexplained"])
    worst["total_cost"] = float(abs(res.total_cost - ref["total_cost"]) / bars["total_cost"])
    print(f"check_defensibility round trip: {len(res.adjustments)} adjustments, cond {ex['cond']:.3g}, worst fractions of "
          "the bars " + ", ".join(f"{a} {v:.3g}" for a, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    # the raw gap is the difference of the group means of the wages themselves
    gap_bar = 2 * (len(y) + 1) * R.U * float(np.mean(np.abs(y)))
    assert abs(res.original_gap - (np.mean(y[:n_a]) - np.mean(y[n_a:]))) <= gap_bar
    assert abs((res.original_gap - res.new_gap) - res.total_cost / n_b) <= 2 * gap_bar + bars["total_cost"] / n_b
    again = b.check_defensibility(opt.adjustments)
    _same(res, again)
    assert all(info[t] >= 0.0 for t in ("gram_ms", "score_ms", "defend_ms", "scatter_ms", "adjust_ms", "rows_ms"))


@pytest.mark.parametrize("which", ["verification", "mock"])
def test_overrides_equal_a_frame_edited_by_hand(ob, which):
    if which == "verification":
        kat = KAT["verification"]
        frame = R.frame_design(kat)[5]
    else:
        kat, frame = _mock_kat(), R.mock_frame()
    grp = np.array(frame[kat["group"]]) == kat["reference_group"]
    ra, rb = int(np.flatnonzero(grp)[3]), int(np.flatnonzero(~grp)[5])  # one reference-group row, one target-group row
    p0, p1 = kat["predictors"][0], kat["predictors"][-1]
    va, vb = frame[p0][ra] + 3.0, frame[p1][rb] + 2.0
    adjs = [(rb, 100.0, {p1: "999"}),                        # replaced as a whole by the later set for rb
            (ra, 0.0, {p0: str(va), "no_such_column": "1", kat["outcome"]: "5"}),
            (7, 50.0),
            (rb, 25.0, {p1: repr(vb), p0: " 12"}),           # " 12" is no Rust float: dropped
            (len(grp) + 5, 10.0, {p0: "1"})]                 # outside the frame: skipped, its override ignored
    b = _builder(ob, kat, frame)
    res = b.check_defensibility(adjs)
    assert b.last_defend_info["n_skipped"] == 1 and [a.index for a in res.adjustments] == [rb, ra, 7, rb]
    edited = {c: list(v) for c, v in frame.items()}
    edited[p0][ra] = va
    edited[p1][rb] = vb
    plain = [(i, v) for i, v, *_ in adjs]
    hand = _builder(ob, kat, edited).check_defensibility(plain)
    _same(res, hand)
    base = _builder(ob, kat, frame).check_defensibility(plain)  # the reference-group row's override moved the model
    assert base.model_coefficients != res.model_coefficients
    assert [c.name for c in base.model_coefficients] == [c.name for c in res.model_coefficients]
    # the first adjustment of rb decides its wage in the gaps; both are returned
    assert res.adjustments[0].new_wage == frame[kat["outcome"]][rb] + 100.0 and res.adjustments[3].new_wage == frame[kat["outcome"]][rb] + 25.0
    assert res.total_cost == ((100.0 + 0.0) + 50.0) + 25.0


def test_messages_and_mixed_input_forms(ob):
    kat, frame = _mock_kat(), R.mock_frame()
    b = _builder(ob, kat, frame)
    opt = b.optimize()
    a0 = opt.adjustments[0]
    res = b.check_defensibility([a0, {"index": a0.index, "value": -30000.0}, (0, -40000.0)], contributions=False)
    assert res.adjustments[0].is_defensible and res.adjustments[0].defensibility_message == D.MSG_OK
    for a in res.adjustments[1:]:
        assert a.is_defensible is False and a.contributions == []
        assert a.defensibility_message == D.message(False, a.new_wage, a.fair_wage_lower_bound)
        assert a.defensibility_message.startswith("Wage is ") and a.new_wage < a.fair_wage_lower_bound - 1.0
    empty = b.check_defensibility([])
    assert empty.adjustments == [] and empty.total_cost == 0.0 and empty.new_gap == empty.original_gap
    # optimize()'s need and required_budget add the same positive f64 terms fair - y in two orders: (c + 1) u each
    n_b = 80
    assert abs(empty.required_budget - opt.required_budget) <= 2 * (n_b + 1) * R.U * opt.required_budget


def _comps(table):
    """ComponentResults by their bytes (a NaN p-value equals itself)."""
    return [(c.name, _bits([c.estimate, c.std_err, c.t_stat, c.p_value, c.ci_lower, c.ci_upper]).tolist()) for c in table]


def _hand_adjusted(frame, outcome, adjs):
    f = {c: list(v) for c, v in frame.items()}
    f[outcome] = [float(v) for v in D.verify_wages(frame[outcome], [a[0] for a in adjs], [a[1] for a in adjs])]
    return f


def test_verify_adjustments_equals_a_fresh_builder_on_the_adjusted_frame(ob, N):
    kat = KAT["verification"]
    frame = R.frame_design(kat)[5]

    def builder(f):
        return _builder(ob, kat, f).bootstrap_reps(64).seed(1234).reference_coefficients(ob.ReferenceCoefficients.Pooled)

    opt = builder(frame).optimize()
    adjs = [(a.index, a.adjustment) for a in opt.adjustments[:200]] + [(opt.adjustments[0].index, 123.25)]  # one row twice
    got = builder(frame).verify_adjustments(adjs)
    adjusted = _hand_adjusted(frame, kat["outcome"], adjs)
    want = builder(adjusted).run()
    assert got.results.to_json() == want.to_json() and got.results.n_failed == want.n_failed
    for f in ("xa_mean", "xb_mean", "beta_star", "residuals"):
        assert np.array_equal(_bits(getattr(got.results, f)), _bits(getattr(want, f))), f
    for table in ("aggregate", "detailed_explained", "detailed_unexplained"):
        assert _comps(getattr(got.results.two_fold, table)) == _comps(getattr(want.two_fold, table))
    assert _comps(got.results.three_fold.aggregate) == _comps(want.three_fold.aggregate)
    assert got.total_gap == want.total_gap and got.explained_gap == want.explained().estimate
    assert got.unexplained_gap == want.unexplained().estimate and got.interaction_gap is None and got.interaction_percentage is None
    assert got.explained_percentage == got.explained_gap / got.total_gap * 100.0
    assert got.unexplained_percentage == got.unexplained_gap / got.total_gap * 100.0
    assert got.unexplained_standard_error == want.unexplained().std_err > 0.0
    assert _comps(got.detailed_explained) == _comps(want.two_fold.detailed_explained) and len(got.detailed_unexplained) > 0
    w = np.array(adjusted[kat["outcome"]])
    grp = np.array(frame[kat["group"]]) == kat["reference_group"]
    s = got.data_summary
    assert (s.total_count, s.group_a_count, s.group_b_count) == (len(w), int(grp.sum()), int((~grp).sum()))
    assert s.group_a_mean == float(np.mean(w[grp])) and s.group_b_mean == float(np.mean(w[~grp]))  # bitwise NumPy's
    assert abs(got.total_gap) < abs(builder(frame).run().total_gap)  # the raises close part of the gap

    three = builder(frame).verify_adjustments(adjs, three_fold=True)
    t = {c.name: c.estimate for c in want.three_fold.aggregate}
    assert (three.explained_gap, three.unexplained_gap, three.interaction_gap) == (t["endowments"], t["coefficients"], t["interaction"])
    assert three.interaction_percentage == three.interaction_gap / three.total_gap * 100.0
    assert three.detailed_explained == [] and three.unexplained_standard_error is None

    none = builder(frame).verify_adjustments([])
    plain = builder(frame).run()
    assert none.results.to_json() == plain.to_json() == builder(frame).decompose().results.to_json()
    with pytest.raises(N.OaxacaError) as e:
        builder(frame).verify_adjustments([(0, 1.0), (len(w), 2.0)])
    assert e.value.code == N.OB_E_INVALID and str(e.value) == f"Adjustment index {len(w)} is out of bounds (dataset has {len(w)} rows)"
