"""The matching checker itself (tests/match_ref.py) against the reference's own test cases
(tests/golden/match_kat.json), the two rules that make the engine's answer well defined (the weight
accumulation and the tie key), and the header's declarations. No GPU compute here."""
import json
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import match_ref as M  # noqa: E402

KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "match_kat.json")))


def _frame(case):
    if "treated" in case:
        return {"treated": case["treated"], "income": case["income"], "education": case["education"]}
    return {"treatment": case["treatment_values"], "outcome": case["outcome_values"], "age": case["age"],
            "education": case["education"]}


def _check(case, w):
    e = case["expect"]
    assert len(w) == e["length"]
    assert all(v >= 0.0 for v in w[:e.get("nonnegative_first", len(w))])
    for i, v in e.get("equals", {}).items():
        assert w[int(i)] == v
    if "sum_rows" in e:
        assert sum(w[i] for i in e["sum_rows"]) >= e["sum_at_least"]


@pytest.mark.parametrize("name", ["matching_basic", "engine_inline", "psm"])
def test_restatement_passes_reference_tests(name):
    case = KAT[name]
    assert case["src"]
    if case["method"] == "psm":
        w = M.match_psm(_frame(case), case["treatment"], case["outcome"], case["covariates"], case["k"])
    else:
        w = M.run_matching(_frame(case), case["treatment"], case["covariates"], case["k"], False)
    _check(case, list(w))


def test_distance_cases():
    e = KAT["euclidean_distance"]
    assert math.sqrt(M.dist2([e["a"]], [e["b"]])[0, 0]) == e["distance"]
    m = KAT["mahalanobis_distance"]
    for case in m["cases"]:
        l = M.cholesky_lower(np.array(case["inv_cov"]))  # d(a, b) = ||a L - b L|| (engine.rs:155-161)
        d = math.sqrt(M.dist2(np.array([m["a"]]) @ l, np.array([m["b"]]) @ l)[0, 0])
        want = case["distance"] if "distance" in case else math.sqrt(case["distance2"])
        assert abs(d - want) <= case["tol"]


def test_logistic_or_gate():
    c = KAT["logistic_or_gate"]
    fit = M.logistic(np.array(c["x"]), np.array(c["y"]), c["max_iter"], c["tol"])
    assert all(fit["scores"][i] < 0.5 for i in c["below_half"])
    assert all(fit["scores"][i] > 0.5 for i in c["above_half"])


def test_weight_accumulation_is_not_m_over_k():
    """engine.rs:206-208 adds 1.0 / k once per match. For k = 3 the sequence leaves m / 3 in the
    last bits for some m, so an engine that divided the count by k would not return the reference's
    weights."""
    t = M.weight_table(3, 1000)
    w, differs = 0.0, 0
    for m in range(1, 1001):
        w += 1.0 / 3.0
        assert t[m] == w
        differs += t[m] != m / 3.0
    assert t[0] == 0.0 and t[1] == 1.0 / 3.0
    print("k = 3: the sequential sum differs from m / 3 for", differs, "of 1000 counts")
    assert differs > 0
    assert all(M.weight_table(2, 50)[m] == m / 2.0 for m in range(51))  # a power of two is exact


def test_tie_key_is_distance_then_position():
    """Controls 1, 3 and 4 are at squared distance exactly 1 from the query, control 0 at 4 and
    control 2 at 0.25: the order is 2, then 1, 3, 4 by position, then 0."""
    q = np.array([[0.0, 0.0]])
    c = np.array([[2.0, 0.0], [1.0, 0.0], [0.5, 0.0], [0.0, -1.0], [-1.0, 0.0]])
    idx, dd = M.knn(q, c, 5)
    assert idx.tolist() == [[2, 1, 3, 4, 0]]
    assert dd.tolist() == [[0.25, 1.0, 1.0, 1.0, 4.0]]
    idx, dd = M.knn(q, c, 3)
    assert idx.tolist() == [[2, 1, 3]]
    idx, dd = M.knn(q, c, 7)  # k > n_c
    assert idx.tolist() == [[2, 1, 3, 4, 0, -1, -1]] and np.isinf(dd[0, 5:]).all()
    frame = {"t": [1, 0, 0, 0, 0, 0], "a": [0.0] + c[:, 0].tolist(), "b": [0.0] + c[:, 1].tolist()}
    w = M.run_matching(frame, "t", ["a", "b"], 2)
    assert w.tolist() == [1.0, 0.0, 0.5, 0.5, 0.0, 0.0]


def test_distance_is_the_unfused_sum_in_covariate_order():
    rng = np.random.default_rng(7)
    q, c = rng.normal(size=(3, 9)), rng.normal(size=(4, 9))
    d = M.dist2(q, c)
    for i in range(3):
        for j in range(4):
            s = 0.0
            for a, b in zip(q[i].tolist(), c[j].tolist()):
                t = a - b
                s = s + t * t
            assert d[i, j] == s


def test_frame_rules():
    f = {"t": [1.0, 0.0, 0.0, 2.0, None], "x": [0.0, 1.0, 5.0, 0.0, 0.0], "y": [1.0, 2.0, 3.0, None, 4.0]}
    assert M.run_matching(f, "t", ["x"], 1).tolist() == [1.0, 1.0, 0.0, 0.0, 0.0]
    assert M.run_matching(f, "t", ["x"], 0).tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
    assert M.run_matching(dict(f, t=[1, 0, 0, 2, None]), "t", ["x"], 1).tolist() == [1.0, 1.0, 0.0, 0.0, 0.0]
    for frame, args, kind, msg in [
        (dict(f, t=["1", "0", "0", "2", None]), ("t", ["x"], 1), "polars", ""),
        (f, ("nope", ["x"], 1), "polars", "not found"),
        (f, ("t", ["nope"], 1), "polars", "not found"),
        (dict(f, x=[0.0, None, 5.0, 0.0, 0.0]), ("t", ["x"], 1), "polars", "null value"),
        (dict(f, x=[0.0, math.inf, 5.0, 0.0, 0.0]), ("t", ["x"], 1), "diag", M.NON_FINITE),
        (dict(f, t=[1.0, 0.0, 3.0, 2.0, None]), ("t", ["x"], 1, True), "diag", M.COV_TOO_FEW),
        (dict(f, x=[0.0, 1.0, 1.0, 0.0, 0.0]), ("t", ["x"], 1, True), "diag", M.COV_SINGULAR),
    ]:
        with pytest.raises(M.MatchError) as e:
            M.run_matching(frame, *args)
        assert e.value.kind == kind and msg in str(e.value)
    for frame, kind, msg in [
        (dict(f, t=[1.0, 1.0, 1.0, 2.0, None]), "group", M.EMPTY_GROUP),
        (dict(f, y=[1.0, None, 3.0, None, 4.0]), "group", M.NULL_OUTCOME),
        (dict(f, y=[1, 2, 3, None, 4]), "polars", "Float64"),
        (dict(f, t=[1, 0, 0, 2, None]), "polars", "Float64"),
    ]:
        with pytest.raises(M.MatchError) as e:
            M.match_psm(frame, "t", "y", ["x"], 1)
        assert e.value.kind == kind and msg in str(e.value)
    with pytest.raises(M.MatchError) as e:
        M.match_psm(f, "t", "nope", ["x"], 1)
    assert e.value.kind == "polars"


def test_inverse_and_cholesky_restatements():
    rng = np.random.default_rng(11)
    for d in (1, 2, 3, 4, 5, 20, 33):
        a = rng.normal(size=(d + 5, d))
        s = a.T @ a
        inv = M.try_inverse(s)
        assert np.allclose(inv @ s, np.eye(d), atol=1e-8)
        l = M.cholesky_lower(inv)
        assert np.allclose(l @ l.T, inv, rtol=1e-10, atol=1e-12) and np.all(np.triu(l, 1) == 0.0)
    assert M.try_inverse(np.zeros((2, 2))) is None
    assert M.try_inverse(np.zeros((6, 6))) is None
    assert M.cholesky_lower(np.array([[1.0, 2.0], [2.0, 1.0]])) is None


def test_header_declares_matching():
    text = open(os.path.join(ROOT, "include", "oaxaca_boot.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for fn in ("ob_knn", "ob_match_logistic", "ob_match_run", "ob_match_results_get", "ob_match_results_info",
               "ob_match_results_free"):
        assert re.search(r"\b%s\s*\(" % fn, code), fn
    for word in ("OB_MATCH_MAX_DIM 64", "OB_MATCH_MAX_K 16", "OB_MATCH_EUCLIDEAN", "OB_MATCH_MAHALANOBIS",
                 "OB_MATCH_PSM", "ob_match_config", "ob_match_info"):
        assert word in code, word
    assert "(squared distance, control position)" in text  # the tie rule is documented
