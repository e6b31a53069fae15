"""The defensibility pass on the GPU over arrays (ob_remedy_defend_rows: the first-wins map, the per-adjustment pass
and the row pass) against tests/defend_ref.py in longdouble on the SAME f64 inputs; fair, leverage and sigma2 come
from NumPy, so only the new kernels are under test. The bars are derived in defend_ref.py's docstring; every test
prints its worst fraction of each bar before it asserts.

Shapes (n_A, n_B), for 256-thread blocks: (37, 91) puts the group boundary inside a wave of one block, (256, 256) is
exact blocks with the boundary on a block edge, (300, 473) three blocks of rows with a ragged tail, (1, 2) less than
a wave. The request lists (defend_ref.adjustment_lists): none, one on an A row, every B row once in shuffled order,
m = 2 n + 3 with every row hit two or three times and values of mixed sign (more adjustment blocks than row blocks),
and nine on one row."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import defend_ref as D  # noqa: E402
import remedy_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(37, 91), (256, 256), (300, 473), (1, 2)]
LISTS = ["none", "one_a_row", "every_b_once", "twice_or_thrice", "all_on_one_row"]
Z = float(R.inverse_cdf_root(0.975))
_CASES = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def case(n_a, n_b):
    """(y, fair, leverage, sigma2, request lists) of a shape, from NumPy alone. Shared and read-only."""
    if (n_a, n_b) not in _CASES:
        k = 4
        x, y = R.fixture(n_a, n_b, k, 100 * n_a + n_b, noise=1.0)
        if n_a > k:
            beta, cov = R.solve(R.gram(x[:n_a], y[:n_a]))
            fair, lev, rss, _ = R.score(x, beta, cov, y[:n_a])
            sigma2 = float(rss / (n_a - k))
        else:  # too few rows for a fit: the pass is indifferent to where its inputs come from
            rng = np.random.default_rng(n_a + n_b)
            fair, lev, sigma2 = y + rng.normal(size=len(y)), rng.uniform(0.05, 0.5, len(y)), 0.8
        lists = {name: (rows, vals) for name, rows, vals in D.adjustment_lists(n_a, n_b, 7 * n_a + n_b)}
        _CASES[(n_a, n_b)] = (y, fair, lev, sigma2, lists)
    return _CASES[(n_a, n_b)]


def compare(ob, y, fair, lev, n_a, sigma2, rows, vals, tag):
    got = ob.remedy_defend_rows(y, fair, lev, n_a, sigma2, rows, vals)
    ref = D.defend_arrays(y, fair, lev, n_a, sigma2, got["z_score"], rows, vals, R.LD)
    f64 = D.defend_arrays(y, fair, lev, n_a, sigma2, got["z_score"], rows, vals)
    m = len(rows)
    assert got["n_adjustments"] == m and np.array_equal(got["row"], rows) and got["z_score"] == ob.normal_inverse_cdf(0.975)
    assert np.array_equal(_bits(got["current_wage"]), _bits(f64["current_wage"]))
    assert np.array_equal(_bits(got["new_wage"]), _bits(f64["new_wage"]))  # one IEEE add
    assert np.array_equal(_bits(got["adjustment"]), _bits(vals)) and np.array_equal(_bits(got["fair_wage"]), _bits(f64["fair_wage"]))
    worst = {}
    if m:
        bar = np.maximum(ref["interval_bar"], 1e-300)
        worst["lower"] = float(np.max(np.abs(got["lower"] - ref["lower"]) / bar))
        worst["upper"] = float(np.max(np.abs(got["upper"] - ref["upper"]) / bar))
        assert not D.too_close(ref).any(), "a fixture row sits within the interval bar of lower - 1: choose another seed"
        assert np.array_equal(got["is_defensible"], ref["is_defensible"])
    sums = list(got["sums"]) + [got["total_cost"]]
    for name, s, want, sbar in zip(D.SUM_NAMES, sums, ref["sums"], ref["sum_bars"]):
        worst[name] = float(abs(R.LD(s) - want) / max(sbar, 1e-300))
    print(f"defend_rows {tag}: m {m}, worst fractions of the bars " + ", ".join(f"{a} {b:.3g}" for a, b in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    # the derived numbers are the header's expressions of those sums (a count of zero gives 0.0)
    n_b = len(y) - n_a
    s = got["sums"]
    assert got["original_gap"] == (s[0] / n_a if n_a else 0.0) - (s[2] / n_b if n_b else 0.0)
    assert got["new_gap"] == (s[1] / n_a if n_a else 0.0) - (s[3] / n_b if n_b else 0.0)
    assert got["original_unexplained_gap"] == (s[4] / n_b if n_b else 0.0)
    assert got["new_unexplained_gap"] == (s[5] / n_b if n_b else 0.0) and got["required_budget"] == s[6]
    return got, ref, f64


@pytest.mark.parametrize("name", LISTS)
@pytest.mark.parametrize("n_a,n_b", SHAPES)
def test_defend_rows_against_restatement(ob, n_a, n_b, name):
    y, fair, lev, sigma2, lists = case(n_a, n_b)
    rows, vals = lists[name]
    got, ref, f64 = compare(ob, y, fair, lev, n_a, sigma2, rows, vals, f"({n_a}, {n_b}) {name}")
    again = ob.remedy_defend_rows(y, fair, lev, n_a, sigma2, rows, vals)  # two calls, the same bytes
    for key in ("current_wage", "new_wage", "fair_wage", "lower", "upper", "sums"):
        assert np.array_equal(_bits(again[key]), _bits(got[key])), key
    assert again["total_cost"] == got["total_cost"] and np.array_equal(again["is_defensible"], got["is_defensible"])
    if name in ("twice_or_thrice", "all_on_one_row"):
        # the reference's own formulation: for every row, walk the list and stop at the first hit
        lit = D.defend_arrays(y, fair, lev, n_a, sigma2, got["z_score"], rows, vals, literal=True)
        for q in range(7):
            assert abs(got["sums"][q] - lit["sums"][q]) <= 2 * ref["sum_bars"][q], D.SUM_NAMES[q]
    if name == "none":
        assert got["total_cost"] == 0.0 and got["sums"][0] == got["sums"][1] and got["sums"][2] == got["sums"][3]


def test_first_adjustment_of_a_row_wins(ob):
    """+1000 then -1000 on one B row and -500 then +500 on one A row: first-wins and last-wins differ by far more
    than any bar."""
    n_a, n_b = 300, 473
    y, fair, lev, sigma2, _ = case(n_a, n_b)
    rows = np.array([n_a + 470, 5, n_a + 470, 5], dtype=np.int64)
    vals = np.array([1000.0, -500.0, -1000.0, 500.0])
    got, ref, _ = compare(ob, y, fair, lev, n_a, sigma2, rows, vals, "first wins")
    base = ob.remedy_defend_rows(y, fair, lev, n_a, sigma2, [], [])
    assert abs((got["sums"][3] - base["sums"][3]) - 1000.0) <= 2 * ref["sum_bars"][3]
    assert abs((got["sums"][1] - base["sums"][1]) + 500.0) <= 2 * ref["sum_bars"][1]
    assert got["is_defensible"].tolist() == [True, bool(ref["is_defensible"][1]), False, bool(ref["is_defensible"][3])]
    assert got["total_cost"] == 0.0


def test_both_sides_of_the_defensibility_line(ob):
    n_a, n_b = 37, 91
    y, fair, lev, sigma2, _ = case(n_a, n_b)
    lo, _ = D.interval(fair, lev, sigma2, Z, np.float64)
    rows = np.array([n_a + 3, n_a + 3, 2, 2], dtype=np.int64)
    vals = np.array([(lo[r] - 1.0 + d) - y[r] for r, d in zip(rows, (0.5, -0.5, 0.5, -0.5))])
    got, ref, _ = compare(ob, y, fair, lev, n_a, sigma2, rows, vals, "the line")
    assert got["is_defensible"].tolist() == [True, False, True, False]
    assert np.all(np.abs(np.abs(np.asarray(ref["slack"], dtype=np.float64)) - 0.5) < 1e-9)  # half a unit from the line


@pytest.mark.parametrize("sigma2", [0.0, 1e-9])
def test_degenerate_variance_collapses_the_interval(ob, sigma2):
    n_a, n_b = 300, 473
    y, fair, lev, _, lists = case(n_a, n_b)
    rows, vals = lists["twice_or_thrice"]
    got, _, _ = compare(ob, y, fair, lev, n_a, sigma2, rows, vals, f"sigma2 {sigma2}")
    assert np.array_equal(_bits(got["lower"]), _bits(got["fair_wage"])) and np.array_equal(_bits(got["upper"]), _bits(got["fair_wage"]))
    above = ob.remedy_defend_rows(y, fair, lev, n_a, np.nextafter(1e-9, 1.0), rows, vals)  # 1e-9 is the rule's own constant
    assert np.all(above["lower"] < above["fair_wage"]) and np.all(above["upper"] > above["fair_wage"])


@pytest.mark.parametrize("n_a,n_b", [(37, 91), (300, 473)])
def test_permuting_unique_indices(ob, n_a, n_b):
    y, fair, lev, sigma2, lists = case(n_a, n_b)
    rows, vals = lists["every_b_once"]
    a = ob.remedy_defend_rows(y, fair, lev, n_a, sigma2, rows, vals)
    p = np.random.default_rng(5).permutation(len(rows))
    b = ob.remedy_defend_rows(y, fair, lev, n_a, sigma2, rows[p], vals[p])
    for key in ("current_wage", "new_wage", "fair_wage", "lower", "upper", "adjustment"):
        assert np.array_equal(_bits(b[key]), _bits(a[key][p])), key
    assert np.array_equal(b["is_defensible"], a["is_defensible"][p]) and np.array_equal(b["row"], a["row"][p])
    assert np.array_equal(_bits(a["sums"]), _bits(b["sums"]))  # the seven row sums: bitwise
    bar = (len(vals) + 1) * R.U * float(np.sum(np.abs(vals)))  # total_cost is added in request order: within its bar
    print(f"permutation ({n_a}, {n_b}): total_cost moved by {abs(a['total_cost'] - b['total_cost']):.3g}, bar {2 * bar:.3g}")
    assert abs(a["total_cost"] - b["total_cost"]) <= 2 * bar


def test_getters_refuse_a_handle_of_another_kind(ob, N):
    import ctypes as C

    y, fair, lev, sigma2, _ = case(37, 91)
    lib = N.lib()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    rq = N.ob_remedy_request(0.0, 0.0, 0.95, 0, 0, 0, 0)
    h = C.c_void_p()
    N.check(lib.ob_remedy_allocate(N.context(None), dp(y), dp(fair), dp(lev), 37, 91, None, sigma2, C.byref(rq), C.byref(h)))
    try:
        info, flags = N.ob_defend_info(), C.POINTER(C.c_int32)()
        assert lib.ob_remedy_results_defend_info(h, C.byref(info)) == N.OB_E_INVALID
        assert lib.ob_remedy_results_defensible(h, C.byref(flags)) == N.OB_OK and not flags
    finally:
        lib.ob_remedy_results_free(h)
