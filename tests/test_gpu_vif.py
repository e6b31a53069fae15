"""VIF on the GPU: ob_vif and its pieces ob_vif_gram and ob_vif_sums against the NumPy restatement
(tests/vif_ref.py, run in longdouble), the reference's own unit cases (tests/golden/vif_kat.json)
through calculate_vif, and OaxacaBuilder.vif().

Shapes (vif_ref.SHAPES) and what each can break: n in {5, 63, 64, 65} at K = 3 are the edges of the Gram's
64-row sub-tile and of the residual pass's 16-row blocks; n = 4099 is several units with a ragged last
one; K in {2, 15, 16, 17, 33, 64, 65, 120} at n = 4099 puts K + 1 (Gram) and K (residuals) at, below and
above each 16-column block edge, past the logit kernel's 64 and at the limit, where the nine block
pairs per wave and the 151 KB of LDS are in use; K = 120 also at n = 2051.

Bars (first-order a-priori rounding bounds, valid for any summation order; u = 2^-53; derived in
vif_ref.py's docstring), each against the longdouble run:
  gram  |G - G*|_ab  <= n u (|Xe|'|Xe|)_ab
  sums  |ss_res - ss_res*|_j <= 2 (K + 2) u sum_i |r_ij| rho_ij + (n + 1) u ss_res_j  at the SAME f64
        coefficients and means the device is given; |ss_tot - ss_tot*|_j <= (n + 3) u ss_tot_j
  vif   relative <= [(2 n + 4) + 2 (K + 2) S_j + 4 + 2 vif_j] u + cond^3 ((n + K + 2) u)^2
Condition: the vif bar is itself <= 1e-9 relative on every fixture, asserted from n, K and
np.linalg.cond through vif_ref.vif_bar_bound. tests/test_vif_host.py shows without a GPU that the f64
restatement sits within 1/8 of each bar. Repeats, the padded leading dimension and OaxacaBuilder.vif()
are bitwise. Each test prints its worst fraction of the bar before it asserts.

The worst fractions measured on an MI355X are in DESIGN.md §5.6.1."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import vif_ref as V  # noqa: E402

pytestmark = pytest.mark.gpu

KAT = json.load(open(os.path.join(HERE, "golden", "vif_kat.json")))
IDS = [f"n{n}-k{k}" for n, k, _ in V.SHAPES]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("n,k,seed", V.SHAPES, ids=IDS)
def test_gram_against_restatement(ob, n, k, seed):
    ref = V.reference(n, k, seed)
    g = ob.vif_gram(ref["x"])
    gl = ref["ld"][1]
    worst = float(np.max(np.abs(g - gl) / ref["gram_bar"]))
    print(f"gram n {n} K {k}: worst fraction of the bar {worst:.3g}")
    assert g.shape == (k + 1, k + 1) and np.array_equal(_bits(g), _bits(g.T)) and g[k, k] == n
    assert worst <= 1.0


@pytest.mark.parametrize("n,k,seed", V.SHAPES, ids=IDS)
def test_sums_against_restatement(ob, n, k, seed):
    ref = V.reference(n, k, seed)
    b, m = ref["f64"][2], ref["f64"][3]
    ss_res, ss_tot = ob.vif_sums(ref["x"], b, m)
    a, t, rb, tb = V.sums_reference(ref["x"], b, m)
    fr, ft = float(np.max(np.abs(ss_res - a) / rb)), float(np.max(np.abs(ss_tot - t) / tb))
    print(f"sums n {n} K {k}: worst fraction of the bar ss_res {fr:.3g}, ss_tot {ft:.3g}")
    assert fr <= 1.0 and ft <= 1.0


@pytest.mark.parametrize("n,k,seed", V.SHAPES, ids=IDS)
def test_vif_against_restatement(ob, n, k, seed):
    ref = V.reference(n, k, seed)
    bound = V.vif_bar_bound(n, k, np.linalg.cond(V.gram(ref["x"])))
    assert ref["vif_bar"].max() <= bound <= 1e-9  # the bar cannot hide an error a user would see
    s = ob.vif(ref["x"])
    sl = ref["ld"][0]
    worst = float(np.max(np.abs(s - sl) / sl / ref["vif_bar"]))
    print(f"vif n {n} K {k}: scores {sl.min():.3g}..{sl.max():.3g}, bar {ref['vif_bar'].max():.3g} relative, "
          f"worst fraction of the bar {worst:.3g}")
    assert worst <= 1.0


def test_leading_dimension_with_nan_padding(ob):
    n, k, seed = V.SHAPES[8]  # (4099, 17)
    ref = V.reference(n, k, seed)
    x, b, m = ref["x"], ref["f64"][2], ref["f64"][3]
    pad = np.full((k, n + 7), np.nan)
    pad[:, :n] = x.T
    xp = pad.T[:n]
    assert xp.strides == (8, 8 * (n + 7))
    # a NaN read from the padding would have spread into its column's sums
    assert np.array_equal(_bits(ob.vif(xp)), _bits(ob.vif(x)))
    assert np.array_equal(_bits(ob.vif_gram(xp)), _bits(ob.vif_gram(x)))
    for got, want in zip(ob.vif_sums(xp, b, m), ob.vif_sums(x, b, m)):
        assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("n,k,seed", [V.SHAPES[3], V.SHAPES[9], V.SHAPES[13]], ids=["n65-k3", "n4099-k33", "n2051-k120"])
def test_repeat_returns_the_same_bytes(ob, n, k, seed):
    ref = V.reference(n, k, seed)
    x, b, m = ref["x"], ref["f64"][2], ref["f64"][3]
    assert np.array_equal(_bits(ob.vif(x)), _bits(ob.vif(x)))
    assert np.array_equal(_bits(ob.vif_gram(x)), _bits(ob.vif_gram(x)))
    first, again = ob.vif_sums(x, b, m), ob.vif_sums(x, b, m)
    assert np.array_equal(_bits(first[0]), _bits(again[0])) and np.array_equal(_bits(first[1]), _bits(again[1]))
    g = ob.vif_gram(x)
    assert np.array_equal(_bits(ob.vif_solve(g, n)), _bits(ob.vif_solve(g, n)))


def test_reference_kats_through_calculate_vif(ob, N):
    k = KAT["calculate_vif"]
    frame = {nm: col for nm, col in zip(k["names"], k["columns"])}
    res = ob.calculate_vif(frame, k["names"])
    assert [r.variable_name for r in res] == k["names"]
    err = max(abs(r.vif_score - v) for r, v in zip(res, k["vif"]))
    print(f"calculate_vif KAT: worst absolute error {err:.3g} (bar {k['abs_tol']})")
    assert err < k["abs_tol"]
    rev = ob.calculate_vif(frame, k["names"][::-1])  # the order given is the order returned
    assert [r.variable_name for r in rev] == k["names"][::-1]
    assert max(abs(r.vif_score - v) for r, v in zip(rev, k["vif"][::-1])) < k["abs_tol"]
    ints = dict(frame, x1=[int(v) for v in frame["x1"]])  # an integer column is cast
    assert [r.vif_score for r in ob.calculate_vif(ints, k["names"])] == [r.vif_score for r in res]
    k = KAT["perfect_multicollinearity"]
    with pytest.raises(N.OaxacaError) as e:
        ob.calculate_vif({nm: col for nm, col in zip(k["names"], k["columns"])}, k["names"])
    assert e.value.code == N.OB_E_LINALG and str(e.value) == "Nalgebra error: " + k["error"]
    with pytest.raises(N.OaxacaError) as e:
        ob.vif(np.array(k["columns"]).T)
    assert e.value.code == N.OB_E_LINALG
    with pytest.raises(N.OaxacaError) as e:
        ob.calculate_vif(frame, ["x1"])
    assert e.value.code == N.OB_E_DIAG and KAT["too_few_predictors"]["error"] in str(e.value)


def test_threshold_scores_infinity(ob):
    x = V.threshold_case()
    rest = V.one_minus_r2(x, V.LD)
    assert np.all(rest <= 1e-11)  # two orders under the 1e-9 rule: the outcome cannot hinge on rounding
    s = ob.vif(x)
    print(f"threshold: 1 - r2 = {[float(v) for v in rest]}, scores {s.tolist()}")
    assert np.isposinf(s).all()


def test_constant_regressand_has_zero_total(ob):
    n, k = 1000, 3
    x = V.fixture(n, k, 5)
    x[:, 1] = 2.5
    means = np.array([x[:, 0].mean(), 2.5, x[:, 2].mean()])
    ss_res, ss_tot = ob.vif_sums(x, np.zeros((k + 1, k)), means)
    assert ss_tot[1] == 0.0 and ss_tot[0] > 0 and ss_tot[2] > 0
    # zero coefficients leave the columns themselves as residuals
    assert ss_res[1] == n * 6.25 and abs(ss_res[0] - np.sum(x[:, 0] ** 2)) <= 4 * n * V.U * np.sum(x[:, 0] ** 2)


def test_builder_vif(ob):
    rng = np.random.default_rng(11)
    n = 60
    edu = rng.normal(12, 2, n)
    frame = {"wage": rng.normal(20, 3, n), "g": ["a" if i % 3 else "b" for i in range(n)], "edu": edu,
             "exp": 0.5 * edu + rng.normal(10, 4, n), "age": rng.integers(20, 60, n),
             "sector": [["x", "y", "z"][i % 3 if i % 7 else 2] for i in range(n)]}
    b = ob.OaxacaBuilder(frame, "wage", "g", "b").predictors(["edu", "exp", "age"]).categorical_predictors(["sector"])
    res = b.vif()
    xa, _, xb, _, names = b.get_data_matrices()
    assert names[0] == "__ob_intercept__" and [r.variable_name for r in res] == names[1:]
    assert names[1:] == ["edu", "exp", "age", "sector_y", "sector_z"]
    want = ob.vif(np.vstack([xa, xb])[:, 1:])
    assert np.array_equal(_bits([r.vif_score for r in res]), _bits(want))
    ref = V.vif(np.vstack([xa, xb])[:, 1:], V.LD)
    assert np.all(np.isfinite(want)) and np.max(np.abs(want - ref) / ref) <= 1e-9


def test_limits(ob, N):
    with pytest.raises(N.OaxacaError) as e:
        ob.vif(np.zeros((1000, 121)))
    assert e.value.code == N.OB_E_UNSUPPORTED
    assert N.OB_VIF_MAX_K == 120
    with pytest.raises(N.OaxacaError) as e:
        ob.vif(V.fixture(7, 7, 1))
    assert e.value.code == N.OB_E_INSUFFICIENT and "n_obs (7) must be strictly greater than k (7)" in str(e.value)
    with pytest.raises(N.OaxacaError) as e:
        ob.vif(np.zeros((10, 1)))
    assert e.value.code == N.OB_E_DIAG
