"""DFL reweighting, host side: the NumPy restatement (tests/dfl_ref.py) against the reference's own
inline tests (tests/golden/dfl_kat.json), and the native Silverman bandwidth against the
restatement; the restatement against its own extended-precision trajectory on the Newton-pass
case table, which proves the bar of tests/test_gpu_dfl_passes.py. No GPU here."""
import json
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dfl_ref as R  # noqa: E402

KAT = json.load(open(os.path.join(HERE, "golden", "dfl_kat.json")))


def _xy(case):
    return np.column_stack(case["x_columns"]), np.array(case["y"])


def test_kat_entries_cite_their_source():
    for name, entry in KAT.items():
        if not name.startswith("_"):
            assert entry["src"], name


def test_ref_logit_simple():
    k = KAT["logit_simple"]
    x, y = _xy(k)
    r = R.logit(y, x, k["max_iter"], k["tol"])
    assert np.all(np.abs(r["coefficients"] - k["coefficients"]) < k["bar"])
    assert r["converged"] and r["iterations"] > 0
    # the iteration count cannot hinge on rounding: the deciding norms are far from tol
    assert r["step_norms"][-1] <= k["tol"] / 2 and r["step_norms"][-2] >= 2 * k["tol"]
    # converged: the probabilities are those of the last iteration's start, not of the final beta
    beta_before = r["coefficients"] - R._cholesky_solve(*_newton_system(x, y, r["predicted_probs"]))
    assert np.allclose(R._probs(x, beta_before), r["predicted_probs"], rtol=0, atol=1e-12)


def _newton_system(x, y, p):
    xt = x * np.sqrt(p * (1 - p))[:, None]
    return xt.T @ xt, x.T @ (y - p)


def test_ref_logit_max_iterations():
    k = KAT["logit_max_iterations"]
    x, y = _xy(KAT["logit_simple"])
    r = R.logit(y, x, k["max_iter"], KAT["logit_simple"]["tol"])
    assert r["converged"] is k["converged"] and r["iterations"] == k["iterations"]
    assert np.array_equal(r["predicted_probs"], R._probs(x, r["coefficients"]))  # recomputed (logit.rs:108-110)


def test_ref_logit_singular():
    k = KAT["logit_singular"]
    x, y = _xy(k)
    with pytest.raises(R.LinalgError) as e:
        R.logit(y, x, k["max_iter"], k["tol"])
    assert k["message"] in str(e.value)


def test_ref_logit_perfect_separation():
    k = KAT["logit_perfect_separation"]
    x, y = _xy(k)
    try:
        r = R.logit(y, x, k["max_iter"], k["tol"])
    except R.LinalgError:
        return
    # in f64 the clamp keeps the information matrix positive definite: 100 iterations, unconverged
    assert not r["converged"] and r["iterations"] == 100


def test_ref_gaussian_kernel():
    bar = KAT["gaussian_kernel"]["bar"]
    k0 = 1.0 / math.sqrt(2.0 * math.pi)
    assert abs(R.gaussian_kernel(np.float64(0.0)) - k0) < bar
    assert abs(R.gaussian_kernel(np.float64(1.0)) - R.gaussian_kernel(np.float64(-1.0))) < bar
    assert abs(R.gaussian_kernel(np.float64(1.0)) - k0 * math.exp(-0.5)) < bar


@pytest.mark.parametrize("name", ["kde_uniform", "kde_weighted"])
def test_ref_kde(name):
    k = KAT[name]
    d = R.kde(k["data"], k["weights"], k["grid"], k["bandwidth"])
    assert len(d) == 1
    phi = [math.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi) for u in k["u"]]
    expected = sum(w * p for w, p in zip(k["w_normalised"], phi)) / k["bandwidth"]
    assert abs(d[0] - expected) < k["bar"]


def test_ref_silverman():
    k = KAT["silverman"]
    assert abs(R.silverman_bandwidth(k["data"]) - k["expected"]) < k["bar"]


def test_ref_dfl_categorical():
    k = KAT["dfl_categorical"]
    x, names = R.design(k["frame"], k["predictors"])
    assert names == ["__ob_intercept__", "x_num", "x_cat_C2", "x_cat_C3"]
    r = R.run_dfl(k["frame"], k["outcome"], k["group"], k["reference_group"], k["predictors"])
    assert len(r["grid"]) == k["grid_points"] and r["group_a"] == "A" and (r["n_a"], r["n_b"]) == (6, 6)
    assert r["converged"] and r["iterations"] == 3
    for key in ("density_a", "density_b", "density_b_counterfactual"):
        assert len(r[key]) == k["grid_points"] and np.all(np.isfinite(r[key])) and np.all(r[key] >= 0)
    assert r["grid"][0] == 10.0 and r["grid"][-1] < 22.0  # the maximum is excluded (dfl.rs:172)


def test_ref_dfl_third_group_and_errors():
    f = {"y": [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0],
         "g": ["b", "a", "c", "a", "b", "c", "a", "b"],
         "x": [0.1, 0.9, 0.4, 0.2, 0.8, 0.5, 0.6, 0.3]}
    r = R.run_dfl(f, "y", "g", "b", ["x"])
    assert r["group_a"] == "a" and (r["n_a"], r["n_b"]) == (3, 3)
    assert len(r["weights"]) == 5  # every non-A row is reweighted, "c" rows included
    with pytest.raises(R.DflError) as e:
        R.run_dfl(dict(f, y=[1, 2, 3, 4, 5, 6, 7, 8]), "y", "g", "b", ["x"])
    assert e.value.kind == "polars"
    with pytest.raises(R.DflError) as e:
        R.run_dfl(dict(f, y=[1.0, None, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]), "y", "g", "b", ["x"])
    assert e.value.kind == "group" and R.NULL_OUTCOME_MESSAGE in str(e.value)
    with pytest.raises(R.DflError) as e:
        R.run_dfl(f, "y", "g", "zz", ["x"])
    assert e.value.kind == "group"


# ---- the Newton-pass case table (dfl_ref.PASS_CASES) and its bar ---------------------------------

def _case_params():
    return [pytest.param(c, id=c.id, marks=[] if R.EXTENDED or not c.big else pytest.mark.skip(reason=R.BIG_SKIP))
            for c in R.PASS_CASES]


def test_logit_trajectory_f64_is_the_restatement():
    """In f64 the trajectory is ``logit`` itself up to the order of its sums."""
    x, y = R.panel(257, 4, 3)
    tr = R.logit_trajectory(y, x, 3, np.float64)
    for t in (1, 2, 3):
        r = R.logit(y, x, t, 0.0)
        assert not r["converged"] and r["iterations"] == t
        assert np.allclose(tr["betas"][t - 1], r["coefficients"], rtol=1e-13, atol=0)
        assert np.allclose(tr["step_norms"][:t], r["step_norms"], rtol=1e-10, atol=0)
        p_t = tr["probs_start"][t] if t < 3 else tr["final_probs"]
        assert np.allclose(p_t, r["predicted_probs"], rtol=0, atol=1e-14)
    assert np.array_equal(tr["probs_start"][0], np.full(257, 0.5)) and len(tr["conds"]) == 3


@pytest.mark.parametrize("case", _case_params())
def test_restatement_within_an_eighth_of_the_bar(case):
    """The f64 restatement against the extended trajectory, every case and every t: beta within 1/8
    of 512 cond(H_t) 2^-52 and the probabilities within 1.25e-13, so the reference alone sits well
    inside the bars tests/test_gpu_dfl_passes.py holds the device to. Worst seen: 0.012 of the bar
    (3000 x 48) and 6.5e-16 (262145 x 17)."""
    x, y = case.data()
    tr = case.trajectory()
    assert len(tr["betas"]) >= case.steps() >= 1
    if case.converges:
        conv, norms = case.converged(), case.converged()["step_norms"]
        # the iteration count cannot hinge on rounding: the deciding norms are far from tol
        assert conv["converged"] and norms[-1] <= 1e-6 / 2 and norms[-2] >= 2 * 1e-6, norms
        assert len(tr["betas"]) == conv["iterations"]
    worst_b = worst_p = 0.0
    for t in range(1, case.steps() + 1):
        r = R.logit(y, x, t, 0.0)  # tol = 0: never converges early
        assert not r["converged"] and r["iterations"] == t
        ref = tr["betas"][t - 1]
        err = float(np.max(np.abs(r["coefficients"] - ref)) / np.max(np.abs(ref)))
        bar = R.beta_bar(tr["conds"][t - 1])
        p_t = tr["probs_start"][t] if t < len(tr["betas"]) else tr["final_probs"]
        perr = float(np.max(np.abs(r["predicted_probs"] - p_t)))
        worst_b, worst_p = max(worst_b, err / bar), max(worst_p, perr)
        assert err <= bar / 8, (case.id, t, err, bar)
        assert perr <= 1.25e-13, (case.id, t, perr)
    print(f"{case.id}: restatement at {worst_b:.4f} of the bar, probabilities off by {worst_p:.2e}")
    assert float(np.max(np.abs(x @ tr["betas"][-1].astype(np.float64)))) < 45.0  # the 1e-12 bar's premise


def test_saturated_case_binds_both_clamps():
    case = next(c for c in R.PASS_CASES if c.saturated)
    tr = case.trajectory()
    lo = [int(np.sum(p == np.longdouble(1e-10))) for p in tr["probs_start"]]
    hi = [int(np.sum(p == np.longdouble(1.0 - 1e-10))) for p in tr["probs_start"]]
    print("saturated case: rows on the lower / upper clamp per iteration", lo, hi)
    assert any(a > 0 and b > 0 for a, b in zip(lo, hi))
    held = range(case.steps())  # ... within the iterations held to the bar, not only later ones
    assert any(lo[t] > 0 and hi[t] > 0 for t in held)


def _silverman_cases():
    rng = np.random.default_rng(11)
    # n * 0.25 whole (4, 8, 100, 1000) and fractional (1, 2, 3, 5, 7, 10, 101, 999), with ties
    for n in (1, 2, 3, 4, 5, 7, 8, 10, 100, 101, 999, 1000):
        yield np.round(rng.normal(20.0, 5.0, n), 0)  # rounded: many ties
        yield rng.normal(-3.0, 0.5, n)
    yield np.full(9, 2.5)  # zero spread


def test_native_silverman_matches_ref(ob):
    for data in _silverman_cases():
        a, b = ob.silverman_bandwidth(data), R.silverman_bandwidth(data)
        assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-12 * abs(b), (len(data), a, b)
    k = KAT["silverman"]
    assert abs(ob.silverman_bandwidth(k["data"]) - k["expected"]) < k["bar"]


def test_native_silverman_rejects_empty(ob, N):
    with pytest.raises(N.OaxacaError) as e:
        ob.silverman_bandwidth([])
    assert e.value.code == N.OB_E_INVALID


def test_dfl_result_surface(ob):
    r = ob.DflResult(np.array([0.0, 1.0]), np.array([0.1, 0.2]), np.array([0.3, 0.4]), np.array([0.5, 0.6]))
    d = json.loads(r.to_json())
    assert list(d) == ["grid", "density_a", "density_b", "density_b_counterfactual"]
    assert d["density_b_counterfactual"] == [0.5, 0.6]
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="matplotlib"):
            r.plot()
