"""DFL reweighting on the GPU: ob_logit, ob_kde and ob_dfl_run / run_dfl against the NumPy
restatement (tests/dfl_ref.py) and the reference's inline tests (tests/golden/dfl_kat.json).

Bars: the reference's own 1e-4 on the statsmodels coefficients; 1e-6 (the project's parity bar,
test_gpu_parity.py) on coefficients relative to max|beta|, on probabilities (absolute) and on each
density relative to that array's maximum; 1e-10 x max density on ob_kde alone: a sum of at most
4099 positive terms (n u ~ 5e-13) plus exp's argument rounding (|u^2 / 2| eps < 1e-13), with two
decades of margin. Each test prints its worst figure before it asserts.

Perfect separation (logit.rs:149-163): the device, like the restatement, runs all 100 iterations
unconverged and returns OB_OK -- the clamp to [1e-10, 1 - 1e-10] keeps the weights positive.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dfl_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

KAT = json.load(open(os.path.join(HERE, "golden", "dfl_kat.json")))
TOL = 1e-6
_D = C.POINTER(C.c_double)


def _dp(a):
    return None if a is None else a.ctypes.data_as(_D)


def _ob_logit(N, x, y, max_iter=100, tol=TOL, ldx=None, want_probs=True):
    """ob_logit through ctypes -> (rc, beta, probs, converged, iterations); x is (n, k)."""
    n, k = x.shape
    ldx = n if ldx is None else ldx
    buf = np.full((k, ldx), np.nan)  # column-major with padding rows the kernel must not read
    buf[:, :n] = x.T
    y = np.ascontiguousarray(y, dtype=np.float64)
    beta, probs = np.full(k, np.nan), np.full(n, np.nan)
    conv, iters = C.c_int32(-1), C.c_int32(-1)
    rc = N.lib().ob_logit(N.context(0), _dp(buf), ldx, _dp(y), n, k, max_iter, tol, _dp(beta),
                          _dp(probs) if want_probs else None, C.byref(conv), C.byref(iters))
    return rc, beta, probs, conv.value, iters.value


def _kat_xy(case):
    return np.column_stack(case["x_columns"]), np.array(case["y"])


def _panel(n, k, seed):
    """Random normal design with an intercept, beta ~ 0.5 / sqrt(K)."""
    rng = np.random.default_rng(seed)
    x = np.column_stack([np.ones(n), rng.normal(size=(n, k - 1))])
    beta = rng.normal(size=k) * 0.5 / np.sqrt(k)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-(x @ beta)))).astype(np.float64)
    return x, y


# ---- logit: the reference's inline tests --------------------------------------------------------

def test_logit_kat_simple(N):
    k = KAT["logit_simple"]
    x, y = _kat_xy(k)
    ref = R.logit(y, x, k["max_iter"], k["tol"])
    assert ref["step_norms"][-1] <= k["tol"] / 2 and ref["step_norms"][-2] >= 2 * k["tol"]
    rc, beta, probs, conv, iters = _ob_logit(N, x, y, k["max_iter"], k["tol"])
    print("logit KAT: beta", beta, "iterations", iters)
    assert rc == N.OB_OK
    assert np.all(np.abs(beta - k["coefficients"]) < k["bar"])
    assert conv == 1 and iters == ref["iterations"]
    assert np.max(np.abs(probs - ref["predicted_probs"])) <= 1e-6


def test_logit_kat_max_iterations(N):
    k = KAT["logit_max_iterations"]
    x, y = _kat_xy(KAT["logit_simple"])
    rc, beta, probs, conv, iters = _ob_logit(N, x, y, k["max_iter"], KAT["logit_simple"]["tol"])
    assert rc == N.OB_OK and conv == 0 and iters == k["iterations"]
    ref = R.logit(y, x, k["max_iter"], KAT["logit_simple"]["tol"])
    assert np.max(np.abs(probs - ref["predicted_probs"])) <= 1e-6  # recomputed with the final beta


def test_logit_kat_singular(N):
    k = KAT["logit_singular"]
    x, y = _kat_xy(k)
    rc, *_ = _ob_logit(N, x, y, k["max_iter"], k["tol"])
    assert rc == N.OB_E_LINALG
    msg = N.lib().ob_last_error().decode()
    assert k["message"] in msg and R.LINALG_MESSAGE in msg


def test_logit_kat_perfect_separation(N):
    k = KAT["logit_perfect_separation"]
    x, y = _kat_xy(k)
    rc, beta, probs, conv, iters = _ob_logit(N, x, y, k["max_iter"], k["tol"])
    print("perfect separation: rc", rc, "converged", conv, "iterations", iters, "beta", beta)
    assert rc in (N.OB_OK, N.OB_E_LINALG)
    if rc == N.OB_OK:
        assert np.all(np.isfinite(beta))


# ---- logit against the restatement --------------------------------------------------------------

LOGIT_CASES = [  # (n, k, ldx, seed)
    (257, 3, None, 1),
    (4099, 9, None, 2),
    (70001, 21, None, 3),
    (3000, 64, None, 4),   # K_max: four column blocks
    (1000, 5, 1037, 5),    # ldx > n
    (37, 4, None, 6),      # fewer rows than a wave's 64-row sub-tile
    (3000, 33, None, 7),   # three column blocks
]


@pytest.mark.parametrize("n,k,ldx,seed", LOGIT_CASES)
def test_logit_matches_ref(N, n, k, ldx, seed):
    x, y = _panel(n, k, seed)
    ref = R.logit(y, x, 100, TOL)
    norms = ref["step_norms"]
    # rounding cannot change the iteration count: the deciding norms are far from tol
    assert ref["converged"] and norms[-1] <= TOL / 2 and norms[-2] >= 2 * TOL, norms
    rc, beta, probs, conv, iters = _ob_logit(N, x, y, 100, TOL, ldx=ldx)
    assert rc == N.OB_OK, N.lib().ob_last_error().decode()
    eb = np.max(np.abs(beta - ref["coefficients"])) / np.max(np.abs(ref["coefficients"]))
    ep = np.max(np.abs(probs - ref["predicted_probs"]))
    print(f"logit n={n} k={k}: iterations {iters} (ref {ref['iterations']}), beta err {eb:.3e}, prob err {ep:.3e}")
    assert conv == 1 and iters == ref["iterations"]
    assert eb <= 1e-6 and ep <= 1e-6


def test_logit_k_limit_and_null_probs(N):
    assert N.OB_LOGIT_MAX_K == 64
    x, y = _panel(200, N.OB_LOGIT_MAX_K + 1, 8)
    rc, *_ = _ob_logit(N, x, y)
    assert rc == N.OB_E_UNSUPPORTED
    x, y = _panel(300, 4, 9)
    rc, beta, _, conv, iters = _ob_logit(N, x, y, want_probs=False)
    rc2, beta2, *_ = _ob_logit(N, x, y)
    assert rc == N.OB_OK and rc2 == N.OB_OK and conv == 1 and np.array_equal(beta, beta2)


def test_logit_python_wrapper(ob):
    x, y = _panel(500, 4, 10)
    beta, probs, conv, iters = ob.logit(y, x)
    ref = R.logit(y, x)
    assert conv and iters == ref["iterations"]
    assert np.max(np.abs(beta - ref["coefficients"])) <= 1e-6 * np.max(np.abs(ref["coefficients"]))
    assert np.max(np.abs(probs - ref["predicted_probs"])) <= 1e-6


# ---- KDE ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3, 255, 257, 4099])
def test_kde_matches_ref(ob, n):
    rng = np.random.default_rng(100 + n)
    data = rng.normal(size=n)
    h = R.silverman_bandwidth(data) if n >= 3 else 0.4
    w_rand = rng.random(n) + 0.05
    w_zero = w_rand.copy()
    w_zero[::3] = 0.0
    if n == 1:
        w_zero = None  # a lone zero weight has no normalisation
    worst = 0.0
    for n_grid in (1, 100, 257):
        grid = np.linspace(-4.0, 4.0, n_grid) if n_grid > 1 else np.array([0.25])
        for w in (None, w_rand, w_zero):
            got = ob.kde(data, grid, h, weights=w)
            ref = R.kde(data, w, grid, h)
            err = np.max(np.abs(got - ref)) / np.max(ref)
            worst = max(worst, err)
            assert got.shape == (n_grid,) and err <= 1e-10, (n, n_grid, err)
    print(f"kde n={n}: worst error / max density {worst:.3e}")


def test_kde_far_tail_is_exact_zero(ob):
    data = np.random.default_rng(7).normal(size=257)
    got = ob.kde(data, np.array([0.0, 1e3, -1e3, 1e200]), 0.3, weights=None)
    assert got[0] > 0 and np.array_equal(got[1:], np.zeros(3))
    got = ob.kde(data, np.array([1e3, 1e200]), 0.3, weights=np.linspace(0.0, 1.0, 257))
    assert np.array_equal(got, np.zeros(2))


# ---- determinism --------------------------------------------------------------------------------

def test_two_runs_give_identical_bytes(ob, N):
    x, y = _panel(4099, 9, 2)
    a, b = _ob_logit(N, x, y), _ob_logit(N, x, y)
    assert a[0] == N.OB_OK and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    rng = np.random.default_rng(3)
    data, w, grid = rng.normal(size=4099), rng.random(4099), np.linspace(-3, 3, 257)
    assert ob.kde(data, grid, 0.2, weights=w).tobytes() == ob.kde(data, grid, 0.2, weights=w).tobytes()


# ---- ob_dfl_run / run_dfl -----------------------------------------------------------------------

def _frame(n, seed, third_group):
    rng = np.random.default_rng(seed)
    labels = ["east", "north", "west"] if third_group else ["north", "west"]
    g = rng.choice(labels, size=n, p=[0.2, 0.45, 0.35] if third_group else [0.55, 0.45])
    is_a = g == "north"
    x1 = rng.normal(size=n) + 0.4 * is_a
    x2 = rng.integers(18, 60, size=n)
    cat = rng.choice(["high", "low", "mid"], size=n, p=[0.3, 0.3, 0.4])
    y = 2.0 + 0.5 * x1 + 0.02 * x2 + 0.3 * (cat == "mid") + 0.4 * is_a + rng.normal(scale=0.7, size=n)
    return {"wage": y.tolist(), "region": g.tolist(), "x1": x1.tolist(), "x2": x2.tolist(), "cat": cat.tolist()}


PREDICTORS = ["x1", "x2", "cat"]


@pytest.fixture(scope="module")
def two_group():
    f = _frame(3000, 21, False)  # reference "west": not the alphabetically first, A = "north"
    return f, "west", R.run_dfl(f, "wage", "region", "west", PREDICTORS)


@pytest.fixture(scope="module")
def three_group():
    f = _frame(3000, 22, True)  # reference "east": A = "north", and "west" rows have target 0 too
    return f, "east", R.run_dfl(f, "wage", "region", "east", PREDICTORS)


def _check_against_ref(res, ref):
    norms = ref["step_norms"]
    assert ref["converged"] and norms[-1] <= TOL / 2 and norms[-2] >= 2 * TOL, norms
    assert res.grid.tobytes() == ref["grid"].tobytes()
    assert (res.n_a, res.n_b, res.group_a) == (ref["n_a"], ref["n_b"], ref["group_a"])
    assert res.logit_iterations == ref["iterations"] and res.logit_converged
    assert abs(res.bandwidth_a - ref["bandwidth_a"]) <= 1e-12 * ref["bandwidth_a"]
    assert abs(res.bandwidth_b - ref["bandwidth_b"]) <= 1e-12 * ref["bandwidth_b"]
    for key in ("density_a", "density_b", "density_b_counterfactual"):
        err = np.max(np.abs(getattr(res, key) - ref[key])) / np.max(ref[key])
        print(f"dfl {key}: error / max {err:.3e}")
        assert err <= 1e-6, (key, err)


def test_dfl_two_groups(ob, two_group):
    f, refgroup, ref = two_group
    assert ref["group_a"] == "north" and ref["n_a"] + ref["n_b"] == 3000
    _check_against_ref(ob.run_dfl(f, "wage", "region", refgroup, PREDICTORS), ref)


def test_dfl_third_group_rows_are_reweighted(ob, three_group):
    f, refgroup, ref = three_group
    assert ref["group_a"] == "north" and ref["n_a"] + ref["n_b"] < 3000
    assert len(ref["weights"]) == 3000 - ref["n_a"] > ref["n_b"]  # every non-A row has target 0
    _check_against_ref(ob.run_dfl(f, "wage", "region", refgroup, PREDICTORS), ref)


def test_dfl_reference_frame(ob):
    k = KAT["dfl_categorical"]
    ref = R.run_dfl(k["frame"], k["outcome"], k["group"], k["reference_group"], k["predictors"])
    assert ref["iterations"] == 3 and ref["step_norms"][-1] <= TOL / 2 and ref["step_norms"][-2] >= 2 * TOL
    res = ob.run_dfl(k["frame"], k["outcome"], k["group"], k["reference_group"], k["predictors"])
    assert len(res.grid) == k["grid_points"] == len(res.density_a) == len(res.density_b_counterfactual)
    _check_against_ref(res, ref)


def test_dfl_grid_size(ob, two_group):
    f, refgroup, _ = two_group
    res = ob.run_dfl(f, "wage", "region", refgroup, PREDICTORS, grid_size=37)
    ref = R.run_dfl(f, "wage", "region", refgroup, PREDICTORS, grid_size=37)
    assert len(res.grid) == 37
    _check_against_ref(res, ref)


def test_dfl_from_csv_equals_run_dfl(ob, two_group, tmp_path):
    f, refgroup, _ = two_group
    names = list(f)
    path = tmp_path / "dfl.csv"
    with open(path, "w") as fh:
        fh.write(",".join(names) + "\n")
        for row in zip(*[f[c] for c in names]):
            fh.write(",".join(repr(v) if isinstance(v, float) else str(v) for v in row) + "\n")
    a = ob.run_dfl_from_csv(str(path), "wage", "region", refgroup, PREDICTORS)
    b = ob.run_dfl(f, "wage", "region", refgroup, PREDICTORS)
    for key in ("grid", "density_a", "density_b", "density_b_counterfactual"):
        assert getattr(a, key).tobytes() == getattr(b, key).tobytes()
    assert (a.n_a, a.n_b, a.group_a, a.logit_iterations) == (b.n_a, b.n_b, b.group_a, b.logit_iterations)


def test_dfl_errors(ob, N):
    f = _frame(200, 23, False)
    with pytest.raises(N.OaxacaError) as e:  # `.f64()?` (dfl.rs:139)
        ob.run_dfl(dict(f, wage=[int(v) for v in f["wage"]]), "wage", "region", "west", PREDICTORS)
    assert e.value.code == N.OB_E_POLARS
    with pytest.raises(N.OaxacaError) as e:  # dfl.rs:145-147
        ob.run_dfl(dict(f, wage=[None] + f["wage"][1:]), "wage", "region", "west", PREDICTORS)
    assert e.value.code == N.OB_E_GROUP and R.NULL_OUTCOME_MESSAGE in str(e.value)
    with pytest.raises(N.OaxacaError) as e:  # stricter than the reference: empty reference group
        ob.run_dfl(f, "wage", "region", "south", PREDICTORS)
    assert e.value.code == N.OB_E_GROUP
    with pytest.raises(N.OaxacaError) as e:  # stricter than the reference: empty group A
        ob.run_dfl(dict(f, region=["west"] * 200), "wage", "region", "west", PREDICTORS)
    assert e.value.code == N.OB_E_GROUP
    with pytest.raises(N.OaxacaError) as e:  # stricter than the reference: null in a predictor
        ob.run_dfl(dict(f, x1=[None] + f["x1"][1:]), "wage", "region", "west", PREDICTORS)
    assert e.value.code == N.OB_E_POLARS
    with pytest.raises(N.OaxacaError) as e:
        ob.run_dfl(f, "wage", "region", "west", ["nope"])
    assert e.value.code == N.OB_E_POLARS
