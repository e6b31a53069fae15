"""Matching on the GPU: ob_knn, ob_match_logistic and ob_match_run / MatchingEngine against the
NumPy restatement (tests/match_ref.py) and the reference's own tests (tests/golden/match_kat.json).

Bars. Euclidean: the device's squared distance is the restatement's sum operation for operation, so
indices are equal and dist2 is bitwise equal, and the weights are equal (==). Mahalanobis and PSM
match on coordinates that differ from the restatement's by rounding (another summation order in the
covariance, the transform and the logistic's sums): each such test first asserts on the restatement
alone that every treated row's k-th and (k+1)-th squared distances are at least 1e-8 apart
relatively, far above that rounding, and then holds the weights to == and dist2 to 1e-9 relative.
Scores: 1e-10 absolute; beta: 1e-6 of max|beta| with equal iteration counts, after the restatement's
deciding step norms are shown to be >= 2 tol and <= tol / 2. Each test prints its worst figure
before it asserts."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dfl_ref  # noqa: E402
import match_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu

KAT = json.load(open(os.path.join(HERE, "golden", "match_kat.json")))
_D = C.POINTER(C.c_double)
GAP = 1e-8


def _dp(a):
    return a.ctypes.data_as(_D)


def _ob_knn(N, q, c, k, ldq=None, ldc=None):
    """ob_knn through ctypes -> (rc, idx, dist2); the padding rows of both inputs are NaN."""
    (n_q, d), n_c = q.shape, c.shape[0]
    ldq, ldc = max(n_q, 1) if ldq is None else ldq, max(n_c, 1) if ldc is None else ldc
    qb, cb = np.full((d, ldq), np.nan), np.full((d, ldc), np.nan)
    qb[:, :n_q], cb[:, :n_c] = q.T, c.T
    idx, dd = np.full((n_q, k), -7, dtype=np.int64), np.full((n_q, k), np.nan)
    rc = N.lib().ob_knn(N.context(0), _dp(qb), ldq, n_q, _dp(cb), ldc, n_c, d, k,
                        idx.ctypes.data_as(C.POINTER(C.c_int64)), _dp(dd))
    return rc, idx, dd


def _assert_knn(N, q, c, k, **ld):
    rc, idx, dd = _ob_knn(N, q, c, k, **ld)
    assert rc == N.OB_OK, N.lib().ob_last_error()
    ridx, rdd = M.knn(q, c, k)
    bad_i, bad_d = int((idx != ridx).sum()), int((dd.view(np.uint64) != rdd.view(np.uint64)).sum())
    print(f"knn {q.shape[0]}x{c.shape[0]}x{q.shape[1]} k={k}: {bad_i} indices differ, {bad_d} dist2 differ bitwise")
    assert bad_i == 0 and bad_d == 0
    return idx, dd


KNN_SHAPES = [(1, 2, 1, 1), (300, 1000, 5, 3), (257, 4099, 20, 1), (65, 513, 33, 5), (64, 70000, 3, 16),
              (1000, 3000, 1, 2), (10, 4, 2, 7)]


@pytest.mark.parametrize("shape", KNN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_knn_euclidean_bitwise(N, shape):
    n_q, n_c, d, k = shape
    q, c = M.knn_data(n_q, n_c, d, seed=100 + d)
    idx, dd = _assert_knn(N, q, c, k)
    if k > n_c:
        assert (idx[:, n_c:] == -1).all() and np.isposinf(dd[:, n_c:]).all()


def test_knn_leading_dimensions(N):
    q, c = M.knn_data(37, 300, 6, seed=3)
    _assert_knn(N, q, c, 4, ldq=41, ldc=333)


def test_knn_exact_duplicates(N):
    """Every control appears three times (and the grid makes many more distances equal), so the
    order within a distance is the position's."""
    rng = np.random.default_rng(5)
    base = rng.integers(-3, 4, size=(200, 2)).astype(np.float64)
    c = np.vstack([base, base, base])
    q = rng.integers(-3, 4, size=(130, 2)).astype(np.float64)
    ridx, rdd = M.knn(q, c, 8)
    assert (rdd[:, 0] == rdd[:, 2]).all()  # the case has the ties it is about
    for chunks in (None, 1, 5):
        with N.option("match_chunks", chunks):
            _assert_knn(N, q, c, 8)


def test_knn_chunked_and_unchunked_agree(N, ob):
    q, c = M.knn_data(300, 5000, 7, seed=9)
    outs = []
    for chunks in (1, None, 3, 4999):
        with N.option("match_chunks", chunks):
            outs.append(_assert_knn(N, q, c, 6))
    for idx, dd in outs[1:]:
        assert idx.tobytes() == outs[0][0].tobytes() and dd.tobytes() == outs[0][1].tobytes()
    i2, d2 = ob.knn(q, c, 6)
    assert i2.tobytes() == outs[0][0].tobytes() and d2.tobytes() == outs[0][1].tobytes()


# ---- ob_match_run ---------------------------------------------------------------------------------

RUN_SHAPES = [(300, 1000, 5, 3), (257, 4099, 20, 1), (65, 513, 33, 5), (64, 70000, 3, 16), (1000, 3000, 1, 2),
              (10, 4, 2, 7)]
_frames = {}


def _frame(shape, mix, int_treatment=False, seed=200):
    key = (shape, mix, int_treatment, seed)
    if key not in _frames:
        n_q, n_c, d, _ = shape
        _frames[key] = M.frame_of(n_q, n_c, d, seed=seed + d, mix=mix, int_treatment=int_treatment)
    return _frames[key]


# Seeds of the PSM frames: the first from 300 on at which the restatement's last two step norms sit
# clear of tol on both sides (>= 2 tol, <= tol / 2), so that the iteration count cannot hinge on rounding.
PSM_CASES = [((300, 1000, 5, 3), 301), ((257, 4099, 20, 1), 304), ((1000, 3000, 1, 2), 300)]
_psm_refs = {}


def _psm_ref(shape, seed):
    if shape not in _psm_refs:
        frame, cov = _frame(shape, False, seed=seed)
        _psm_refs[shape] = M.match_psm(frame, "treat", "y", cov, shape[3], detail=True)
    return _psm_refs[shape]


def _neighbors_close(res, ref, rel):
    """The engine's neighbour rows equal the restatement's and dist2 is within ``rel``."""
    rrows = np.where(ref["idx"] >= 0, ref["control"][np.maximum(ref["idx"], 0)], -1)
    assert np.array_equal(res.treated_rows, ref["treated"])
    fin = np.isfinite(ref["dist2"])
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(res.neighbor_dist2[fin] - ref["dist2"][fin]) / np.maximum(ref["dist2"][fin], 1e-300)
    worst = float(err.max()) if err.size else 0.0
    print(f"neighbour rows differ: {int((res.neighbor_rows != rrows).sum())}, worst relative dist2 error {worst:.3e}")
    assert np.array_equal(res.neighbor_rows, rrows)
    assert np.array_equal(np.isfinite(res.neighbor_dist2), fin) and worst <= rel


@pytest.mark.parametrize("shape", RUN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_match_run_euclidean(ob, N, shape):
    frame, cov = _frame(shape, False, int_treatment=shape[2] == 5)
    k = shape[3]
    ref = M.run_matching(frame, "treat", cov, k, False, detail=True)
    eng = ob.MatchingEngine(frame, "treat", "no_such_outcome", cov)  # the outcome is never read
    res = eng.run(k, N.OB_MATCH_EUCLIDEAN)
    print("weights differ:", int((res.weights != ref["weights"]).sum()), "of", len(ref["weights"]))
    assert res.n_treated == shape[0] and res.n_control == shape[1]
    assert np.array_equal(res.weights, ref["weights"])
    assert (res.weights[[i for i, v in enumerate(frame["treat"]) if v is None or v == 2]] == 0.0).all()
    _neighbors_close(res, ref, 0.0)
    assert eng.run_matching(k, False) == ref["weights"].tolist()


@pytest.mark.parametrize("shape", RUN_SHAPES[:4], ids=lambda s: "x".join(map(str, s)))
def test_match_run_mahalanobis(ob, N, shape):
    frame, cov = _frame(shape, True)
    k = shape[3]
    ref = M.run_matching(frame, "treat", cov, k, True, detail=True)
    gap = float(M.kth_gap(ref["xt"], ref["xc"], k).min())
    print(f"smallest relative gap between the k-th and (k+1)-th squared distance: {gap:.3e}")
    assert gap >= GAP
    eng = ob.MatchingEngine(frame, "treat", "y", cov)
    res = eng.run(k, N.OB_MATCH_MAHALANOBIS)
    print("weights differ:", int((res.weights != ref["weights"]).sum()), "of", len(ref["weights"]))
    assert np.array_equal(res.weights, ref["weights"])
    _neighbors_close(res, ref, 1e-9)
    assert np.array_equal(eng.match_nearest_neighbor(k, True), ref["weights"])
    idx, dd = eng.neighbors(k, True)
    assert np.array_equal(idx, res.neighbor_rows) and np.array_equal(dd, res.neighbor_dist2)


@pytest.mark.parametrize("shape,seed", PSM_CASES, ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))
def test_match_run_psm(ob, N, shape, seed):
    frame, cov = _frame(shape, False, seed=seed)
    k, tol = shape[3], 1e-6
    ref = _psm_ref(shape, seed)
    fit = ref["fit"]
    norms = fit["step_norms"]
    print(f"restatement: {fit['iterations']} iterations, last step norms {norms[-2]:.3e}, {norms[-1]:.3e}")
    assert norms[-1] <= tol / 2 and norms[-2] >= 2 * tol
    gap = float(M.kth_gap(ref["xt"], ref["xc"], k).min())
    print(f"smallest relative gap between the k-th and (k+1)-th squared distance: {gap:.3e}")
    assert gap >= GAP
    beta, scores, conv, iters = ob.match_logistic(ref["design"], ref["target"], 100, tol)
    berr = float(np.abs(beta - fit["coefficients"]).max() / np.abs(fit["coefficients"]).max())
    serr = float(np.abs(scores - fit["scores"]).max())
    print(f"beta error {berr:.3e} of max|beta|, score error {serr:.3e}, iterations {iters} vs {fit['iterations']}")
    assert conv and iters == fit["iterations"] and berr <= 1e-6 and serr <= 1e-10
    res = ob.MatchingEngine(frame, "treat", "y", cov).run(k, N.OB_MATCH_PSM)
    print("weights differ:", int((res.weights != ref["weights"]).sum()), "of", len(ref["weights"]))
    assert res.logistic_iterations == fit["iterations"] and res.logistic_converged
    assert np.array_equal(res.weights, ref["weights"])
    _neighbors_close(res, ref, np.inf)  # the rows; dist2 has a test of its own below
    assert ob.MatchingEngine(frame, "treat", "y", cov).match_psm(k) == ref["weights"].tolist()


@pytest.mark.parametrize("shape,seed", PSM_CASES, ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))
def test_match_run_psm_dist2(ob, N, shape, seed):
    """dist2 of the PSM match within 1e-9 relative of the restatement's. A squared difference of two
    scores that are |D| apart moves by 2 e / |D| relatively when each score carries an error e; the
    smallest matched |D| of these frames is 6e-8 to 3e-6 (printed), so the bar asks for scores good
    to a few 1e-17, below one rounding of exp. Measured on an MI355X: worst relative error 7.8e-11,
    8.2e-10 and 7.1e-10 for the three cases, at smallest score differences of 2.9e-6, 6.0e-8 and 1.4e-7."""
    frame, cov = _frame(shape, False, seed=seed)
    ref = _psm_ref(shape, seed)
    fin = np.isfinite(ref["dist2"])
    print(f"smallest matched score difference of the restatement: {float(np.sqrt(ref['dist2'][fin].min())):.3e}")
    res = ob.MatchingEngine(frame, "treat", "y", cov).run(shape[3], N.OB_MATCH_PSM)
    _neighbors_close(res, ref, 1e-9)


# ---- the reference's own tests ------------------------------------------------------------------------

def _kat_frame(case):
    if "treated" in case:
        return {"treated": case["treated"], "income": case["income"], "education": case["education"]}
    return {"treatment": case["treatment_values"], "outcome": case["outcome_values"], "age": case["age"],
            "education": case["education"]}


@pytest.mark.parametrize("name", ["matching_basic", "engine_inline", "psm"])
def test_reference_kats(ob, name):
    case = KAT[name]
    eng = ob.MatchingEngine(_kat_frame(case), case["treatment"], case["outcome"], case["covariates"])
    w = eng.match_psm(case["k"]) if case["method"] == "psm" else eng.run_matching(case["k"], False)
    e = case["expect"]
    print(name, "weights[:4] =", w[:4], "sum_rows =", [w[i] for i in e.get("sum_rows", [])])
    assert len(w) == e["length"]
    assert all(v >= 0.0 for v in w[:e.get("nonnegative_first", len(w))])
    for i, v in e.get("equals", {}).items():
        assert w[int(i)] == v
    if "sum_rows" in e:
        assert sum(w[i] for i in e["sum_rows"]) >= e["sum_at_least"]


# ---- errors ---------------------------------------------------------------------------------------------

def _raises(ob, N, code, text, fn):
    with pytest.raises(ob.OaxacaError) as e:
        fn()
    print(e.value.code, str(e.value))
    assert e.value.code == code and text in str(e.value)


def test_error_paths(ob, N):
    f = {"t": [1.0, 0.0, 0.0, 2.0, None, 0.0], "x": [0.0, 1.0, 5.0, 0.0, 0.0, 2.0],
         "y": [1.0, 2.0, 3.0, None, 4.0, 5.0]}
    E = ob.MatchingEngine
    eu, ma = N.OB_MATCH_EUCLIDEAN, N.OB_MATCH_MAHALANOBIS
    _raises(ob, N, N.OB_E_POLARS, "Polars error: ", lambda: E(dict(f, t=["1", "0", "0", "2", None, "0"]), "t", "y", ["x"]).run(1, eu))
    _raises(ob, N, N.OB_E_POLARS, "not found: nope", lambda: E(f, "nope", "y", ["x"]).run(1, eu))
    _raises(ob, N, N.OB_E_POLARS, "not found: nope", lambda: E(f, "t", "y", ["nope"]).run(1, eu))
    _raises(ob, N, N.OB_E_POLARS, "null value in covariate column `x`",
            lambda: E(dict(f, x=[0.0, None, 5.0, 0.0, 0.0, 2.0]), "t", "y", ["x"]).run(1, eu))
    _raises(ob, N, N.OB_E_DIAG, "Diagnostic error: non-finite covariate",
            lambda: E(dict(f, x=[0.0, np.inf, 5.0, 0.0, 0.0, 2.0]), "t", "y", ["x"]).run(1, eu))
    _raises(ob, N, N.OB_E_DIAG, "Diagnostic error: non-finite covariate",
            lambda: E(dict(f, x=[np.nan, 1.0, 5.0, 0.0, 0.0, 2.0]), "t", "y", ["x"]).run(1, ma))
    _raises(ob, N, N.OB_E_DIAG, "Not enough data points to calculate covariance",
            lambda: E(dict(f, t=[1.0, 0.0, 3.0, 2.0, None, 3.0]), "t", "y", ["x"]).run(1, ma))
    _raises(ob, N, N.OB_E_DIAG, "Covariance matrix is singular and cannot be inverted",
            lambda: E(dict(f, x=[0.0, 1.0, 1.0, 0.0, 0.0, 1.0]), "t", "y", ["x"]).run(1, ma))
    _raises(ob, N, N.OB_E_DIAG, "Diagnostic error: Cholesky decomposition failed",  # a NaN covariance has a NaN inverse
            lambda: E(dict(f, x=[0.0, np.nan, 5.0, 0.0, 0.0, 2.0]), "t", "y", ["x"]).run(1, ma))
    # PSM: prepare_data's checks, then the treatment's dtype
    _raises(ob, N, N.OB_E_GROUP, "Invalid group variable: One group is empty",
            lambda: E(dict(f, t=[1.0, 1.0, 1.0, 2.0, None, 1.0]), "t", "y", ["x"]).match_psm(1))
    _raises(ob, N, N.OB_E_POLARS, "not found: nope", lambda: E(f, "t", "nope", ["x"]).match_psm(1))
    _raises(ob, N, N.OB_E_POLARS, "expected `Float64`", lambda: E(dict(f, y=[1, 2, 3, None, 4, 5]), "t", "y", ["x"]).match_psm(1))
    _raises(ob, N, N.OB_E_GROUP, "Invalid group variable: Null values in outcomes",
            lambda: E(dict(f, y=[1.0, None, 3.0, None, 4.0, 5.0]), "t", "y", ["x"]).match_psm(1))
    _raises(ob, N, N.OB_E_POLARS, "expected `Float64`", lambda: E(dict(f, t=[1, 0, 0, 2, None, 0]), "t", "y", ["x"]).match_psm(1))
    assert E(f, "t", "y", ["x"]).run_matching(1, False) == [1.0, 1.0, 0.0, 0.0, 0.0, 0.0]  # the null outcome row is in no group
    assert len(E(f, "t", "y", ["x"]).match_psm(1)) == 6
    assert E(f, "t", "y", ["x"]).run_matching(0, False) == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0]  # k = 0 selects nothing
    assert E(dict(f, t=[1.0, 3.0, 3.0, 2.0, None, 3.0]), "t", "y", ["x"]).run_matching(2, False) == [1.0] + [0.0] * 5


def test_logistic_singular_hessian(ob, N):
    """Two identical columns of 2^20 over 8 rows: every Hessian entry is exactly 2^41 at beta = 0,
    whose ulp absorbs the 1e-6 ridge, so LU meets an exactly zero pivot (logistic.rs:95). With an
    all-zero design the ridge alone keeps the Hessian regular and the fit stops after one step."""
    x = np.full((8, 2), 2.0 ** 20)
    y = np.array([0.0, 1.0] * 4)
    with pytest.raises(M.MatchError) as e:
        M.logistic(x, y)
    assert str(e.value) == M.HESSIAN_SINGULAR
    _raises(ob, N, N.OB_E_DIAG, "Diagnostic error: Hessian is singular", lambda: ob.match_logistic(x, y))
    z = np.zeros((4, 1))
    beta, scores, conv, iters = ob.match_logistic(z, y[:4])
    ref = M.logistic(z, y[:4])
    assert beta.tolist() == ref["coefficients"].tolist() == [0.0] and scores.tolist() == [0.5] * 4
    assert conv and iters == ref["iterations"] == 1


def test_limits(ob, N):
    q, c = np.zeros((2, 65)), np.zeros((3, 65))
    rc, _, _ = _ob_knn(N, q, c, 1)
    assert rc == N.OB_E_UNSUPPORTED and "65 covariates" in N.lib().ob_last_error().decode()
    rc, _, _ = _ob_knn(N, q[:, :3], c[:, :3], 17)
    assert rc == N.OB_E_UNSUPPORTED and "k = 17" in N.lib().ob_last_error().decode()
    f = {"t": [1.0, 0.0, 0.0], **{f"x{j}": [0.0, 1.0, 2.0] for j in range(65)}}
    _raises(ob, N, N.OB_E_UNSUPPORTED, "65 covariates", lambda: ob.MatchingEngine(f, "t", "y", [f"x{j}" for j in range(65)]).run(1, 0))
    _raises(ob, N, N.OB_E_UNSUPPORTED, "k = 17", lambda: ob.MatchingEngine(f, "t", "y", ["x0"]).run(17, 0))


# ---- determinism, CSV, and the untouched DFL logit ----------------------------------------------------------

def test_two_runs_give_identical_bytes(ob, N):
    q, c = M.knn_data(64, 70000, 3, seed=103)
    a, b = _ob_knn(N, q, c, 16), _ob_knn(N, q, c, 16)
    assert a[0] == b[0] == N.OB_OK and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    for shape, mix, method in (((300, 1000, 5, 3), True, N.OB_MATCH_MAHALANOBIS), ((1000, 3000, 1, 2), False, N.OB_MATCH_PSM),
                               ((257, 4099, 20, 1), False, N.OB_MATCH_EUCLIDEAN)):
        frame, cov = _frame(shape, mix)
        w = [ob.MatchingEngine(frame, "treat", "y", cov).run(shape[3], method).weights.tobytes() for _ in range(2)]
        assert w[0] == w[1]


def test_match_units_from_csv(ob, tmp_path):
    frame, cov = M.frame_of(40, 120, 3, seed=77, extras=False)
    path = tmp_path / "units.csv"
    names = list(frame)
    with open(path, "w") as fh:
        fh.write(",".join(names) + "\n")
        for r in range(len(frame["treat"])):
            fh.write(",".join(repr(frame[c][r]) for c in names) + "\n")
    loaded = ob.read_csv(path)
    for method, direct in (("euclidean", lambda e: e.run_matching(2, False)), ("mahalanobis", lambda e: e.run_matching(2, True)),
                           ("psm", lambda e: e.match_psm(2)), ("anything else", lambda e: e.run_matching(2, False))):
        w = ob.match_units(path, "treat", "y", cov, k=2, method=method)
        assert w == direct(ob.MatchingEngine(loaded, "treat", "y", cov)), method
        assert len(w) == 160 and w.count(1.0) >= 40
    assert ob.match_units(path, "treat", "y", cov, k=2) == M.run_matching(frame, "treat", cov, 2).tolist()


def test_dfl_logit_bytes_unchanged(ob):
    """ob_logit shares its Newton-pass kernel with ob_match_logistic (a template parameter switches
    the clamp off). The golden arrays were recorded on an MI355X from the commit before that change."""
    gold = np.load(os.path.join(HERE, "golden", "dfl_logit_3000x17_seed45.npz"))
    x, y = dfl_ref.panel(3000, 17, 45)
    beta, probs, conv, iters = ob.logit(y, x)
    print("beta bytes equal:", beta.tobytes() == gold["beta"].tobytes(), "probs bytes equal:",
          probs.tobytes() == gold["probs"].tobytes())
    assert int(conv) == int(gold["converged"]) and iters == int(gold["iterations"])
    assert beta.tobytes() == gold["beta"].tobytes() and probs.tobytes() == gold["probs"].tobytes()
