"""Host pieces of the Tobit decomposition: the numpy restatement is a maximiser and reduces to least
squares without censoring, the stable inverse Mills ratio, the panels of the GPU tests, the aggregation of given rows,
the shape limits and every refusal before any device work. No GPU."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tobit_ref as R  # noqa: E402
import test_gpu_tobit as TG  # noqa: E402
import test_gpu_tobit_fit as TF  # noqa: E402
from test_gpu_parity import RTOL, SEED, close  # noqa: E402

REPS = 64 + 3


@pytest.fixture
def no_gpu(N):
    if N.device_count() > 0:
        pytest.skip("a GPU is visible")


def _code(N, fn):
    with pytest.raises(N.OaxacaError) as e:
        fn()
    return e.value.code, str(e.value)


@pytest.mark.parametrize("limits", ["both", "lower", "upper"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_ref_fit_is_the_maximiser(O, weighted, limits):
    """Concavity in eta makes this sufficient: the log-likelihood at eta-hat lies strictly above its value at the
    start and at eta-hat +- 1e-3 in every coordinate."""
    xa, ya, _, _, wa, _, lower, upper = R.panel(3, weighted)
    if limits == "lower":
        upper = None
    if limits == "upper":
        lower, ya = None, ya + 0.37  # no row sits at a lower limit any more
    cw = np.ones(len(ya)) if wa is None else wa
    start = R.ols_start(xa, ya, wa)
    eta, passes, ok, norms = R.fit(O, xa, ya, cw, np.ones(len(ya)), start, lower, upper)
    assert ok and passes <= 25 and eta[-1] > 0.0
    top = R.loglik(O, xa, ya, cw, eta, lower, upper)
    assert top > R.loglik(O, xa, ya, cw, start, lower, upper)
    for j in range(len(eta)):
        for d in (-1e-3, 1e-3):
            e = eta.copy()
            e[j] += d
            assert top > R.loglik(O, xa, ya, cw, e, lower, upper), (j, d)


def test_ref_without_censoring_is_least_squares(O):
    xa, _, _, _, _, _, _, _ = R.panel(4)
    rng = np.random.default_rng(5)
    y = xa @ np.array([1.0, 0.5, -0.25, 2.0]) + 0.7 * rng.normal(size=len(xa))
    for lower, upper in ((None, None), (y.min() - 1.0, y.max() + 1.0)):  # limits that no row reaches
        eta, _, ok, _ = R.fit(O, xa, y, np.ones(len(y)), np.ones(len(y)), R.ols_start(xa, y), lower, upper)
        assert ok
        beta, s2 = eta[:-1] / eta[-1], 1.0 / eta[-1] ** 2
        b_ols = np.linalg.lstsq(xa, y, rcond=None)[0]
        rss_n = np.sum((y - xa @ b_ols) ** 2) / len(y)
        assert close(beta, b_ols, 0.0)[0] and abs(s2 - rss_n) <= RTOL * rss_n


def test_lambda_is_stable(ob, O):
    """Both the engine's lambda (host evaluation of the kernels' branches) and the restatement's agree with the
    oracle's phi / Phi where that quotient is accurate (Phi well above the underflow: z >= -30), and stay finite,
    positive and decreasing down to z = -40. The bound is the oracle's own error: phi and Phi each carry
    exp(-z^2 / 2) on a rounded argument, up to eps z^2 / 2 relative apiece, and a few ulp of their own and of the
    quotient: (8 + 2 z^2) eps."""
    z = np.linspace(-30.0, 8.0, 7601)
    want = O._npdf(z) / O._ncdf(z)
    bound = (8.0 + 2.0 * z * z) * np.finfo(float).eps
    for got in (ob.tobit_lambda(z), R.lam(O, z)):
        print(f"lambda against the oracle: worst {np.max(np.abs(got - want) / want / bound):.2f} of the bound")
        assert (np.abs(got - want) <= bound * want).all()
    z = np.linspace(-40.0, 10.0, 20001)
    for got in (ob.tobit_lambda(z), R.lam(O, z)):
        assert np.isfinite(got).all() and (got > 0.0).all() and (np.diff(got) <= 0.0).all()
        t = -z[z < -20.0]  # lambda(-t) = t + 1 / t - 2 / t^3 + 10 / t^5 - ..: alternating, within 2 / t^3 of two terms
        assert (np.abs(got[z < -20.0] - (t + 1.0 / t)) <= 2.0 / t ** 3).all()
    assert (np.abs(ob.tobit_lambda(z) - R.lam(O, z)) <= (8.0 + 2.0 * z * z) * np.finfo(float).eps * R.lam(O, z)).all()


# the panels of test_gpu_tobit.py's test_rows_match_ref, each with the limit configurations it runs under
PANELS = sorted({(k, w) for k, w, _, _ in TG.CASES})


@pytest.mark.parametrize("k,weighted", PANELS, ids=[f"{k}-{'weighted' if w else 'unweighted'}" for k, w in PANELS])
def test_gpu_panels_drop_nothing(O, k, weighted):
    """The panels of test_gpu_tobit.py: about a quarter of each group at the lower limit and a tenth at the upper,
    every replicate kept and every fit converged, under both references' shared fits."""
    for limits in sorted({lim for kk, w, _, lim in TG.CASES if (kk, w) == (k, weighted)}):
        xa, ya, xb, yb, wa, wb, lower, upper = TG.panel(k, weighted, limits)
        for y in (ya, yb):
            assert lower is None or 0.12 <= np.mean(y == lower) <= 0.40
            assert upper is None or 0.03 <= np.mean(y == upper) <= 0.20
        point, etas, norms = R.decompose(O, xa, ya, xb, yb, wa, wb, None, None, R.GROUP_A, lower, upper)
        assert point is not None and max(len(v) for v in norms) <= 25
        rows, ok, all_norms = R.boot(O, xa, ya, xb, yb, wa, wb, SEED, 0, REPS, etas, R.GROUP_A, lower, upper)
        assert ok.all() and np.isfinite(rows).all()
        assert max(len(v) for pair in all_norms for v in pair) <= 25
        expl, unex, endow, coef, inter, total = point[:6]
        eps = 64 * np.finfo(float).eps * max(1.0, abs(total))
        assert abs(expl + unex - total) <= eps and abs(endow + coef + inter - total) <= eps
        assert abs(point[6:6 + k].sum() - expl) <= 4 * k * eps and abs(point[6 + k:6 + 2 * k].sum() - unex) <= 4 * k * eps


@pytest.mark.parametrize("g", TF.GROUPS, ids=["A", "B"])
@pytest.mark.parametrize("k", TF.DIM_KS)
def test_fit_cases_leave_the_pass_count_decided(O, k, g):
    """What test_gpu_tobit_fit.py's comparison at every dimension rests on: every fit of the restatement converges,
    and at least three quarters of a case's fits take no step within a factor 10 of the stopping threshold, so that
    their pass counts are compared exactly. The replicate ids are distinct and ascending."""
    _, counts, point, fits, ids = TF.dim_case(O, k, g)
    assert point[2] and all(f[2] for f in fits) and max(f[1] for f in [point] + fits) <= 25
    assert TF.margin_share(point, fits) >= TF.MARGIN_SHARE
    assert len(ids) == TF.REPS == len(counts) and (np.diff(ids) > 0).all()
    assert np.array_equal(counts[-1], R.counts(O, SEED, ids[-1], g, counts.shape[1]))


@pytest.mark.parametrize("g", TF.GROUPS, ids=["A", "B"])
@pytest.mark.parametrize("k", TF.GUARD_KS)
def test_guard_cases_halve(O, k, g):
    """From theta x 20 the restatement halves two or three steps and still converges, in 10 to 14 passes; the trace
    has one entry per pass and does not change what fit returns without it."""
    (x, y, w, lower, upper), eta0, (eta, passes, ok, norms, halved) = TF.guard_case(O, k, g)
    assert ok and 2 <= sum(halved) <= 3 and 10 <= passes <= 14 and len(halved) == passes == len(norms)
    plain = R.fit(O, x, y, w, np.ones(len(y)), eta0, lower, upper)
    assert len(plain) == 4 and np.array_equal(plain[0], eta) and plain[1:] == (passes, ok, norms)
    if (k, g) == (1, R.GROUP_A):
        assert (sum(halved), passes) == (2, 11)


def test_chol_case_fails_in_its_first_pass(O):
    """test_gpu_tobit_fit.py's failed factor: 34 counted uncensored rows (more than K), column 2 zero on every counted
    row, so the restatement's first Cholesky has an exact zero pivot: one pass, not ok, eta at its start. The same
    holds for the draws of the batch case that lose their even rows; its unit-count replicates converge."""
    x, y, lower, upper, c, eta0 = TF.chol_case()
    assert np.sum(c[R.classes(y, lower, upper) == 0]) == 34 > x.shape[1] and not x[c > 0, 2].any()
    info = R.tobit_pass(O, x, y, c.astype(float), eta0, lower, upper)[0]
    assert not info[2].any() and R.chol_solve(info, np.ones(4)) is None
    eta, passes, ok, norms = R.fit(O, x, y, c.astype(float), c, eta0, lower, upper)
    assert (passes, ok, norms) == (1, False, []) and np.array_equal(eta, eta0)
    counts = TF.batch_counts(O)
    got = [R.fit(O, x, y, cr.astype(float), cr, eta0, lower, upper)[1:3] for cr in counts[[0, 1, 62, 63, 64, 65, 66]]]
    assert got[1][1] and got[1][0] >= 2 and got[4] == (0, False)
    assert [got[i] for i in (0, 2, 3, 5, 6)] == [(1, False)] * 5
    assert all(np.array_equal(counts[r], counts[1]) for r in range(1, 62))


@pytest.mark.parametrize("k", [1, 17, 31])
def test_score_hp_sees_a_wrong_eta(O, k):
    """The relative score in mpmath at the restatement's fit (group B, weighted) is that of a maximiser found in
    f64, below 1e-12; with its first entry moved by a relative 1e-6 it is above 1e-8: four orders over the bar
    test_gpu_tobit_fit.py sets for the device's eta."""
    pytest.importorskip("mpmath")
    (x, y, w, lower, upper), _, point, _, _ = TF.dim_case(O, k, R.GROUP_B)
    at_fit = R.score_hp(x, y, w, point[0], lower, upper)
    moved = point[0].copy()
    moved[0] *= 1.0 + 1e-6
    off = R.score_hp(x, y, w, moved, lower, upper)
    print(f"k={k}: score_hp {at_fit:.2e} at the fit, {off:.2e} beside it")
    assert at_fit < 1e-12 and off > 1e-8


def test_ols_cases_have_steps_to_take(O):
    """Without censoring the restatement takes several passes from the shifted start and ends at weighted least
    squares in long double to a few ulp."""
    for k in TF.OLS_KS:
        for g in TF.GROUPS:
            _, _, ref, (beta, sigma) = TF.ols_case(O, k, g)
            assert ref[2] and ref[1] >= 3 and TF.ols_err(ref[0], beta, sigma) <= 1e-14


def test_row_len_and_shape(ob, N):
    for k in (1, 3, 9, 31):
        assert ob.tobit_row_len(k) == 6 + 7 * k + 17 == R.row_len(k)
    assert ob.tobit_row_len(0) == 0 and N.OB_TOBIT_MAX_K == 31
    ob.tobit_check_shape(31, 32, 32)
    assert _code(N, lambda: ob.tobit_check_shape(32, 100, 100))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.tobit_check_shape(3, 3, 100))[0] == N.OB_E_INSUFFICIENT
    assert _code(N, lambda: ob.tobit_check_shape(3, 100, 3))[0] == N.OB_E_INSUFFICIENT
    assert _code(N, lambda: ob.tobit_check_shape(0, 100, 100))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.tobit_check_shape(3, 2 ** 31, 100))[0] == N.OB_E_UNSUPPORTED


def test_finish_rows_on_arrays(ob, O):
    k = 3
    xa, ya, xb, yb, wa, wb, lower, upper = R.panel(k)
    point, etas, _ = R.decompose(O, xa, ya, xb, yb, None, None, None, None, R.GROUP_B, lower, upper)
    rows, ok, _ = R.boot(O, xa, ya, xb, yb, None, None, SEED, 0, 12, etas, R.GROUP_B, lower, upper)
    rows, ok = rows.copy(), ok.copy()
    rows[4], ok[4] = np.nan, 0
    res = ob.tobit_finish_rows(point, k, rows, ok)
    assert res.n_failed == 1 and res.total_gap == point[5] and res.names == ["x0", "x1", "x2"]
    kept = rows[ok.astype(bool)]
    tables = ((res.two_fold, [0, 1]), (res.three_fold, [2, 3, 4]), (res.detailed_explained, range(6, 6 + k)),
              (res.detailed_unexplained, range(6 + k, 6 + 2 * k)), (res.latent, range(6 + 7 * k, 6 + 7 * k + 3)))
    for comps, cols in tables:
        assert len(comps) == len(cols)
        for c, col in zip(comps, cols):
            se, p, (lo, hi) = ob.bootstrap_stats(kept[:, col], point[col])
            assert c.estimate == point[col] and (c.std_err, c.p_value, c.ci_lower, c.ci_upper) == (se, p, lo, hi)
    assert [c.name for c in res.latent] == ["explained", "unexplained", "total_gap"]
    assert res.expected_values[("A", "beta_a")] - res.expected_values[("B", "beta_b")] == res.total_gap
    back = json.loads(res.to_json())
    assert back["n_failed"] == 1 and back["latent"][2]["estimate"] == point[6 + 7 * k + 2]
    with pytest.raises(ValueError):
        ob.tobit_finish_rows(point[:-1], k, rows, ok)


def _frame(k=3, weighted=True):
    xa, ya, xb, yb, wa, wb, lower, upper = R.panel(k, weighted)
    n = len(ya) + len(yb)
    f = {"y": np.concatenate([ya, yb]).tolist(), "g": ["A"] * len(ya) + ["B"] * len(yb),
         "cat": [("u", "v")[i % 2] for i in range(n)], "firm": [i // 7 for i in range(n)],
         "sel": [float(i % 2) for i in range(n)]}
    for j in range(1, k):
        f[f"x{j}"] = np.concatenate([xa[:, j], xb[:, j]]).tolist()
    f["w"] = np.concatenate([wa, wb]).tolist()
    return f, [f"x{j}" for j in range(1, k)], lower, upper


def _builder(ob, f, xs):
    return ob.OaxacaBuilder(f, "y", "g", "B").predictors(xs).bootstrap_reps(4).seed(1)


def test_refusals_come_before_any_device_work(ob, N, no_gpu):
    f, xs, lower, upper = _frame()
    RC = ob.ReferenceCoefficients

    def run(b, lo=lower, hi=upper):
        return _code(N, lambda: b.decompose_tobit(lo, hi))

    for ref in (r for r in RC if r not in (RC.GroupA, RC.GroupB)):  # Pooled, Weighted, Cotton, Neumark
        code, msg = run(_builder(ob, f, xs).reference_coefficients(ref))
        assert code == N.OB_E_UNSUPPORTED and msg.startswith("tobit decomposition: reference coefficients other than"), msg
    code, msg = run(_builder(ob, f, xs).categorical_predictors(["cat"]).normalize(["cat"]))
    assert (code, msg) == (N.OB_E_UNSUPPORTED, "tobit decomposition: normalized categoricals are outside its scope")
    code, msg = run(_builder(ob, f, xs).heckman_selection("sel", ["x1"]))
    assert (code, msg) == (N.OB_E_UNSUPPORTED, "tobit decomposition: Heckman selection settings are outside its scope")
    code, msg = run(_builder(ob, f, xs).cluster("firm"))
    assert (code, msg) == (N.OB_E_UNSUPPORTED, "tobit decomposition: the cluster bootstrap is outside its scope")
    # the limits
    for lo, hi in ((float("nan"), upper), (lower, float("inf")), (1.0, 1.0), (2.0, 1.0)):
        assert run(_builder(ob, f, xs), lo, hi)[0] == N.OB_E_INVALID
    assert "lies below the lower limit" in run(_builder(ob, f, xs), 0.5, upper)[1]
    assert "lies above the upper limit" in run(_builder(ob, f, xs), lower, upper - 0.5)[1]
    assert run(_builder(ob, f, xs), 0.5, upper)[0] == run(_builder(ob, f, xs), lower, upper - 0.5)[0] == N.OB_E_INVALID
    # the columns
    g = dict(f, x1=[None if i == 5 else v for i, v in enumerate(f["x1"])])
    code, msg = run(_builder(ob, g, xs))
    assert code == N.OB_E_INVALID and "null" in msg
    g = dict(f, x1=[float("nan") if i == 5 else v for i, v in enumerate(f["x1"])])
    code, msg = run(_builder(ob, g, xs))
    assert code == N.OB_E_INVALID and "non-finite" in msg
    g = dict(f, w=[-1.0 if i == 5 else v for i, v in enumerate(f["w"])])
    code, msg = run(_builder(ob, g, xs).weights("w"))
    assert code == N.OB_E_INVALID and "negative weight" in msg
    # a group whose uncensored rows do not exceed K: every row of A but three at the lower limit
    y = np.array(f["y"])
    is_a = np.array(f["g"]) == "A"
    unc = np.flatnonzero(is_a & (y != lower) & (y != upper))
    y[unc[3:]] = lower
    code, msg = run(_builder(ob, dict(f, y=y.tolist()), xs))
    assert code == N.OB_E_INSUFFICIENT and "uncensored rows (3)" in msg
    # more columns than the limit
    wide = dict(f)
    names = []
    rng = np.random.default_rng(0)
    for j in range(31):
        wide[f"z{j}"] = rng.normal(size=len(y)).tolist()
        names.append(f"z{j}")
    assert run(_builder(ob, wide, names))[0] == N.OB_E_UNSUPPORTED
    # a point fit that fails: a predictor that is zero in every row leaves the least-squares start without a Cholesky
    # factor (its pivot is exactly 0), which is found on the host, before the context is read
    code, msg = run(_builder(ob, dict(f, x2=[0.0] * len(y)), xs))
    assert code == N.OB_E_LINALG and msg.endswith("tobit decomposition: the censored-normal fit of the point estimate failed"), msg
    # good arguments leave the missing device as the error
    assert run(_builder(ob, f, xs).weights("w"))[0] == N.OB_E_HIP


def test_array_entry_points_check_before_the_device(ob, N, no_gpu):
    xa, ya, _, _, _, _, lower, upper = R.panel(3)
    eta = R.ols_start(xa, ya)
    assert _code(N, lambda: ob.tobit_pass(xa, ya, eta, 0.5, upper))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.tobit_pass(xa, ya, eta * -1.0, lower, upper))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.tobit_pass(xa, ya, np.tile(eta, (65, 1)), lower, upper))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.tobit_fit(xa * 2.0, ya, lower, upper))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.tobit_fit(xa, ya, 2.0, 1.0))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.tobit_means(xa, ya, np.stack([eta, eta]), lower, upper, w=-np.ones(len(ya))))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.tobit_rows(xa, ya, xa, ya, lower, upper, reference_coefficients=ob.ReferenceCoefficients.Pooled))[0] \
        == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.tobit_fit(xa, ya, lower, upper))[0] == N.OB_E_HIP
    with pytest.raises(ValueError):
        ob.tobit_means(xa, ya, eta, lower, upper)
