"""Host pieces of the distribution-regression decomposition: the identities of the numpy
restatement, the row length and shape limits, the thresholds, the rearranged inverse, the aggregation of given rows
and every refusal before any device work. No GPU."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dr_ref as D  # noqa: E402
import reweight_ref as R  # noqa: E402

TAUS = np.array([0.1, 0.25, 0.5, 0.75, 0.9])


def _code(N, fn):
    with pytest.raises(N.OaxacaError) as e:
        fn()
    return e.value.code, str(e.value)


def test_row_len_and_shape(ob, N):
    for T, nq in ((2, 1), (5, 5), (50, 5), (64, 32)):
        assert ob.dr_row_len(T, nq) == 6 * nq + 7 * T + 1 == D.row_len(T, nq)
    assert ob.dr_row_len(1, 5) == 0 and ob.dr_row_len(5, 0) == 0
    assert (N.OB_DR_MAX_K, N.OB_DR_MAX_T, N.OB_DR_MAX_Q) == (D.MAX_K, D.MAX_T, D.MAX_Q) == (32, 64, 32)
    ob.dr_check_shape(32, 33, 33, 64, 32)
    ob.dr_check_shape(1, 2, 2, 2, 1)
    assert _code(N, lambda: ob.dr_check_shape(33, 100, 100, 5, 5))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.dr_check_shape(3, 100, 100, 65, 5))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.dr_check_shape(3, 100, 100, 5, 33))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.dr_check_shape(3, 100, 100, 1, 5))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.dr_check_shape(3, 100, 100, 5, 0))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.dr_check_shape(3, 3, 100, 5, 5))[0] == N.OB_E_INSUFFICIENT
    assert _code(N, lambda: ob.dr_check_shape(3, 100, 3, 5, 5))[0] == N.OB_E_INSUFFICIENT
    assert _code(N, lambda: ob.dr_check_shape(0, 100, 100, 5, 5))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.dr_check_shape(3, 2 ** 31, 100, 5, 5))[0] == N.OB_E_UNSUPPORTED


def test_thresholds_match_numpy(ob, N):
    rng = np.random.default_rng(8)
    y = rng.normal(size=1935)
    for T, lo, hi in ((50, 0.05, 0.95), (5, 0.1, 0.9), (17, 0.1, 0.9), (2, 0.0, 1.0), (64, 0.01, 0.99)):
        got = ob.dr_thresholds(y, T, lo, hi)
        assert np.array_equal(got, D.thresholds(y, T, lo, hi)) and len(got) == T
        want = np.quantile(y, np.linspace(lo, hi, T))  # numpy's own interpolation differs in the last bits only
        assert np.all(np.abs(got - want) <= 1e-13 * np.maximum(np.abs(want), 1.0))
        assert np.all(np.diff(got) > 0)
    # a heaped outcome: half the rows sit on one value, so neighbouring levels give the same threshold
    heaped = np.concatenate([np.full(500, 2.0), rng.normal(size=500) + 5.0, rng.normal(size=50) - 5.0])
    got = ob.dr_thresholds(heaped, 50)
    assert np.array_equal(got, D.thresholds(heaped, 50)) and 2 <= len(got) < 50
    assert np.all(np.diff(got) > 0) and (got == 2.0).sum() == 1
    assert _code(N, lambda: ob.dr_thresholds(y, 65))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.dr_thresholds(y, 1))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.dr_thresholds(y, 5, 0.9, 0.1))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.dr_thresholds(np.array([1.0, np.nan]), 5))[0] == N.OB_E_INVALID


def test_quantiles_match_ref(ob, N):
    thr = np.array([1.0, 2.0, 4.0, 5.0, 7.0, 11.0])
    cases = {
        "non-monotone": np.array([0.10, 0.35, 0.30, 0.60, 0.55, 0.90]),  # the rearrangement swaps two pairs
        "flat run": np.array([0.10, 0.40, 0.40, 0.40, 0.70, 0.90]),
        "monotone": np.array([0.05, 0.20, 0.45, 0.50, 0.80, 0.95]),
    }
    taus = np.array([0.02, 0.05, 0.10, 0.2, 0.3, 0.4, 0.45, 0.5, 0.6, 0.9, 0.95, 0.97])
    for name, f in cases.items():
        q, re, edge = ob.dr_quantiles(f, thr, taus)
        wq, wre, wedge = D.quantiles(f, thr, taus)
        assert np.array_equal(re, np.sort(f)) and np.array_equal(re, wre), name
        assert np.array_equal(edge, wedge), name
        assert np.all(np.abs(q - wq) <= 1e-15 * np.abs(wq)), name
        assert np.all(np.diff(q) >= 0), name  # the inverse of a non-decreasing function
        for i, tau in enumerate(taus):
            if tau <= re[0]:  # below (or exactly at) F~_1: the first threshold
                assert q[i] == thr[0] and edge[i] == 1
            elif tau > re[-1]:
                assert q[i] == thr[-1] and edge[i] == 2
            else:
                assert edge[i] == 0 and thr[0] < q[i] <= thr[-1]
            at = np.flatnonzero(re == tau)
            if len(at) and tau > re[0]:  # a tau exactly equal to an F~_t: that threshold (the first of a flat run)
                assert q[i] == thr[at[0]], (name, tau)
    assert cases["flat run"][1] in taus and cases["non-monotone"][0] in taus
    assert _code(N, lambda: ob.dr_quantiles(cases["monotone"], thr, [0.0]))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.dr_quantiles(cases["monotone"], thr, [1.0]))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.dr_quantiles(cases["monotone"], thr[::-1].copy(), [0.5]))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.dr_quantiles(np.full(6, np.nan), thr, [0.5]))[0] == N.OB_E_INVALID
    assert _code(N, lambda: ob.dr_quantiles(np.zeros(65), np.arange(65.0), [0.5]))[0] == N.OB_E_UNSUPPORTED


@pytest.mark.parametrize("weighted", [False, True])
def test_ref_identities(weighted):
    k = 3
    xa, ya, xb, yb, wa, wb = R.panel(k, weighted, n_a=650, n_b=1285)
    thr = D.thresholds(np.concatenate([ya, yb]), 5, 0.1, 0.9)
    row, info = D.decompose(xa, ya, xb, yb, thr, TAUS, wa, wb)
    T, nq = len(thr), len(TAUS)
    assert row is not None and np.isfinite(row).all() and row[-1] == info["passes"].max()
    qe, qs = row[:3 * nq].reshape(3, nq), row[3 * nq:6 * nq].reshape(3, nq)
    de, fr = row[6 * nq:6 * nq + 3 * T].reshape(3, T), row[6 * nq + 3 * T:-1].reshape(4, T)
    assert np.all(np.abs(qe[1] + qe[2] - qe[0]) <= 1e-12) and np.all(np.abs(de[1] + de[2] - de[0]) <= 1e-12)
    assert np.array_equal(qe[0], qs[0] - qs[1]) and np.array_equal(de[0], fr[0] - fr[1])
    # a logit with an intercept reproduces the weighted share of its own sample under every threshold
    w_a, w_b = (np.ones(len(ya)) if wa is None else wa), (np.ones(len(yb)) if wb is None else wb)
    for t, c in enumerate(thr):
        assert abs(fr[0][t] - np.sum(w_a * (ya <= c)) / w_a.sum()) <= 1e-9
        assert abs(fr[1][t] - np.sum(w_b * (yb <= c)) / w_b.sum()) <= 1e-9
    # identical coefficients in both groups: no structure effect
    row2, _ = D.decompose(xa, ya, xa, ya, thr, TAUS, wa, wa)
    nq2 = len(TAUS)
    assert np.all(row2[:3 * nq2] == 0.0)


def test_finish_rows_match_ref(ob, O, N):
    """dr_finish on rows of the restatement, two of them failed: every component is the point entry with the
    oracle's bootstrap statistics of its column over the rows kept."""
    k = 3
    xa, ya, xb, yb, wa, wb = R.panel(k, True, n_a=300, n_b=400)
    thr = D.thresholds(np.concatenate([ya, yb]), 5, 0.1, 0.9)
    point, _ = D.decompose(xa, ya, xb, yb, thr, TAUS, wa, wb)
    rng = np.random.default_rng(2)
    reps = 24
    rows, ok = np.full((reps, len(point)), np.nan), np.zeros(reps, dtype=np.uint8)
    for r in range(reps):
        if r in (3, 17):
            continue
        row, _ = D.decompose(xa, ya, xb, yb, thr, TAUS, wa, wb, rng.multinomial(300, np.full(300, 1 / 300)),
                             rng.multinomial(400, np.full(400, 1 / 400)))
        assert row is not None
        rows[r], ok[r] = row, 1
    res = ob.dr_finish_rows(point, thr, TAUS, rows, ok)
    want = D.aggregate(O, point, rows, ok)
    T, nq = len(thr), len(TAUS)
    assert res.n_failed == 2 and np.array_equal(res.thresholds, thr) and np.array_equal(res.quantiles, TAUS)
    comps = []
    for table, parts in ((res.quantile_effects, D.EFFECTS), (res.quantile_values, ("A", "B", "C")),
                         (res.distribution_effects, D.EFFECTS), (res.cdf, ("AA", "BB", "AB", "BA"))):
        assert tuple(table) == parts
        for part in parts:
            assert [c.name for c in table[part]] == [f"{part}@{i}" for i in range(len(table[part]))]
            comps += table[part]
    assert len(comps) == 6 * nq + 7 * T == len(want)
    for c, w in zip(comps, want):
        assert c.estimate == w[0], c.name
        for got, exp in ((c.std_err, w[1]), (c.ci_lower, w[2]), (c.ci_upper, w[3])):
            assert abs(got - exp) <= 1e-12 * max(abs(exp), 1.0), (c.name, got, exp)
    for key, i in (("AA", 0), ("BB", 1), ("AB", 2)):
        assert np.array_equal(res.cdf_rearranged[key], np.sort(point[6 * nq + 3 * T + i * T:6 * nq + 3 * T + (i + 1) * T]))
    res.beta_a, res.beta_b, res.passes = np.zeros((T, k)), np.zeros((T, k)), np.zeros((2, T), dtype=int)  # no fits here
    js = json.loads(res.to_json())
    assert js["n_failed"] == 2 and js["thresholds"] == [float(v) for v in thr]
    assert js["quantile_effects"]["total"][2]["estimate"] == res.quantile_effects["total"][2].estimate
    with pytest.raises(ValueError):
        ob.dr_finish_rows(point[:-1], thr, TAUS, rows, ok)


def _frame(n=80, n_x=2):
    rng = np.random.default_rng(4)
    f = {"y": rng.normal(size=n).tolist(), "g": np.where(np.arange(n) % 2 == 0, "A", "B").tolist(),
         "w": rng.uniform(0.5, 2.0, n).tolist(), "s": (rng.random(n) < 0.7).astype(float).tolist(),
         "firm": [f"f{i % 5}" for i in range(n)], "cat": [("u", "v", "w")[i % 3] for i in range(n)]}
    for j in range(n_x):
        f[f"x{j}"] = rng.normal(size=n).tolist()
    return f


def _dr_config(N, taus=TAUS, thresholds=None, n_thresholds=5, lo=0.1, hi=0.9):
    dp = C.POINTER(C.c_double)
    keep = [np.ascontiguousarray(taus, dtype=np.float64)]
    dr = N.ob_dr_config()
    dr.quantiles, dr.n_quantiles = keep[0].ctypes.data_as(dp), len(keep[0])
    if thresholds is not None:
        keep.append(np.ascontiguousarray(thresholds, dtype=np.float64))
        dr.thresholds, dr.n_thresholds = keep[1].ctypes.data_as(dp), len(keep[1])
    else:
        dr.thresholds, dr.n_thresholds = None, n_thresholds
    dr.lo, dr.hi = lo, hi
    return dr, keep


def test_refusals_before_device_work(ob, N):
    lib = N.lib()
    fake = C.create_string_buffer(4096)  # no context at all: every check must come before it is read
    ctx = C.cast(fake, C.c_void_p)

    def prepare(builder, run=False, **dr_kw):
        cols, ncol, nrow = builder._frame.as_c()
        cfg, keep = builder._config()
        dr, keep2 = _dr_config(N, **dr_kw)
        h = C.c_void_p()
        fn = lib.ob_builder_run_dr if run else lib.ob_builder_prepare_dr
        rc = fn(ctx, cols, ncol, nrow, C.byref(cfg), C.byref(dr), C.byref(h))
        assert not h.value and fake.raw == bytes(4096)
        return rc, lib.ob_last_error().decode()

    def base(f=None, xs=("x0", "x1")):
        return ob.OaxacaBuilder(_frame() if f is None else f, "y", "g", "B").predictors(list(xs)).seed(1)

    for run in (False, True):
        assert prepare(base().categorical_predictors(["cat"]).normalize(["cat"]), run)[0] == N.OB_E_UNSUPPORTED
        assert prepare(base().heckman_selection("s", ["x0"]), run)[0] == N.OB_E_UNSUPPORTED
        assert prepare(base(), run, n_thresholds=65)[0] == N.OB_E_UNSUPPORTED
        assert prepare(base(), run, taus=np.linspace(0.01, 0.99, 33))[0] == N.OB_E_UNSUPPORTED
    rc, msg = prepare(base().normalize(["cat"]))
    assert rc == N.OB_E_UNSUPPORTED and "normalized" in msg
    rc, msg = prepare(base().heckman_selection("s", ["x0"]))
    assert rc == N.OB_E_UNSUPPORTED and "Heckman" in msg
    assert prepare(base(), thresholds=np.arange(65.0))[0] == N.OB_E_UNSUPPORTED
    # K = 33 > OB_DR_MAX_K
    wide = _frame(n=200, n_x=32)
    rc, msg = prepare(base(wide, [f"x{j}" for j in range(32)]))
    assert rc == N.OB_E_UNSUPPORTED and "32" in msg
    # thresholds that are not strictly increasing and finite, a tau outside (0, 1), too few of either
    for thr in ([0.0, 0.0, 1.0], [1.0, 0.5], [0.0, np.nan, 1.0], [0.0, np.inf], [0.3]):
        assert prepare(base(), thresholds=thr)[0] == N.OB_E_INVALID, thr
    for taus in ([0.0, 0.5], [0.5, 1.0], [-0.1], [np.nan], []):
        assert prepare(base(), taus=taus)[0] == N.OB_E_INVALID, taus
    assert prepare(base(), n_thresholds=1)[0] == N.OB_E_INVALID
    assert prepare(base(), lo=0.9, hi=0.1)[0] == N.OB_E_INVALID
    # a null and a non-finite value in a named column (the weights column included)
    for col, bad in (("x0", None), ("x1", float("nan")), ("y", float("inf")), ("w", None), ("w", float("nan"))):
        f = _frame()
        f[col][3] = bad
        rc, msg = prepare(base(f).weights("w"))
        assert rc == N.OB_E_INVALID and f"`{col}`" in msg, (col, bad, msg)
    f = _frame()
    f["g"][5] = None
    assert prepare(base(f))[0] == N.OB_E_INVALID
    assert prepare(base(xs=("x0", "nope")))[0] == N.OB_E_COLUMN
    # a group with rows <= K
    small = _frame(n=8, n_x=3)
    rc, msg = prepare(base(small, ["x0", "x1", "x2"]))
    assert rc == N.OB_E_INSUFFICIENT, msg
    # a constant outcome leaves one distinct threshold
    const = _frame()
    const["y"] = [1.0] * 80
    assert prepare(base(const))[0] == N.OB_E_INVALID
    # sample weights, categoricals and any reference_coefficients pass every check: the null context is what is left
    good = base().weights("w").categorical_predictors(["cat"]).reference_coefficients(ob.ReferenceCoefficients.Pooled)
    cols, ncol, nrow = good._frame.as_c()
    cfg, keep = good._config()
    dr, keep2 = _dr_config(N)
    h = C.c_void_p()
    rc = lib.ob_builder_prepare_dr(None, cols, ncol, nrow, C.byref(cfg), C.byref(dr), C.byref(h))
    assert rc == N.OB_E_INVALID and "null pointer" in lib.ob_last_error().decode()
    assert lib.ob_builder_prepare_dr(None, cols, ncol, nrow, C.byref(cfg), C.byref(dr), None) == N.OB_E_INVALID
    assert lib.ob_builder_prepare_dr(None, cols, ncol, nrow, C.byref(cfg), None, C.byref(h)) == N.OB_E_INVALID


def test_cluster_is_refused(ob, N):
    b = ob.OaxacaBuilder(_frame(), "y", "g", "B").predictors(["x0", "x1"]).cluster("firm")
    for fn in (b.prepare_distribution, b.decompose_distribution):
        code, msg = _code(N, fn)
        assert code == N.OB_E_UNSUPPORTED and "cluster" in msg


def test_piece_argument_errors(ob, N):
    x = np.column_stack([np.ones(10), np.arange(10.0)])
    y = np.arange(10.0)
    assert _code(N, lambda: ob.dr_logit_pass(x[:, ::-1], y, [4.5], np.zeros((1, 2))))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.dr_logit_pass(x, y, np.arange(65.0), np.zeros((65, 2))))[0] == N.OB_E_UNSUPPORTED
    assert _code(N, lambda: ob.dr_cdf(x, np.zeros((129, 2))))[0] == N.OB_E_UNSUPPORTED
    wide = np.column_stack([np.ones(40)] + [np.arange(40.0)] * 32)
    assert _code(N, lambda: ob.dr_cdf(wide, np.zeros((1, 33))))[0] == N.OB_E_UNSUPPORTED
    with pytest.raises(ValueError):
        ob.dr_cdf(x, np.zeros((1, 2)), counts=np.full(10, 256))
    with pytest.raises(ValueError):
        ob.dr_logit_pass(x, y, [1.0, 2.0], np.zeros((1, 2)))
