"""The leave-one-out pass on the MI355X (ob_jackknife.hip) against the references of tests/jackknife_ref.py:
brute force (the oracle on the panel without the row) and the numpy closed form. Tolerance: J.TOL = 8 E with E
the closed form's measured error against brute force (see jackknife_ref's docstring and DESIGN.md §5.10), as a
mixed error max|d| / max(|ref|, |total_gap|)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jackknife_ref as J  # noqa: E402

pytestmark = pytest.mark.gpu

REF_IDS = list(J.REFS)


def _engine_rows(ob, ref, data, n_num=None):
    xa, ya, wa, xb, yb, wb = data
    return ob.jackknife_rows(xa, ya, wa, xb, yb, wb, ref, n_num=n_num)


def _compare(ob, O, ref, data, n_num=None, expect_drop=()):
    """Engine rows against brute force (on the rows J.brute_rows picks) and against the closed form (all rows)."""
    xa, ya, wa, xb, yb, wb = data
    rows = J.brute_rows(len(ya), len(yb), xa.shape[1])
    bt, rcs = J.brute(O, ref, xa, ya, wa, xb, yb, wb, rows, n_num)
    bad = set(int(r) for r in rows[rcs != 0])
    assert bad == set(expect_drop)  # precondition: every other brute-force pass returned rc 0
    theta, kept, n_dropped = _engine_rows(ob, ref, data, n_num)
    n_a = len(ya)
    assert n_dropped == (sum(1 for r in expect_drop if r < n_a), sum(1 for r in expect_drop if r >= n_a))
    assert set(np.flatnonzero(kept == 0).tolist()) == set(expect_drop)
    gap = J.point(O, ref, xa, ya, wa, xb, yb, wb, n_num)[5]
    good = rcs == 0
    e_brute = J.mixed_error(theta[rows[good]], bt[good], gap)
    cf, cf_kept = J.closed_form(ref, xa, ya, wa, xb, yb, wb)
    assert np.array_equal(cf_kept, kept.astype(bool))
    e_closed = J.mixed_error(theta[cf_kept], cf[cf_kept], gap)
    print(f"mixed error: vs brute force {e_brute:.3e}, vs closed form {e_closed:.3e} (TOL {J.TOL:.3e})")
    assert e_brute <= J.TOL
    assert e_closed <= J.TOL
    return theta, kept


@pytest.mark.parametrize("weighted", [False, True], ids=["ols", "wls"])
@pytest.mark.parametrize("ref", REF_IDS)
@pytest.mark.parametrize("shape", J.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_rows_match_brute_force(ob, O, shape, ref, weighted):
    data = J.panel(O, shape[0], shape[1], shape[2], weighted, 11 + shape[2])
    _compare(ob, O, J.REFS[ref], data)


@pytest.mark.parametrize("weighted", [False, True], ids=["ols", "wls"])
@pytest.mark.parametrize("ref", REF_IDS)
def test_rows_with_dummy_columns(ob, O, ref, weighted):
    """n_num = 2: the oracle's pooled fit has its indicator between the numeric and the dummy columns."""
    _compare(ob, O, J.REFS[ref], J.dummy_panel(O, 61, 45, weighted, 5), n_num=2)


@pytest.mark.parametrize("ref", REF_IDS)
def test_single_member_dummy_is_dropped(ob, O, ref):
    """Row 7 is the only member of a dummy in A: the fit without it is singular, brute force fails for exactly
    that row, the engine counts one dropped row in A and marks it; every other row matches."""
    data = J.dummy_panel(O, 61, 45, False, 5, single_member=True)
    theta, kept = _compare(ob, O, J.REFS[ref], data, n_num=2, expect_drop=(7,))
    assert np.isnan(theta[7]).all() and kept[7] == 0


@pytest.mark.parametrize("ref", REF_IDS)
def test_zero_weight_row(ob, O, ref):
    """A zero-weight row changes no sum: its theta_(i) is the closed form's, with beta and the means unchanged,
    so for the group's own reference coefficients it is the point estimate itself."""
    data = J.zero_weight_panel(O)
    theta, kept = _compare(ob, O, J.REFS[ref], data)
    xa, ya, wa, xb, yb, wb = data
    pt = J.point(O, J.REFS[ref], *data)
    for i in (5, len(ya) + 9):
        assert kept[i] == 1
        assert J.mixed_error(theta[i], pt, pt[5]) <= J.TOL


@pytest.mark.parametrize("ref", REF_IDS)
def test_multi_block_sums(ob, O, ref):
    """n_A = 5,000, n_B = 3,001, p = 5: several waves and blocks per group. The power sums' statistics against
    the closed form's, and two calls return the same bytes. Both sides form the deviations d from the changes
    themselves (J.closed_form(deviations=True), jack_delta in the kernel): jack_bias multiplies d's mean by
    m_g - 1, so d = theta_(i) - theta_hat taken as a difference would put (m_g - 1) roundings of theta_hat into it,
    3e-12 of the total gap here in numpy f64 against a longdouble run, more than the bound. The longdouble run of
    the same formulas is printed beside it."""
    xa, ya, wa, xb, yb, wb = data = J.panel(O, 5000, 3001, 5, True, 21)
    r = J.REFS[ref]
    panel = ob.Panel(xa, ya, xb, yb, wa, wb, device=0)
    try:
        a, b = panel.jackknife(r), panel.jackknife(r)
    finally:
        panel.close()
    assert a.n_dropped == (0, 0) and a.n_used == (5000, 3001)
    for f in ("estimate", "accel", "std_err", "bias", "sums"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes()
    d, kept = J.closed_form(r, *data, deviations=True)
    assert kept.all()
    pt = J.point(O, r, *data)
    assert J.mixed_error(a.estimate, pt, pt[5]) <= 1e-9  # the engine's own point estimate (SURVEY §8c bound)
    sums, used = J.power_sums(d, kept, np.zeros(d.shape[1]), 5000)
    want = J.finish(sums, used)
    ld, _, ld_hat = J.closed_form(r, *data, with_point=True, dtype=np.longdouble)
    want_ld = J.finish(*J.power_sums((ld - ld_hat[None, :]).astype(np.float64), kept, np.zeros(d.shape[1]), 5000))
    got = np.stack([a.accel, a.std_err, a.bias], axis=1)
    for j, name in enumerate(("accel", "jack_se", "jack_bias")):
        e = J.mixed_error(got[:, j], want[:, j], pt[5])
        print(f"{name}: mixed error {e:.3e} (TOL {J.TOL:.3e}); against the longdouble run "
              f"{J.mixed_error(got[:, j], want_ld[:, j], pt[5]):.3e}, the f64 reference against it "
              f"{J.mixed_error(want[:, j], want_ld[:, j], pt[5]):.3e}")
    for j in range(3):
        assert J.mixed_error(got[:, j], want[:, j], pt[5]) <= J.TOL
    assert ob.jackknife_last_timing() > 0.0


def _frame(O, n, p, seed):
    d = O.synthetic_panel(n, p, False, seed=seed)
    x = np.vstack([d["xa"], d["xb"]])
    f = {f"x{j}": x[:, j].tolist() for j in range(p)}
    f["y"] = np.concatenate([d["ya"], d["yb"]]).tolist()
    f["g"] = ["M"] * len(d["ya"]) + ["F"] * len(d["yb"])
    return f, [f"x{j}" for j in range(p)]


def test_builder_run_bca(ob, O, N):
    f, preds = _frame(O, 2000, 5, 31)
    mk = lambda: ob.OaxacaBuilder(f, "y", "g", "F").predictors(preds).bootstrap_reps(999).seed(77)
    plain, bca = mk().run(), mk().run_bca(0.95)
    assert plain.jackknife is None and bca.jackknife
    tables = lambda r: {"two_fold": r.two_fold.aggregate, "three_fold": r.three_fold.aggregate,
                        "detailed_explained": r.two_fold.detailed_explained,
                        "detailed_unexplained": r.two_fold.detailed_unexplained}
    pr = mk().prepare()
    try:
        rows, ok = pr.boot(0, 999)
        assert ok.all()
        jk = pr.jackknife()
        assert jk.n_dropped == (0, 0)
        again = pr.finish_bca(rows, ok, 0.95)
    finally:
        pr.close()
    col = {("two_fold", "explained"): 0, ("two_fold", "unexplained"): 1, ("three_fold", "endowments"): 2,
           ("three_fold", "coefficients"): 3, ("three_fold", "interaction"): 4}
    names = ["__ob_intercept__"] + preds
    for j, nm in enumerate(names):
        col[("detailed_explained", nm)] = 6 + j
        col[("detailed_unexplained", nm)] = 6 + len(names) + j
    for t, comps in tables(bca).items():
        for c0, c1, c2 in zip(tables(plain)[t], comps, tables(again)[t]):
            assert (c0.name, c0.estimate, c0.std_err, c0.p_value, c0.t_stat) == \
                   (c1.name, c1.estimate, c1.std_err, c1.p_value, c1.t_stat)
            j = col[(t, c1.name)]
            info = bca.jackknife[(t, c1.name)]
            assert info["accel"] == jk.accel[j] and info["std_err"] == jk.std_err[j] and info["bias"] == jk.bias[j]
            want = J.bca(rows[:, j], c1.estimate, jk.accel[j], 0.95)
            assert want["flag"] == info["flag"]
            if want["flag"] == 0:
                for key in ("alpha_lo", "alpha_hi"):
                    assert abs(want[key] * 999 - round(want[key] * 999)) > 1e-6
                assert (c1.ci_lower, c1.ci_upper) == (want["ci_lower"], want["ci_upper"])
            else:
                assert np.isnan(c1.ci_lower) and np.isnan(c1.ci_upper)
            assert (c2.ci_lower, c2.ci_upper) == (c1.ci_lower, c1.ci_upper) or want["flag"] != 0
    # the jackknife standard error is an independent check of the bootstrap one: same order
    e = bca.explained()
    assert 0.5 < bca.jackknife[("two_fold", "explained")]["std_err"] / e.std_err < 2.0


def test_finish_bca_on_sharded_rows(ob, O, N):
    f, preds = _frame(O, 2000, 5, 31)
    b = ob.OaxacaBuilder(f, "y", "g", "F").predictors(preds).bootstrap_reps(999).seed(77)
    want = b.run_bca(0.9)
    b._ctx = N.rank_context(0, 0, 1, N.unique_id())
    pr = b.prepare()
    try:
        rows, ok = pr.boot_sharded(0, 999)
        got = pr.finish_bca(rows, ok, 0.9)
    finally:
        pr.close()
    for x, y in zip(want.two_fold.aggregate + want.two_fold.detailed_explained + want.two_fold.detailed_unexplained
                    + want.three_fold.aggregate,
                    got.two_fold.aggregate + got.two_fold.detailed_explained + got.two_fold.detailed_unexplained
                    + got.three_fold.aggregate):
        assert x.name == y.name and x.estimate == y.estimate and x.std_err == y.std_err
        assert (x.ci_lower, x.ci_upper) == (y.ci_lower, y.ci_upper) or (np.isnan(x.ci_lower) and np.isnan(y.ci_lower))
    assert got.jackknife == want.jackknife or all(
        got.jackknife[k]["accel"] == want.jackknife[k]["accel"] for k in want.jackknife)


def test_limits_on_a_panel(ob, O, N):
    """The unsupported panels are refused (before any device work) through the panel entry points too."""
    d = O.synthetic_panel(200, 3, False, seed=2)
    ya2 = np.column_stack([d["ya"], d["ya"] * 2])
    yb2 = np.column_stack([d["yb"], d["yb"] * 2])
    p2 = ob.Panel(d["xa"], ya2, d["xb"], yb2, device=0)
    try:
        with pytest.raises(N.OaxacaError) as e:
            p2.jackknife(0)
        assert e.value.code == N.OB_E_UNSUPPORTED
    finally:
        p2.close()
    small = ob.Panel(d["xa"][:5], d["ya"][:5], d["xb"], d["yb"], device=0)
    try:
        with pytest.raises(N.OaxacaError) as e:
            small.jackknife_rows(0)
        assert e.value.code == N.OB_E_INSUFFICIENT
    finally:
        small.close()
    f, preds = _frame(O, 400, 3, 3)
    plain = ob.OaxacaBuilder(f, "y", "g", "F").predictors(preds).bootstrap_reps(8).seed(1).run()
    assert plain.jackknife is None
