"""ob_tobit_fit, the Newton driver of the Tobit front end (ob_tobit_step_kernel), on its own: every
eta, flag and pass count against the numpy restatement tests/tobit_ref.py at the dimensions D = K + 1 where a lane
layout, a padding rule or the size of the kernel's arrays changes (2, 3, 16, 17, 18, 32); the device's eta against
the likelihood itself (tobit_ref.score_hp, mpmath); least squares without censoring; the halving guard; a Cholesky
factor that fails; and failed fits beside fits that run on in one batch.

Groups of 130 and 257 rows (tobit_ref.panel): a ragged sub-tile, and a one-row second tile. The case builders below
are plain numpy and are shared with test_tobit_host.py, which checks without a device the conditions these tests rest
on (the margin share, the halvings, the failed factor, what score_hp can see)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tobit_ref as R  # noqa: E402
from test_gpu_parity import RTOL, SEED, close  # noqa: E402

pytestmark = pytest.mark.gpu

REPS = 64 + 3  # a ragged second block of replicates
DIM_KS = (1, 2, 15, 16, 17, 31)
GUARD_KS = (1, 2, 16, 17, 31)
OLS_KS = (3, 17, 31)
HP_REPS = (0, 31, 66)  # the replicates whose eta meets the likelihood, beside the point fit
GROUPS = (R.GROUP_A, R.GROUP_B)
MARGIN_SHARE = 0.75


def group(k, g, weighted=True, censored=True):
    """(x, y, w, lower, upper) of one group of tobit_ref.panel; without censoring the rows at a limit are ordinary
    values."""
    p = R.panel(k, weighted)
    x, y, w = p[2 * g], p[2 * g + 1], p[4 + g]
    w = np.ones(len(y)) if w is None else w
    return (x, y, w) + ((p[6], p[7]) if censored else (None, None))


_ref = {}


def dim_case(O, k, g):
    """The restatement's side of (a): the point fit from the least-squares start and REPS replicate fits from the
    point fit (as a boot starts them), each (eta, passes, ok, norms) -> (inputs, counts (REPS, n), point fit,
    replicate fits, replicate ids). Computed once and shared (read-only).

    The replicates: Newton's steps square, so about half of all fits take a step within a factor 10 of 1e-6 and no
    run of consecutive replicate ids has three quarters of its fits outside that band (35 to 93 % over ids 0 .. 66 of
    these cases). The ids are therefore walked upwards from 0 and one is left out only where keeping it would put
    more than a fifth of the replicates inside the band; what decides is the restatement's step norms alone, never
    the device. Fits inside the band stay in every case: they take the within-1 side of the pass-count check."""
    if ("dim", k, g) not in _ref:
        x, y, w, lower, upper = group(k, g)
        ones = np.ones(len(y))
        point = R.fit(O, x, y, w, ones, R.ols_start(x, y, w), lower, upper)
        ids, counts, fits, inside = [], [], [], 0
        r = 0
        while len(ids) < REPS:
            assert r < 10 * REPS, "fewer than a tenth of the restatement's fits stay clear of the band"
            c = R.counts(O, SEED, r, g, len(y))
            f = R.fit(O, x, y, c * w, c, point[0], lower, upper)
            band = not R.margin_ok(f[3])
            if not band or 5 * (inside + 1) <= len(ids) + 1:
                ids.append(r)
                counts.append(c)
                fits.append(f)
                inside += band
            r += 1
        counts = np.stack(counts)
        counts.setflags(write=False)
        _ref[("dim", k, g)] = ((x, y, w, lower, upper), counts, point, fits, ids)
    return _ref[("dim", k, g)]


def margin_share(point, fits):
    return float(np.mean([R.margin_ok(f[3]) for f in [point] + fits]))


def guard_case(O, k, g):
    """(d): the least-squares start with theta x 20, from which the first steps leave theta > 0 and are halved ->
    (inputs, eta0, the restatement's traced fit)."""
    if ("guard", k, g) not in _ref:
        x, y, w, lower, upper = group(k, g)
        eta0 = R.ols_start(x, y, w)
        eta0[k] *= 20.0
        _ref[("guard", k, g)] = ((x, y, w, lower, upper), eta0,
                                 R.fit(O, x, y, w, np.ones(len(y)), eta0, lower, upper, trace=True))
    return _ref[("guard", k, g)]


def wls_longdouble(x, y, w):
    """Weighted least squares in np.longdouble by Cholesky on the normal equations -> (beta, sigma),
    sigma^2 = sum w r^2 / sum w."""
    xl, yl, wl = (np.asarray(a, dtype=np.longdouble) for a in (x, y, w))
    m, b = (xl * wl[:, None]).T @ xl, xl.T @ (wl * yl)
    k = len(b)
    l = np.zeros((k, k), dtype=np.longdouble)
    for j in range(k):
        l[j, j] = np.sqrt(m[j, j] - l[j, :j] @ l[j, :j])
        for i in range(j + 1, k):
            l[i, j] = (m[i, j] - l[i, :j] @ l[j, :j]) / l[j, j]
    for i in range(k):
        b[i] = (b[i] - l[i, :i] @ b[:i]) / l[i, i]
    for i in range(k - 1, -1, -1):
        b[i] = (b[i] - l[i + 1:, i] @ b[i + 1:]) / l[i, i]
    r = yl - xl @ b
    return b, np.sqrt(np.sum(wl * r * r) / np.sum(wl))


def ols_err(eta, beta, sigma):
    """The relative error of beta = delta / theta (against its largest entry) and of sigma = 1 / theta."""
    k = len(beta)
    e = np.asarray(eta, dtype=np.longdouble)
    return float(max(np.max(np.abs(e[:k] / e[k] - beta)) / np.max(np.abs(beta)), abs(1 / e[k] - sigma) / sigma))


def ols_case(O, k, g):
    """(c): no limit, so the maximiser is weighted least squares; the start has delta x 0.5 and theta x 1.5, so that
    the fit has steps to take -> (inputs, eta0, the restatement's fit, (beta, sigma) in long double)."""
    if ("ols", k, g) not in _ref:
        x, y, w, _, _ = group(k, g, censored=False)
        eta0 = R.ols_start(x, y, w)
        eta0[:k] *= 0.5
        eta0[k] *= 1.5
        _ref[("ols", k, g)] = ((x, y, w), eta0, R.fit(O, x, y, w, np.ones(len(y)), eta0), wls_longdouble(x, y, w))
    return _ref[("ols", k, g)]


def chol_case():
    """(e): group A of panel(3) with column 2 zeroed on the odd rows and only the odd rows counted: -H has an exact
    zero pivot -> (x, y, lower, upper, counts, eta0)."""
    xa, ya, _, _, _, _, lower, upper = R.panel(3)
    x = xa.copy()
    x[1::2, 2] = 0.0
    c = np.ones(len(ya), dtype=int)
    c[0::2] = 0
    return x, ya, lower, upper, c, R.ols_start(x, ya)


def batch_counts(O):
    """(f): 67 replicates on chol_case's frame. 63: its counts (the factor fails in pass 1); 64: censored rows only
    (dropped before a pass); 0, 62, 65, 66: bootstrap draws with the even rows zeroed; the rest: every row once."""
    x, y, lower, upper, c, _ = chol_case()
    counts = np.ones((REPS, len(y)), dtype=int)
    for r in (0, 62, 65, 66):
        counts[r] = R.counts(O, SEED, r, R.GROUP_A, len(y))
        counts[r, 0::2] = 0
    counts[63] = c
    counts[64] = 0
    counts[64, np.flatnonzero((y == lower) | (y == upper))[:3]] = [40, 40, 50]
    return counts


_dev = {}


def dim_device(ob, O, k, g):
    """The device's side of (a), shared by (a) and (b): one call for the point fit, one for the 67 replicates."""
    if (k, g) not in _dev:
        (x, y, w, lower, upper), counts, point, _, _ = dim_case(O, k, g)
        _dev[(k, g)] = (ob.tobit_fit(x, y, lower, upper, w=w), ob.tobit_fit(x, y, lower, upper, w=w, counts=counts, eta0=point[0]))
    return _dev[(k, g)]


def check_fit(N, got, want, what):
    """One fit as (a) asks: done and not failed, eta under RTOL of its largest entry, the pass count equal where
    rounding cannot decide it and within 1 elsewhere -> eta's error."""
    (eta, flag, passes), (w_eta, w_passes, w_ok, w_norms) = got, want[:4]
    assert w_ok, what
    assert flag == N.OB_TOBIT_DONE, (what, flag)
    good, worst = close(eta, w_eta, np.max(np.abs(w_eta)), RTOL)
    assert good, (what, worst)
    if R.margin_ok(w_norms):
        assert passes == w_passes, (what, passes, w_passes)
    assert abs(int(passes) - w_passes) <= 1, (what, passes, w_passes)
    return worst


@pytest.mark.parametrize("g", GROUPS, ids=["A", "B"])
@pytest.mark.parametrize("k", DIM_KS)
def test_fits_match_ref_at_every_dimension(ob, O, N, k, g):
    _, _, point, fits, ids = dim_case(O, k, g)
    share = margin_share(point, fits)
    assert share >= MARGIN_SHARE, share  # else the pass counts below would check nothing
    (p_eta, p_flags, p_passes), (eta, flags, passes) = dim_device(ob, O, k, g)
    assert np.isfinite(p_eta).all() and np.isfinite(eta).all()
    worst = check_fit(N, (p_eta[0], p_flags[0], p_passes[0]), point, "point")
    print(f"k={k} group={g}: point eta worst {worst:.3e}, {p_passes[0]} passes")
    worst = max(check_fit(N, (eta[r], flags[r], passes[r]), fits[r], r) for r in range(REPS))
    print(f"k={k} group={g}: replicate eta worst {worst:.3e}, passes {passes.min()}..{passes.max()}, margin share {share:.2f}, ids {ids[0]}..{ids[-1]}")


@pytest.mark.parametrize("g", GROUPS, ids=["A", "B"])
@pytest.mark.parametrize("k", DIM_KS)
def test_device_eta_is_the_maximiser(ob, O, k, g):
    """The restatement runs the kernels' iteration, so a score term wrong in both would pass the comparison above.
    Here the device's eta meets the likelihood: the score of a Newton fit is quadratic in the last step taken, so a
    last step that differs by rounding moves it by a small factor, hence 100 x the restatement's own score, floored
    at 1e-12; an eta wrong by a relative 1e-6 scores about 1e-6 (test_tobit_host.py)."""
    pytest.importorskip("mpmath")
    (x, y, w, lower, upper), counts, point, fits, _ = dim_case(O, k, g)
    (p_eta, _, _), (eta, _, _) = dim_device(ob, O, k, g)
    sides = [("point", w, p_eta[0], point[0])] + [(r, counts[r] * w, eta[r], fits[r][0]) for r in HP_REPS]
    for what, cw, got, want in sides:
        s_dev, s_ref = R.score_hp(x, y, cw, got, lower, upper), R.score_hp(x, y, cw, want, lower, upper)
        print(f"k={k} group={g} {what}: score_hp device {s_dev:.2e} restatement {s_ref:.2e}")
        assert s_dev <= max(100.0 * s_ref, 1e-12), (what, s_dev, s_ref)


@pytest.mark.parametrize("g", GROUPS, ids=["A", "B"])
@pytest.mark.parametrize("k", OLS_KS)
def test_no_censoring_is_least_squares(ob, O, N, k, g):
    (x, y, w), eta0, ref, (beta, sigma) = ols_case(O, k, g)
    assert ref[2] and ref[1] >= 2
    bar = max(100.0 * ols_err(ref[0], beta, sigma), 1e-12)
    eta, flags, passes = ob.tobit_fit(x, y, w=w, eta0=eta0)
    err = ols_err(eta[0], beta, sigma)
    print(f"k={k} group={g}: least-squares error device {err:.2e} restatement {ols_err(ref[0], beta, sigma):.2e}, {passes[0]} passes")
    assert flags[0] == N.OB_TOBIT_DONE and err <= bar, (err, bar)
    res = ob.tobit(x, y, w=w)
    err = ols_err(res["eta"], beta, sigma)
    e_direct = float(max(np.max(np.abs(res["beta"] - beta)) / np.max(np.abs(beta)), abs(res["sigma"] - sigma) / sigma))
    print(f"k={k} group={g}: tobit() error {e_direct:.2e}, {res['passes']} passes")
    assert err <= bar and e_direct <= bar, (err, e_direct, bar)
    assert res["converged"] is True and res["passes"] >= 1
    assert res["beta"].shape == (k,) and res["eta"].shape == (k + 1,)


@pytest.mark.parametrize("g", GROUPS, ids=["A", "B"])
@pytest.mark.parametrize("k", GUARD_KS)
def test_the_guard_halves_the_step(ob, O, N, k, g):
    (x, y, w, lower, upper), eta0, ref = guard_case(O, k, g)
    assert sum(ref[4]) >= 1, ref[4]  # the restatement halved: the device meets the same steps
    eta, flags, passes = ob.tobit_fit(x, y, lower, upper, w=w, eta0=eta0)
    worst = check_fit(N, (eta[0], flags[0], passes[0]), ref, "guard")
    print(f"k={k} group={g}: {sum(ref[4])} halvings, {ref[1]} passes (device {passes[0]}), eta worst {worst:.3e}")


def test_a_failed_cholesky_counts_its_pass(ob, O, N):
    x, y, lower, upper, c, eta0 = chol_case()
    assert np.sum(c[R.classes(y, lower, upper) == 0]) > x.shape[1] and not x[c > 0, 2].any()
    assert R.fit(O, x, y, c.astype(float), c, eta0, lower, upper)[1:3] == (1, False)
    eta, flags, passes = ob.tobit_fit(x, y, lower, upper, counts=c[None, :], eta0=eta0)
    assert flags[0] == N.OB_TOBIT_DONE | N.OB_TOBIT_FAILED and passes[0] == 1
    assert np.isfinite(eta).all() and eta[0].tobytes() == eta0.tobytes()


def test_failed_fits_leave_their_neighbours_alone(ob, O, N):
    """Replicates 63 and 64, either side of the 64-replicate block boundary, end in round 1 with their codes while
    the batch runs on: every replicate has the bytes of its own counts run alone, and the outcome (converged or
    not, the pass count) that the restatement gives it. The draws of replicates 0, 62, 65 and 66 lose their even
    rows, so column 2 is zero on their rows as well and their factor fails like replicate 63's; the fits that run on
    are those that count every row once."""
    x, y, lower, upper, _, eta0 = chol_case()
    counts = batch_counts(O)
    eta, flags, passes = ob.tobit_fit(x, y, lower, upper, counts=counts, eta0=eta0)
    failed = N.OB_TOBIT_DONE | N.OB_TOBIT_FAILED
    assert (flags[63], passes[63]) == (failed, 1) and eta[63].tobytes() == eta0.tobytes()
    assert (flags[64], passes[64]) == (failed, 0) and eta[64].tobytes() == eta0.tobytes()
    assert flags[1] == N.OB_TOBIT_DONE and passes[1] >= 2 and np.isfinite(eta).all()
    alone, want = {}, {}
    for r in range(REPS):
        key = counts[r].tobytes()
        if key not in alone:
            alone[key] = ob.tobit_fit(x, y, lower, upper, counts=counts[r:r + 1], eta0=eta0)
            want[key] = R.fit(O, x, y, counts[r].astype(float), counts[r], eta0, lower, upper)
        a_eta, a_flags, a_passes = alone[key]
        assert eta[r].tobytes() == a_eta[0].tobytes() and flags[r] == a_flags[0] and passes[r] == a_passes[0], r
        _, w_passes, w_ok, w_norms = want[key]
        assert flags[r] == (N.OB_TOBIT_DONE if w_ok else failed), (r, flags[r])
        assert abs(int(passes[r]) - w_passes) <= (0 if not w_ok or R.margin_ok(w_norms) else 1), (r, passes[r], w_passes)
