"""Each Newton pass of ob_logit, and the launch shapes of ob_kde that tests/test_gpu_dfl.py leaves
out, against extended-precision references (tests/dfl_ref.py: logit_trajectory, kde).

A converged beta is fixed by the gradient alone, so a wrong information matrix (a dropped row, a
wrong p (1 - p), two swapped pairs) only bends the path to it. These tests hold every iterate
beta_t, t = 1 .. min(iterations, 4), to 512 cond(H_t) 2^-52 of the extended recursion (dfl_ref.beta_bar;
tests/test_dfl_host.py shows the f64 restatement within 1/8 of it), over the case table
dfl_ref.PASS_CASES: every column-block edge, full and ragged sub-tiles, and n > 262144 where a wave
loops over more than one sub-tile (spu = 2, 3).

Probabilities: 1e-12 absolute. |d p| <= |d eta| / 4 and |d eta| <~ k eps |eta| + |d beta| |x|, with
|eta| < 45 in every case (asserted on the CPU). KDE: 1e-10 x max density as in test_gpu_dfl.py; the
largest case adds 8 shuffle levels and 1024 chunks serially, about 1032 u = 1.1e-13 relative.
Each test prints its worst figure as a fraction of its bar before it asserts.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dfl_ref as R  # noqa: E402
from test_gpu_dfl import _check_against_ref  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-6
P_BAR = 1e-12
LD = np.longdouble
_D = C.POINTER(C.c_double)
SENTINEL = -7.25


def _dp(a):
    return a.ctypes.data_as(_D)


def _logit(N, x, y, max_iter, tol, ldx=None):
    """ob_logit through ctypes -> (rc, beta, probs, converged, iterations); x is (n, k). The padding
    rows of the column-major buffer hold NaN; beta and probs start as SENTINEL."""
    n, k = x.shape
    ldx = n if ldx is None else ldx
    buf = np.full((k, ldx), np.nan)
    buf[:, :n] = x.T
    y = np.ascontiguousarray(y, dtype=np.float64)
    beta, probs = np.full(k, SENTINEL), np.full(n, SENTINEL)
    conv, iters = C.c_int32(-1), C.c_int32(-1)
    rc = N.lib().ob_logit(N.context(0), _dp(buf), ldx, _dp(y), n, k, max_iter, tol, _dp(beta), _dp(probs),
                          C.byref(conv), C.byref(iters))
    return rc, beta, probs, conv.value, iters.value


def _case_params(cases):
    return [pytest.param(c, id=c.id, marks=[] if R.EXTENDED or not c.big else pytest.mark.skip(reason=R.BIG_SKIP))
            for c in cases]


def _probs_at(tr, t):
    """The extended probabilities at beta_t."""
    return tr["probs_start"][t] if t < len(tr["betas"]) else tr["final_probs"]


def _check_trajectory(N, case, ldx):
    """ob_logit(max_iter = t, tol = 0) for every t against the extended trajectory -> the worst
    fractions of the beta bar and of the probability bar, and the outputs of each t."""
    x, y = case.data()
    tr = case.trajectory()
    worst_b = worst_p = 0.0
    outs = []
    for t in range(1, case.steps() + 1):
        rc, beta, probs, conv, iters = _logit(N, x, y, t, 0.0, ldx=ldx)
        assert rc == N.OB_OK, N.lib().ob_last_error().decode()
        ref = tr["betas"][t - 1]
        err = float(np.max(np.abs(beta.astype(LD) - ref)) / np.max(np.abs(ref)))
        bar = R.beta_bar(tr["conds"][t - 1])
        perr = float(np.max(np.abs(probs.astype(LD) - _probs_at(tr, t))))  # ob_logit_probs_kernel
        print(f"logit pass {case.id} t={t}: beta err {err:.3e} = {err / bar:.4f} of the bar (cond {tr['conds'][t - 1]:.2f}),"
              f" prob err {perr:.3e} = {perr / P_BAR:.4f} of the bar")
        worst_b, worst_p = max(worst_b, err / bar), max(worst_p, perr / P_BAR)
        assert conv == 0 and iters == t
        assert err <= bar, (case.id, t, err, bar)
        assert perr <= P_BAR, (case.id, t, perr)
        outs.append((beta, probs))
    print(f"logit passes {case.id}: worst beta error {worst_b:.4f} of the bar, worst probability error {worst_p:.4f} of the bar")
    return outs


@pytest.mark.parametrize("case", _case_params(R.PASS_CASES))
def test_each_newton_pass_matches_extended_ref(N, case):
    _check_trajectory(N, case, case.ldx)


@pytest.mark.parametrize("case", _case_params([c for c in R.PASS_CASES if c.converges]))
def test_converged_run_matches_extended_ref(N, case):
    x, y = case.data()
    ref, tr = case.converged(), case.trajectory()
    norms = ref["step_norms"]
    assert ref["converged"] and norms[-1] <= TOL / 2 and norms[-2] >= 2 * TOL, norms
    rc, beta, probs, conv, iters = _logit(N, x, y, 100, TOL, ldx=case.ldx)
    assert rc == N.OB_OK, N.lib().ob_last_error().decode()
    assert conv == 1 and iters == ref["iterations"] == len(tr["betas"])
    # the pass kernel's own write of p at the last iteration's start (logit.rs:98-105)
    perr = float(np.max(np.abs(probs.astype(LD) - tr["probs_start"][iters - 1])))
    last = tr["betas"][-1]
    err = float(np.max(np.abs(beta.astype(LD) - last)) / np.max(np.abs(last)))
    bar = R.beta_bar(tr["conds"][-1])
    print(f"converged {case.id}: {iters} iterations, prob err {perr:.3e} = {perr / P_BAR:.4f} of the bar,"
          f" beta err {err:.3e} = {err / bar:.4f} of the bar")
    assert perr <= P_BAR
    if iters <= case.steps():  # the last iterate is one of those held to the bar
        assert err <= bar


@pytest.mark.parametrize("n,seed", [(64, 44), (4099, 44)])
def test_intercept_only_closed_form(N, n, seed):
    x, y = R.panel(n, 1, seed)
    ref = R.logit(y, x, 100, TOL)
    norms = ref["step_norms"]
    assert ref["converged"] and norms[-1] <= TOL / 2 and norms[-2] >= 2 * TOL, norms
    m = LD(np.sum(y)) / LD(n)
    assert 0 < m < 1
    exact = float(np.log(m / (1 - m)))
    # Newton converges quadratically: the next step is about norms[-1]^2, far under the bar
    assert norms[-1] ** 2 < 1e-13
    rc, beta, probs, conv, iters = _logit(N, x, y, 100, TOL)
    assert rc == N.OB_OK and conv == 1 and iters == ref["iterations"]
    err = abs(beta[0] - exact)
    print(f"k=1 n={n}: beta {beta[0]!r}, log(m / (1 - m)) {exact!r}, error {err:.3e} = {err / 1e-12:.4f} of the bar")
    assert err <= 1e-12


PADDED = [("128x16", 128 + 64), ("3000x49", 3001), ("262145x3", 262145 + 63)]


@pytest.mark.parametrize("case_id,ldx", PADDED)
def test_padding_rows_are_never_read(N, case_id, ldx):
    """ldx > n with NaN in every padding row: the same bytes as the dense call, inside the bar."""
    case = next(c for c in R.PASS_CASES if c.id == case_id)
    if case.big and not R.EXTENDED:
        pytest.skip(R.BIG_SKIP)
    x, y = case.data()
    padded = _check_trajectory(N, case, ldx)
    t = len(padded)
    rc, beta, probs, _, _ = _logit(N, x, y, t, 0.0)
    assert rc == N.OB_OK
    assert beta.tobytes() == padded[-1][0].tobytes() and probs.tobytes() == padded[-1][1].tobytes()


@pytest.mark.parametrize("n,k,row,col", [(1000, 17, 999, 16), (262145, 3, 262144, 1), (300, 5, 0, 0)])
def test_nan_in_a_live_row_is_a_linalg_error(N, n, k, row, col):
    x, y = R.panel(n, k, 77)
    x[row, col] = np.nan
    rc, beta, probs, conv, iters = _logit(N, x, y, 100, TOL)
    assert rc == N.OB_E_LINALG
    assert R.LINALG_MESSAGE in N.lib().ob_last_error().decode()
    # nothing else: no coefficients, no probabilities, no convergence report
    assert np.all(beta == SENTINEL) and np.all(probs == SENTINEL) and (conv, iters) == (-1, -1)


def test_two_runs_at_spu_2_give_identical_bytes(N):
    case = next(c for c in R.PASS_CASES if c.id == "262145x3")
    x, y = case.data()
    for max_iter, tol in ((2, 0.0), (100, TOL)):
        a, b = _logit(N, x, y, max_iter, tol), _logit(N, x, y, max_iter, tol)
        assert a[0] == N.OB_OK and a[3:] == b[3:]
        assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


# ---- KDE launch geometry ------------------------------------------------------------------------

KDE_SHAPES = [  # (n, n_grid): chunks, grid groups
    (262145 + 300, 1),   # the 1024-chunk cap (chunk = 257, the last chunk short), one grid point
    (262145 + 300, 2),   # ... grid remainder 2 of the four points per thread
    (262145 + 300, 3),   # ... remainder 3 (these three run 1022 chunks of 257)
    (263167, 1),         # all 1024 chunks, the last one short by one
    (300, 16388),        # 4097 grid groups: one chunk wanted, one chunk run
    (257, 5),            # two chunks, grid remainder 1 in the second group
]


@pytest.mark.parametrize("n,n_grid", KDE_SHAPES)
def test_kde_launch_shapes_match_ref(ob, n, n_grid):
    rng = np.random.default_rng(1000 + n + n_grid)
    data = rng.normal(size=n)
    h = R.silverman_bandwidth(data)
    w_rand = rng.random(n) + 0.05
    w_zero = w_rand.copy()
    w_zero[::3] = 0.0
    grid = np.linspace(-3.5, 3.5, n_grid) if n_grid > 3 else np.array([0.25, -1.5, 2.75][:n_grid])
    worst = 0.0
    for name, w in (("none", None), ("random", w_rand), ("every third zero", w_zero)):
        got = ob.kde(data, grid, h, weights=w)
        ref = R.kde(data, w, grid, h)
        err = float(np.max(np.abs(got - ref)) / np.max(ref))
        print(f"kde n={n} n_grid={n_grid} weights {name}: error / max density {err:.3e} = {err / 1e-10:.5f} of the bar")
        worst = max(worst, err)
        assert got.shape == (n_grid,) and np.all(ref > 0)
        assert err <= 1e-10, (n, n_grid, name, err)
    print(f"kde n={n} n_grid={n_grid}: worst {worst / 1e-10:.5f} of the bar")


# ---- the weight clamp of dfl.rs:151 --------------------------------------------------------------

def _separated_frame(n=3000, seed=61, shift=5.0):
    """Two groups whose predictor x1 differs by ``shift``: N(shift, 1) in group A ("north"), N(0, 2^2)
    in "west", and 14 west rows beyond A's mean (shift + 5 .. shift + 6). West's lower half gets
    p < 0.0001 and those 14 rows p > 0.9999, so min(max(p, 0.0001), 0.9999) binds on both sides."""
    rng = np.random.default_rng(seed)
    g = rng.choice(["north", "west"], size=n, p=[0.55, 0.45])
    is_a = g == "north"
    x1 = np.where(is_a, rng.normal(size=n) + shift, 2.0 * rng.normal(size=n))
    x1[np.flatnonzero(~is_a)[:14]] = shift + 5.0 + rng.random(14)
    x2 = rng.integers(18, 60, size=n)
    y = 2.0 + 0.05 * x1 + 0.02 * x2 + 0.4 * is_a + rng.normal(scale=0.7, size=n)
    return {"wage": y.tolist(), "region": g.tolist(), "x1": x1.tolist(), "x2": x2.tolist()}


def test_dfl_weight_clamp_binds(ob):
    f = _separated_frame()
    x, _ = R.design(f, ["x1", "x2"])
    y = np.array([1.0 if v == "north" else 0.0 for v in f["region"]])
    fit = R.logit(y, x, 100, TOL)
    p_b = fit["predicted_probs"][y == 0.0]
    high, low = int(np.sum(p_b > 0.9999)), int(np.sum(p_b < 0.0001))
    norms = fit["step_norms"]
    print(f"weight clamp frame: {high} non-A rows above 0.9999, {low} below 0.0001, step norms {norms[-2:]}")
    assert high >= 10 and low >= 10
    assert fit["converged"] and norms[-1] <= TOL / 2 and norms[-2] >= 2 * TOL, norms
    ref = R.run_dfl(f, "wage", "region", "west", ["x1", "x2"])
    assert ref["group_a"] == "north" and ref["iterations"] == fit["iterations"]
    # the clamp decides the result: without it the counterfactual density moves far beyond the bar
    w = ref["weights"]
    assert np.isclose(w.max(), 9999.0 * ref["n_b"] / ref["n_a"], rtol=1e-12) and np.sum(w == w.max()) == high
    assert np.isclose(w.min(), (0.0001 / 0.9999) * ref["n_b"] / ref["n_a"], rtol=1e-12) and np.sum(w == w.min()) == low
    _check_against_ref(ob.run_dfl(f, "wage", "region", "west", ["x1", "x2"]), ref)
