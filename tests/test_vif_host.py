"""VIF without a GPU: the NumPy restatement (tests/vif_ref.py) against the reference's own unit cases
(tests/golden/vif_kat.json), ob_vif_solve against the restatement bit for bit, the argument errors that
every entry point raises before any device work, and the condition that tests/test_gpu_vif.py relies on,
shown here on the restatement alone for every shape it uses: the f64 restatement is within 1/8 of each
bar (vif_ref.py's docstring) of its own longdouble run, so the bars leave the device 7/8 of their width.

The one exception is the Gram at n = 5: its bar, n u sum|terms|, is five roundings wide and a single
correctly rounded product and sum already use one of them, so no f64 evaluation can stay within an
eighth of it; there the restatement is held to half the bar."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import vif_ref as V  # noqa: E402

KAT = json.load(open(os.path.join(HERE, "golden", "vif_kat.json")))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _kat_x(name):
    return np.array(KAT[name]["columns"], dtype=np.float64).T


def test_restatement_reproduces_kats():
    k = KAT["calculate_vif"]
    for dtype in (np.float64, V.LD):
        assert np.max(np.abs(V.vif(_kat_x("calculate_vif"), dtype) - np.array(k["vif"]))) < 1e-9
    k = KAT["perfect_multicollinearity"]
    with pytest.raises(V.VifRefError) as e:
        V.vif(_kat_x("perfect_multicollinearity"))
    assert e.value.kind == "linalg" and str(e.value) == k["error"]
    assert [str(v) for v in e.value.partial] == k["scores_before_failure"]  # inf, inf, then x3's fit fails
    with pytest.raises(V.VifRefError) as e:
        V.vif(np.ones((5, 1)))
    assert e.value.kind == "diagnostic" and str(e.value) == KAT["too_few_predictors"]["error"]
    with pytest.raises(V.VifRefError) as e:
        V.vif(V.fixture(3, 3, 1))
    assert e.value.kind == "insufficient"


@pytest.mark.parametrize("n,k", [(5, 3), (40, 2), (40, 4), (200, 5), (300, 17), (300, 33)])
def test_solve_is_the_restatement_bit_for_bit(ob, n, k):
    """ob_vif_solve on the restatement's own Gram returns the restatement's coefficients bit for bit: the
    operation order is the same. The order is nalgebra's, written out term by term in
    vif_ref.solve_sequential. oracle._chol_solve_nalgebra, which the f64 restatement solves with, states the
    same order but hands its back-substitution's dot product to BLAS, which fuses each product into its sum
    and regroups long sums; it agrees bit for bit only where that cannot matter (K = 2: one-term dot
    products) and to a backward-stable solve's rounding everywhere."""
    x = _kat_x("calculate_vif") if (n, k) == (5, 3) else V.fixture(n, k, n + k)
    g = V.gram(x)
    got = ob.vif_solve(g, n)
    assert got.shape == (k + 1, k) and not got[np.arange(k), np.arange(k)].any()
    assert np.array_equal(_bits(got), _bits(V.solve_sequential(g, n, k)))
    ref = V.solve(g, n, k)
    if k == 2:
        assert np.array_equal(_bits(got), _bits(ref))
    assert np.max(np.abs(got - ref)) <= 8 * k * V.U * np.linalg.cond(g) * np.max(np.abs(ref))


def test_solve_fails_on_the_collinear_gram(ob, N):
    g = V.gram(_kat_x("perfect_multicollinearity"))
    with pytest.raises(N.OaxacaError) as e:
        ob.vif_solve(g, 5)
    assert e.value.code == N.OB_E_LINALG and KAT["perfect_multicollinearity"]["error"] in str(e.value)
    assert str(e.value).startswith("Nalgebra error: ")
    g = V.gram(V.fixture(50, 4, 2))
    g[1, 1] = np.nan  # a NaN reaches a pivot and fails there, as in the reference
    with pytest.raises(N.OaxacaError) as e:
        ob.vif_solve(g, 50)
    assert e.value.code == N.OB_E_LINALG


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _rc(N, rc):
    return rc, N.lib().ob_last_error().decode()


@pytest.mark.parametrize("n,k,code,text", [
    (10, 1, "OB_E_DIAG", "Diagnostic error: VIF calculation requires at least two predictors."),
    (10, 0, "OB_E_DIAG", "VIF calculation requires at least two predictors."),
    (1000, 121, "OB_E_UNSUPPORTED", "at most 120"),
    (7, 7, "OB_E_INSUFFICIENT",
     "Insufficient data: Insufficient data for OLS calculation: n_obs (7) must be strictly greater than k (7)"),
    (3, 7, "OB_E_INSUFFICIENT", "n_obs (3) must be strictly greater than k (7)"),
])
def test_shape_errors_come_before_any_device_work(N, n, k, code, text):
    """With no context at all: the shape is refused before anything else is looked at."""
    lib = N.lib()
    x = np.zeros((max(n, 1), max(k, 1)), order="F")
    out = np.zeros((k + 1) * (k + 1) + 1)
    calls = [
        lambda: lib.ob_vif(None, _dp(x), max(n, 1), n, k, _dp(out)),
        lambda: lib.ob_vif_gram(None, _dp(x), max(n, 1), n, k, _dp(out)),
        lambda: lib.ob_vif_sums(None, _dp(x), max(n, 1), n, k, _dp(out), _dp(out), _dp(out), _dp(out)),
        lambda: lib.ob_vif_solve(_dp(out), n, k, _dp(out)),
    ]
    for call in calls:
        rc, msg = _rc(N, call())
        assert rc == getattr(N, code) and text in msg, (rc, msg)
    assert N.OB_VIF_MAX_K == 120


def _run(ob, N, frame, names):
    cols, ncol, nrow = ob.Frame(frame).as_c()
    arr = (C.c_char_p * max(len(names), 1))(*[s.encode() for s in names])
    out = np.zeros(max(len(names), 1))
    return _rc(N, N.lib().ob_vif_run(None, cols, ncol, nrow, C.cast(arr, C.POINTER(C.c_char_p)), len(names), _dp(out)))


def test_frame_errors_come_before_any_device_work(ob, N):
    f = {"a": [1.0, 2.0, 4.0, 8.0, 9.0], "b": [3, 1, 4, 1, 5], "s": ["p", "q", "p", "q", "p"],
         "m": np.ma.masked_array([1.0, 2.0, 3.0, 4.0, 5.0], mask=[0, 0, 1, 0, 0])}
    rc, msg = _run(ob, N, f, ["a"])
    assert rc == N.OB_E_DIAG and KAT["too_few_predictors"]["error"] in msg
    rc, msg = _run(ob, N, f, ["a", "b", "a"])
    assert rc == N.OB_E_INVALID and "duplicate" in msg and "`a`" in msg
    rc, msg = _run(ob, N, f, ["a", "nope"])
    assert rc == N.OB_E_COLUMN and "Column not found: nope" in msg
    rc, msg = _run(ob, N, f, ["a", "s"])
    assert rc == N.OB_E_POLARS and "`s`" in msg
    rc, msg = _run(ob, N, f, ["a", "m"])  # deliberate: the reference reads the null as 0.0 or as missing
    assert rc == N.OB_E_INVALID and "null value" in msg and "`m`" in msg
    rc, msg = _run(ob, N, {"a": [1.0, 2.0], "b": [2, 1]}, ["a", "b"])
    assert rc == N.OB_E_INSUFFICIENT and "n_obs (2) must be strictly greater than k (2)" in msg
    rc, msg = _run(ob, N, f, ["a", "b"])  # a good call gets as far as asking for the context
    assert rc == N.OB_E_INVALID and "null pointer" in msg


@pytest.mark.parametrize("n,k,seed", V.SHAPES, ids=[f"n{n}-k{k}" for n, k, _ in V.SHAPES])
def test_gpu_inputs_satisfy_the_bars(n, k, seed):
    ref = V.reference(n, k, seed)
    x = ref["x"]
    s, g, b, m, a, t = ref["f64"]
    sl, gl = ref["ld"][:2]
    assert ref["cond"] <= 4e4 and 1.0 < sl.min() and sl.max() <= 17.0
    assert ref["vif_bar"].max() <= ref["vif_bar_bound"] <= 1e-9
    fg = float(np.max(np.abs(g - gl) / ref["gram_bar"]))
    a2, t2, rb, tb = V.sums_reference(x, b, m)  # the sums at the SAME f64 coefficients, as the device gets them
    fs = float(max(np.max(np.abs(a - a2) / rb), np.max(np.abs(t - t2) / tb)))
    fv = float(np.max(np.abs(s - sl) / sl / ref["vif_bar"]))
    print(f"n {n} K {k}: cond {ref['cond']:.3g}, vif {sl.min():.3g}..{sl.max():.3g}, vif bar {ref['vif_bar'].max():.3g} "
          f"(bound {ref['vif_bar_bound']:.3g}); f64 vs longdouble: gram {fg:.3g}, sums {fs:.3g}, vif {fv:.3g} of the bar")
    assert fg <= (0.5 if n == 5 else 0.125) and fs <= 0.125 and fv <= 0.125


def test_threshold_case_is_decided_away_from_rounding():
    """The 1e-9 rule of the GPU test's near-collinear pair: 1 - r2 is two orders below the threshold."""
    x = V.threshold_case()
    rest = V.one_minus_r2(x, V.LD)
    assert np.all(rest <= 1e-11) and np.all(rest > 0)
    assert np.isinf(V.vif(x)).all()
