"""The weighted RIF pass on the GPU: ob_rif_stat_weighted against the numpy reference of
tests/wrif_ref.py within 8 E per statistic (floor 1e-12; E is what `python tests/wrif_ref.py` measures against
longdouble), at w = 1 against ob_rif_stat and the host's ob_rif, and the properties of the pass: weights scaled by a
power of two, a repeated call and (on distinct y) a permutation of the rows give the same bytes. All tests need an
MI355X.

Sizes n = 2, 3, 64, 257, block + 1 and 70,001; lognormal weights with sigma = 2 and exact zeros (wrif_ref.inputs);
ties, a tie run across the scan-block boundary with unequal weights inside it, constant y, exact zeros in y.

Every quantile input is asserted to lie clear of a step of Y(t) on the CPU reference first (wrif_ref.step_margins:
each t at least 1e-9 n from every run-end S, or on it exactly under unit weights; q at least 1e-9 |q| from every y_i
that it does not equal by construction). The last run-end S at t = n is not counted: it is n up to rounding, and
Y(n) is the last value on either side of it. A q that is one of the y_i exactly (f = 0, or both order statistics one
value, the usual case under heavy weights) is computed as Y + f * 0 and is that value on both sides.

Largest mixed errors seen on the MI355X beside the 1e-12 bound: variance 1.48e-15, gini 4.67e-14 (n = 70,001, the
reference's own cumsum error), quantile 9.9e-16, iqr 3.5e-16; at w = 1 against ob_rif_stat 0 (variance, gini, iqr)
and against the host's ob_rif 8.7e-15 (quantile)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rif_stat_ref as U  # noqa: E402
import wrif_ref as W  # noqa: E402

pytestmark = pytest.mark.gpu

ALL_TAUS = sorted({t for s, kw in W.STATS for t in W.stat_taus(s, kw)})


@pytest.fixture(scope="module")
def data(ob):
    """The inputs for the library's scan block and their f64 references, computed once (read-only)."""
    block = ob.rif_scan_block()
    ins = W.inputs(block)
    refs = {}
    for name, (y, w) in ins.items():
        y.setflags(write=False)
        w.setflags(write=False)
        for i, (s, kw) in enumerate(W.stats_for(name)):
            refs[(name, i)] = W.rif_statistic(y, w, s, **kw)
    return block, ins, refs


def _check(ob, data, name):
    _, ins, refs = data
    y, w = ins[name]
    m_t, m_q = W.step_margins(y, w, ALL_TAUS)
    assert m_t >= 1e-9 and m_q >= 1e-9, (name, m_t, m_q)
    worst = {}
    for i, (stat, kw) in enumerate(W.stats_for(name)):
        rif, value = ob.rif_statistic_weighted(y, w, stat, **kw)
        ref_rif, ref_value = refs[(name, i)]
        e = W.mixed_error(rif, value, ref_rif, ref_value)
        worst[stat] = max(worst.get(stat, 0.0), e)
        print(f"{name} n={len(y)} {stat} {kw}: mixed error {e:.3e} (bound {W.TOL[stat]:.1e})")
        assert np.all(np.isfinite(rif)) and e <= W.TOL[stat], (name, stat, kw, e)
    return worst


@pytest.mark.parametrize("name", ["n2", "n3", "n64"])
def test_one_wave_no_carry(ob, data, name):
    _check(ob, data, name)


def test_first_block_boundary(ob, data):
    _check(ob, data, "n257")
    _check(ob, data, f"n{data[0] + 1}")


def test_several_blocks_with_carries(ob, data):
    _check(ob, data, "n70001")


def test_ties_with_random_weights(ob, data):
    """Tied rows share S and GL of their run's end, whatever their own weights: one RIF value per y value."""
    for name in ("ties", "straddle"):
        _check(ob, data, name)
        y, w = data[1][name]
        for stat, kw in W.STATS:
            rif, _ = ob.rif_statistic_weighted(y, w, stat, **kw)
            for v in np.unique(y)[:12]:
                assert len(np.unique(rif[y == v])) == 1, (name, stat, v)
    y, w = data[1]["straddle"]
    top = y == np.max(y)
    assert np.sum(top) == 5 and len(np.unique(w[top])) == 5  # unequal weights inside the run over the boundary


def test_constant_outcome(ob, data):
    _check(ob, data, "constant")
    _check(ob, data, "constant_ln")
    y, w = data[1]["constant"]
    rif, value = ob.rif_statistic_weighted(y, w, "variance")
    assert np.array_equal(rif, np.zeros(len(y))) and value == 0.0


def test_exact_zeros_among_positive_values(ob, data):
    _check(ob, data, "zeros")


@pytest.mark.parametrize("name", ["n3", "n257", "ties", "n1025"])
def test_unit_weights_match_the_unweighted_pass(ob, data, name):
    """w = 1 against ob_rif_stat (variance, Gini, iqr) and the host's ob_rif (quantile), within the same tolerance."""
    y = U.inputs(data[0])[name if name != "n1025" else f"n{data[0] + 1}"]
    one = np.ones(len(y))
    for stat, kw in W.STATS:
        rif, value = ob.rif_statistic_weighted(y, one, stat, **kw)
        if stat == "quantile":
            ref = ob.rif(y, kw["tau"])
            ref_value = U.quantile_rif(y, kw["tau"])[1]
        else:
            ref, ref_value = ob.rif_statistic(y, stat, **kw)
        e = W.mixed_error(rif, value, ref.astype(np.longdouble), ref_value)
        print(f"{name} w=1 {stat} {kw}: against the unweighted pass {e:.3e}")
        assert e <= W.TOL[stat], (name, stat, kw, e)
        if stat == "iqr":
            host = ob.rif(y, kw["upper"]) - ob.rif(y, kw["lower"])
            eh = float(np.max(np.abs(rif - host) / np.maximum(np.abs(host), abs(ref_value))))
            assert eh <= W.TOL[stat], (name, kw, eh)


def test_scaled_weights_give_the_same_bytes(ob, data):
    for name in ("n257", "straddle", "n70001"):
        y, w = data[1][name]
        for stat, kw in W.STATS:
            a, va = ob.rif_statistic_weighted(y, w, stat, **kw)
            b, vb = ob.rif_statistic_weighted(y, w * 128.0, stat, **kw)
            assert a.tobytes() == b.tobytes() and va == vb, (name, stat)


def test_determinism(ob, data):
    for name in ("n257", "n70001"):
        y, w = data[1][name]
        for stat, kw in W.STATS:
            a, va = ob.rif_statistic_weighted(y, w, stat, **kw)
            b, vb = ob.rif_statistic_weighted(y, w, stat, **kw)
            assert a.tobytes() == b.tobytes() and va == vb
    t = ob.rif_last_timing()
    assert t["sort_ms"] > 0 and t["scan_ms"] > 0 and t["scatter_ms"] > 0 and t["kde_ms"] > 0


def test_row_order(ob, data):
    """Distinct y: a permutation of the rows gives the same statistic bytes and, undone, the same RIF bytes (every
    sum, W included, runs over the sorted rows). With ties the rows of a run keep their input order, so unequal
    weights inside it are added in another order: within tolerance."""
    block = data[0]
    rng = np.random.default_rng(3)
    y, w = data[1][f"n{block + 1}"]
    perm = rng.permutation(len(y))
    for stat, kw in W.STATS:
        a, va = ob.rif_statistic_weighted(y, w, stat, **kw)
        b, vb = ob.rif_statistic_weighted(y[perm], w[perm], stat, **kw)
        c, vc = ob.rif_statistic_weighted(y[::-1].copy(), w[::-1].copy(), stat, **kw)
        assert va == vb == vc, stat
        assert np.array_equal(a[perm], b) and np.array_equal(a[::-1], c), stat
    y, w = data[1]["ties"]
    perm = rng.permutation(len(y))
    for i, (stat, kw) in enumerate(W.STATS):
        b, vb = ob.rif_statistic_weighted(y[perm], w[perm], stat, **kw)
        ref_rif, ref_value = data[2][("ties", i)]
        assert W.mixed_error(b, vb, ref_rif[perm], ref_value) <= W.TOL[stat], stat
