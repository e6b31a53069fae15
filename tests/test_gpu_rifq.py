"""The per-replicate RIF of a quantile on the GPU (csrc/ob_rifq.hip) against the numpy restatement
tests/rifq_ref.py: q, the row prefix and N_le exactly, the bandwidth, density, masked sums and Gram y-pairs to the
bound of §5.18, ties, a constant outcome, more than one chunk, the point pass and bitwise determinism.

Shapes: n = 2, 130, 256, 257, 513 -- one ragged tile, one full tile, a tile and one row (two chunks), three tiles
(three chunks, and row prefixes that cut the first, the middle and the last chunk). Counts come from the oracle's
OBRS-3 stream and from a hand-made image with long zero runs and one count of 200.

Bound: E is the f64 restatement's largest mixed error against an np.longdouble run over these inputs (rifq_ref.
restatement_error, at most 7.4e-16 on x86-64), so 8 E is below the 1e-12 floor and the floor is the bound. The mixed
error of a quantity is max |got - ref| over a replicate's values relative to the largest |ref| among them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rifq_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

_state = {}


def bounds(O):
    if "bounds" not in _state:
        _state["bounds"] = {k: R.bound(v) for k, v in R.restatement_error(O).items()}
    return _state["bounds"]


def all_cases(O):
    if "cases" not in _state:
        cs = R.cases(O)
        for _, y, x, c, _ in cs:
            for a in (y, x, c):
                a.setflags(write=False)
        _state["cases"] = cs
    return _state["cases"]


def compare(got, r, y, x, rep, bd, label):
    """One replicate of a rifq_pass result against its restatement r."""
    T = len(r["q"])
    assert [got["q"][rep, t] for t in range(T)] == r["q"], label  # bitwise
    assert [int(got["n_le"][rep, t]) for t in range(T)] == r["n_le"], label
    assert got["n_le"][rep].tolist() == [float(v) for v in r["n_le"]], label
    assert got["floored"][rep].tolist() == r["floored"], label
    errs = {"bw": R.mixed_err(got["bw"][rep], r["bw"]), "f": R.mixed_err(got["f"][rep], np.array(r["f"]))}
    errs["t"] = max(R.mixed_err(got["t"][rep, t], r["t"][t]) for t in range(T))
    errs["gy"] = max(R.mixed_err(got["gy"][rep, t], r["gy"][t]) for t in range(T))
    for t in range(T):  # T_0 = N_le is an exact integer
        assert got["t"][rep, t, 0] == r["n_le"][t], label
    for key, e in errs.items():
        assert e <= bd[key], (label, key, e)
    return errs


@pytest.mark.parametrize("idx", range(len(R.SIZES) + 2))
def test_pass_matches_restatement(ob, O, idx):
    name, y, x, cs, taus = all_cases(O)[idx]
    bd = bounds(O)
    got = ob.rifq_pass(y, taus, counts=cs, x=x)
    worst = {k: 0.0 for k in bd}
    for rep, c in enumerate(cs):
        r = R.restate(y, c, taus, x)
        R.check_steps(r)
        for k, e in compare(got, r, y, x, rep, bd, (name, rep)).items():
            worst[k] = max(worst[k], e)
    print(name, {k: f"{v:.2e}" for k, v in worst.items()})
    if name == "const130":  # spread fallback 1.0 and a constant RIF
        assert np.all(got["bw"] == 0.9 * 1.0 * 130.0 ** -0.2)
        assert np.all(got["n_le"] == 130.0) and np.all(got["q"] == 3.25)
    if name == "ties257":  # every quantile sits inside a tie run: the prefix ends past the run
        for rep in range(len(cs)):
            for t in range(len(taus)):
                qv = got["q"][rep, t]
                assert got["n_le"][rep, t] == float(cs[rep][y <= qv].sum()) and (y == qv).sum() > 1


def test_point_pass_is_the_unit_count_pass(ob, O):
    bd = bounds(O)
    for n in (2, 257, 513):
        y, x = R.panel(n, 2)
        point = ob.rifq_pass(y, R.TAUS, x=x)
        unit = ob.rifq_pass(y, R.TAUS, counts=np.ones((1, n), dtype=int), x=x)
        for key in ("q", "bw", "f", "n_le", "t", "gy"):
            assert point[key].tobytes() == unit[key].tobytes(), (n, key)
        r = R.restate(y, np.ones(n, dtype=int), R.TAUS, x)
        compare(point, r, y, x, 0, bd, ("point", n))
        for t, tau in enumerate(R.TAUS):  # and so the oracle's rif of the sample itself
            want = O.rif(y, tau)
            A = point["q"][0, t] + tau / point["f"][0, t]
            got = np.where(y <= point["q"][0, t], A - 1.0 / point["f"][0, t], A)
            assert np.all(np.abs(got - want) <= 1e-12 * np.maximum(np.abs(want), 1.0))


@pytest.mark.parametrize("p", [0, 8, 31])
def test_design_widths(ob, O, p):
    """No predictors, K = 9 and the K = 32 limit, three chunks."""
    bd = bounds(O)
    n = 513
    y, x = R.panel(n, p)
    cs = R.stream_counts(O, n, 3, first=7)
    got = ob.rifq_pass(y, R.TAUS, counts=cs, x=x if p else None)
    assert got["t"].shape == (3, 3, p + 1) and got["gy"].shape == (3, 3, p + 2)
    for rep, c in enumerate(cs):
        r = R.restate(y, c, R.TAUS, x if p else None)
        R.check_steps(r)
        print(p, compare(got, r, y, x, rep, bd, (p, rep)))


def test_bitwise_determinism(ob, O):
    """A replicate's values do not depend on its batch, its slot or the other quantiles of the pass."""
    n = 513
    y, x = R.panel(n, 2)
    cs = R.stream_counts(O, n, 67)
    keys = ("q", "bw", "f", "n_le", "t", "gy")
    full = ob.rifq_pass(y, R.TAUS, counts=cs, x=x)
    again = ob.rifq_pass(y, R.TAUS, counts=cs, x=x)
    for key in keys:
        assert full[key].tobytes() == again[key].tobytes(), key
    for lo, hi in ((0, 1), (40, 56), (16, 67), (66, 67)):  # boots of 1, 16 and 51; a replicate moved to slot 0
        part = ob.rifq_pass(y, R.TAUS, counts=cs[lo:hi], x=x)
        for key in keys:
            assert part[key].tobytes() == full[key][lo:hi].tobytes(), (lo, hi, key)
    for t, tau in enumerate(R.TAUS):  # tau_t alone is element t of the three-tau pass
        one = ob.rifq_pass(y, [tau], counts=cs, x=x)
        for key in ("q", "f", "n_le", "t", "gy"):
            assert one[key][:, 0].tobytes() == np.ascontiguousarray(full[key][:, t]).tobytes(), (tau, key)
        assert one["bw"].tobytes() == full["bw"].tobytes()


def test_eight_quantiles_and_timing(ob, O):
    bd = bounds(O)
    n = 257
    y, x = R.panel(n, 2)
    taus = tuple(np.linspace(0.1, 0.9, 8))
    cs = R.stream_counts(O, n, 2, first=3)
    got = ob.rifq_pass(y, taus, counts=cs, x=x)
    for rep, c in enumerate(cs):
        r = R.restate(y, c, taus, x)
        R.check_steps(r)
        compare(got, r, y, x, rep, bd, ("eight", rep))
        assert all(a <= b for a, b in zip(r["p"], r["p"][1:]))
    tm = ob.rifq_last_timing()
    assert tm["search_ms"] > 0.0 and tm["density_ms"] > 0.0 and tm["patch_ms"] > 0.0
