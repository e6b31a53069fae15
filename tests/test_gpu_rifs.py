"""The per-replicate RIFs of the variance, the Gini and quantile ranges on the GPU (csrc/ob_rifs.hip)
against the numpy restatement tests/rifs_ref.py: nu and the Gram y-pairs to the bound of §5.19, a range's nu bitwise,
ties, a tie run across a chunk and a sub-tile boundary, a constant outcome, exact zeros, a Gini resample of mean 0,
the point pass and bitwise determinism.

Shapes: n = 2, 130, 256, 257, 513 -- one ragged tile, one full tile, a tile and one row (two chunks), three tiles
(three chunks; the count tile is 256 rows, the sub-tile 64) -- with K = 3, 1, 9, 3 and 32, so both instantiations of
the row passes (K <= 8 and K <= 32) run over one and several chunks. Counts come from the oracle's OBRS-3 stream and
from rifq_ref.hand_counts (long zero runs and one count of 200).

Bound: E is the f64 restatement's largest mixed error against an np.longdouble run over these inputs
(rifs_ref.restatement_error, at most 3.2e-15 on x86-64), so 8 E is below the 1e-12 floor and the floor is the bound.
The mixed error is rifs_ref.mixed_err's. A range's q and N_le are those of ob_rifq.hip's kernels, which this pass
calls: rifs_pass does not return them, so the test asserts nu = q_hi - q_lo bitwise against the restatement and q and
N_le bitwise through rifq_pass on the same counts."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rifq_ref as R  # noqa: E402
import rifs_ref as F  # noqa: E402

pytestmark = pytest.mark.gpu

_state = {}
KEYS = ("nu", "gy", "floored", "ok")


def bounds(O):
    if "bounds" not in _state:
        _state["bounds"] = {k: {q: F.bound(v) for q, v in e.items()} for k, e in F.restatement_error(O).items()}
    return _state["bounds"]


def all_cases(O):
    if "cases" not in _state:
        cs = F.cases(O)
        for _, y, x, c, _ in cs:
            for a in (y, x, c):
                if a is not None:
                    a.setflags(write=False)
        _state["cases"] = cs
    return _state["cases"]


def compare(got, r, stats, rep, bd, label):
    """One replicate of a rifs_pass result against its restatement r -> the worst error per statistic and quantity."""
    worst = {}
    for s, (name, p) in enumerate(stats):
        assert bool(got["ok"][rep, s]) and r["ok"][s], (label, name)
        assert bool(got["floored"][rep, s]) == r["floored"][s], (label, name)
        s_nu, s_gy = r["scale"][s]
        e_nu, e_gy = F.mixed_err(got["nu"][rep, s], r["nu"][s], s_nu), F.mixed_err(got["gy"][rep, s], r["gy"][s], s_gy)
        print(label, name, p, f"nu {e_nu:.2e} gy {e_gy:.2e}")
        assert e_nu <= bd[name]["nu"], (label, name, "nu", e_nu)
        assert e_gy <= bd[name]["gy"], (label, name, "gy", e_gy)
        if name == "iqr":
            assert got["nu"][rep, s] == r["nu"][s], (label, name)  # q_hi - q_lo of bitwise q
        worst[(name, "nu")] = max(worst.get((name, "nu"), 0.0), e_nu)
        worst[(name, "gy")] = max(worst.get((name, "gy"), 0.0), e_gy)
    return worst


@pytest.mark.parametrize("idx", range(len(F.SIZES) + 4))
def test_pass_matches_restatement(ob, O, idx):
    name, y, x, cs, stats = all_cases(O)[idx]
    bd = bounds(O)
    got = ob.rifs_pass(y, stats, counts=cs, x=x)
    k = 1 if x is None else x.shape[1] + 1
    assert got["nu"].shape == (len(cs), len(stats)) and got["gy"].shape == (len(cs), len(stats), k + 1)
    taus = F.range_taus(stats)
    gq = ob.rifq_pass(y, taus, counts=cs, x=x)
    for rep, c in enumerate(cs):
        r = F.restate(y, c, stats, x)
        F.check_ranges(r)
        compare(got, r, stats, rep, bd, (name, rep))
        assert gq["q"][rep].tolist() == r["rq"]["q"] and gq["n_le"][rep].tolist() == [float(v) for v in r["rq"]["n_le"]]
    if name == "const130":  # d = 0 on every row: the variance and its pairs are exactly 0, and so is every range
        assert np.all(got["nu"][:, 0] == 0.0) and np.all(got["gy"][:, 0] == 0.0)
        assert np.all(got["nu"][:, 2:] == 0.0)
        assert np.all(np.abs(got["nu"][:, 1] + 1.0) <= 1e-12)  # one tie run: R = mu, G = 1 - 2
    if name == "ties257":
        assert len(F.tie_runs(y)) > 10
    if name == "straddle513":  # the hand counts sit on both sides of the chunk and the sub-tile boundary
        runs = F.tie_runs(y)
        assert (250, 262) in runs and (60, 70) in runs
        c = cs[-1]
        assert c[250:256].sum() > 0 and c[256:262].sum() > 0 and c[60:64].sum() > 0 and c[64:70].sum() > 0
    if name == "zeros257":
        assert (y == 0.0).sum() == 20 and F.tie_runs(y)[0] == (0, 20)


def test_gini_resample_of_mean_zero_is_flagged(ob, O):
    """Every draw on a zero row: mu = 0, the Gini is flagged not ok (nu NaN, pairs 0); the other statistics stand."""
    y, x = R.panel(130, 2)
    y = y.copy()
    y[:5] = 0.0
    c = np.zeros((2, 130), dtype=np.int64)
    c[0, 2] = 130
    c[1] = R.stream_counts(O, 130, 1)[0]
    stats = (("variance", {}), ("gini", {}))
    got = ob.rifs_pass(y, stats, counts=c, x=x)
    assert got["ok"].tolist() == [[True, False], [True, True]]
    assert np.isnan(got["nu"][0, 1]) and np.all(got["gy"][0, 1] == 0.0)
    r = F.restate(y, c[1], stats, x)
    compare(got, r, stats, 1, bounds(O), ("mu0", 1))
    r0 = F.restate(y, c[0], stats[:1], x)
    assert F.mixed_err(got["gy"][0, 0], r0["gy"][0], r0["scale"][0][1]) <= F.FLOOR


def test_point_pass_is_the_unit_count_pass(ob, O):
    bd = bounds(O)
    for n, p in ((2, 2), (257, 2), (513, 8)):
        y, x = R.panel(n, p)
        point = ob.rifs_pass(y, F.STATS, x=x)
        unit = ob.rifs_pass(y, F.STATS, counts=np.ones((1, n), dtype=int), x=x)
        for key in KEYS:
            assert point[key].tobytes() == unit[key].tobytes(), (n, key)
        r = F.restate(y, np.ones(n, dtype=int), F.STATS, x)
        compare(point, r, F.STATS, 0, bd, ("point", n))


def test_bitwise_determinism(ob, O):
    """A replicate's values do not depend on its batch, its slot or the other statistics of the pass."""
    n = 513
    y, x = F.straddle()
    cs = R.stream_counts(O, n, 67)
    full = ob.rifs_pass(y, F.STATS, counts=cs, x=x)
    again = ob.rifs_pass(y, F.STATS, counts=cs, x=x)
    for key in KEYS:
        assert full[key].tobytes() == again[key].tobytes(), key
    for lo, hi in ((0, 1), (40, 56), (16, 67), (66, 67)):  # boots of 1, 16 and 51; a replicate moved to slot 0
        part = ob.rifs_pass(y, F.STATS, counts=cs[lo:hi], x=x)
        for key in KEYS:
            assert part[key].tobytes() == full[key][lo:hi].tobytes(), (lo, hi, key)
    for s, stat in enumerate(F.STATS):  # a statistic alone is element s of the five-statistic pass
        one = ob.rifs_pass(y, [stat], counts=cs, x=x)
        for key in KEYS:
            assert one[key][:, 0].tobytes() == np.ascontiguousarray(full[key][:, s]).tobytes(), (stat, key)
    tm = ob.rifs_last_timing()  # of the last pass: one range
    assert tm["rifq_ms"] > 0.0 and tm["finish_ms"] > 0.0 and tm["moment_ms"] == 0.0 and tm["gini_ms"] == 0.0
    ob.rifs_pass(y, ["gini"], counts=cs[:3], x=x)
    tm = ob.rifs_last_timing()
    assert min(tm[k] for k in ("moment_ms", "scan_ms", "gini_ms", "tie_ms", "finish_ms")) > 0.0 and tm["rifq_ms"] == 0.0
