"""Level-1 tile counts where `ob_level1_kernel` draws Knuth-Yao samples with the register-resident
walk (`ob_spec.h` `ob_ky_walk`) and the low popcount from the stream's first call, on the MI355X.

A node of at least 4,096 draws splits by one stream per B(4096) sample, one per set bit 11 .. 7 of
its count and one for the popcount of its low seven bits. The walk reads the first word of the
stream's first Philox call from a register and falls back to the bit-at-a-time stream when it
leaves the nine LDS-staged columns. None of that may move a count: the level-1 tile counts and the
per-row counts (`ob_debug_counts`) must equal the oracle's (`orc_level1_counts`, and the bincount
of `orc_resample_indices`) bit for bit at every group size below, over 8 replicates each.

T = tiles of 256 rows. Levels of at most 128 nodes share a node among several threads, deeper
levels give a thread whole nodes; more than 40,960 tiles run as subtrees of depth 15 (J > 0).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 0x0B5EED
# (first replicate id, replicates): 8 per group, ids at zero, mid-range and past 2^31
REPS = ((0, 3), (9_998, 3), (2**31 + 17, 2))

CASES = {
    # the smallest nodes that split by Knuth-Yao: one B(4096) stream alone / the same plus a low
    # popcount of one bit
    "n4096_n4097": (4096, 4097),
    # one B(4096) stream, all five digit streams and a low popcount of 127 bits, beside the last node
    # count at which every level shares its nodes among threads (T = 256 * 255 + 1 rows: 255 tiles
    # and a one-row tail)
    "n8191_T256_tail1": (8191, 256 * 255 + 1),
    # T = 257: the first size past the small path, the tile level owned by threads; T = 1,025, just
    # past a power of two: half of the last level's children are rejected and round 1 is at its
    # fullest
    "T257_T1025": (256 * 257, 256 * 1025),
    # a tree shaped like the benchmark's (T = 1,954, D = 11, partial tail), whose later rounds run
    # mostly empty nodes
    "T1954_tail": (256 * 1954 - 37, 1000),
    # unequal groups in one launch: a single Knuth-Yao node beside a tree of depth 11 (T = 1,172)
    "n4096_n300001": (4096, 300_001),
}


def _panel(ob, na, nb):
    rng = np.random.default_rng(na + nb)
    xa = rng.normal(size=(na, 1))
    xb = rng.normal(size=(nb, 1)) + 0.1
    return ob.Panel(xa, 1.0 + 0.5 * xa[:, 0] + rng.normal(size=na), xb, 0.8 + 0.4 * xb[:, 0] + rng.normal(size=nb),
                    None, None)


def _check(ob, O, na, nb, reps):
    panel = _panel(ob, na, nb)
    try:
        for g, n in ((0, na), (1, nb)):
            for first, count in reps:
                l1, rc = panel.debug_counts(SEED, first, count, g)
                for r in range(count):
                    rep = first + r
                    assert np.array_equal(l1[r], O.level1_counts(SEED, rep, g, n)), f"level 1, group {g}, rep {rep}"
                    assert int(l1[r].sum()) == n
                    want = np.bincount(O.resample_indices(SEED, rep, g, n), minlength=n)
                    assert want.max() < 256
                    assert np.array_equal(rc[r], want.astype(np.uint8)), f"rows, group {g}, rep {rep}"
    finally:
        panel.close()


@pytest.mark.parametrize("case", sorted(CASES))
def test_level1_frame_counts_bitwise(ob, O, case):
    na, nb = CASES[case]
    _check(ob, O, na, nb, REPS)


def test_level1_frame_counts_bitwise_subtrees(ob, O):
    """The smallest group that runs as subtrees (J > 0): 40,961 tiles, D = 16, two subtrees of depth
    15 under one top level, the second holding a single tile. 10.5M rows; eight replicates' tile
    counts, and the per-row counts of the first of each run of replicate ids (the oracle takes half
    a second per replicate at this size, the panel 270 MB)."""
    n = 256 * 40_960 + 77
    panel = _panel(ob, n, 5000)
    try:
        for first, count in REPS:
            l1, rc = panel.debug_counts(SEED, first, count, 0)
            for r in range(count):
                assert np.array_equal(l1[r], O.level1_counts(SEED, first + r, 0, n)), f"level 1, rep {first + r}"
                assert int(l1[r].sum()) == n
            want = np.bincount(O.resample_indices(SEED, first, 0, n), minlength=n)
            assert want.max() < 256
            assert np.array_equal(rc[0], want.astype(np.uint8)), f"rows, rep {first}"
    finally:
        panel.close()


def test_level1_frame_boot_rows_match_oracle(ob, O):
    """64 replicates of a 20,000-row x 3-predictor WLS panel through `ob_boot_run`, against the
    oracle's reference-algorithm bootstrap on the same stream at tests/test_gpu_parity.py's
    tolerance (no file under tests/golden/ has this shape): |engine - oracle| <= 1e-6 *
    max(|oracle|, |total_gap|), equal failure masks."""
    d = O.synthetic_panel(20_000, 3, True, seed=7)
    panel = ob.Panel(d["xa"], d["ya"], d["xb"], d["yb"], d["wa"], d["wb"])
    try:
        rows, ok = panel.boot(SEED, 0, 64, ob.ReferenceCoefficients.Pooled)
    finally:
        panel.close()
    cfg = O.PassConfig(4, 3, O.REF["pooled"], True)
    xa, xb = O.with_intercept(d["xa"]), O.with_intercept(d["xb"])
    rc, orow = O.single_pass(cfg, xa, d["ya"], d["wa"], xb, d["yb"], d["wb"])
    orows, ook = O.boot_ref(cfg, xa, d["ya"], d["wa"], xb, d["yb"], d["wb"], SEED, 0, 64, full=False)
    assert rc == 0 and np.array_equal(ok, ook)
    m = ok.astype(bool)
    assert m.all()
    assert np.all(np.abs(rows[m] - orows[m]) <= 1e-6 * np.maximum(np.abs(orows[m]), abs(orow[5])))
