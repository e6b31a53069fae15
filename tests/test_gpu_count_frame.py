"""Level-2 counts across every branch of `ob_count_kernel`'s per-tile frame, on the MI355X.

A count block walks a run of 8 tiles of the two groups' joint tile list. While the draws of one tile
run, one of its waves publishes the next tile's level-1 counts, call prefix and call map into the
other half of double-buffered LDS tables; a full tile's part calls (m % 16 draws) go by whole Philox
words and at most three single bytes. None of that may move a count: the per-row counts
(`ob_debug_counts`) must equal the bincount of the oracle's resample indices bit for bit, for runs
that end early, exactly and in a second block, runs that straddle the group boundary, every
sub-tile count of a partial last tile, and partial replicate batches (lanes with m = 0 in the scan
and the map). Each case runs under both `gram_path` settings; `ob_debug_counts` itself reads the f64
image (r * 17 words), the i8 image is checked through the Gram and boot tests.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 0x0B5EED
T = 256
# (first replicate id, replicates): 1, 63, 64, 65 and 130 replicates, ids at zero, small and past 2^31
REPS = ((0, 1), (5, 63), (2**31 + 17, 64), (9, 65), (3, 130))

CASES = {
    "one_full_tile": (T, T),
    "run_of_7": (3 * T, 4 * T),            # the block's run ends early
    "run_of_8": (4 * T, 4 * T),            # exactly one run
    "run_of_9": (T, 8 * T),                # a second block of one tile
    "run_of_17": (9 * T, 8 * T),           # two runs and a tile; the second run straddles the groups
    "straddle_partial": (700, 1500),       # group 0's last tile partial, group 1 starts mid-run
    "tail_1_63": (T + 1, T + 63),          # last tiles of 1 and 63 rows (one sub-tile)
    "tail_64_65": (T + 64, T + 65),        # 64 rows (one sub-tile, exactly) and 65 (two)
}
# Seeds of the part-call and map edge case, found with the oracle (group 0, tile 0 of 3 full tiles).
EDGE_SEED = 0x0B5EED
EDGE_FIRST = 0


def _panel(ob, na, nb):
    rng = np.random.default_rng(na + nb)
    xa = rng.normal(size=(na, 1))
    xb = rng.normal(size=(nb, 1)) + 0.1
    return ob.Panel(xa, 1.0 + 0.5 * xa[:, 0] + rng.normal(size=na), xb, 0.8 + 0.4 * xb[:, 0] + rng.normal(size=nb),
                    None, None)


_ORACLE = {}


def _want(O, seed, rep, g, n):
    """The oracle's level-1 and per-row counts, computed once and shared by both image paths."""
    key = (seed, rep, g, n)
    if key not in _ORACLE:
        rows = np.bincount(O.resample_indices(seed, rep, g, n), minlength=n)
        assert rows.max() < 128
        l1 = O.level1_counts(seed, rep, g, n)
        rows = rows.astype(np.uint8)
        rows.setflags(write=False)
        _ORACLE[key] = (l1, rows)
    return _ORACLE[key]


def _check(ob, O, na, nb, reps, path, seed=SEED):
    panel = _panel(ob, na, nb)
    try:
        with ob._native.option("gram_path", path):
            for g, n in ((0, na), (1, nb)):
                for first, count in reps:
                    l1, rc = panel.debug_counts(seed, first, count, g)
                    for r in range(count):
                        wl1, wrows = _want(O, seed, first + r, g, n)
                        assert np.array_equal(l1[r], wl1), f"level 1, group {g}, rep {first + r}"
                        assert np.array_equal(rc[r], wrows), f"rows, group {g}, rep {first + r}"
    finally:
        panel.close()


@pytest.mark.parametrize("path", (2, 1), ids=("i8", "f64"))
@pytest.mark.parametrize("case", sorted(CASES))
def test_count_frame_bitwise(ob, O, case, path):
    na, nb = CASES[case]
    _check(ob, O, na, nb, REPS, path)


@pytest.mark.parametrize("path", (2, 1), ids=("i8", "f64"))
def test_count_frame_part_call_and_map_edges(ob, O, path):
    """One full tile whose 64 replicates have part calls of no draws (m % 16 = 0), of bytes only
    (1..3), of exactly one word (4) and of three words and three bytes (15), and whose whole-call
    counts spread over at least four indices past the dense prefix (cmax - cmin >= 4), so the call
    map holds ragged windows. The properties are asserted from the oracle's level-1 counts."""
    n = 3 * T
    m = np.array([O.level1_counts(EDGE_SEED, EDGE_FIRST + r, 0, n)[0] for r in range(64)], dtype=np.int64)
    nd = m % 16
    assert (nd == 0).any() and ((nd >= 1) & (nd <= 3)).any() and (nd == 4).any() and (nd == 15).any()
    c = m // 16
    assert c.max() - c.min() >= 4
    _check(ob, O, n, T, ((EDGE_FIRST, 64),), path, seed=EDGE_SEED)
