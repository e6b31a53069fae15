"""Level-1 tile counts across every branch of `ob_level1_kernel`'s per-level chain, on the MI355X.

The kernel hands counts from level to level through two LDS buffers: levels of at most 128 nodes
share a node among several threads (each takes every 2^sh-th popcount word; atomics, then the right
child), deeper levels give a thread whole nodes. A popcount node's full words are counted without
bit masks and only its partial last word with them, by whichever thread's word sequence reaches
it. None of that may move a count: the level-1 tile counts and the per-row counts
(`ob_debug_counts`) must equal the oracle's (`orc_level1_counts`, and the bincount of
`orc_resample_indices`) bit for bit at every tree shape below.

T = tiles of 256 rows, D = ceil(log2 T) levels. Nodes below 4,096 draws split by popcount words,
larger ones by Knuth-Yao samples over the digits of their count.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 0x0B5EED
# (first replicate id, replicates): ids at zero, small, and past 2^31
REPS = ((0, 2), (5, 1), (2**31 + 17, 1))

CASES = {
    # depth 0 and 1: no level below the root to hand off to; both groups below 4,096 draws
    # (popcount words only, no Knuth-Yao sample)
    "T1_T2": (200, 512),
    # the small path (tile level and running counts in LDS): full last tile / partial tail
    "T256_full_T256_tail": (256 * 256, 256 * 256 - 100),
    # the first large path: the last split goes straight to m1, the right edge rejects
    # (2k + 1 >= T), a second round runs; T = 257 with a partial tail, T = 300 full
    "T257_T300": (257 * 256 - 13, 300 * 256),
    # ll = 8 is the first one-thread-per-node level (the seam between the two thread mappings);
    # beside it a group below 4,096 draws with a partial tail (T = 12)
    "T513_n3000": (513 * 256 - 5, 3000),
    # the two blockIdx.y of one launch at different depths (D = 9 and D = 11)
    "T300_T1025": (300 * 256 - 31, 1025 * 256 - 9),
    # past 2^20 draws: Knuth-Yao digits down to level 8, where a thread owns whole nodes of
    # 4,096 draws and more (T = 4,098, D = 13)
    "n_2p20": ((1 << 20) + 333, 777),
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
                    want = np.bincount(O.resample_indices(SEED, rep, g, n), minlength=n)
                    assert want.max() < 256
                    assert np.array_equal(rc[r], want.astype(np.uint8)), f"rows, group {g}, rep {rep}"
                    assert int(l1[r].sum()) == n
    finally:
        panel.close()


@pytest.mark.parametrize("case", sorted(CASES))
def test_level1_chain_counts_bitwise(ob, O, case):
    na, nb = CASES[case]
    _check(ob, O, na, nb, REPS)


def test_level1_chain_counts_bitwise_500k(ob, O):
    """configs[1]'s group (n = 500,000: T = 1,954, D = 11; Knuth-Yao levels 0-6, a shared-node
    popcount level 7, one-thread-per-node levels 8-10, two tree rounds and the direct draws),
    four replicates."""
    _check(ob, O, 500_000, 1000, ((0, 1), (9_999, 2), (2**31 + 17, 1)))
