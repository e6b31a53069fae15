"""The segment loop of the boot driver the eight model front ends share (csrc/ob_model.hip): a boot of
one segment and three replicates against its two halves and against a short boot, byte for byte, for seven of them
(the density decomposition's boundary test lives in test_gpu_density.py); and the refusals that the builder answers
for a handle of each kind through one dispatch.

FIT_SEG and REFIT_SEG are the front ends' segment lengths, the `seg_reps` of its boot plan in csrc/ob_model.hpp: kRefitSegReps = 2048 for
the two refits, kFitSegReps = 4096 for binary, reweight, dr, tobit and nopo. On these frames (groups of 130 and 257 rows, three
tiles) the count-image budget allows far more, so seg_reps is the segment. Frames and K = 3 are those of the front
ends' own determinism tests; the refits run three outputs, so that the [T][n_total] stride of the row blocks is
crossed at s0 > 0; reweight, dr, tobit and nopo also run with hk_batch = 1 (batches of 64), so that a batch ends inside
the second segment's three replicates. The second segment is where a Tobit boot writes rows at s0 + b0 and reads
counts drawn at first_rep + s0; nopo draws its own counts (its plan's `draws` is false), so there the segment callback
itself calls engine_counts(first_rep + s0)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nopo_ref as NR  # noqa: E402
import rifq_ref as RQ  # noqa: E402
import test_gpu_binary as TB  # noqa: E402
import test_gpu_dr as TD  # noqa: E402
import test_gpu_reweight as TW  # noqa: E402
import test_gpu_rifq_decompose as TQ  # noqa: E402
import test_gpu_rifs_decompose as TS  # noqa: E402
import test_gpu_tobit as TT  # noqa: E402

pytestmark = pytest.mark.gpu


def _tobit(ob):
    b, lower, upper = TT.builder(ob, 3, True, TT.R.GROUP_A)
    return b.prepare_tobit(lower, upper)


FIT_SEG, REFIT_SEG = 4096, 2048  # kFitSegReps, kRefitSegReps (csrc/ob_model.hpp)

HANDLES = {
    "binary": (FIT_SEG, lambda ob: TB.builder(ob, 3, TB.R.WEIGHTED).prepare_binary()),
    "reweight": (FIT_SEG, lambda ob: TW.builder(ob, 3, True).prepare_reweighted()),
    "dr": (FIT_SEG, lambda ob: TD.builder(ob, 3, True).prepare_distribution(TD.TAUS, n_thresholds=5, lo=0.1, hi=0.9)),
    "rifq": (REFIT_SEG, lambda ob: TQ.builder(ob, 3, "Weighted").prepare_quantiles_refit(RQ.TAUS)),
    "rifs": (REFIT_SEG, lambda ob: TS.builder(ob, 3, "Pooled").prepare_statistics_refit(TS.THREE)),
    "tobit": (FIT_SEG, _tobit),
    "nopo": (FIT_SEG, lambda ob: NR.panel("main", True).builder(ob).prepare_nopo()),
}
CASES = [(name, 0) for name in HANDLES] + [("reweight", 1), ("dr", 1), ("tobit", 1), ("nopo", 1)]


@pytest.mark.parametrize("name,hk_batch", CASES)
def test_a_boot_across_a_segment_boundary(ob, N, name, hk_batch):
    seg, prepare = HANDLES[name]
    pr = prepare(ob)
    try:
        def boots():
            return pr.boot(0, seg + 3), pr.boot(0, seg), pr.boot(seg, 3), pr.boot(0, 67)

        if hk_batch:
            with N.option("hk_batch", hk_batch):
                (full, ok), (r0, k0), (r1, k1), (rs, ks) = boots()
        else:
            (full, ok), (r0, k0), (r1, k1), (rs, ks) = boots()
    finally:
        pr.close()
    axis = full.ndim - 2  # rows: [reps][row_len], the refits' [outputs][reps][row_len]
    assert full.shape[axis] == seg + 3 and ok.shape[-1] == seg + 3
    if name in ("rifq", "rifs"):
        assert full.shape[0] == 3
    assert full.tobytes() == np.concatenate([r0, r1], axis=axis).tobytes()
    assert ok.tobytes() == np.concatenate([k0, k1], axis=-1).tobytes()
    assert np.ascontiguousarray(full[..., :67, :]).tobytes() == rs.tobytes()
    assert np.ascontiguousarray(ok[..., :67]).tobytes() == ks.tobytes()
    assert ok.any()


# The texts of the parent commit's ladders (ob_builder.cpp's ob_prepared_boot_sharded, ob_jackknife.cpp's
# prepared_jack_check), copied from its source.
SHARDED = {
    "binary": "binary decomposition: sharded runs are outside its scope",
    "reweight": "reweighted decomposition: sharded runs are outside its scope",
    "dr": "distribution regression: sharded runs are outside its scope",
    "rifq": "quantile refit: sharded runs are outside its scope",
    "rifs": "statistics refit: sharded runs are outside its scope",
    "tobit": "tobit decomposition: sharded runs are outside its scope",
    "nopo": "matching decomposition: sharded runs are outside its scope",
}
JACKKNIFE = {
    "binary": "jackknife: binary decompositions (BCa included) are outside its scope",
    "reweight": "jackknife: reweighted decompositions (BCa included) are outside its scope",
    "dr": "jackknife: distribution-regression decompositions (BCa included) are outside its scope",
    "rifq": "jackknife: refitted quantile decompositions (BCa included) are outside its scope",
    "rifs": "jackknife: refitted statistic decompositions (BCa included) are outside its scope",
    "tobit": "jackknife: tobit decompositions (BCa included) are outside its scope",
    "nopo": "jackknife: matching decompositions (BCa included) are outside its scope",
}


@pytest.mark.parametrize("name", list(HANDLES))
def test_refusals_keep_their_code_and_text(ob, N, name):
    pr = HANDLES[name][1](ob)
    try:
        with pytest.raises(N.OaxacaError) as e:
            pr.boot_sharded(0, 4)
        assert e.value.code == N.OB_E_UNSUPPORTED and str(e.value) == SHARDED[name]
        with pytest.raises(N.OaxacaError) as e:
            pr.jackknife()
        assert e.value.code == N.OB_E_UNSUPPORTED and str(e.value) == JACKKNIFE[name]
    finally:
        pr.close()
