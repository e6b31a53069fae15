#!/usr/bin/env python
"""Times the matching distance pass (ob_match_run, Euclidean) at 100k x 100k x 20 and
500k x 500k x 20 treated x controls x covariates, k = 1 and 5, and writes profiles/match_time.json.
Run by hand on an MI355X:

    python tools/match_time.py [--shapes 100000x100000x20,500000x500000x20 --ks 1,5 --out PATH]

knn_ms is the HIP-event time of the distance kernel and its merge (ob_match_results_info); the whole
call is a host clock around MatchingEngine.run, which returns after the results are on the host.
Two warm-ups, then the median of seven, with min and max beside it. A pair-dimension is one
(treated, control, covariate) triple: a subtract, a multiply and an add, none of them fused, so the
rate is held against half of the f64 vector peak of DESIGN.md §5.0 (78.6 TFLOP/s counts an FMA as
two). The CPU figure is the NumPy restatement (tests/match_ref.py) on a 2,000 x 100k slice of the
same data, scaled to the full shape: it is the checker, not the reference crate.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F64_VALU_PEAK_TFLOPS = 78.6  # DESIGN.md §5.0, an FMA counted as two
OPS_PER_PAIR_DIM = 3


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100000x100000x20,500000x500000x20")
    ap.add_argument("--ks", default="1,5")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_time.json"))
    args = ap.parse_args()

    import match_ref as M

    ob = importlib.import_module("oaxaca-blinder-rs_amd")
    N = ob._native
    runs = []
    for shape in args.shapes.split(","):
        n_q, n_c, d = (int(v) for v in shape.split("x"))
        q, c = M.knn_data(n_q, n_c, d, seed=1)
        frame = {"treat": np.concatenate([np.ones(n_q), np.zeros(n_c)])}
        cov = [f"x{j}" for j in range(d)]
        frame.update({nm: np.concatenate([q[:, j], c[:, j]]) for j, nm in enumerate(cov)})
        eng = ob.MatchingEngine(frame, "treat", "y", cov)
        eng._frame.as_c()  # column buffers converted once, outside the timed calls
        sq, sc = q[:2000], c[:100000]
        t0 = time.perf_counter()
        ridx, _ = M.knn(sq, sc, 5)
        cpu_s = time.perf_counter() - t0
        cpu_scaled = cpu_s * (n_q * n_c) / (len(sq) * len(sc))
        for k in (int(v) for v in args.ks.split(",")):
            knn_ms, prep_ms, whole_ms, res = [], [], [], None
            for i in range(args.warmup + args.repeats):
                t0 = time.perf_counter()
                res = eng.run(k, N.OB_MATCH_EUCLIDEAN)
                t1 = time.perf_counter()
                if i >= args.warmup:
                    knn_ms.append(res.knn_ms)
                    prep_ms.append(res.prep_ms)
                    whole_ms.append((t1 - t0) * 1e3)
            if len(sc) == n_c:  # the slice's controls are all the controls: the neighbours must agree
                got = res.neighbor_rows[:len(sq), :min(k, 5)] - n_q
                assert np.array_equal(got, ridx[:, :min(k, 5)]), "engine and restatement disagree"
            rate = n_q * n_c * d / (statistics.median(knn_ms) * 1e-3)
            runs.append({
                "treated": n_q, "controls": n_c, "covariates": d, "k": k,
                "knn_ms": spread(knn_ms), "prep_ms": spread(prep_ms), "whole_call_ms": spread(whole_ms),
                "pair_dims_per_s": rate,
                "frac_of_f64_valu_non_fma_rate": rate * OPS_PER_PAIR_DIM / (F64_VALU_PEAK_TFLOPS / 2 * 1e12),
                "cpu_checker": {"what": "tests/match_ref.py (NumPy f64 restatement, the checker, not the crate) on a "
                                        f"{len(sq)} x {len(sc)} slice, k = 5, scaled by the pair count",
                                "slice_s": cpu_s, "scaled_to_shape_s": cpu_scaled},
            })
            print(json.dumps(runs[-1]), flush=True)
    out = {"metric": "ob_match_run (Euclidean) distance pass", "warmup": args.warmup, "repeats": args.repeats,
           "ops_per_pair_dim": OPS_PER_PAIR_DIM, "f64_valu_peak_tflops_fma_as_two": F64_VALU_PEAK_TFLOPS,
           "whole_call_note": "host clock; includes the frame copy, the gather of both groups, the uploads and the "
                              "download of the neighbour lists",
           "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
