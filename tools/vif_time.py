#!/usr/bin/env python
"""Times the VIF path on two synthetic designs (1,000,000 x 20 and 1,000,000 x 120; tests/vif_ref.py's
generator) and prints one JSON line. Run by hand on an MI355X:

    python tools/vif_time.py [--rows N --ks 20,120 --warmup W --repeats R --ref-fits F] [--out PATH]

Per shape: the Gram pass and the residual pass are HIP-event times from ob_vif_last_timing (each with
its ordered reduce; the residual pass includes the ss_tot kernel), the host solves are the K Cholesky
solves by the host clock, and the whole call is a host clock around vif(), which adds the upload of the
n x K predictors from pageable host memory and the small copies. Medians over the repeats, with min and
max beside them.

For scale only, the NumPy restatement's auxiliary fits on the same data: each fit forms its own Z'Z and
Z'y over the n rows, solves and takes explicit residuals, as the reference does K times. The first
--ref-fits of the K fits are timed and the figure for all K is that time scaled by K / fits; both are
recorded. There is no pass or fail threshold.
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


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def ref_fits(x, fits):
    """The reference's loop body for the first `fits` predictors, in NumPy f64."""
    import vif_ref as V

    n, k = x.shape
    out = []
    t0 = time.perf_counter()
    for j in range(fits):
        z = np.concatenate([np.delete(x, j, axis=1), np.ones((n, 1))], axis=1)
        y = x[:, j]
        beta = V._chol_solve(z.T @ z, z.T @ y, np.float64)
        r = y - z @ beta
        d = y - y.sum() / n
        out.append(1.0 / (1.0 - (1.0 - (r @ r) / (d @ d))))
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--ks", default="20,120")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ref-fits", type=int, default=4)
    ap.add_argument("--out", default=None, help="also write the JSON to this path")
    args = ap.parse_args()

    import vif_ref as V

    ob = importlib.import_module("oaxaca-blinder-rs_amd")
    shapes = []
    for k in (int(s) for s in args.ks.split(",")):
        n = args.rows
        x = np.asfortranarray(V.fixture(n, k, 1000 + k))
        gram, solve, sums, whole, scores = [], [], [], [], None
        for i in range(args.warmup + args.repeats):
            t0 = time.perf_counter()
            scores = ob.vif(x)
            t1 = time.perf_counter()
            if i >= args.warmup:
                t = ob.vif_last_timing()
                gram.append(t["gram_ms"])
                solve.append(t["solve_ms"])
                sums.append(t["sums_ms"])
                whole.append((t1 - t0) * 1e3)
        fits = min(args.ref_fits, k)
        ref_ms, ref_scores = ref_fits(x, fits)
        rel = float(np.max(np.abs(scores[:fits] - ref_scores) / np.abs(ref_scores)))
        shapes.append({
            "rows": n, "predictors": k, "x_bytes": n * k * 8,
            "gram_pass_ms": spread(gram), "host_solves_ms": spread(solve), "residual_pass_ms": spread(sums),
            "whole_call_ms": spread(whole),
            "gram_flop": 2 * n * (k + 1) * (k + 2) // 2, "residual_flop": 2 * n * (k + 1) * k,
            "numpy_restatement": {"fits_timed": fits, "fits_timed_ms": ref_ms, "all_k_fits_ms_scaled": ref_ms * k / fits,
                                  "max_rel_diff_of_timed_scores": rel},
            "vif_min": float(np.min(scores)), "vif_max": float(np.max(scores)),
        })
    out = {"metric": "ob_vif on synthetic correlated designs", "shapes": shapes, "warmup": args.warmup,
           "repeats": args.repeats,
           "whole_call_note": "host clock; the upload of the predictors from pageable memory is included",
           "numpy_note": "the reference's own K fits restated in NumPy f64 on the host CPUs, for scale only"}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
