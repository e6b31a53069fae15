"""Times the matching decomposition on an MI355X: 1,000,000 rows (500,000 a group), 2,000
replicates, at about 1,200 and about 50,000 cells, weighted and unweighted, beside the numpy restatement on one thread
and beside the time the cell pass's count-image bytes take at the achievable HBM rate. Writes
profiles/nopo_time.json. No speed target: the yardsticks are that bound and the restatement.

    python tools/nopo_time.py [--rows 1000000] [--reps 2000] [--ref-reps 8]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("OMP_NUM_THREADS", "1")

HBM_BYTES_PER_S = 6.3e12  # achievable on the MI355X (a float4 copy: 79 % of the 8 TB/s peak)
IMAGE_BYTES = 64 * 17 * 4  # one 64-row sub-tile of 64 replicates


def frame(n, levels, seed):
    """Two numeric matching columns of `levels` values each (about levels^2 cells), B shifted against A so that some
    cells hold one group only."""
    rng = np.random.default_rng(seed)
    g = np.where(np.arange(n) % 2 == 0, "A", "B")
    shift = (g == "B") * 0.15 * levels
    a = np.clip(np.rint(rng.normal(levels / 2 + shift, levels / 5)), 0, levels - 1)
    b = np.clip(np.rint(rng.normal(levels / 2 - shift, levels / 5)), 0, levels - 1)
    y = 10.0 + 0.03 * a + 0.02 * b + (g == "A") * 0.4 + rng.normal(size=n)
    return {"y": y, "g": g.tolist(), "a": a, "b": b, "w": rng.uniform(0.5, 2.0, n)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--ref-reps", type=int, default=8, help="replicates the numpy restatement is timed on")
    args = ap.parse_args()
    ob = importlib.import_module("oaxaca-blinder-rs_amd")
    import nopo_ref as R

    out = {"rows": args.rows, "replicates": args.reps, "hbm_bytes_per_s": HBM_BYTES_PER_S, "cases": []}
    for levels in (35, 224):
        f = frame(args.rows, levels, 3)
        for weighted in (False, True):
            b = ob.OaxacaBuilder(f, "y", "g", "B").predictors(["a", "b"]).bootstrap_reps(args.reps).seed(7)
            if weighted:
                b = b.weights("w")
            t0 = time.perf_counter()
            pr = b.prepare_nopo()
            prepare_s = time.perf_counter() - t0
            with pr:
                pr.boot(0, 64)  # warm-up
                t0 = time.perf_counter()
                rows, ok = pr.boot(0, args.reps)
                boot_s = time.perf_counter() - t0
                t = ob.nopo_last_timing()
                info = pr.nopo_info()
            n_a, n_b = int(info["n_cell_a"].sum()), int(info["n_cell_b"].sum())
            subtiles = sum((n + 63) // 64 for n in (n_a, n_b))
            image_bytes = subtiles * ((args.reps + 63) // 64) * IMAGE_BYTES
            # the restatement on one thread: the per-cell sums and the terms of ref-reps replicates, scaled
            cell, w = info["row_cell"], (f["w"] if weighted else np.ones(args.rows))
            ga = np.array(f["g"]) == "A"
            rng = np.random.default_rng(1)
            t0 = time.perf_counter()
            for _ in range(args.ref_reps):
                sums = []
                for m in (ga, ~ga):
                    n = int(m.sum())
                    c = np.bincount(rng.integers(0, n, n), minlength=n)
                    sums += R.sums(f["y"][m], w[m], cell[m], info["n_cells"], c)
                R.terms(*sums)
            ref_s = (time.perf_counter() - t0) / args.ref_reps * args.reps
            case = {"cells": int(info["n_cells"]), "support_cells": int(info["n_support_cells"]), "weighted": weighted,
                    "n_failed": int(len(ok) - ok.sum()), "prepare_s": prepare_s, "boot_s": boot_s,
                    "cell_ms": t["cell_ms"], "row_ms": t["row_ms"], "counts_ms": t["counts_ms"],
                    "count_image_bytes": image_bytes, "hbm_bound_ms": image_bytes / HBM_BYTES_PER_S * 1e3,
                    "numpy_one_thread_s": ref_s, "numpy_replicates_timed": args.ref_reps}
            print(json.dumps(case), flush=True)
            out["cases"].append(case)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "nopo_time.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
