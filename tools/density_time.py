"""Times the bootstrapped DFL density decomposition on an MI355X: 1,000,000 rows (500,000 a
group), K = 4 and K = 21 design columns, 100 grid points, 2,000 replicates, weighted and unweighted. Records the logit,
density and finish times separately, the numpy restatement on one thread (a few replicates, scaled) and the time the
density pass's MFMA work would take at the f64 matrix peak. Writes profiles/density_time.json. No speed target: the
yardsticks are that bound and the restatement.

    python tools/density_time.py [--rows 1000000] [--reps 2000] [--ref-reps 2] [--out profiles/density_time.json]
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

F64_MATRIX_FLOPS = 78.6e12  # the MI355X's f64 MFMA peak (DESIGN.md §5.0's yardstick for ob_gram_kernel)
GRID = 100


def frame(n, k, seed):
    """Two groups of n / 2 rows with shifted covariates, as tests/reweight_ref.panel draws them."""
    rng = np.random.default_rng(seed)
    p = k - 1
    g = np.where(np.arange(n) % 2 == 0, "A", "B")
    x = rng.normal(size=(n, p)) + (g == "A")[:, None] * 0.6 / np.sqrt(p)
    beta = 0.5 / np.sqrt(p) * (-1.0) ** np.arange(p)
    y = 2.0 + 0.4 * (g == "A") + x @ beta + 0.5 * rng.normal(size=n)
    f = {"y": y, "g": g.tolist(), "w": rng.uniform(0.5, 2.0, n)}
    for j in range(p):
        f[f"x{j + 1}"] = np.ascontiguousarray(x[:, j])
    return f, [f"x{j + 1}" for j in range(p)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--ref-reps", type=int, default=2, help="replicates the numpy restatement is timed on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density_time.json"))
    args = ap.parse_args()
    ob = importlib.import_module("oaxaca-blinder-rs_amd")
    import density_ref as D

    out = {"rows": args.rows, "replicates": args.reps, "grid": GRID, "f64_matrix_flops_per_s": F64_MATRIX_FLOPS,
           "cases": []}
    for k in (4, 21):
        f, xs = frame(args.rows, k, 3)
        for weighted in (False, True):
            b = ob.OaxacaBuilder(f, "y", "g", "B").predictors(xs).bootstrap_reps(args.reps).seed(7)
            if weighted:
                b = b.weights("w")
            t0 = time.perf_counter()
            pr = b.prepare_density(grid_size=GRID)
            prepare_s = time.perf_counter() - t0
            with pr:
                pr.boot(0, 64)  # warm-up
                t0 = time.perf_counter()
                rows, ok = pr.boot(0, args.reps)
                boot_s = time.perf_counter() - t0
                t = ob.density_last_timing()
                info = pr.density_info()
            # the pass's multiply-adds: one weight row over A's rows, two over B's, at every grid point; the kernel
            # issues them on grid tiles of 16 columns (112 for 100 points)
            macs = float(args.reps) * (info["n_a"] + 2 * info["n_b"]) * GRID
            macs_issued = macs / GRID * ((GRID + 15) // 16 * 16)
            # the restatement on one thread: ref-reps replicates, scaled
            xa, ya, xb, yb, _ = b.get_data_matrices()
            ga = np.array(f["g"]) == "A"
            wa, wb = (f["w"][ga], f["w"][~ga]) if weighted else (None, None)
            rng = np.random.default_rng(1)
            t0 = time.perf_counter()
            for _ in range(args.ref_reps):
                ca = np.bincount(rng.integers(0, len(ya), len(ya)), minlength=len(ya))
                cb = np.bincount(rng.integers(0, len(yb), len(yb)), minlength=len(yb))
                D.decompose(xa, ya, xb, yb, info["grid"], info["bandwidth_a"], info["bandwidth_b"], wa, wb, ca, cb)
            ref_s = (time.perf_counter() - t0) / args.ref_reps * args.reps
            case = {"k": k, "weighted": weighted, "n_failed": int(len(ok) - ok.sum()), "prepare_s": prepare_s,
                    "boot_s": boot_s, "logit_ms": t["logit_ms"], "logit_passes": t["logit_passes"],
                    "logit_launches": t["logit_launches"], "density_ms": t["density_ms"], "finish_ms": t["finish_ms"],
                    "density_multiply_adds": macs, "mfma_bound_ms": 2.0 * macs / F64_MATRIX_FLOPS * 1e3,
                    "mfma_bound_issued_ms": 2.0 * macs_issued / F64_MATRIX_FLOPS * 1e3,
                    "numpy_one_thread_s": ref_s, "numpy_replicates_timed": args.ref_reps}
            case["density_over_bound"] = case["density_ms"] / case["mfma_bound_ms"]
            print(json.dumps(case), flush=True)
            out["cases"].append(case)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
