"""Times the cluster bootstrap at 1,000,000 x 20 WLS with 10,000 replicates at C = 1,000,
50,000 and 500,000 clusters of Zipf sizes, and writes profiles/cluster_time.json: the four phase times of
ob_cluster_last_timing (gram = the one pass that forms Q, counts, apply, solve) and replicates/s, beside the
row-level bootstrap of the same panel, seed and replicate count on the same machine. There is no target.

    python tools/cluster_time.py [--rows 1000000] [--p 20] [--reps 10000] [--clusters 1000,50000,500000] [--repeats 3]
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def zipf_clusters(n, c, rng, s=1.3):
    """n rows over c clusters, every cluster at least one row, the rest by Zipf(s) shares (tools/akm_time.py)."""
    share = 1.0 / np.arange(1, c + 1) ** s
    sizes = 1 + rng.multinomial(n - c, share / share.sum())
    return rng.permutation(np.repeat(np.arange(c, dtype=np.int64), sizes))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--p", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10_000)
    ap.add_argument("--clusters", default="1000,50000,500000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_time.json"))
    a = ap.parse_args()
    import oracle as O

    ob = importlib.import_module("oaxaca-blinder-rs_amd")
    d = O.synthetic_panel(a.rows, a.p, True, seed=20260424)
    na, nb = len(d["ya"]), len(d["yb"])
    rng = np.random.default_rng(7)
    xs = [f"x{j}" for j in range(a.p)]
    frame = {"y": np.concatenate([d["ya"], d["yb"]]), "g": np.array(["A"] * na + ["B"] * nb),
             "w": np.concatenate([d["wa"], d["wb"]])}
    x = np.vstack([d["xa"], d["xb"]])
    for j, nm in enumerate(xs):
        frame[nm] = np.ascontiguousarray(x[:, j])

    def builder():
        return (ob.OaxacaBuilder(frame, "y", "g", "B").predictors(xs).weights("w").bootstrap_reps(a.reps)
                .reference_coefficients(0).seed(0x0B5EED))

    res = {"rows": na + nb, "p": a.p, "weighted": True, "replicates": a.reps, "repeats": a.repeats, "zipf_s": 1.3,
           "cases": []}
    pr = builder().prepare()  # the yardstick: the row-level bootstrap of the same panel
    try:
        pr.boot(0, a.reps)
        wall = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            pr.boot(0, a.reps)
            wall.append(time.perf_counter() - t0)
        t = pr.timing()
        kern = t["level1_ms"] + t["counts_ms"] + t["gram_ms"] + t["reduce_ms"] + t["solve_ms"]
        res["row_bootstrap"] = {"call_s_median": statistics.median(wall), "kernel_ms": kern,
                                "replicates_per_s": a.reps / statistics.median(wall)}
        print("rows", res["row_bootstrap"], flush=True)
    finally:
        pr.close()
    for c in [int(v) for v in a.clusters.split(",")]:
        frame["firm"] = zipf_clusters(na + nb, c, rng)
        pr = builder().cluster("firm").prepare()
        try:
            pr.boot(0, a.reps)
            first = ob.cluster_last_timing()  # this call formed Q
            wall, phases = [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                pr.boot(0, a.reps)
                wall.append(time.perf_counter() - t0)
                phases.append(ob.cluster_last_timing())
            med = {k: statistics.median(ph[k] for ph in phases) for k in ("counts_ms", "apply_ms", "solve_ms")}
            case = {"clusters": c, "largest_cluster_rows": pr.cluster_info["max_cluster_rows"],
                    "gram_ms": first["gram_ms"], **med, "call_s_median": statistics.median(wall),
                    "replicates_per_s": a.reps / statistics.median(wall)}
            res["cases"].append(case)
            print(case, flush=True)
        finally:
            pr.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
