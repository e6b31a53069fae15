#!/usr/bin/env python
"""Times OaxacaBuilder.optimize and a 50-step efficient_frontier on a synthetic 1,000,000 x 20 wage frame.

    python tools/remedy_time.py [--rows N --k K --warmup W --repeats R] [--out PATH]

Per pass: the HIP-event time (ob_remedy_info, ob_remedy_frontier's ms), the bytes the pass must read from HBM
(its inputs once) and the rate the two give; the whole calls by the host clock (frame conversion, design
build, point estimate and upload included). Writes profiles/remedy_time.json."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remedy_time.json"))
    args = ap.parse_args()
    ob = importlib.import_module("oaxaca-blinder-rs_amd")
    rng = np.random.default_rng(20260424)
    n, k = args.rows, args.k
    x = rng.normal(size=(n, k))
    ref = rng.random(n) < 0.5
    wage = 30.0 + x @ rng.uniform(0.5, 2.0, k) + rng.normal(size=n) - 2.0 * (~ref)
    frame = {"wage": wage, "g": np.where(ref, "a", "b")}
    names = [f"x{j}" for j in range(k)]
    frame.update({nm: x[:, j] for j, nm in enumerate(names)})
    b = ob.OaxacaBuilder(ob.Frame(frame), "wage", "g", "a").predictors(names)
    runs = []
    for it in range(args.warmup + args.repeats):
        t0 = time.perf_counter()
        res = b.optimize()
        t1 = time.perf_counter()
        pts = b.efficient_frontier(steps=50)
        t2 = time.perf_counter()
        if it >= args.warmup:
            info = dict(b.last_remedy_info)
            runs.append({"optimize_s": t1 - t0, "frontier_s": t2 - t1, **{a: info[a] for a in info if a.endswith("_ms")},
                         **b.last_frontier_ms})
    med = {a: float(np.median([r[a] for r in runs])) for a in runs[0]}
    info = b.last_remedy_info
    n_a, n_b, m = int(info["n_a"]), int(info["n_b"]), int(info["n_adjustments"])
    kk = k + 1  # design columns
    bytes_read = {"gram_ms": 8 * n_a * kk, "score_ms": 8 * (n * k + n_a) + 8 * n * k,  # x twice: operand and epilogue
                  "classify_ms": 8 * 3 * n_b, "order_ms": 16 * 12 * m * 2, "allocate_ms": 8 * 12 * m + 16 * 12 * m,
                  "xty_ms": 8 * n * (k + 3), "rss_ms": 8 * n * (k + 3)}
    passes = {a: {"ms": med[a], "bytes_read": int(bytes_read[a]), "GBps": bytes_read[a] / med[a] / 1e6 if med[a] > 0 else None}
              for a in bytes_read}
    out = {"metric": "optimize and 50-step efficient_frontier on a synthetic wage frame", "rows": n, "predictors": k,
           "n_a": n_a, "n_b": n_b, "adjustments": m, "warmup": args.warmup, "repeats": args.repeats,
           "optimize_s": med["optimize_s"], "frontier_s": med["frontier_s"], "passes": passes,
           "required_budget": info["required_budget"], "t_first": pts[0].t_statistic, "t_last": pts[-1].t_statistic,
           "total_cost": res.total_cost}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
