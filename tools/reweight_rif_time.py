#!/usr/bin/env python
"""Times the weighted RIF pass and the reweighted decomposition of statistics:
  * ob_rif_stat_weighted at 500,000 rows beside ob_rif_stat on the same values, per statistic: host-clock ms of the
    call and the pass's HIP-event ms (sort, scans, quantile pieces and densities, scatter);
  * a three-statistic reweighted run (gini, quantile 0.5, iqr 0.9/0.1) at 1,000,000 rows, K = 4 and 2,000 replicates
    beside the three single runs: host-clock seconds, and whether the tables agree bitwise.
Writes profiles/reweight_rif_time.json.

    python tools/reweight_rif_time.py [--rif-rows 500000] [--rows 1000000] [--reps 2000] [--repeats 3] [--out ...]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from reweight_time import panel, spread  # noqa: E402

STATS = [("gini", {}), ("quantile", {"tau": 0.5}), ("iqr", {"upper": 0.9, "lower": 0.1})]


def timed(fn, repeats):
    fn()  # warm-up
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rif-rows", type=int, default=500_000)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reweight_rif_time.json"))
    a = ap.parse_args()
    ob = importlib.import_module("oaxaca-blinder-rs_amd")
    rng = np.random.default_rng(20261020)
    y = rng.lognormal(3.0, 0.5, a.rif_rows)
    w = rng.lognormal(0.0, 2.0, a.rif_rows)
    out = {"metric": "weighted RIF pass and reweighted decomposition of statistics", "warmup": 1, "repeats": a.repeats,
           "rif_rows": a.rif_rows, "rif": [], "note": "call_ms: host clock around the call, copies included; the "
           "kernel ms are the pass's HIP events (ob_rif_last_timing)"}
    for stat, kw in [("variance", {})] + STATS:
        rec = {"stat": stat, **kw}
        rec["weighted_call_ms"] = spread(timed(lambda: ob.rif_statistic_weighted(y, w, stat, **kw), a.repeats))
        rec["weighted_kernel_ms"] = ob.rif_last_timing()
        if stat != "quantile":
            rec["unweighted_call_ms"] = spread(timed(lambda: ob.rif_statistic(y, stat, **kw), a.repeats))
            rec["unweighted_kernel_ms"] = ob.rif_last_timing()
        out["rif"].append(rec)
        print(json.dumps(rec))
    f, xs = panel(a.rows, 4)
    f["y"] = np.exp(f["y"] - 2.0)  # positive, for the Gini
    b = ob.OaxacaBuilder(f, "y", "g", "B").predictors(xs).bootstrap_reps(a.reps).seed(0x0B5EED)
    b.decompose_reweighted_statistics(STATS[:1])  # warm-up
    t_many, t_single = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        many = b.decompose_reweighted_statistics(STATS)
        t_many.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        single = [b.decompose_reweighted(s, **kw) for s, kw in STATS]
        t_single.append(time.perf_counter() - t0)
    same = all([c.__dict__ for c in m.aggregate] == [c.__dict__ for c in s.aggregate] for m, s in zip(many, single))
    out["reweighted"] = {
        "rows": a.rows, "k": 4, "replicates": a.reps, "statistics": [{"stat": s, **kw} for s, kw in STATS],
        "three_in_one_run_s": {k: v for k, v in spread(t_many).items()},
        "three_single_runs_s": {k: v for k, v in spread(t_single).items()},
        "speedup": statistics.median(t_single) / statistics.median(t_many), "tables_bitwise_equal": bool(same),
        "last_boot_kernel_ms": ob.reweight_last_timing(),
        "statistics_abc": [list(m.statistics) for m in many], "total_gaps": [m.total_gap for m in many]}
    print(json.dumps(out["reweighted"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")


if __name__ == "__main__":
    main()
