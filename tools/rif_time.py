"""Times the RIF statistics pass (ob_rif_stat) at 500,000 rows per group for the three
statistics and writes profiles/rif_time.json. There is no target: the HIP-event times of the sort, the scans and
sums, the quantile pieces and densities, and the scatter are reported beside the whole call on the host clock and
beside the host's quantile RIF (ob_rif at two quantiles: a std::sort and an exp loop each) on the same data.
Warm-up runs first, then `--repeats` timed calls; median and minimum are kept.

    python tools/rif_time.py [--rows 500000] [--repeats 10] [--warmup 3]
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

STATS = [("variance", {}), ("gini", {}), ("iqr", {"upper": 0.9, "lower": 0.1})]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=500_000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rif_time.json"))
    a = ap.parse_args()
    ob = importlib.import_module("oaxaca-blinder-rs_amd")
    rng = np.random.default_rng(20261020)
    groups = [rng.lognormal(3.0, 0.5, a.rows), rng.lognormal(3.1, 0.6, a.rows)]
    res = {"rows_per_group": a.rows, "groups": 2, "repeats": a.repeats, "warmup": a.warmup,
           "scan_block": ob.rif_scan_block(), "statistics": {}}
    for stat, kw in STATS:
        for _ in range(a.warmup):
            ob.rif_statistic(groups[0], stat, **kw)
        parts = {k: [] for k in ("sort_ms", "scan_ms", "kde_ms", "scatter_ms", "device_ms", "call_ms")}
        for _ in range(a.repeats):
            t = dict.fromkeys(parts, 0.0)
            t0 = time.perf_counter()
            for y in groups:
                ob.rif_statistic(y, stat, **kw)
                for k, v in ob.rif_last_timing().items():
                    t[k] += v
            t["call_ms"] = 1e3 * (time.perf_counter() - t0)
            t["device_ms"] = t["sort_ms"] + t["scan_ms"] + t["kde_ms"] + t["scatter_ms"]
            for k in parts:
                parts[k].append(t[k])
        res["statistics"][stat] = {**{k + "_median": statistics.median(v) for k, v in parts.items()},
                                   **{k + "_min": min(v) for k, v in parts.items()}, "params": kw}
        print(stat, res["statistics"][stat], flush=True)
    host = []
    for _ in range(max(a.repeats // 2, 1)):  # the yardstick: the host RIF of both groups at two quantiles
        t0 = time.perf_counter()
        for y in groups:
            ob.rif(y, 0.9)
            ob.rif(y, 0.1)
        host.append(1e3 * (time.perf_counter() - t0))
    res["host_ob_rif_two_quantiles_ms_median"] = statistics.median(host)
    res["host_ob_rif_two_quantiles_ms_min"] = min(host)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
