"""Times the jackknife sums pass (ob_jackknife) at 1,000,000 x 20 WLS for the four reference
modes and writes profiles/jackknife_time.json. There is no target: the HIP-event time of the pass (kernel and
ordered reduce) is reported beside the panel's bytes over the HBM bandwidth and beside the numpy closed form on
the same panel. Warm-up runs first, then `--repeats` timed calls; median and minimum are kept.

    python tools/jackknife_time.py [--rows 1000000] [--p 20] [--repeats 10] [--warmup 3]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 8.0e12  # MI355X peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--p", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jackknife_time.json"))
    a = ap.parse_args()
    import oracle as O
    import jackknife_ref as J

    ob = importlib.import_module("oaxaca-blinder-rs_amd")
    d = O.synthetic_panel(a.rows, a.p, True, seed=20260424)
    panel = ob.Panel(d["xa"], d["ya"], d["xb"], d["yb"], d["wa"], d["wb"], device=0)
    panel_bytes = 8 * a.rows * (a.p + 2)  # x, y, w read once (the epilogue's second read of x hits the cache)
    res = {"rows": a.rows, "p": a.p, "weighted": True, "panel_bytes": panel_bytes,
           "hbm_floor_ms": 1e3 * panel_bytes / HBM_BYTES_PER_S, "repeats": a.repeats, "warmup": a.warmup, "modes": {}}
    try:
        for name, ref in J.REFS.items():
            for _ in range(a.warmup):
                panel.jackknife(ref)
            ms, wall = [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                r = panel.jackknife(ref)
                wall.append(1e3 * (time.perf_counter() - t0))
                ms.append(ob.jackknife_last_timing())
            t0 = time.perf_counter()
            J.closed_form(ref, d["xa"], d["ya"], d["wa"], d["xb"], d["yb"], d["wb"])
            np_ms = 1e3 * (time.perf_counter() - t0)
            res["modes"][name] = {"pass_ms_median": statistics.median(ms), "pass_ms_min": min(ms),
                                  "call_ms_median": statistics.median(wall), "numpy_closed_form_ms": np_ms,
                                  "n_dropped": list(r.n_dropped)}
            print(name, res["modes"][name], flush=True)
    finally:
        panel.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
