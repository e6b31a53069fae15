#!/usr/bin/env python
"""Times the distribution-regression bootstrap at 1,000,000 rows, 500k a group, with K = 4 and
K = 21 design columns, T = 19 and T = 50 thresholds and 2,000 replicates: per-kernel HIP-event ms (threshold logit
passes, distribution pass, rows), replicates/s by the host clock, and the numpy restatement (tests/dr_ref.py) of
one replicate on the same panel and counts, one thread. Writes profiles/dr_time.json.

    python tools/dr_time.py [--rows 1000000] [--reps 2000] [--repeats 3] [--out profiles/dr_time.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

TAUS = (0.1, 0.25, 0.5, 0.75, 0.9)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--widths", default="4,21")
    ap.add_argument("--thresholds", default="19,50")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dr_time.json"))
    a = ap.parse_args()
    ob = importlib.import_module("oaxaca-blinder-rs_amd")
    import dr_ref as D
    import oracle as O
    import reweight_ref as R
    from reweight_time import panel

    O.build()
    out = {"metric": "distribution-regression bootstrap: per-kernel ms and replicates/s", "rows": a.rows,
           "replicates": a.reps, "warmup": 1, "repeats": a.repeats, "cases": [],
           "rate_note": "host clock around boot(): resample counts, logit passes and steps, the distribution pass, "
                        "rows and the copy of the rows"}
    for k in (int(v) for v in a.widths.split(",")):
        f, xs = panel(a.rows, k)
        b = ob.OaxacaBuilder(f, "y", "g", "B").predictors(xs).bootstrap_reps(a.reps).seed(0x0B5EED)
        xa, ya, xb, yb, _ = b.get_data_matrices()
        for T in (int(v) for v in a.thresholds.split(",")):
            pr = b.prepare_distribution(TAUS, n_thresholds=T)
            try:
                info = pr.dr_info()
                pr.boot(0, a.reps)  # warm-up
                rate, logit, cdf, rows_ms, passes, launches, ok_n = [], [], [], [], 0, 0, 0
                for rep in range(a.repeats):
                    t0 = time.perf_counter()
                    rows, ok = pr.boot(0, a.reps)
                    dt = time.perf_counter() - t0
                    t = ob.dr_last_timing()
                    rate.append(a.reps / dt)
                    logit.append(t["pass_ms"] / max(t["launches"], 1))
                    cdf.append(t["cdf_ms"])
                    rows_ms.append(t["row_ms"])
                    passes, launches, ok_n = t["passes"], t["launches"], int(ok.sum())
            finally:
                pr.close()
            ca, cb = R.counts(O, 0x0B5EED, 0, 0, len(ya)), R.counts(O, 0x0B5EED, 0, 1, len(yb))
            t0 = time.perf_counter()
            want, winfo = D.decompose(xa, ya, xb, yb, info["thresholds"], np.array(TAUS), None, None, ca, cb)
            cpu_s = time.perf_counter() - t0
            scale = abs(want[len(TAUS) // 2])
            err = float(np.max(np.abs(rows[0] - want) / np.maximum(np.abs(want), scale)))
            out["cases"].append({
                "k": k, "thresholds": len(info["thresholds"]), "logit_pass_ms": spread(logit), "passes": passes,
                "launches": launches, "cdf_ms": spread(cdf), "rows_kernel_ms": spread(rows_ms),
                "replicates_per_s": spread(rate), "ok_replicates_last_boot": ok_n,
                "cpu_restatement_s_per_replicate": cpu_s, "cpu_restatement_replicates_per_s": 1.0 / cpu_s,
                "speedup_vs_cpu_restatement": statistics.median(rate) * cpu_s,
                "replicate_0_max_rel_err_vs_restatement": err,
                "restatement_passes": int(winfo["passes"].max())})
            print(json.dumps(out["cases"][-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")


if __name__ == "__main__":
    main()
