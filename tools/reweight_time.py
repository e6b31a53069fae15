#!/usr/bin/env python
"""Times the reweighted Oaxaca-Blinder bootstrap at the row count of BASELINE.json configs[1] --
1,000,000 rows, 500k a group -- with K = 4 and K = 21 design columns and 2,000 replicates: per-kernel HIP-event ms
(logit passes, Grams, rows), replicates/s by the host clock, and the numpy restatement (tests/reweight_ref.py) of
one replicate on the same panel and counts, one thread. Writes profiles/reweight_time.json.

    python tools/reweight_time.py [--rows 1000000] [--reps 2000] [--repeats 3] [--out profiles/reweight_time.json]
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


def panel(n, k, seed=20260424):
    rng = np.random.default_rng(seed + k)
    g = np.where(np.arange(n) % 2 == 0, "A", "B")
    x = rng.normal(size=(n, k - 1)) + 0.5 / np.sqrt(k - 1) * (g == "A")[:, None]
    beta = 0.5 / np.sqrt(k - 1) * (-1.0) ** np.arange(k - 1)
    y = 2.0 + 0.3 * (g == "A") + x @ beta + 0.15 * (g == "B") * x[:, 0] ** 2 + 0.5 * rng.normal(size=n)
    f = {"y": y, "g": g.tolist()}
    for j in range(k - 1):
        f[f"x{j}"] = np.ascontiguousarray(x[:, j])
    return f, [f"x{j}" for j in range(k - 1)]


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reweight_time.json"))
    a = ap.parse_args()
    ob = importlib.import_module("oaxaca-blinder-rs_amd")
    import oracle as O
    import reweight_ref as R

    O.build()
    out = {"metric": "reweighted Oaxaca-Blinder bootstrap: per-kernel ms and replicates/s", "rows": a.rows,
           "replicates": a.reps, "warmup": 1, "repeats": a.repeats, "widths": [],
           "rate_note": "host clock around boot(): resample counts, logit passes and steps, the three Grams, rows "
                        "and the copy of the rows"}
    for k in (4, 21):
        f, xs = panel(a.rows, k)
        b = ob.OaxacaBuilder(f, "y", "g", "B").predictors(xs).bootstrap_reps(a.reps).seed(0x0B5EED)
        pr = b.prepare_reweighted()
        try:
            pr.boot(0, a.reps)  # warm-up
            rate, logit, gram, rows_ms, passes, launches, ok_n = [], [], [], [], 0, 0, 0
            for rep in range(a.repeats):
                t0 = time.perf_counter()
                rows, ok = pr.boot(0, a.reps)
                dt = time.perf_counter() - t0
                t = ob.reweight_last_timing()
                rate.append(a.reps / dt)
                logit.append(t["logit_ms"] / max(t["logit_launches"], 1))
                gram.append(t["gram_ms"])
                rows_ms.append(t["row_ms"])
                passes, launches, ok_n = t["logit_passes"], t["logit_launches"], int(ok.sum())
            point = pr.point_row()
        finally:
            pr.close()
        xa, ya, xb, yb, _ = b.get_data_matrices()
        ca, cb = R.counts(O, 0x0B5EED, 0, 0, len(ya)), R.counts(O, 0x0B5EED, 0, 1, len(yb))
        t0 = time.perf_counter()
        want, norms = R.decompose(xa, ya, xb, yb, None, None, ca, cb)
        cpu_s = time.perf_counter() - t0
        err = float(np.max(np.abs(rows[0] - want) / np.maximum(np.abs(want), abs(want[0]))))
        out["widths"].append({
            "k": k, "logit_pass_ms": spread(logit), "logit_passes": passes, "logit_launches": launches,
            "grams_ms": spread(gram), "rows_kernel_ms": spread(rows_ms), "replicates_per_s": spread(rate),
            "ok_replicates_last_boot": ok_n, "total_gap": float(point[0]),
            "specification_error": float(point[4]), "reweighting_error": float(point[6]),
            "cpu_restatement_s_per_replicate": cpu_s, "cpu_restatement_replicates_per_s": 1.0 / cpu_s,
            "speedup_vs_cpu_restatement": statistics.median(rate) * cpu_s,
            "replicate_0_max_rel_err_vs_restatement": err, "restatement_passes": len(norms)})
        print(json.dumps(out["widths"][-1]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")


if __name__ == "__main__":
    main()
