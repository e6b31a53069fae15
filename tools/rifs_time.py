#!/usr/bin/env python
"""Times the per-replicate RIF pass of the variance, the Gini and a quantile range (ob_rifs_pass) on
one group of the shape of BASELINE.json configs[3] -- 500,000 of its 1,000,000 rows, 20 predictors, variance, Gini
and iqr(0.9, 0.1) -- over a batch of replicates whose counts are multinomial draws: HIP-event ms per kernel (medians),
the same per replicate, and replicate 0 against the numpy restatement (tests/rifs_ref.py). Writes
profiles/rifs_time.json.

It then times a bootstrap step at configs[3]'s shape -- 1,000,000 rows x 20 predictors, two groups, the three
statistics -- with the refit (prepare_statistics_refit + boot: host clock and ob_rifs_last_timing) beside the fixed-RIF
step (ob.Panel with the three RIF columns of ob_rif_stat as outcomes, the panel decompose_statistics builds, boot
through the same engine), and records the ratio.

    python tools/rifs_time.py [--rows 500000] [--reps 128] [--step-reps 2048] [--repeats 3] [--out profiles/rifs_time.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STATS = (("variance", {}), ("gini", {}), ("iqr", {"upper": 0.9, "lower": 0.1}))
KERNELS = ("moment_ms", "scan_ms", "gini_ms", "tie_ms", "finish_ms", "rifq_ms")


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def step_times(ob, rows, p, reps, repeats):
    """One bootstrap step of `reps` replicates of the three statistics over rows x p, two groups: refit beside fixed
    RIF."""
    import time

    rng = np.random.default_rng(20260424)
    g = np.where(np.arange(rows) % 2 == 0, "A", "B")
    x = rng.normal(size=(rows, p))
    y = np.exp(1.4 + 0.25 * (g == "A") + x @ (0.3 / np.sqrt(p) * np.ones(p)) + 0.5 * rng.normal(size=rows))
    f = {"y": y, "g": g.tolist()}
    for j in range(p):
        f[f"x{j}"] = np.ascontiguousarray(x[:, j])
    xs = [f"x{j}" for j in range(p)]
    b = ob.OaxacaBuilder(f, "y", "g", "B").predictors(xs).bootstrap_reps(reps).seed(0x0B5EED)
    pr = b.prepare_statistics_refit(STATS)
    try:
        pr.boot(0, reps)  # warm-up
        wall, kern = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            pr.boot(0, reps)
            wall.append(1e3 * (time.perf_counter() - t0))
            kern.append(ob.rifs_last_timing())
    finally:
        pr.close()
    a, bm = g == "A", g == "B"
    ya = np.stack([ob.rif_statistic(y[a], s, **kw)[0] for s, kw in STATS], axis=1)
    yb = np.stack([ob.rif_statistic(y[bm], s, **kw)[0] for s, kw in STATS], axis=1)
    panel = ob.Panel(x[a], ya, x[bm], yb, None, None, device=0)
    panel.boot(0x0B5EED, 0, reps, ob.ReferenceCoefficients.GroupA)  # warm-up (digit images)
    fixed = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        panel.boot(0x0B5EED, 0, reps, ob.ReferenceCoefficients.GroupA)
        fixed.append(1e3 * (time.perf_counter() - t0))
    med = {k: statistics.median([t[k] for t in kern]) for k in kern[0]}
    return {"rows": rows, "predictors": p, "statistics": [s for s, _ in STATS], "replicates": reps, "warmup": 1,
            "repeats": repeats, "refit_boot_ms_host_clock": spread(wall), "refit_kernel_ms": med,
            "fixed_rif_boot_ms_host_clock": spread(fixed),
            "ratio_refit_to_fixed": statistics.median(wall) / statistics.median(fixed),
            "note": "host clock around boot() with the copy of the rows; the fixed-RIF step runs the i8 Gram over a "
                    "three-outcome panel, the refit the f64 Gram and three solves"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=500_000)
    ap.add_argument("--predictors", type=int, default=20)
    ap.add_argument("--reps", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step-reps", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rifs_time.json"))
    a = ap.parse_args()
    ob = importlib.import_module("oaxaca-blinder-rs_amd")
    import rifq_ref as R
    import rifs_ref as F

    y, x = R.panel(a.rows, a.predictors)
    y = np.exp(y - 1.0)  # a wage: positive, still ascending
    rng = np.random.default_rng(20260424)
    counts = rng.multinomial(a.rows, np.full(a.rows, 1.0 / a.rows), size=a.reps)
    assert counts.max() < 256
    ob.rifs_pass(y, STATS, counts=counts, x=x)  # warm-up
    times = {k: [] for k in KERNELS}
    for _ in range(a.repeats):
        got = ob.rifs_pass(y, STATS, counts=counts, x=x)
        t = ob.rifs_last_timing()
        for k in KERNELS:
            times[k].append(t[k])
    r = F.restate(y, counts[0], STATS, x)
    err = {}
    for s, (name, _) in enumerate(STATS):
        err[name] = {"nu": F.mixed_err(got["nu"][0, s], r["nu"][s], r["scale"][s][0]),
                     "gy": F.mixed_err(got["gy"][0, s], r["gy"][s], r["scale"][s][1])}
    total = sum(statistics.median(v) for v in times.values())
    out = {"metric": "per-replicate RIF pass of the variance, the Gini and iqr(0.9, 0.1) over one group: per-kernel "
                     "HIP-event ms", "rows": a.rows, "predictors": a.predictors, "statistics": [s for s, _ in STATS],
           "replicates": a.reps, "warmup": 1, "repeats": a.repeats}
    out.update({k: spread(v) for k, v in times.items()})
    out["kernels_ms_per_replicate_and_group"] = total / a.reps
    out["replicate_0_vs_restatement"] = err
    out["step"] = step_times(ob, 2 * a.rows, a.predictors, a.step_reps, a.repeats)
    out["ratio_to_fixed_rif_step"] = out["step"]["ratio_refit_to_fixed"]
    print(json.dumps(out))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")


if __name__ == "__main__":
    main()
