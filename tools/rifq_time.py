#!/usr/bin/env python
"""Times the per-replicate quantile RIF pass (ob_rifq_pass) on one group of the shape of
BASELINE.json configs[3] -- 500,000 of its 1,000,000 rows, 20 predictors, tau = 0.1 / 0.5 / 0.9 -- over a batch of
replicates whose counts are multinomial draws: HIP-event ms of the search, density and patch kernels (medians), the
same per replicate, and replicate 0 against the numpy restatement (tests/rifq_ref.py). Writes profiles/rifq_time.json.

It then times a bootstrap step at configs[3]'s shape -- 1,000,000 rows x 20 predictors, two groups, tau = 0.1 / 0.5 /
0.9 -- with the refit (prepare_quantiles_refit + boot: host clock and ob_rifq_last_timing) beside the fixed-RIF step
(ob.Panel with the three host RIF columns as outcomes, the panel decompose_quantiles builds, boot through the same
engine), and records the ratio.

    python tools/rifq_time.py [--rows 500000] [--reps 128] [--step-reps 2048] [--repeats 3] [--out profiles/rifq_time.json]
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

TAUS = (0.1, 0.5, 0.9)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def step_times(ob, rows, p, reps, repeats):
    """One bootstrap step of `reps` replicates at three quantiles over rows x p, two groups: refit beside fixed RIF."""
    import time

    rng = np.random.default_rng(20260424)
    g = np.where(np.arange(rows) % 2 == 0, "A", "B")
    x = rng.normal(size=(rows, p))
    y = 2.4 + 0.25 * (g == "A") + x @ (0.3 / np.sqrt(p) * np.ones(p)) + 0.5 * rng.normal(size=rows)
    f = {"y": y, "g": g.tolist()}
    for j in range(p):
        f[f"x{j}"] = np.ascontiguousarray(x[:, j])
    xs = [f"x{j}" for j in range(p)]
    b = ob.OaxacaBuilder(f, "y", "g", "B").predictors(xs).bootstrap_reps(reps).seed(0x0B5EED)
    pr = b.prepare_quantiles_refit(TAUS)
    try:
        pr.boot(0, reps)  # warm-up
        wall, kern = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            pr.boot(0, reps)
            wall.append(1e3 * (time.perf_counter() - t0))
            kern.append(ob.rifq_last_timing())
    finally:
        pr.close()
    a, bm = g == "A", g == "B"
    ya = np.stack([ob.rif(y[a], t) for t in TAUS], axis=1)
    yb = np.stack([ob.rif(y[bm], t) for t in TAUS], axis=1)
    panel = ob.Panel(x[a], ya, x[bm], yb, None, None, device=0)
    panel.boot(0x0B5EED, 0, reps, ob.ReferenceCoefficients.GroupA)  # warm-up (digit images)
    fixed = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        panel.boot(0x0B5EED, 0, reps, ob.ReferenceCoefficients.GroupA)
        fixed.append(1e3 * (time.perf_counter() - t0))
    med = {k: statistics.median([t[k] for t in kern]) for k in kern[0]}
    return {"rows": rows, "predictors": p, "taus": list(TAUS), "replicates": reps, "warmup": 1, "repeats": repeats,
            "refit_boot_ms_host_clock": spread(wall), "refit_kernel_ms": med,
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rifq_time.json"))
    a = ap.parse_args()
    ob = importlib.import_module("oaxaca-blinder-rs_amd")
    import rifq_ref as R

    y, x = R.panel(a.rows, a.predictors)
    rng = np.random.default_rng(20260424)
    counts = rng.multinomial(a.rows, np.full(a.rows, 1.0 / a.rows), size=a.reps)
    assert counts.max() < 256
    ob.rifq_pass(y, TAUS, counts=counts, x=x)  # warm-up
    search, density, patch = [], [], []
    for _ in range(a.repeats):
        got = ob.rifq_pass(y, TAUS, counts=counts, x=x)
        t = ob.rifq_last_timing()
        search.append(t["search_ms"])
        density.append(t["density_ms"])
        patch.append(t["patch_ms"])
    r = R.restate(y, counts[0], TAUS, x)
    err = {"q_equal": [got["q"][0, i] for i in range(3)] == r["q"],
           "n_le_equal": got["n_le"][0].tolist() == [float(v) for v in r["n_le"]],
           "bw": R.mixed_err(got["bw"][0], r["bw"]), "f": R.mixed_err(got["f"][0], np.array(r["f"])),
           "t": max(R.mixed_err(got["t"][0, i], r["t"][i]) for i in range(3)),
           "gy": max(R.mixed_err(got["gy"][0, i], r["gy"][i]) for i in range(3))}
    total = statistics.median(search) + statistics.median(density) + statistics.median(patch)
    out = {"metric": "per-replicate quantile RIF pass over one group: per-kernel HIP-event ms", "rows": a.rows,
           "predictors": a.predictors, "taus": list(TAUS), "replicates": a.reps, "warmup": 1, "repeats": a.repeats,
           "search_ms": spread(search), "density_ms": spread(density), "patch_ms": spread(patch),
           "kernels_ms_per_replicate_and_group": total / a.reps,
           "replicate_0_vs_restatement": err,
           "step": step_times(ob, 2 * a.rows, a.predictors, a.step_reps, a.repeats)}
    out["ratio_to_fixed_rif_step"] = out["step"]["ratio_refit_to_fixed"]
    print(json.dumps(out))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")


if __name__ == "__main__":
    main()
