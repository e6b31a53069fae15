#!/usr/bin/env python
"""Times the Tobit decomposition's bootstrap at the row count of BASELINE.json configs[1] --
1,000,000 rows, 500k a group -- on a censored-normal outcome (lower = 0 cutting about a quarter, an upper limit
cutting about a tenth), K = 4 and K = 21 design columns, weighted and unweighted, 2,000 replicates: the per-pass and
means-pass HIP-event ms, the passes a replicate takes, replicates/s by the host clock, the numpy restatement
(tests/tobit_ref.py) of one replicate on one thread, decompose_binary's rate at the same shape (read from
profiles/binary_time.json, which tools/binary_time.py writes) and the time the pass's multiply-adds take at the
78.6 TFLOP/s f64 matrix peak. Writes profiles/tobit_time.json.

    python tools/tobit_time.py [--rows 1000000] [--reps 2000] [--repeats 3] [--out profiles/tobit_time.json]
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

PEAK_FLOPS = 78.6e12  # f64 matrix peak of an MI355X
SEED = 0x0B5EED


def panel(n, k, weighted, seed=20261021):
    rng = np.random.default_rng(seed + k)
    g = np.where(np.arange(n) % 2 == 0, "A", "B")
    x = rng.normal(size=(n, k - 1))
    beta = 0.5 / np.sqrt(k - 1) * (-1.0) ** np.arange(k - 1)
    ystar = 0.25 * (g == "A") + x @ beta + rng.normal(size=n)
    ystar -= np.quantile(ystar, 0.25)
    upper = float(np.round(np.quantile(ystar, 0.90), 2))
    f = {"y": np.clip(ystar, 0.0, upper), "g": g.tolist()}
    for j in range(k - 1):
        f[f"x{j}"] = np.ascontiguousarray(x[:, j])
    if weighted:
        f["w"] = rng.uniform(0.5, 2.0, n)
    return f, [f"x{j}" for j in range(k - 1)], 0.0, upper


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tobit_time.json"))
    a = ap.parse_args()
    ob = importlib.import_module("oaxaca-blinder-rs_amd")
    import oracle as O
    import tobit_ref as R

    O.build()
    binary = {}
    try:
        with open(os.path.join(ROOT, "profiles", "binary_time.json")) as fh:
            binary = {w["k"]: w["replicates_per_s"]["median"] for w in json.load(fh)["widths"]}
    except (OSError, KeyError, ValueError):
        pass
    out = {"metric": "Tobit decomposition bootstrap: per-kernel ms, passes and replicates/s", "rows": a.rows,
           "replicates": a.reps, "warmup": 1, "repeats": a.repeats, "reference_coefficients": "GroupA", "widths": [],
           "rate_note": "host clock around boot(): resample counts, Newton passes and steps, means pass, rows and the "
                        "copy of the rows"}
    for k in (4, 21):
        for weighted in (False, True):
            f, xs, lower, upper = panel(a.rows, k, weighted)
            b = ob.OaxacaBuilder(f, "y", "g", "B").predictors(xs).bootstrap_reps(a.reps).seed(SEED)
            if weighted:
                b = b.weights("w")
            pr = b.prepare_tobit(lower, upper)
            try:
                info = pr.tobit_info()
                pr.boot(0, a.reps)  # warm-up
                rate, per_pass, means, rows_ms = [], [], [], []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    rows, ok = pr.boot(0, a.reps)
                    dt = time.perf_counter() - t0
                    t = ob.tobit_last_timing()
                    rate.append(a.reps / dt)
                    per_pass.append(t["pass_ms"] / max(t["pass_launches"], 1))
                    means.append(t["means_ms"])
                    rows_ms.append(t["row_ms"])
                point = pr.point_row()
            finally:
                pr.close()
            mats = b.get_data_matrices()
            xa, ya, xb, yb = mats[:4]
            wa = wb = None
            if weighted:
                w = np.asarray(f["w"])
                ga = np.asarray(f["g"]) == "A"
                wa, wb = w[ga], w[~ga]
            ca, cb = R.counts(O, SEED, 0, 0, len(ya)), R.counts(O, SEED, 0, 1, len(yb))
            t0 = time.perf_counter()
            want = R.decompose(O, xa, ya, xb, yb, wa, wb, ca, cb, R.GROUP_A, lower, upper, start=info["eta"])[0]
            cpu_s = time.perf_counter() - t0
            err = float(np.max(np.abs(rows[0][:-2] - want[:-2]) / np.maximum(np.abs(want[:-2]), abs(want[5]))))
            d = k + 1
            # a pass multiplies every (row, replicate) weight into d (d + 1) / 2 pair products and d gradient columns
            flops = 2.0 * a.rows * a.reps * (d * (d + 1) / 2 + d)
            bound_ms = flops / PEAK_FLOPS * 1e3
            rec = {"k": k, "weighted": weighted, "pass_ms": spread(per_pass), "batch_rounds": t["passes"],
                   "pass_launches": t["pass_launches"],
                   "passes_per_replicate": {"mean": float(rows[ok.astype(bool)][:, -2:].mean()),
                                            "max": float(rows[ok.astype(bool)][:, -2:].max())},
                   "means_pass_ms": spread(means), "rows_kernel_ms": spread(rows_ms), "replicates_per_s": spread(rate),
                   "ok_replicates_last_boot": int(ok.sum()), "total_gap": float(point[5]),
                   "censored_share": {"left_a": float(point[-6]), "right_a": float(point[-5]),
                                      "left_b": float(point[-4]), "right_b": float(point[-3])},
                   "cpu_restatement_s_per_replicate": cpu_s,
                   "speedup_vs_cpu_restatement": statistics.median(rate) * cpu_s,
                   "replicate_0_max_rel_err_vs_restatement": err,
                   "pass_multiply_add_ms_at_matrix_peak": bound_ms,
                   "pass_over_matrix_peak_bound": statistics.median(per_pass) / bound_ms,
                   "binary_replicates_per_s_parent": binary.get(k),
                   "rate_over_binary": (statistics.median(rate) / binary[k]) if k in binary else None}
            out["widths"].append(rec)
            print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")


if __name__ == "__main__":
    main()
