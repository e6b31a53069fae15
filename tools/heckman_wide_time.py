#!/usr/bin/env python
"""Times the Heckman two-step bootstrap on configs[1]'s panel shape (bench.py's heckman_frame:
1,000,000 x 20 plus a selection equation) at several widths of the selection equation and prints one
JSON line. Run by hand on an MI355X:

    python tools/heckman_wide_time.py [--rows N --reps R --widths 3,7,8,16,31 --warmup W --repeats K]
                                      [--bench-parent FILE --bench-this FILE] [--out PATH]

Per width (selection predictors; ks = width + 1 probit columns): milliseconds per probit pass (HIP
events around the probit kernel, summed over a boot's launches and divided by their number), the
probit iterations, the IMR-sums pass and replicates/s by the host clock around boot(); medians over
the repeats. Widths up to 7 run the register-resident kernels, wider ones ob_heck_wide_kernel, for
which the MFMA work of a pass, 2 * replicates * rows * (ks (ks + 1) / 2 + ks) flop, is also given as a
fraction of the f64 MFMA peak (padding columns and converged replicates are not counted as work, so
the fraction falls as replicates converge). The selection predictors are z1, z2, then the panel's own
x columns, then independent standard normal columns q1.. that the selection rule does not read.

--bench-parent / --bench-this: `bench.py --heckman` result lines of the parent commit and of this tree,
taken on the same machine, copied into the output as they are. There is no pass or fail threshold.
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


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def last_json_line(path):
    with open(path) as fh:
        lines = [ln for ln in fh if ln.lstrip().startswith("{")]
    return json.loads(lines[-1]) if lines else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--preds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--widths", default="3,7,8,16,31")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--bench-parent", default=None)
    ap.add_argument("--bench-this", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heckman_wide_time.json"))
    args = ap.parse_args()

    import bench

    ob = importlib.import_module("oaxaca-blinder-rs_amd")
    frame, names, zs3 = bench.heckman_frame(args.rows, args.preds)
    n = len(frame["y"])
    widths = [int(w) for w in args.widths.split(",")]
    pool = list(zs3) + [nm for nm in names if nm not in zs3]
    rng = np.random.default_rng(31)
    for j in range(max(0, max(widths) - len(pool))):
        frame[f"q{j + 1}"] = rng.normal(size=n)
        pool.append(f"q{j + 1}")
    out_widths = []
    for w in widths:
        zs, ks = pool[:w], w + 1
        b = (ob.OaxacaBuilder(frame, "y", "g", "F").predictors(names).heckman_selection("s", zs)
             .bootstrap_reps(args.reps).seed(0x0B5EED))
        pr = b.prepare()
        try:
            pass_ms, sums_ms, iters, rate, n_ok = [], [], [], [], 0
            for i in range(args.warmup + args.repeats):
                t0 = time.perf_counter()
                _, ok = pr.boot(i * args.reps, args.reps)
                dt = time.perf_counter() - t0
                tm = pr.timing()
                if i >= args.warmup:
                    pass_ms.append(tm["probit_ms"] / max(1, tm["probit_launches"]))
                    sums_ms.append(tm["heck_sums_ms"])
                    iters.append(tm["probit_iterations"])
                    rate.append(args.reps / dt)
                    n_ok = int(np.asarray(ok).astype(bool).sum())
        finally:
            pr.close()
        rec = {"selection_predictors": w, "ks": ks, "path": "wide (f64 MFMA)" if ks > 8 else "narrow (registers)",
               "probit_pass_ms": spread(pass_ms), "probit_iterations": max(iters), "imr_sums_ms": spread(sums_ms),
               "replicates_per_s": spread(rate), "ok_replicates_last_boot": n_ok}
        if ks > 8:
            flop = 2.0 * args.reps * n * (ks * (ks + 1) // 2 + ks)
            tf = flop / (statistics.median(pass_ms) * 1e-3) / 1e12
            rec["mfma_flop_per_pass"] = flop
            rec["mfma_tflops"] = tf
            rec["frac_of_f64_mfma_peak"] = tf / bench.F64_MFMA_PEAK_TFLOPS
        out_widths.append(rec)
    out = {"metric": "Heckman two-step bootstrap by width of the selection equation (configs[1] panel shape)",
           "rows": n, "predictors": args.preds, "replicates": args.reps, "warmup": args.warmup, "repeats": args.repeats,
           "f64_mfma_peak_tflops": bench.F64_MFMA_PEAK_TFLOPS, "widths": out_widths,
           "rate_note": "host clock around boot(): resample, Gram, probit passes, IMR sums, solve and the copy of the rows",
           "bench_heckman_parent": last_json_line(args.bench_parent) if args.bench_parent else None,
           "bench_heckman_this_tree": last_json_line(args.bench_this) if args.bench_this else None}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
