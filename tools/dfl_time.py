#!/usr/bin/env python
"""Times ob_dfl_run on BASELINE.json configs[1]'s panel shape (1,000,000 rows x 20 predictors,
oracle.synthetic_panel) and prints one JSON line. Run by hand on an MI355X:

    python tools/dfl_time.py [--rows N --preds P --warmup W --repeats R] [--cpu]

Kernel figures are HIP-event times from ob_dfl_results_info (the Newton-pass launches of the logit,
the three KDE launches); the whole call is a host clock around run_dfl, which returns after the
results are on the host. Medians over the repeats, with min and max beside them. --cpu adds the
NumPy restatement (tests/dfl_ref.py) on the same frame as a CPU baseline: it is the checker, not
the reference crate, and is labelled as such.
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

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec


def frame_of(rows, preds):
    import oracle as O

    d = O.synthetic_panel(rows, preds, False)
    x = np.vstack([d["xa"], d["xb"]])
    names = [f"x{j + 1}" for j in range(preds)]
    frame = {"y": np.concatenate([d["ya"], d["yb"]]),
             "g": np.array(["M"] * len(d["ya"]) + ["F"] * len(d["yb"]), dtype=object)}
    frame.update({nm: np.ascontiguousarray(x[:, j]) for j, nm in enumerate(names)})
    return frame, names


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--preds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cpu", action="store_true", help="also time tests/dfl_ref.py on the same frame")
    args = ap.parse_args()

    ob = importlib.import_module("oaxaca-blinder-rs_amd")
    frame, names = frame_of(args.rows, args.preds)
    fr = ob.Frame(frame)
    fr.as_c()  # column buffers converted once, outside the timed calls
    per_iter, kde_ms, whole_ms, res = [], [], [], None
    for i in range(args.warmup + args.repeats):
        t0 = time.perf_counter()
        res = ob.run_dfl(fr, "y", "g", "F", names)
        t1 = time.perf_counter()
        if i >= args.warmup:
            per_iter.append(res.logit_ms / res.logit_iterations)
            kde_ms.append(res.kde_ms)
            whole_ms.append((t1 - t0) * 1e3)
    k = args.preds + 1
    pass_bytes = args.rows * k * 8 + args.rows * 8  # X and y read once per Newton pass
    gbps = pass_bytes / (statistics.median(per_iter) * 1e-3) / 1e9
    out = {
        "metric": "ob_dfl_run on configs[1]'s panel shape",
        "rows": args.rows, "predictors": args.preds, "logit_columns": k, "grid_points": len(res.grid),
        "n_a": res.n_a, "n_b": res.n_b, "logit_iterations": res.logit_iterations,
        "logit_converged": res.logit_converged,
        "logit_ms_per_iteration": spread(per_iter),
        "kde_ms_three_launches": spread(kde_ms),
        "whole_call_ms": spread(whole_ms),
        "logit_pass": {"bytes_per_iteration": pass_bytes, "achieved_gbps": gbps, "peak_gbps": HBM_PEAK_GBPS,
                       "frac_of_hbm_peak": gbps / HBM_PEAK_GBPS,
                       "note": "HIP events around the pass + reduce launches of one iteration"},
        "kde_exp_evaluations": 3 * len(res.grid) * (args.rows // 2),
        "warmup": args.warmup, "repeats": args.repeats,
        "whole_call_note": "host clock; includes building X on the host and the uploads of X, y and the outcomes",
    }
    if args.cpu:
        import dfl_ref as R

        lists = {c: (v.tolist() if isinstance(v, np.ndarray) else list(v)) for c, v in frame.items()}
        t0 = time.perf_counter()
        ref = R.run_dfl(lists, "y", "g", "F", names)
        out["cpu_baseline"] = {"what": "tests/dfl_ref.py (NumPy f64 restatement, the checker) on the host cores",
                               "whole_call_ms": (time.perf_counter() - t0) * 1e3,
                               "iterations": ref["iterations"]}
        out["max_density_error_vs_cpu"] = max(
            float(np.max(np.abs(getattr(res, key) - ref[key])) / np.max(ref[key]))
            for key in ("density_a", "density_b", "density_b_counterfactual"))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
