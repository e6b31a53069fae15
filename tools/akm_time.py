#!/usr/bin/env python
"""Times the AKM path on one synthetic panel (1,000,000 rows, about 200k workers, about 20k firms with
Zipf 1.3 firm sizes, 5 controls; tests/akm_ref.py's generator) and prints one JSON line. Run by hand on
an MI355X:

    python tools/akm_time.py [--rows N --workers W --firms F --controls K --warmup W --repeats R] [--out PATH]

Kernel figures are HIP-event times from ob_akm_results_info: the demean loop over the batch of
1 + K columns divided by its iteration count (the slowest column's), and the recover_fe loop likewise.
The whole call is a host clock around AkmBuilder.run(), which includes the frame copy, the connected
set, the counting sorts and the uploads. Medians over the repeats, with min and max beside them.

Bytes of one demean iteration, as the kernels issue them: the worker pass reads the batch twice (sum,
then apply) and writes it once, the firm pass reads the worker pass's output twice and the previous
batch once and writes once, and each pass reads its row list twice: 7 n C 8 + 4 n 4 bytes. The 48 MB
batch and its copy sit in the 256 MiB Infinity Cache between launches, so the rate is held against
the 6.29 TB/s HBM figure only as a yardstick, not as HBM traffic.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_TBPS = 6.29


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--workers", type=int, default=200_000)
    ap.add_argument("--firms", type=int, default=20_000)
    ap.add_argument("--controls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON to this path")
    args = ap.parse_args()

    import akm_ref as A

    ob = importlib.import_module("oaxaca-blinder-rs_amd")
    d = A.panel(args.rows, args.workers, args.firms, args.controls, 7, zipf=True)
    n, c = len(d["y"]), args.controls + 1
    names = [f"x{j}" for j in range(args.controls)]
    frame = {"worker": d["widx"].astype(np.int64), "firm": d["fidx"].astype(np.int64), "y": d["y"]}
    frame.update({nm: np.ascontiguousarray(d["x"][:, j]) for j, nm in enumerate(names)})
    fr = ob.Frame(frame)
    fr.as_c()
    demean_it, recover_it, whole, ols, res = [], [], [], [], None
    for i in range(args.warmup + args.repeats):
        t0 = time.perf_counter()
        res = ob.AkmBuilder(fr, "y", "worker", "firm").controls(names).run()
        t1 = time.perf_counter()
        if i >= args.warmup:
            demean_it.append(res.info["demean_ms"] / max(res.info["demean_iterations"]))
            recover_it.append(res.info["recover_ms"] / res.info["recover_iterations"])
            ols.append(res.info["ols_ms"])
            whole.append((t1 - t0) * 1e3)
    it_bytes = 7 * n * c * 8 + 4 * n * 4
    tbps = it_bytes / (statistics.median(demean_it) * 1e-3) / 1e12
    firm_sizes = np.bincount(d["fidx"])
    out = {
        "metric": "ob_akm_run on a synthetic Zipf panel",
        "rows_kept": n, "workers": d["nw"], "firms": d["nf"], "controls": args.controls, "batch_columns": c,
        "largest_firm_rows": int(firm_sizes.max()), "largest_worker_rows": int(np.bincount(d["widx"]).max()),
        "firms_per_schedule": {"lane": int((firm_sizes <= A.LANE_MAX).sum()),
                               "wave": int(((firm_sizes > A.LANE_MAX) & (firm_sizes <= A.WAVE_MAX)).sum()),
                               "block": int((firm_sizes > A.WAVE_MAX).sum())},
        "demean_iterations": res.info["demean_iterations"], "recover_iterations": res.info["recover_iterations"],
        "launches_per_demean_iteration": res.info["launches_per_iteration"],
        "demean_ms_per_iteration": spread(demean_it),
        "recover_fe_ms_per_iteration": spread(recover_it),
        "ols_r2_ms": spread(ols),
        "whole_run_ms": spread(whole),
        "demean_iteration": {"bytes_issued": it_bytes, "batch_bytes": n * c * 8, "achieved_tbps": tbps,
                             "hbm_tbps": HBM_TBPS, "frac_of_hbm": tbps / HBM_TBPS,
                             "note": "the batch and its copy sit in the Infinity Cache; the poll's flag read "
                                     "(every akm_poll iterations) is inside the loop's events"},
        "beta": res.beta, "r2": res.r2, "warmup": args.warmup, "repeats": args.repeats,
        "whole_run_note": "host clock; frame copy, connected set, counting sorts and uploads included",
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
