#!/usr/bin/env python
"""Times OaxacaBuilder.check_defensibility on a synthetic 1,000,000 x 20 wage frame, feeding optimize()'s own
adjustments back.

    python tools/defend_time.py [--rows N --k K --warmup W --repeats R] [--out PATH]

Per pass of the defensibility step (the first-wins scatter, the per-adjustment pass, the row pass): the HIP-event
time (ob_defend_info), the bytes the pass must read from HBM (its inputs once) and the rate the two give. The
yardstick is measured in the same run on the same box: ob_vif's residual pass (vif_sums_device) over the same
n x k predictors, which streams them once. The whole check_defensibility() call by the host clock (frame
conversion, design build and upload included). No time is fixed in advance. Writes profiles/defend_time.json."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "defend_time.json"))
    args = ap.parse_args()
    ob = importlib.import_module("oaxaca-blinder-rs_amd")
    rng = np.random.default_rng(20260424)  # tools/remedy_time.py's frame
    n, k = args.rows, args.k
    x = rng.normal(size=(n, k))
    ref = rng.random(n) < 0.5
    wage = 30.0 + x @ rng.uniform(0.5, 2.0, k) + rng.normal(size=n) - 2.0 * (~ref)
    frame = {"wage": wage, "g": np.where(ref, "a", "b")}
    names = [f"x{j}" for j in range(k)]
    frame.update({nm: x[:, j] for j, nm in enumerate(names)})
    b = ob.OaxacaBuilder(ob.Frame(frame), "wage", "g", "a").predictors(names)
    adjustments = [(a.index, a.adjustment) for a in b.optimize().adjustments]
    xf = np.asfortranarray(x)
    runs, stream = [], []
    for it in range(args.warmup + args.repeats):
        ob.vif(xf)
        sums_ms = ob.vif_last_timing()["sums_ms"]
        t0 = time.perf_counter()
        res = b.check_defensibility(adjustments, contributions=False)
        t1 = time.perf_counter()
        if it >= args.warmup:
            info = b.last_defend_info
            runs.append({"check_defensibility_s": t1 - t0, **{a: info[a] for a in info if a.endswith("_ms")}})
            stream.append(sums_ms)
    med = {a: float(np.median([r[a] for r in runs])) for a in runs[0]}
    info = b.last_defend_info
    n_a, n_b, m = int(info["n_a"]), int(info["n_b"]), int(info["n_adjustments"])
    # scatter: the rows of the adjustments (4 B) and one 4-byte atomic each; the memset of first[n] is written, not read
    # adjust: row (4) and value (8), then y, fair and leverage of its row (24, gathered)
    # rows: y (8) and first (4) of every row, fair (8) of B's rows, one gathered value (8) per adjusted row
    bytes_read = {"scatter_ms": 8 * m, "adjust_ms": 36 * m, "rows_ms": 12 * n + 8 * n_b + 8 * m}
    stream_ms = float(np.median(stream))
    stream_gbps = 8 * n * k / stream_ms / 1e6
    passes = {a: {"ms": med[a], "bytes_read": int(bytes_read[a]), "GBps": bytes_read[a] / med[a] / 1e6 if med[a] > 0 else None,
                  "fraction_of_stream_rate": bytes_read[a] / med[a] / 1e6 / stream_gbps if med[a] > 0 else None}
              for a in bytes_read}
    out = {"metric": "check_defensibility on a synthetic wage frame, optimize()'s adjustments fed back", "rows": n,
           "predictors": k, "n_a": n_a, "n_b": n_b, "adjustments": m, "warmup": args.warmup, "repeats": args.repeats,
           "check_defensibility_s": med["check_defensibility_s"], "passes": passes,
           "gram_ms": med["gram_ms"], "score_ms": med["score_ms"], "defend_ms": med["defend_ms"],
           "stream_yardstick": {"what": "ob_vif residual pass (vif_sums_device) on the same n x k predictors, same run",
                                "ms": stream_ms, "bytes_read": 8 * n * k, "GBps": stream_gbps},
           "reference_lookup_comparisons": float(n) * m,
           "total_cost": res.total_cost, "required_budget": res.required_budget, "new_unexplained_gap": res.new_unexplained_gap,
           "defensible": int(sum(a.is_defensible for a in res.adjustments))}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
