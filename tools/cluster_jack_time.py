"""Times the delete-one-cluster jackknife pass at the shapes of tools/cluster_time.py:
1,000,000 x 20 WLS at C = 1,000, 50,000 and 500,000 clusters of Zipf 1.3 sizes, 3 warm-up calls and then 10 timed
with HIP events (ob_cluster_jackknife_last_timing: the kernel with its ordered sums). It writes
profiles/cluster_jack_time.json. There is no target; the yardsticks are the clustered boot of the same panel
(profiles/cluster_time.json, read if present) and the numpy closed form of group A's downdate solves on the host
(the device pass does both groups: under the GroupA rule that is about twice this work).

    python tools/cluster_jack_time.py [--rows 1000000] [--p 20] [--clusters 1000,50000,500000] [--warmup 3] [--calls 10]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cluster_time import zipf_clusters  # noqa: E402


def numpy_closed_form(x1, y, w, ids, c, beta, g):
    """Seconds for the per-cluster downdate solves of one group on the host (group_a rule: no pooled fit)."""
    t0 = time.perf_counter()
    order = np.argsort(ids, kind="stable")
    bounds = np.searchsorted(ids[order], np.arange(c + 1))
    for cc in range(c):
        idx = order[bounds[cc]:bounds[cc + 1]]
        if len(idx) == 0:
            continue
        xc, wc = x1[idx], w[idx]
        q = (xc * wc[:, None]).T @ xc
        np.linalg.solve(g - q, (xc * wc[:, None]).T @ y[idx] - q @ beta)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--p", type=int, default=20)
    ap.add_argument("--clusters", default="1000,50000,500000")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_jack_time.json"))
    a = ap.parse_args()
    import oracle as O

    ob = importlib.import_module("oaxaca-blinder-rs_amd")
    d = O.synthetic_panel(a.rows, a.p, True, seed=20260424)
    na, nb = len(d["ya"]), len(d["yb"])
    rng = np.random.default_rng(7)
    xs = [f"x{j}" for j in range(a.p)]
    frame = {"y": np.concatenate([d["ya"], d["yb"]]), "g": np.array(["A"] * na + ["B"] * nb),
             "w": np.concatenate([d["wa"], d["wb"]])}
    x = np.vstack([d["xa"], d["xb"]])
    for j, nm in enumerate(xs):
        frame[nm] = np.ascontiguousarray(x[:, j])
    boot, boot_reps = {}, None
    bpath = os.path.join(ROOT, "profiles", "cluster_time.json")
    if os.path.exists(bpath):
        with open(bpath) as f:
            prof = json.load(f)
        boot, boot_reps = {c["clusters"]: c for c in prof.get("cases", [])}, prof.get("replicates")
    res = {"rows": na + nb, "p": a.p, "weighted": True, "warmup": a.warmup, "calls": a.calls, "zipf_s": 1.3, "cases": []}
    xa1 = np.hstack([np.ones((na, 1)), d["xa"]])
    ga = (xa1 * d["wa"][:, None]).T @ xa1
    beta_a = np.linalg.solve(ga, (xa1 * d["wa"][:, None]).T @ d["ya"])
    for c in [int(v) for v in a.clusters.split(",")]:
        ids = zipf_clusters(na + nb, c, rng)
        frame["firm"] = ids
        b = ob.OaxacaBuilder(frame, "y", "g", "B").predictors(xs).weights("w").reference_coefficients(0).seed(0x0B5EED)
        ms = []
        for i in range(a.warmup + a.calls):  # a handle keeps its result: a fresh one per call, Q formed before the pass
            pr = b.cluster("firm").prepare()
            try:
                pr.boot(0, 16)
                jk = pr.cluster_jackknife()
                if i >= a.warmup:
                    ms.append(ob.cluster_jackknife_last_timing())
            finally:
                pr.close()
        case = {"clusters": c, "pass_ms_median": statistics.median(ms), "pass_ms_min": min(ms), "pass_ms_max": max(ms),
                "kept": list(jk.n_used), "dropped": list(jk.n_dropped),
                "numpy_group_a_s": numpy_closed_form(xa1, d["ya"], d["wa"], ids[:na], c, beta_a, ga)}
        if c in boot:
            case["clustered_boot_call_s"] = boot[c].get("call_s_median")
            case["clustered_boot_replicates"] = boot_reps
        res["cases"].append(case)
        print(case, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
