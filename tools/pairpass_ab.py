#!/usr/bin/env python
"""A/B of two builds of the library over the pair-product pass kernels: the in-tree library against
another one (the parent commit's, built beside it). Every entry point runs in a fresh child process per library
(OB_LIB_PATH), on seeded inputs at the edge shapes of the pass tests; the child prints the SHA-256 of each output's
bytes. Every pair of hashes must be equal: every sum has a fixed order and no arithmetic moved. Then the project's
timers (TIMERS) run under both libraries, alternated --rounds times; a field whose HEAD median lies outside the parent's
spread on the slow side is a failure. --register-check REV needs no GPU: it compiles the four files at REV and in the
tree and fails where a kernel's occupancy drops or its scratch grows. Both write into profiles/pairpass_ab.json; the
exit status is 1 on any failure.

    python tools/pairpass_ab.py --register-check HEAD~1
    python tools/pairpass_ab.py --old PATH/liboaxaca_boot_parent.so [--rounds 3] [--quick] [--no-timers]
"""
import argparse
import hashlib
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [1, 5, 6, 11, 31, 32]
NS = [65, 257]
SEED = 0x0B5EED


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def inputs(n, k):
    rng = np.random.default_rng(1000 * n + k)
    x = np.column_stack([np.ones(n), rng.normal(size=(n, k - 1))])
    y = rng.normal(size=n)
    d = (rng.random(n) < 0.5).astype(float)
    w = rng.uniform(0.5, 2.0, n)
    c = rng.integers(0, 4, n).astype(np.uint8)
    coefs = rng.normal(size=(17, k)) * 0.4 / np.sqrt(k)
    return rng, x, y, d, w, c, coefs


def frame(n, k, weighted=True, censor=False, nz=0):
    rng = np.random.default_rng(7 * n + k)
    g = np.where(np.arange(n) % 2 == 0, "A", "B")
    x = rng.normal(size=(n, k - 1))
    y = 0.25 * (g == "A") + x @ (0.5 / np.sqrt(k - 1) * (-1.0) ** np.arange(k - 1)) + rng.normal(size=n)
    f = {"g": g.tolist()}
    if censor:
        y = np.clip(y - np.quantile(y, 0.25), 0.0, None)
    f["y"] = y
    for j in range(k - 1):
        f[f"x{j}"] = np.ascontiguousarray(x[:, j])
    if weighted:
        f["w"] = rng.uniform(0.5, 2.0, n)
    if nz:
        z = rng.normal(size=(n, nz))
        f["s"] = (0.5 + z @ (0.3 * (-0.8) ** np.arange(nz)) + rng.normal(size=n) > 0).astype(float)
        for j in range(nz):
            f[f"z{j}"] = np.ascontiguousarray(z[:, j])
    return f, [f"x{j}" for j in range(k - 1)]


def child(rows):
    sys.path.insert(0, ROOT)
    ob = importlib.import_module("oaxaca-blinder-rs_amd")
    out = {"hashes": {}}
    H = out["hashes"]
    for n in NS:
        for k in KS:
            rng, x, y, d, w, c, coefs = inputs(n, k)
            H[f"reweight_logit_pass n={n} k={k}"] = sha(*ob.reweight_logit_pass(x, d, coefs, w=w, counts=c))
            b = d == 0
            H[f"reweight_gram n={n} k={k}"] = sha(*ob.reweight_gram(x[b], y[b], coefs, w=w[b], counts=c[b]))
            thr = np.linspace(np.quantile(y, 0.1), np.quantile(y, 0.9), 17)
            H[f"dr_logit_pass n={n} k={k} T=17"] = sha(*ob.dr_logit_pass(x, y, thr, coefs, w=w, counts=c))
            if k <= 31:
                yc = np.clip(y + 0.5, 0.0, 2.0)
                etas = np.column_stack([coefs, rng.uniform(0.8, 1.25, 17)])
                H[f"tobit_pass n={n} k={k}"] = sha(*ob.tobit_pass(x, yc, etas, 0.0, 2.0, w=w, counts=c))
                if n > 4 * k:
                    cr = rng.integers(0, 4, size=(65, n)).astype(np.uint8)
                    H[f"tobit_fit n={n} k={k} reps=65"] = sha(*ob.tobit_fit(x, yc, 0.0, 2.0, w=w, counts=cr))
    for n, k in [(3001, 9), (3001, 17), (3001, 32)]:  # the wide probit pass and step (k > 8)
        rng = np.random.default_rng(n + k)
        z = np.column_stack([np.ones(n), rng.normal(size=(n, k - 1))])
        s = (0.3 + z[:, 1:] @ (0.5 * (-0.8) ** np.arange(k - 1)) + rng.normal(size=n) > 0).astype(float)
        beta, conv, iters = ob.probit(z, s)
        H[f"probit n={n} k={k}"] = sha(beta, np.array([conv, iters]))

    n, reps = rows, 200
    f, xs = frame(n, 9)
    b = ob.OaxacaBuilder(f, "y", "g", "B").predictors(xs).weights("w").bootstrap_reps(reps).seed(SEED)
    pr = b.prepare_reweighted()
    try:
        rows, ok = pr.boot(0, reps)
    finally:
        pr.close()
    H["frame reweighted k=9 reps=200"] = sha(rows, ok)
    pr = b.prepare_distribution([0.1, 0.5, 0.9], n_thresholds=17, lo=0.1, hi=0.9)
    try:
        rows, ok = pr.boot(0, reps)
    finally:
        pr.close()
    H["frame distribution k=9 T=17 reps=200"] = sha(rows, ok)
    f, xs = frame(n, 9, censor=True)
    pr = (ob.OaxacaBuilder(f, "y", "g", "B").predictors(xs).weights("w").bootstrap_reps(reps).seed(SEED)
          .prepare_tobit(0.0, None))
    try:
        rows, ok = pr.boot(0, reps)
    finally:
        pr.close()
    H["frame tobit k=9 reps=200"] = sha(rows, ok)
    f, xs = frame(n, 3, weighted=False, nz=16)
    pr = (ob.OaxacaBuilder(f, "y", "g", "B").predictors(xs).heckman_selection("s", [f"z{j}" for j in range(16)])
          .bootstrap_reps(reps).seed(SEED).prepare())
    try:
        rows, ok = pr.boot(0, reps)
    finally:
        pr.close()
    H["frame heckman ks=17 reps=200"] = sha(rows, ok)
    print("PAIRPASS_AB " + json.dumps(out), flush=True)


def run_child(lib, rows):
    env = dict(os.environ)
    if lib:
        env["OB_LIB_PATH"] = lib
    else:
        env.pop("OB_LIB_PATH", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--rows", str(rows)], env=env, capture_output=True, text=True,
                       timeout=900)
    for line in p.stdout.splitlines():
        if line.startswith("PAIRPASS_AB "):
            return json.loads(line[len("PAIRPASS_AB "):])
    raise SystemExit(f"child failed under {lib or 'the in-tree library'} (exit {p.returncode}):\n{p.stdout[-2000:]}\n"
                     f"{p.stderr[-4000:]}")


# The project's own timers that reach these kernels (density_time.py through the shared logit loop), and the arguments
# --quick trims them with so that the alternation fits one GPU visit.
TIMERS = {"reweight_time.py": ["--repeats", "3"], "dr_time.py": ["--repeats", "3"], "tobit_time.py": ["--repeats", "3"],
          "heckman_wide_time.py": ["--repeats", "3"], "density_time.py": []}
QUICK = {"reweight_time.py": ["--rows", "200000", "--reps", "1000"],
         "dr_time.py": ["--rows", "200000", "--reps", "200", "--thresholds", "19"],
         "tobit_time.py": ["--rows", "200000", "--reps", "1000"],
         "heckman_wide_time.py": ["--rows", "200000", "--reps", "1000", "--widths", "16,31"],
         "density_time.py": ["--rows", "200000", "--reps", "1000"]}


def leaves(node, path=""):
    """(path, number) of every numeric leaf of a timer's JSON."""
    if isinstance(node, dict):
        for k, v in node.items():
            yield from leaves(v, f"{path}/{k}")
    elif isinstance(node, list):
        for i, v in enumerate(node):
            yield from leaves(v, f"{path}/{i}")
    elif isinstance(node, (int, float)) and not isinstance(node, bool):
        yield path, float(node)


def timed_fields(doc):
    """The medians a timer reports of GPU-event ms (lower is better) and of replicates/s (higher is better); what it
    reports of the one-thread CPU restatement or reads from another file is left out."""
    out = {}
    for path, v in leaves(doc):
        low = path.lower()
        last = low.rsplit("/", 1)[-1]  # a spread's median, or a plain *_ms figure (density_time.py runs once)
        if not (last == "median" or last.endswith("_ms")) or any(w in low for w in ("cpu", "speedup", "parent", "binary", "bound")):
            continue
        if "ms" in low:
            out[path] = (v, -1)
        elif "per_s" in low:
            out[path] = (v, 1)
    return out


def run_timer(name, extra, lib, tmp):
    env = dict(os.environ)
    if lib:
        env["OB_LIB_PATH"] = lib
    else:
        env.pop("OB_LIB_PATH", None)
    out = os.path.join(tmp, name + ".json")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", name), "--out", out] + extra, env=env,
                       capture_output=True, text=True, timeout=1500)
    if p.returncode != 0:
        raise SystemExit(f"{name} failed under {lib or 'the in-tree library'} (exit {p.returncode}):\n{p.stderr[-4000:]}")
    with open(out) as fh:
        return timed_fields(json.load(fh))


def time_libraries(old, rounds, quick, tmp):
    """Every timer under the parent's library and the in-tree one, alternated `rounds` times. A field fails where HEAD's
    median over the rounds lies outside the parent's spread over its rounds on the slow side."""
    runs = {name: {"parent": [], "head": []} for name in TIMERS}
    for _ in range(rounds):
        for side, lib in (("parent", old), ("head", None)):
            for name, args in TIMERS.items():
                runs[name][side].append(run_timer(name, args + (QUICK[name] if quick else []), lib, tmp))
    report, slow = {}, []
    for name, r in runs.items():
        report[name] = {"arguments": TIMERS[name] + (QUICK[name] if quick else []), "fields": {}}
        for path, (_, sign) in r["head"][0].items():
            rec = {}
            for side in ("parent", "head"):
                v = [x[path][0] for x in r[side]]
                rec[side] = {"repeats": v, "median": statistics.median(v), "min": min(v), "max": max(v)}
            if sign < 0:
                rec["slower_than_parents_spread"] = rec["head"]["median"] > rec["parent"]["max"]
            else:
                rec["slower_than_parents_spread"] = rec["head"]["median"] < rec["parent"]["min"]
            report[name]["fields"][path] = rec
            if rec["slower_than_parents_spread"]:
                slow.append(f"{name}{path}")
    return report, slow


REG_FILES = ["ob_heckman.hip", "ob_reweight.hip", "ob_dr.hip", "ob_tobit.hip"]
REG_KERNELS = ("ob_heck_wide_kernel", "ob_rw_kernel", "ob_dr_kernel", "ob_tobit_kernel", "ob_rw_step_kernel",
               "ob_dr_step_kernel", "ob_tobit_step_kernel", "ob_probit_wide_step_kernel")


def resource_usage(csrc, tmp):
    """{kernel: [VGPR, AGPR, scratch B/lane, occupancy]} of the pass and step kernels of the four files under csrc."""
    import re
    procs = [subprocess.Popen(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-DOB_TUNING=0",
                               "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", f, "-o",
                               os.path.join(tmp, f + ".o")], cwd=csrc, stderr=subprocess.PIPE, text=True) for f in REG_FILES]
    usage, name = {}, None
    for p in procs:
        err = p.communicate()[1]
        if p.returncode != 0:
            raise SystemExit(err[-4000:])
        for line in err.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                sym = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
                sym = sym.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
                name = sym if sym.startswith(REG_KERNELS) else None
                if name:
                    usage[name] = [None] * 4
            for i, key in enumerate(("VGPRs:", "AGPRs:", "ScratchSize [bytes/lane]:", "Occupancy [waves/SIMD]:")):
                m = re.search(re.escape(key) + r" (\d+)", line)
                if m and name and " " + key in line:
                    usage[name][i] = int(m.group(1))
    return usage


def register_check(parent_rev, tmp):
    """Compiles the four files at parent_rev and in the tree; a kernel fails where its occupancy drops or its scratch
    grows."""
    old = os.path.join(tmp, "parent")
    os.makedirs(old)
    tar = subprocess.run(["git", "-C", ROOT, "archive", parent_rev, "oaxaca-blinder-rs_amd/csrc", "include"],
                         capture_output=True, check=True).stdout
    subprocess.run(["tar", "-x", "-C", old], input=tar, check=True)
    up = resource_usage(os.path.join(old, "oaxaca-blinder-rs_amd", "csrc"), tmp)
    uh = resource_usage(os.path.join(ROOT, "oaxaca-blinder-rs_amd", "csrc"), tmp)
    table, bad = {"compiler": "hipcc -O3 --offload-arch=gfx950", "parent": parent_rev,
                  "columns": ["VGPR", "AGPR", "scratch B/lane", "occupancy waves/SIMD"], "kernels": {}}, []
    for k in sorted(up):
        table["kernels"][k] = {"parent": up[k], "head": uh.get(k)}
        if k not in uh or uh[k][3] < up[k][3] or uh[k][2] > up[k][2]:
            bad.append(k)
    return table, bad


def main():
    import tempfile
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--old", help="the other library (the parent commit's build)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=200_000, help="rows of the four frame runs")
    ap.add_argument("--no-timers", action="store_true", help="hashes only")
    ap.add_argument("--quick", action="store_true", help="the timers at 200,000 rows and fewer replicates")
    ap.add_argument("--register-check", metavar="REV", help="needs no GPU: compile the four files at REV and in the tree, "
                    "compare registers, scratch and occupancy, and keep the table in --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairpass_ab.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.rows)
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            out = json.load(fh)
    failures = []
    with tempfile.TemporaryDirectory() as tmp:
        if a.register_check:
            out["registers"], bad = register_check(a.register_check, tmp)
            failures += [f"registers: {k}" for k in bad]
        else:
            if not a.old or not os.path.exists(a.old):
                raise SystemExit("--old must name the parent commit's library")
            old = os.path.abspath(a.old)
            hp, hh = run_child(old, a.rows)["hashes"], run_child(None, a.rows)["hashes"]
            out["hashes"] = {k: {"parent": hp.get(k), "head": hh[k], "equal": hp.get(k) == hh[k]} for k in hh}
            differ = [k for k, v in out["hashes"].items() if not v["equal"]]
            out.update({"metric": "pair-product pass front ends: parent library against HEAD", "frame_rows": a.rows,
                        "frame_replicates": 200, "shapes": {"n": NS, "k": KS}, "all_hashes_equal": not differ})
            failures += [f"hash: {k}" for k in differ]
            if not a.no_timers:
                out["timers"], slow = time_libraries(old, a.rounds, a.quick, tmp)
                out["timer_rounds"] = a.rounds
                failures += [f"slower: {k}" for k in slow]
    out["register_failures" if a.register_check else "failures"] = failures
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"failures": failures}))
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())

