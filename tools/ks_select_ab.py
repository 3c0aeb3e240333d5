#!/usr/bin/env python3
"""A/B of the fast-mode upwind select on the C3 workload (4096 envs x 256 points, fast mode, 250 sub-steps per launch):
lib/libkspde.so (masked FMA, KS_MASKED_SELECT in csrc/ks_kernels.hip) against lib/libkspde_cndmask.so (the same sources
with -DKS_UPWIND_CNDMASK: two v_cndmask per point).

One fresh child process per library and round, order A B A B ...; a timing is ONE pair of HIP events around SECONDS (>= 0.3 s)
of back-to-back launches after as long a warm-up (bench.py::KSRun.timed).  Every child runs under its own time
limit and the driver stops at the first non-zero exit.  Writes profiles/ks_select_ab.json (and a copy into every
--copy-to directory): every round's ms per launch, the median and the spread (max - min) per library, and the verdict:
a gain only if the gap of the medians exceeds three times the larger spread.

usage: tools/ks_select_ab.py [--rounds 5] [--copy-to DIR ...]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "model-based-pde-control_amd")
LIBS = (("masked", "libkspde.so"), ("cndmask", "libkspde_cndmask.so"))
SECONDS = 1.0     # per timing and per warm-up (the floor is 0.3 s: longer timings narrow the round-to-round spread)
CHILD_TIMEOUT = 180
ACTION_SETS = 64


def child():
    for p in (ROOT, PKG):
        sys.path.insert(0, p)
    import torch
    import bench
    import kspde
    dev = torch.device("cuda:0")
    run = bench.KSRun(kspde, "c3", 0, dev, 0, ACTION_SETS, "fast")
    step = run.one_step
    run.one_step = lambda i: step(i % ACTION_SETS)
    sync = run.stream.synchronize
    _, probe_ms = run.timed(20, 5, sync)
    n = int(math.ceil(SECONDS / (probe_ms * 1e-3))) + 1
    _, ms = run.timed(n, n, sync)
    print(json.dumps({"ms_per_launch": ms, "launches": n, "warmup_launches": n, "layout": run.stepper.layout(),
                      "lib": os.path.basename(os.environ.get("KSPDE_LIB", "libkspde.so"))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--copy-to", action="append", default=[], metavar="DIR", help="also write the result file into DIR")
    args = ap.parse_args()
    if args.child:
        return child()
    assert args.rounds >= 5, "at least five rounds"
    rounds = {name: [] for name, _ in LIBS}
    detail = []
    for r in range(args.rounds):
        for name, lib in LIBS:
            env = dict(os.environ, KSPDE_LIB=os.path.join(PKG, "lib", lib))
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, timeout=CHILD_TIMEOUT,
                               capture_output=True, text=True)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                sys.exit(f"round {r} {lib}: child exited with {p.returncode}; stopping")
            rec = json.loads(p.stdout.strip().splitlines()[-1])
            rounds[name].append(rec["ms_per_launch"])
            detail.append(dict(rec, round=r, library=lib))
            print(f"round {r} {lib:22s} {rec['ms_per_launch']:.5f} ms per launch ({rec['launches']} launches)", flush=True)
    med = {k: statistics.median(v) for k, v in rounds.items()}
    spread = {k: max(v) - min(v) for k, v in rounds.items()}
    gap = med["cndmask"] - med["masked"]
    margin = 3.0 * max(spread.values())
    out = {"workload": "c3: 4096 envs x 256 points, fast mode, 250 sub-steps per launch",
           "method": f"one fresh process per library and round, order A B A B; one HIP event pair around >= {SECONDS} s of "
                     f"back-to-back launches after as many warm-up launches (bench.py::KSRun.timed)",
           "libraries": dict((k, "lib/" + v) for k, v in LIBS),
           "ms_per_launch_by_round": rounds, "median_ms": med, "spread_ms": spread,
           "gap_ms_cndmask_minus_masked": gap, "gap_relative": gap / med["cndmask"], "required_gap_ms": margin,
           "gain": bool(gap > margin), "children": detail}
    text = json.dumps(out, indent=1)
    for d in [os.path.join(ROOT, "profiles")] + args.copy_to:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "ks_select_ab.json"), "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: out[k] for k in ("median_ms", "spread_ms", "gap_ms_cndmask_minus_masked", "gap_relative",
                                          "required_gap_ms", "gain")}))


if __name__ == "__main__":
    main()
