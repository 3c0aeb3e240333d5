#!/usr/bin/env python3
"""A/B of two builds of libkspde.so on the C3 workload (4096 envs x 256 points, fast mode, 250 sub-steps per launch), or
on another workload and mode of bench.py (--workload c2|c3, --mode fast|exact).

--libs select (default)  lib/libkspde.so (masked FMA, KS_MASKED_SELECT in csrc/ks_kernels.hip) against
                         lib/libkspde_cndmask.so (the same sources with -DKS_UPWIND_CNDMASK: two v_cndmask per point);
                         writes profiles/ks_select_ab.json
--libs loop              lib/libkspde.so against lib/libkspde_loop0.so (-DKS_LOOP0: the sub-step loop with the
                         prologue's waits and the stage-4 copies still in it); writes profiles/ks_loop_ab.json
--libs A.so B.so         any two libraries (paths; the candidate first, the baseline second); --out names the file

One fresh child process per library and round, order A B A B ...; a timing is ONE pair of HIP events around SECONDS (>= 0.3 s)
of back-to-back launches after as long a warm-up (bench.py::KSRun.timed).  Every child runs under its own time
limit and the driver stops at the first non-zero exit.  Writes the result file into profiles/ (and a copy into every
--copy-to directory): every round's ms per launch, the median and the spread (max - min) per library, and the verdict:
a gain only if the gap of the medians exceeds three times the larger spread.

usage: tools/ks_select_ab.py [--libs select|loop|A.so B.so] [--out NAME.json] [--workload c3] [--mode fast] [--rounds 5]
                             [--copy-to DIR ...]
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
PAIRS = {"select": ((("masked", "libkspde.so"), ("cndmask", "libkspde_cndmask.so")), "ks_select_ab.json"),
         "loop": ((("shed", "libkspde.so"), ("loop0", "libkspde_loop0.so")), "ks_loop_ab.json")}
SECONDS = 1.0     # per timing and per warm-up (the floor is 0.3 s: longer timings narrow the round-to-round spread)
CHILD_TIMEOUT = 180
ACTION_SETS = 64


def child(workload, mode):
    for p in (ROOT, PKG):
        sys.path.insert(0, p)
    import torch
    import bench
    import kspde
    dev = torch.device("cuda:0")
    run = bench.KSRun(kspde, workload, 0, dev, 0, ACTION_SETS, mode)
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
    ap.add_argument("--libs", nargs="+", default=["select"], metavar="PAIR|LIB",
                    help="select, loop, or the paths of two libraries (candidate, baseline)")
    ap.add_argument("--out", default=None, metavar="NAME.json", help="file name under profiles/ (needed with two paths)")
    ap.add_argument("--workload", choices=["c2", "c3"], default="c3")
    ap.add_argument("--mode", choices=["fast", "exact"], default="fast")
    args = ap.parse_args()
    if args.child:
        return child(args.workload, args.mode)
    if len(args.libs) == 1:
        LIBS, out_name = PAIRS[args.libs[0]]
        LIBS = tuple((n, os.path.join(PKG, "lib", f)) for n, f in LIBS)
    else:
        assert len(args.libs) == 2 and args.out, "--libs takes a pair's name, or two paths together with --out"
        LIBS = tuple((n, os.path.abspath(f)) for n, f in zip(("a", "b"), args.libs))
        out_name = None
    out_name = args.out or out_name
    (cand, _), (base, _) = LIBS
    assert args.rounds >= 5, "at least five rounds"
    rounds = {name: [] for name, _ in LIBS}
    detail = []
    for r in range(args.rounds):
        for name, lib in LIBS:
            env = dict(os.environ, KSPDE_LIB=lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--workload", args.workload, "--mode",
                                args.mode], env=env, timeout=CHILD_TIMEOUT,
                               capture_output=True, text=True)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                sys.exit(f"round {r} {os.path.basename(lib)}: child exited with {p.returncode}; stopping")
            rec = json.loads(p.stdout.strip().splitlines()[-1])
            rounds[name].append(rec["ms_per_launch"])
            detail.append(dict(rec, round=r, library=os.path.relpath(lib, ROOT)))
            print(f"round {r} {os.path.basename(lib):22s} {rec['ms_per_launch']:.5f} ms per launch ({rec['launches']} launches)", flush=True)
    med = {k: statistics.median(v) for k, v in rounds.items()}
    spread = {k: max(v) - min(v) for k, v in rounds.items()}
    gap = med[base] - med[cand]
    margin = 3.0 * max(spread.values())
    E, N = {"c2": (1024, 64), "c3": (4096, 256)}[args.workload]
    out = {"workload": f"{args.workload}: {E} envs x {N} points, {args.mode} mode, 250 sub-steps per launch",
           "method": f"one fresh process per library and round, order A B A B; one HIP event pair around >= {SECONDS} s of "
                     f"back-to-back launches after as many warm-up launches (bench.py::KSRun.timed)",
           "libraries": dict((k, os.path.relpath(v, ROOT)) for k, v in LIBS),
           "ms_per_launch_by_round": rounds, "median_ms": med, "spread_ms": spread,
           f"gap_ms_{base}_minus_{cand}": gap, "gap_relative": gap / med[base], "required_gap_ms": margin,
           "gain": bool(gap > margin), "children": detail}
    text = json.dumps(out, indent=1)
    for d in [os.path.join(ROOT, "profiles")] + args.copy_to:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, out_name), "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: out[k] for k in ("median_ms", "spread_ms", f"gap_ms_{base}_minus_{cand}", "gap_relative",
                                          "required_gap_ms", "gain")}))


if __name__ == "__main__":
    main()
