#!/usr/bin/env python3
"""ms per optimizer step of the surrogate's TBPTT step with and without gradient-norm clipping, at B = 64, T = 20, tau = 10,
tbtt = 15, N = 64 and 256, on three routes:
  * captured            ``GraphedTBPTTStep``: forward + backward + Adam inside the gradient reduction, one replayed graph
  * captured_clip       the same with ``clip=0.5``: the reduction also writes per-block sums of squares and one more launch
                        (``sur_clip_adam_apply``) clips the global norm and applies Adam
  * split_graphs_clip   the clipping route without the captured clip: ``training_step`` (``GraphedAutogradStep``: forward
                        and backward as two replayed graphs) -> zero_grad -> backward -> ``clip_grad_norm_`` -> ``PackAdam.step``
The routes are alternated in one process after warm-up (``--rounds`` windows each, every window at least 0.5 s,
device events; the order of the routes rotates from round to round, so that none always follows the same neighbour); the
figure of a route is the median of its windows.  GPU only: without a device it is an error.
Prints one JSON object; ``--out FILE`` also writes it there.

Usage (repo root, on an MI355X):  python tools/clip_step_bench.py --out profiles/clip_step_bench.json
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "model-based-pde-control_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

B, T, TAU, TBTT, CLIP = 64, 20, 10, 15, 0.5
MIN_WINDOW_S = 0.5        # the floor every timed window is held to; --window is what the windows aim at


def module_for(n, dev):
    from pdecontrol.surrogates.bench_tbptt import build_module
    m = build_module(dev, N=n)
    m.tau, m.tbtt = TAU, TBTT
    return m


def routes(n, dev):
    from pdecontrol.surrogates import hipops
    from pdecontrol.surrogates.bench_tbptt import synthetic_batch
    from pdecontrol.surrogates.graph_step import GraphedTBPTTStep
    batch = synthetic_batch(B=B, T=T, N=n, device=dev)
    shape = tuple(batch[0].shape)
    plain = GraphedTBPTTStep(module_for(n, dev), shape)
    clipped = GraphedTBPTTStep(module_for(n, dev), shape, clip=CLIP)
    assert plain.adam_in_flush and clipped.adam_in_flush and clipped.grad_norm is not None
    plain.step(*batch)
    clipped.step(*batch)
    eager = module_for(n, dev)
    opt = eager.configure_optimizers()[0][0]
    assert isinstance(opt, hipops.PackAdam)

    def closure():
        out = eager.training_step(batch, 0)
        opt.zero_grad(set_to_none=True)
        out["loss"].backward()
        torch.nn.utils.clip_grad_norm_(eager.surrogate.parameters(), CLIP)
        opt.step()

    closure()
    assert "_split_steps" in eager.__dict__, "training_step did not take the split-graph route"
    return {"captured": plain.step, "captured_clip": clipped.step, "split_graphs_clip": closure}, clipped


def window(fn, reps, dev):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize(dev)
    return start.elapsed_time(end)        # ms


def timed(fn, reps, dev, min_ms=1e3 * MIN_WINDOW_S):
    """(ms, reps) of one window of at least ``min_ms``: a window that came out shorter is taken again with more steps."""
    while True:
        ms = window(fn, reps, dev)
        if ms >= min_ms:
            return ms, reps
        reps = math.ceil(1.25 * reps * min_ms / ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.65, help="seconds a timed window aims at (never below 0.5)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_step_bench.py needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda", 0)
    rec = {"what": "surrogate TBPTT optimizer step with and without gradient-norm clipping, ms per step (median of the "
                   "windows; device events; routes alternated in one process)",
           "B": B, "T": T, "tau": TAU, "tbtt": TBTT, "clip": CLIP, "rounds": args.rounds, "target_window_s": args.window,
           "min_window_s": MIN_WINDOW_S,
           "device": torch.cuda.get_device_name(dev), "rows": []}
    for n in (64, 256):
        fns, clipped = routes(n, dev)
        reps = {}
        for name, fn in fns.items():
            window(fn, args.warmup, dev)
            per_step = window(fn, args.warmup, dev) / args.warmup
            reps[name] = max(10, math.ceil(1e3 * args.window / per_step))
        times = {name: [] for name in fns}
        windows = {name: [] for name in fns}
        names, order = list(fns), []
        for r in range(args.rounds):
            order.append(names[r % len(names):] + names[:r % len(names)])
            for name in order[-1]:
                ms, reps[name] = timed(fns[name], reps[name], dev)
                times[name].append(ms / reps[name])
                windows[name].append(round(ms / 1e3, 3))
        assert all(w >= MIN_WINDOW_S for ws in windows.values() for w in ws), windows
        med = {name: statistics.median(v) for name, v in times.items()}
        rec["rows"].append({"N": n, "ms_per_step": {k: round(v, 4) for k, v in med.items()},
                            "windows_ms_per_step": {k: [round(x, 4) for x in v] for k, v in times.items()},
                            "window_s": windows, "reps": reps, "order": order,
                            "clip_minus_plain_us": round(1e3 * (med["captured_clip"] - med["captured"]), 2),
                            "clip_over_plain": round(med["captured_clip"] / med["captured"], 4),
                            "captured_clip_faster_than_split_graphs_clip": med["captured_clip"] < med["split_graphs_clip"],
                            "pipelined": {"captured": fns["captured"].__self__.used_pipelined,
                                          "captured_clip": clipped.used_pipelined},
                            "last_grad_norm": float(clipped.grad_norm[0])})
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
