#!/usr/bin/env python3
"""ms per optimizer step of the latent ConvLSTM surrogate (KSLatentConvolutionalLSTM / ...N) at B = 64, T = 20, N = 64 and
256.

Default: training_step + backward + the optimizer of configure_optimizers (torch Adam), on
  * fused       the fused HIP kernels (hipops.fused_latent_rollout per TBPTT chunk, loss in torch),
  * plain       the same step with the fused kernels switched off (ops.fused(False), the PDECONTROL_FUSED=0 switch),
  * autoreg     for context, the autoregressive KSAutoRegConvolutionalLSTM's launch-by-launch fused step (split graphs off,
                PackAdam) at the same shape.
Record only: there is no target.

``--captured --parent-root DIR``: the captured latent step against what it replaces.  Three routes, each measured in a
process of its own, alternated over ``--rounds`` rounds, median and range per route and N:
  * p   ``fused_step`` of the tree at DIR (a checkout of the parent commit with its libraries built: there the captured step
        of a latent module is a hipGraph over the eager chunk loop, the torch loss and torch Adam),
  * a   the eager step above (this tree),
  * b   ``fused_step`` of this tree (hipops.fused_latent_tbptt_train: sur_tbptt_decoded_loss, Adam in the flush).
The claim "b is faster than p" is recorded as met where median(p) - median(b) exceeds the two ranges together, so that
process-to-process spread cannot carry it.  The record goes under the key "captured_step" of ``--out`` (the rest of an
existing file is kept).

Prints one JSON line; ``--out FILE`` also writes it there.

Usage (repo root, on an MI355X):  python tools/latent_tbptt_bench.py --steps 30 --warmup 5 --out profiles/latent_tbptt_bench.json
                                  python tools/latent_tbptt_bench.py --captured --parent-root DIR --out profiles/latent_tbptt_bench.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _root():
    """The tree whose packages this process imports: ``--root DIR`` (the legs of ``--captured``) or this file's own."""
    if "--root" in sys.argv[1:-1]:
        return os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
    return HERE


ROOT = _root()
for p in (ROOT, os.path.join(ROOT, "model-based-pde-control_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

B, T = 64, 20


def module_for(factory, n, dev):
    import pdecontrol.architectures as arch
    from pdecontrol.surrogates.training import PDETrainingModule
    torch.manual_seed(0)
    f = getattr(arch, factory)()
    sur = f.surrogate(delta=0.25, dscaling=None, tau=5, **f.model(N=n))
    m = PDETrainingModule(surrogate=sur, loss=torch.nn.MSELoss(reduction="none"), tstep=0.25, delta=0.25, tau=5, tbtt=10)
    m.split_graphs = False   # the launch-by-launch step
    return m.to(dev)


def batch_for(n, dev):
    g = torch.Generator().manual_seed(1)
    return ((torch.rand(B, T, 1, n, generator=g) * 2 - 1).to(dev), (torch.rand(B, T, 1, n, generator=g) * 2 - 1).to(dev))


def time_steps(module, batch, steps, warmup):
    opt = module.configure_optimizers()[0][0]

    def step(i):
        opt.zero_grad(set_to_none=True)
        out = module.training_step(batch, i)
        out["loss"].backward()
        opt.step()

    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        step(i)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps, type(opt).__name__


def time_fused_step(module, batch, steps, warmup):
    for _ in range(warmup):                 # the first call captures
        module.fused_step(batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        module.fused_step(batch)
    torch.cuda.synchronize()
    step = module.__dict__["_last_graphed_step"]
    return 1e3 * (time.perf_counter() - t0) / steps, "Adam in the flush" if step.adam_in_flush else "torch Adam in the graph"


def leg(kind, steps, warmup):
    """One route at both widths in this process; prints {"64": ms, "256": ms, "optimizer": ...}."""
    dev = torch.device("cuda", 0)
    out = {"root": ROOT}
    for n in (64, 256):
        module = module_for("KSLatentConvolutionalLSTMN", n, dev)
        ms, opt = (time_steps if kind == "eager" else time_fused_step)(module, batch_for(n, dev), steps, warmup)
        out[str(n)], out["optimizer"] = ms, opt
    print("LEG " + json.dumps(out))


def captured(args):
    routes = {"p": ("fused_step", os.path.abspath(args.parent_root)), "a": ("eager", HERE), "b": ("fused_step", HERE)}
    seen = {r: {"64": [], "256": []} for r in routes}
    optimizer = {}
    for _ in range(args.rounds):
        for r, (kind, root) in routes.items():
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", kind, "--steps", str(args.steps), "--warmup", str(args.warmup),
                   "--root", root]
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
            lines = [line for line in res.stdout.splitlines() if line.startswith("LEG ")]
            if res.returncode != 0 or not lines:
                raise SystemExit(f"route {r} failed ({res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}")
            got = json.loads(lines[-1][4:])
            assert os.path.samefile(got["root"], root), (got["root"], root)
            optimizer[r] = got["optimizer"]
            for n in ("64", "256"):
                seen[r][n].append(got[n])
    rec = {"what": "latent surrogate optimizer step, ms per step: p = fused_step of the parent commit, a = eager step, "
                   "b = captured latent step; one process per measurement, routes alternated",
           "B": B, "T": T, "tau": 5, "tbtt": 10, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "optimizer": optimizer, "rows": []}
    for n in ("64", "256"):
        row = {"N": int(n)}
        for r in routes:
            v = seen[r][n]
            row[r] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        gain = row["p"]["median"] - row["b"]["median"]
        spread = (row["p"]["max"] - row["p"]["min"]) + (row["b"]["max"] - row["b"]["min"])
        row["claim_b_below_p_by_more_than_both_ranges"] = "met" if gain > spread else "missed"
        row["gain_ms"], row["ranges_ms"] = round(gain, 4), round(spread, 4)
        rec["rows"].append(row)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--captured", action="store_true", help="the three-route comparison p / a / b")
    ap.add_argument("--parent-root", default=None, help="--captured: a checkout of the parent commit with its libraries built")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--leg", choices=("eager", "fused_step"), default=None, help="internal: one route of --captured")
    ap.add_argument("--root", default=None, help="internal: the tree a leg imports")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg, args.steps or 1000, args.warmup)
        return
    if args.captured:
        if not args.parent_root:
            ap.error("--captured needs --parent-root")
        args.steps = args.steps or 1000
        rec = {"captured_step": captured(args)}
    else:
        rec = default_record(args.steps or 30, args.warmup)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        if args.captured and os.path.exists(args.out):       # keep the eager record the file already holds
            try:
                rec = {**json.load(open(args.out)), **rec}
            except ValueError:
                pass
        with open(args.out, "w") as f:
            f.write(json.dumps(rec) + "\n")


def default_record(steps, warmup):
    from pdecontrol.surrogates import hipops, ops
    dev = torch.device("cuda", 0)
    rec = {"what": "latent surrogate TBPTT optimizer step (training_step + backward + optimizer.step), ms per step",
           "B": B, "T": T, "tau": 5, "tbtt": 10, "steps": steps, "warmup": warmup,
           "device": torch.cuda.get_device_name(dev), "rows": []}
    for n in (64, 256):
        batch = batch_for(n, dev)
        latent = module_for("KSLatentConvolutionalLSTMN", n, dev)
        assert ops.use_fused_latent_for(latent.surrogate, batch[0])
        ms, opt = time_steps(latent, batch, steps, warmup)
        rec["rows"].append({"N": n, "path": "latent fused", "ms_per_step": round(ms, 4), "optimizer": opt})
        with ops.fused(False):
            latent = module_for("KSLatentConvolutionalLSTMN", n, dev)
            ms, opt = time_steps(latent, batch, steps, warmup)
        rec["rows"].append({"N": n, "path": "latent plain PyTorch-ROCm (PDECONTROL_FUSED=0)", "ms_per_step": round(ms, 4),
                            "optimizer": opt})
        autoreg = module_for("KSAutoRegConvolutionalLSTMN", n, dev)
        assert hipops.fused_supported(autoreg.surrogate)
        ms, opt = time_steps(autoreg, batch, steps, warmup)
        rec["rows"].append({"N": n, "path": "autoreg fused eager (context)", "ms_per_step": round(ms, 4), "optimizer": opt})
    return rec


if __name__ == "__main__":
    main()
