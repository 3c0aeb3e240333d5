#!/usr/bin/env python3
"""ms per optimizer step of the delay-embedding surrogate (KSDelayCNNSurrogateFactory) at B = 64, T = 20, N = 64:
training_step + backward + the optimizer of configure_optimizers (torch Adam), on
  * fused       the whole-rollout HIP kernels (delay_hip.fused_delay_rollout per TBPTT chunk, loss in torch),
  * plain       the same step with the fused kernels switched off (ops.fused(False), the PDECONTROL_FUSED=0 switch),
plus one imagined world-env step: a 3-member PDEEnsemble rollout of 100 envs, one step from a carried context (what
WorldVecEnv.step asks of the ensemble), no grad.  Every shape is warmed up and the device synchronised before the clock
is read.  Record only.  Prints one JSON line; ``--out FILE`` also writes it there.

Usage (repo root, on an MI355X):  python tools/delay_tbptt_bench.py --steps 20 --warmup 3 --out profiles/delay_tbptt_bench.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "model-based-pde-control_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def module_for(dev, seed=0):
    import pdecontrol.architectures as arch
    from pdecontrol.surrogates.training import PDETrainingModule
    torch.manual_seed(seed)
    f = arch.KSDelayCNNSurrogateFactory()
    sur = f.surrogate(delta=0.25, dscaling=None, tau=5, **f.model())
    return PDETrainingModule(surrogate=sur, loss=torch.nn.MSELoss(reduction="none"), tstep=0.25, delta=0.25, tau=5,
                             tbtt=10).to(dev)


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


def time_world_step(dev, steps, warmup):
    from pdecontrol.surrogates.surrogate import PDEEnsemble
    members = [module_for(dev, seed) for seed in range(3)]
    ens = PDEEnsemble(members, num_elites=3)
    g = torch.Generator().manual_seed(2)
    states = (torch.rand(100, 1, 1, 64, generator=g) * 2 - 1).to(dev)
    actions = (torch.rand(100, 1, 1, 4, generator=g) * 2 - 1).to(dev)
    times, targets = torch.zeros(1), torch.full((1,), 0.25)
    with torch.no_grad():
        ro = ens.rollout(states, actions, times, targets)
        hidden = ro.hidden
        for _ in range(warmup):
            ens.rollout(states, actions, times, targets, hidden=hidden)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            ens.rollout(states, actions, times, targets, hidden=hidden)
        torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pdecontrol.surrogates import ops
    dev = torch.device("cuda", 0)
    b, t = 64, 20
    rec = {"what": "delay surrogate TBPTT optimizer step (training_step + backward + optimizer.step), ms per step; "
                   "world: 3-member ensemble one-step rollout of 100 envs, ms per step",
           "B": b, "T": t, "tau": 5, "tbtt": 10, "N": 64, "steps": args.steps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(dev), "rows": []}
    g = torch.Generator().manual_seed(1)
    batch = ((torch.rand(b, t, 1, 64, generator=g) * 2 - 1).to(dev), (torch.rand(b, t, 1, 4, generator=g) * 2 - 1).to(dev))
    m = module_for(dev)
    assert ops.use_fused_delay_for(m.surrogate, batch[0])
    ms, opt = time_steps(m, batch, args.steps, args.warmup)
    rec["rows"].append({"path": "delay fused", "ms_per_step": round(ms, 4), "optimizer": opt})
    with ops.fused(False):
        ms_plain, opt = time_steps(module_for(dev), batch, max(3, args.steps // 4), 1)
    rec["rows"].append({"path": "delay plain PyTorch-ROCm (PDECONTROL_FUSED=0)", "ms_per_step": round(ms_plain, 4),
                        "optimizer": opt})
    rec["speedup_fused_vs_plain"] = round(ms_plain / ms, 2)
    rec["rows"].append({"path": "world step fused (3 members x 100 envs, one-step rollout)",
                        "ms_per_step": round(time_world_step(dev, args.steps, args.warmup), 4)})
    with ops.fused(False):
        rec["rows"].append({"path": "world step plain PyTorch-ROCm (3 members x 100 envs)",
                            "ms_per_step": round(time_world_step(dev, max(3, args.steps // 4), 1), 4)})
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
