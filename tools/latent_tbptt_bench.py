#!/usr/bin/env python3
"""ms per optimizer step of the latent ConvLSTM surrogate (KSLatentConvolutionalLSTM / ...N) at B = 64, T = 20, N = 64 and
256: training_step + backward + the optimizer of configure_optimizers (torch Adam), on
  * fused       the fused HIP kernels (hipops.fused_latent_rollout per TBPTT chunk, loss in torch),
  * plain       the same step with the fused kernels switched off (ops.fused(False), the PDECONTROL_FUSED=0 switch),
  * autoreg     for context, the autoregressive KSAutoRegConvolutionalLSTM's launch-by-launch fused step (split graphs off,
                PackAdam) at the same shape.
Record only: there is no target.  Prints one JSON line; ``--out FILE`` also writes it there.

Usage (repo root, on an MI355X):  python tools/latent_tbptt_bench.py --steps 30 --warmup 5 --out profiles/latent_tbptt_bench.json
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


def module_for(factory, n, dev):
    import pdecontrol.architectures as arch
    from pdecontrol.surrogates.training import PDETrainingModule
    torch.manual_seed(0)
    f = getattr(arch, factory)()
    sur = f.surrogate(delta=0.25, dscaling=None, tau=5, **f.model(N=n))
    m = PDETrainingModule(surrogate=sur, loss=torch.nn.MSELoss(reduction="none"), tstep=0.25, delta=0.25, tau=5, tbtt=10)
    m.split_graphs = False   # the launch-by-launch step (the latent model has no captured step)
    return m.to(dev)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pdecontrol.surrogates import hipops, ops
    dev = torch.device("cuda", 0)
    b, t = 64, 20
    rec = {"what": "latent surrogate TBPTT optimizer step (training_step + backward + optimizer.step), ms per step",
           "B": b, "T": t, "tau": 5, "tbtt": 10, "steps": args.steps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(dev), "rows": []}
    for n in (64, 256):
        g = torch.Generator().manual_seed(1)
        batch = ((torch.rand(b, t, 1, n, generator=g) * 2 - 1).to(dev), (torch.rand(b, t, 1, n, generator=g) * 2 - 1).to(dev))
        latent = module_for("KSLatentConvolutionalLSTMN", n, dev)
        assert ops.use_fused_latent_for(latent.surrogate, batch[0])
        ms, opt = time_steps(latent, batch, args.steps, args.warmup)
        rec["rows"].append({"N": n, "path": "latent fused", "ms_per_step": round(ms, 4), "optimizer": opt})
        with ops.fused(False):
            latent = module_for("KSLatentConvolutionalLSTMN", n, dev)
            ms, opt = time_steps(latent, batch, args.steps, args.warmup)
        rec["rows"].append({"N": n, "path": "latent plain PyTorch-ROCm (PDECONTROL_FUSED=0)", "ms_per_step": round(ms, 4),
                            "optimizer": opt})
        autoreg = module_for("KSAutoRegConvolutionalLSTMN", n, dev)
        assert hipops.fused_supported(autoreg.surrogate)
        ms, opt = time_steps(autoreg, batch, args.steps, args.warmup)
        rec["rows"].append({"N": n, "path": "autoreg fused eager (context)", "ms_per_step": round(ms, 4), "optimizer": opt})
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
