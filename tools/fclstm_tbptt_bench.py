#!/usr/bin/env python3
"""ms per optimizer step of the two fully-connected LSTM baselines (KSAutoRegFullyConnectedLSTM, KSLatentLSTM) at B = 64,
T = 20, tau = 5, tbtt = 10, N = 64: training_step + backward + the optimizer of configure_optimizers (torch Adam), on
  * on    the whole-rollout HIP kernels (ops.fused_fc(True): fclstm_hip.fused_fc_rollout per TBPTT chunk, loss in torch),
  * off   the same step of the same process with the switch off (the default: plain PyTorch-ROCm kernels),
each as five repeated medians over ``--steps`` individually timed steps (the legs alternate, repeat by repeat), with the
min-max spread of the five; the device kernel launches of one step of either leg (torch.profiler); plus one imagined
world-env step: a 3-member PDEEnsemble rollout of 100 rows, one step from a carried hidden state, no grad.  Every shape is
warmed up and the device synchronised before the clock is read.  Record only.  Prints one JSON line; ``--out FILE`` also
writes it there.

``--parity LOG`` does not run anything on the GPU: it folds the per-case figures tests/test_fclstm_surrogate_gpu.py appended
to LOG (fclstm_parity_observed.jsonl next to the gradient parity log of tests/conftest.py, one run of ``pytest -m gpu`` on
that file) into ``--out``.

Usage (repo root, on an MI355X):  python tools/fclstm_tbptt_bench.py --steps 20 --warmup 3 --out profiles/fclstm_tbptt_bench.json
                                  python tools/fclstm_tbptt_bench.py --parity LOG --out profiles/fclstm_parity_observed.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "model-based-pde-control_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

FACTORIES = ("KSAutoRegFullyConnectedLSTM", "KSLatentLSTM")
REPEATS = 5


def module_for(factory, dev, seed=0):
    import pdecontrol.architectures as arch
    from pdecontrol.surrogates.training import PDETrainingModule
    torch.manual_seed(seed)
    f = getattr(arch, factory)()
    sur = f.surrogate(delta=0.25, dscaling=None, tau=5, **f.model())
    return PDETrainingModule(surrogate=sur, loss=torch.nn.MSELoss(reduction="none"), tstep=0.25, delta=0.25, tau=5,
                             tbtt=10).to(dev)


class Stepper:
    def __init__(self, module, batch):
        self.module, self.batch = module, batch
        self.opt = module.configure_optimizers()[0][0]

    def step(self, i=0):
        self.opt.zero_grad(set_to_none=True)
        out = self.module.training_step(self.batch, i)
        out["loss"].backward()
        self.opt.step()

    def median_ms(self, steps):
        times = []
        for i in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            self.step(i)
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(times)

    def launches(self):
        """Device kernel launches of one optimizer step, or None where the profiler is not available."""
        try:
            from torch.profiler import ProfilerActivity, profile
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                self.step()
                torch.cuda.synchronize()
            return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        except Exception:          # record only: the count is a courtesy, the timings are the record
            return None


def time_world_step(factory, dev, steps, warmup):
    from pdecontrol.surrogates.surrogate import PDEEnsemble
    ens = PDEEnsemble([module_for(factory, dev, seed) for seed in range(3)], num_elites=3)
    g = torch.Generator().manual_seed(2)
    states = (torch.rand(100, 1, 1, 64, generator=g) * 2 - 1).to(dev)
    actions = (torch.rand(100, 1, 1, 4, generator=g) * 2 - 1).to(dev)
    times, targets = torch.zeros(1), torch.full((1,), 0.25)
    with torch.no_grad():
        hidden = ens.rollout(states, actions, times, targets).hidden
        for _ in range(warmup):
            ens.rollout(states, actions, times, targets, hidden=hidden)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            ens.rollout(states, actions, times, targets, hidden=hidden)
        torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def fold_parity(log, out):
    rows = [json.loads(line) for line in open(log) if line.strip()]
    fwd, grad = "forward_err_of_scale", "gradient_err_of_scale"
    worst = lambda key, who: max(r[key][who] for r in rows)
    ratio = lambda key: max(r[key]["kernels"] / r[key]["fp32_cpu"] for r in rows)
    doc = {"what": "tests/test_fclstm_surrogate_gpu.py::test_fc_rollout_forward_and_gradients on an MI355X: per case, the "
                   "largest error of the sur_fc_* kernels and of fp32 PyTorch on the CPU against the same module in fp64 on "
                   "the CPU; forward: max |x - ref| / max(1, max |ref|) over every returned tensor; gradient: max |g - ref| / "
                   "max |ref| over every input and parameter gradient",
           "bars": {"forward_atol_of_scale": 2e-5, "forward_rtol": 2e-4, "gradient_of_scale": 2e-4},
           "max": {"forward": {"kernels": worst(fwd, "kernels"), "fp32_cpu": worst(fwd, "fp32_cpu")},
                   "gradient": {"kernels": worst(grad, "kernels"), "fp32_cpu": worst(grad, "fp32_cpu")}},
           "max_ratio_kernels_over_fp32_cpu": {"forward": ratio(fwd), "gradient": ratio(grad)},
           "cases": rows}
    text = json.dumps(doc, indent=1) + "\n"
    if out:
        with open(out, "w") as f:
            f.write(text)
    print(json.dumps({k: doc[k] for k in ("max", "max_ratio_kernels_over_fp32_cpu")}), f"({len(rows)} cases)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parity", default=None, metavar="LOG")
    args = ap.parse_args()
    if args.parity:
        fold_parity(args.parity, args.out)
        return
    from pdecontrol.surrogates import ops
    dev = torch.device("cuda", 0)
    b, t = 64, 20
    rec = {"what": "FC-LSTM surrogate TBPTT optimizer step (training_step + backward + optimizer.step), ms per step: five "
                   "medians per leg, switch on (whole-rollout HIP kernels) and off (plain PyTorch-ROCm) in one process; "
                   "world: 3-member ensemble one-step rollout of 100 rows from a carried hidden state, ms per step",
           "B": b, "T": t, "tau": 5, "tbtt": 10, "N": 64, "steps": args.steps, "warmup": args.warmup, "repeats": REPEATS,
           "device": torch.cuda.get_device_name(dev), "rows": []}
    g = torch.Generator().manual_seed(1)
    batch = ((torch.rand(b, t, 1, 64, generator=g) * 2 - 1).to(dev), (torch.rand(b, t, 1, 4, generator=g) * 2 - 1).to(dev))
    for factory in FACTORIES:
        legs = {True: Stepper(module_for(factory, dev), batch), False: Stepper(module_for(factory, dev), batch)}
        medians, launches = {True: [], False: []}, {}
        for flag, leg in legs.items():
            with ops.fused_fc(flag):
                assert ops.use_fused_fc_for(leg.module.surrogate, batch[0]) == flag
                for i in range(args.warmup):
                    leg.step(i)
        for _ in range(REPEATS):
            for flag, leg in legs.items():
                with ops.fused_fc(flag):
                    medians[flag].append(leg.median_ms(args.steps))
        for flag, leg in legs.items():
            with ops.fused_fc(flag):
                launches[flag] = leg.launches()
        on, off = medians[True], medians[False]
        row = {"factory": factory, "optimizer": type(legs[True].opt).__name__,
               "on_ms_medians": [round(x, 4) for x in on], "off_ms_medians": [round(x, 4) for x in off],
               "on_ms": round(statistics.median(on), 4), "off_ms": round(statistics.median(off), 4),
               "on_spread_ms": round(max(on) - min(on), 4), "off_spread_ms": round(max(off) - min(off), 4),
               "margin_ms": round(min(off) - max(on), 4),
               "speedup_on_vs_off": round(statistics.median(off) / statistics.median(on), 2),
               "launches_per_step_on": launches[True], "launches_per_step_off": launches[False]}
        with ops.fused_fc(True):
            row["world_step_on_ms"] = round(time_world_step(factory, dev, args.steps, args.warmup), 4)
        with ops.fused_fc(False):
            row["world_step_off_ms"] = round(time_world_step(factory, dev, args.steps, args.warmup), 4)
        rec["rows"].append(row)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
