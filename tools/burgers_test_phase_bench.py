#!/usr/bin/env python3
"""Timings of the surrogate test phase on a Burgers env (pdecontrol.surrogates.test_phase.test_surrogate) on an MI355X.
Record only: the parent of this tool's commit could run neither tier on this env, so the torch tier is the yardstick.

Shape: one batch, N = 512, B = 128, T = 35 steps, a ``BurgersFNO`` surrogate with seeded random weights under the
controller's connector (a frozen ``ScaleTransform`` observation scaling, actions forced to full width and scaled),
``env = BurgersBatchedVecEnv(1, N=512)``.

  kernel   the epoch on the kernel tier: the fused rollout plus bg_eval_rows and bg_eval_fold into the device accumulator,
           one copy of 1 + 20 T doubles (and the kept sequences) at the end
  torch    ``tier="torch"``: ``test_step``'s host lines (copies to the CPU, 2 B T ``reward_func`` calls, two round trips
           through ``env.rhs``, some forty torch CPU reductions)
  rollout  the fused rollout of the batch alone, for the share of the metric section in either epoch

Two warm-up calls of every path, then the paths alternated over ``--rounds`` rounds, one call a round; the host clock
around a device synchronisation; every round, the median and the range are reported.

  --parity FILE.jsonl  collect the records tests/test_bg_eval_gpu.py appends (largest deviations of the module's kernel
                       tier from the fp64 restatement and of the torch tier from the kernel tier, per table family) into
                       ``--out`` (profiles/burgers_test_phase_parity.json)

Usage (repo root, on an MI355X):  python tools/burgers_test_phase_bench.py --out profiles/burgers_test_phase_bench.json
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

N, B, T, TAU = 512, 128, 35, 5


def build(dev):
    from pdecontrol.architectures.fno import BurgersFNO
    from pdecontrol.surrogates.training import PDETrainingModule
    from pdegym.burgers import BurgersBatchedVecEnv
    from pdegym.common import transforms as tr
    env = BurgersBatchedVecEnv(1, N=N, device=dev.index)
    tstep = env.cfg_steps * env.dt
    # the controller's connector (pdecontrol/mbrl/mbrl.py:146-187) with fixed bounds
    oscaling = tr.ScaleTransform(bounds=(np.full((1, 1, 1), -3.0, np.float32), np.full((1, 1, 1), 3.0, np.float32)),
                                 batched=True, aggregate=True, frozen=True)
    forcing = tr.BatchTransform(env.forcing)
    low = np.asarray(env.single_action_space.low)[np.newaxis, ...]
    high = np.asarray(env.single_action_space.high)[np.newaxis, ...]
    lo, hi = np.squeeze(forcing(low), axis=0), np.squeeze(forcing(high), axis=0)
    pdescaling = tr.BatchTransform(tr.ScaleTransform(bounds=(lo, hi), scale=(-1, 1), aggregate=True, frozen=True))
    sensor = tr.BatchTransform(tr.SensorTransform(stride=1))
    stransf = tr.SampleTransform([oscaling, sensor], [forcing, pdescaling, sensor])
    g = torch.Generator().manual_seed(0)
    x = torch.linspace(0, 2 * np.pi, N + 1)[:-1]
    raw = sum(torch.rand(B * T, 1, 1, generator=g) / (k + 1) * torch.sin((k + 1) * x + 6 * torch.rand(B * T, 1, 1, generator=g))
              for k in range(4))
    raw_actions = 2 * torch.rand(B * T, 1, 4, generator=g) - 1
    states = stransf.otransf(raw).reshape(B, T, 1, N)
    actions = stransf.atransf(raw_actions).reshape(B, T, 1, N)
    torch.manual_seed(0)
    f = BurgersFNO()
    sur = f.surrogate(delta=tstep, dscaling=None, tau=TAU, **f.model())
    module = PDETrainingModule(surrogate=sur, loss=torch.nn.MSELoss(reduction="none"), tstep=tstep, delta=tstep, env=env,
                               stransf=stransf, tau=TAU, tbtt=10).to(dev)
    return module, [(states.to(dev), actions.to(dev))]


def timed(call):
    """ms of one call between two device synchronisations, on the host clock."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def collect_parity(path, out):
    rows = [json.loads(line) for line in open(path) if line.strip()]
    fields = ("largest_relative_deviation_kernel_tier_vs_fp64_restatement",
              "largest_deviation_over_largest_entry_torch_tier_vs_kernel_tier")
    worst = {field: {} for field in fields}
    for r in rows:
        for field in fields:
            for family, val in r[field].items():
                worst[field][family] = max(worst[field].get(family, 0.0), float(val))
    rec = {"what": "largest deviations that tests/test_bg_eval_gpu.py::test_test_step_on_a_burgers_env observed on gfx950, per "
                   "table family (MSE, states, rewards, derivatives): the fp32 tables of test_step's kernel tier (bg_eval_rows + "
                   "bg_eval_fold) against the fp64 numpy restatement applied to the returned rows, relative, bound rtol 1e-6; "
                   "and the torch tier (ops.fused(False)) against the kernel tier, over the table's largest entry, bound rtol "
                   "2e-4, atol 2e-5",
           "shape": rows[-1]["shape"] if rows else None, "records": len(rows), "bars": rows[-1]["bars"] if rows else None,
           **worst}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(worst))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parity", default=None)
    args = ap.parse_args()
    if args.parity:
        return collect_parity(args.parity, args.out or os.path.join(ROOT, "profiles", "burgers_test_phase_parity.json"))
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    from pdecontrol.surrogates import test_phase
    module, loader = build(dev)

    def rollout():
        with torch.no_grad():
            for s, a in loader:
                module._full_rollout(s, a)

    reports = {}

    def epoch(tier):
        reports[tier] = test_phase.test_surrogate(module, dataloaders=loader, tier=tier)

    paths = {"kernel": lambda: epoch("kernel"), "torch": lambda: epoch("torch"), "rollout": rollout}
    for call in paths.values():
        for _ in range(2):                                              # two warm-up calls each
            call()
    ms = {name: [] for name in paths}
    for _ in range(args.rounds):
        for name, call in paths.items():
            ms[name].append(round(timed(call), 4))
    rec = {"what": "surrogate test phase on a Burgers env, BurgersFNO with random weights, one batch of N = 512, B = 128, "
                   "T = 35, ScaleTransform observations, l2control: ms per call of test_surrogate on the kernel tier "
                   "(bg_eval_rows + bg_eval_fold), on tier='torch' (test_step's host lines) and of the fused rollout alone; two "
                   "warm-up calls, paths alternated, host clock around a device synchronisation; every round, the median and "
                   "the range",
           "N": N, "B": B, "T": T, "rounds": args.rounds, "device": torch.cuda.get_device_name(dev),
           "ms_per_batch": {k: {"rounds": v, "median": round(float(np.median(v)), 4), "min": min(v), "max": max(v)}
                            for k, v in ms.items()}}
    med = {k: rec["ms_per_batch"][k]["median"] for k in ms}
    rec["metric_section_ms_per_batch"] = {"kernel": round(med["kernel"] - med["rollout"], 4),
                                          "torch": round(med["torch"] - med["rollout"], 4)}
    k, t = reports["kernel"], reports["torch"]
    assert (k.tier, t.tier) == ("kernel", "torch")
    # both tiers computed the same epoch: the largest difference over the largest entry of the torch tier's table
    rec["tiers_agree_to"] = max(float(np.nanmax(np.abs(k.tables[n] - t.tables[n])) / np.nanmax(np.abs(t.tables[n])))
                                for n in t.tables)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
