#!/usr/bin/env python3
"""Timings of the surrogate test phase (pdecontrol.surrogates.test_phase.test_surrogate) on an MI355X.  Record only.

Shape: the offline evaluation's own -- ``KSAutoRegConvolutionalLSTM``, N = 64, B = 128, T = tau + target_length = 35
steps, 8 batches an epoch, observations through a fitted ``Normalize``, the l2control reward of the default env.

  kernel   the epoch on the kernel tier: per batch the fused rollout plus ks_eval_rows_device and ks_eval_fold_device into
           one device accumulator, one copy of 1 + 25 T doubles (and the kept sequences) at the end
  torch    ``tier="torch"``: the loop over ``test_step``'s host lines -- the lines the module ran before the kernel tier
           existed (copies to the CPU, 2 B T ``reward_func`` calls, two round trips through the ``ks_rhs`` hook, some forty
           torch CPU reductions)
  rollout  the fused rollout of the 8 batches alone, for the share of the metric section in either epoch

Every path is warmed up by one epoch; the paths are alternated over ``--rounds`` rounds; a kernel or rollout window
repeats its epoch until it lasts ``--min-seconds``; every window ends in a device synchronisation.  ms per batch =
window / batches; all rounds and the median are reported.

  --parity FILE.jsonl  collect the records tests/_eval_rows_cases.py appends (largest deviation from the recorded
                       fixture) into ``--out`` (profiles/test_phase_parity_observed.json)

Usage (repo root, on an MI355X):  python tools/test_phase_bench.py --out profiles/test_phase_bench.json
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

N, B, T, BATCHES, TAU = 64, 128, 35, 8, 5


def build(dev):
    from pdecontrol.architectures import KSAutoRegConvolutionalLSTM
    from pdecontrol.surrogates.training import PDETrainingModule
    from pdegym.common import transforms as tr
    from pdegym.kuramoto import KuramotoSivashinskyEnv
    env = KuramotoSivashinskyEnv()
    g = torch.Generator().manual_seed(0)
    x = torch.linspace(0, 2 * np.pi, N + 1)[:-1]
    raw = sum(2.0 * torch.rand(BATCHES * B, T, 1, 1, generator=g) * torch.sin((k + 1) * x + 6 * torch.rand(BATCHES * B, T, 1, 1, generator=g))
              for k in range(3))
    raw_actions = 2 * torch.rand(BATCHES * B, T, 1, 4, generator=g) - 1
    oscaling, pdescaling = tr.Normalize(aggregate=True, batched=True), tr.Normalize(aggregate=True, batched=True)
    forcing = tr.BatchTransform(env.forcing)
    oscaling.update(raw.reshape(-1, 1, N))
    pdescaling.update(forcing(raw_actions.reshape(-1, 1, 4)))
    stransf = tr.SampleTransform(oscaling, tr.Operation([forcing, pdescaling]))
    states = stransf.otransf(raw.reshape(-1, 1, N)).reshape(BATCHES, B, T, 1, N)
    actions = stransf.atransf(raw_actions.reshape(-1, 1, 4)).reshape(BATCHES, B, T, 1, N)
    torch.manual_seed(0)
    f = KSAutoRegConvolutionalLSTM()
    sur = f.surrogate(delta=0.25, dscaling=None, tau=TAU, **f.model())
    module = PDETrainingModule(surrogate=sur, loss=torch.nn.MSELoss(reduction="none"), tstep=0.25, delta=0.25, env=env,
                               stransf=stransf, tau=TAU, tbtt=10).to(dev)
    loader = [(states[i].to(dev), actions[i].to(dev)) for i in range(BATCHES)]
    return module, loader


def window(call, min_seconds):
    """(ms per call, calls) over one window of at least ``min_seconds`` that ends in a device synchronisation."""
    n = 1
    while True:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            call()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return 1e3 * dt / n, n
        n = max(2 * n, int(1.3 * n * min_seconds / max(dt, 1e-6)))


def collect_parity(path, out):
    rows = [json.loads(line) for line in open(path) if line.strip()]
    worst = {}
    for r in rows:
        for name, val in r["largest_deviation_over_largest_reference_entry"].items():
            key = r["label"] + ":" + name
            worst[key] = max(worst.get(key, 0.0), float(val))
    rec = {"what": "largest |value - reference| over the table's largest reference entry that tests/_eval_rows_cases.py::"
                   "check_fixture_case observed for the MSE and the 25 per-step tables of ks_eval_rows_device + "
                   "ks_eval_fold_device against tests/golden/evalstep_golden.npz (the reference's own test_step; bound: rtol "
                   "2e-5, atol 2e-5 of that entry), on the CPU twin and on gfx950",
           "worst_per_label": {label: max(v for k, v in worst.items() if k.startswith(label + ":")) for label in
                               sorted({r["label"] for r in rows})},
           "worst": worst}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["worst_per_label"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parity", default=None)
    args = ap.parse_args()
    if args.parity:
        return collect_parity(args.parity, args.out or os.path.join(ROOT, "profiles", "test_phase_parity_observed.json"))
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
        call()                                                          # warm-up: one epoch each
    ms = {name: [] for name in paths}
    for _ in range(args.rounds):
        for name, call in paths.items():
            t, _n = window(call, 0.0 if name == "torch" else args.min_seconds)      # a torch epoch is seconds long
            ms[name].append(round(t / BATCHES, 4))
    rec = {"what": "surrogate test phase, KSAutoRegConvolutionalLSTM, N = 64, B = 128, T = 35, 8 batches an epoch, Normalize "
                   "observations, l2control: ms per batch of test_surrogate on the kernel tier, on tier='torch' (the host "
                   "lines test_step ran before the kernel tier) and of the fused rollout alone; paths alternated, every "
                   "round and the median reported",
           "N": N, "B": B, "T": T, "batches": BATCHES, "rounds": args.rounds, "min_seconds_per_window": args.min_seconds,
           "device": torch.cuda.get_device_name(dev),
           "ms_per_batch": {k: {"rounds": v, "median": round(float(np.median(v)), 4), "min": min(v), "max": max(v)}
                            for k, v in ms.items()}}
    med = {k: rec["ms_per_batch"][k]["median"] for k in ms}
    rec["torch_over_kernel"] = round(med["torch"] / med["kernel"], 1)
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
