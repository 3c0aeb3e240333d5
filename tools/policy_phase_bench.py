#!/usr/bin/env python3
"""Timings of the controller's policy-update phase on an MI355X (pdecontrol/mbrl/policy_phase.py).  Record only.

The replay pair is a controller's: ``--imagined`` (32 000) imagined transitions in episodes of 50 steps and ``--real``
(4 000) real ones in episodes of 250, N = 64 observations, 4 actions, with the controller's two connectors (observations
scaled by running extrema, actions mapped from their bounds to [-1, 1]).  The agent is the SAC agent of tools/sac_bench.py
(hidden 256, automatic entropy tuning, no logger).  B = 256.  Three routes, alternated over ``--rounds`` rounds in one
process, every route warmed up, every window between two device synchronisations:

  (a) loader        the reference's ``DataLoader`` / ``RandomSampler`` / ``ConcatDataset`` feeding ``agent.update`` on the
                    GPU: the route of the parent commit.  ``--loader-updates`` (10) updates per window.
  (b) update_many   ``agent.update_many`` over ``--updates`` (200) batches already on the device: the floor without any
                    sampling (five device-to-device copies, two noise draws and one graph replay per update).
  (c) phase         ``update_policy`` for ``--updates`` updates; its plan time, its pack time (packing both replays into
                    HBM and uploading the rows) and the time of its updates are listed separately, and the device time of
                    ``rp_gather`` alone is taken with events around ``--updates`` launches.

(c) is judged against (b): the updates of (c) may take, per update, at most (b) plus the ``rp_gather`` device time plus
the spread (max - min over the rounds) of (b).  The record says whether they do, and by how much they miss otherwise.

  --profile-run   one warmed-up phase and nothing else: the program to put behind ``rocprofv3 --kernel-trace --stats``

Usage (repo root, on an MI355X):  python tools/policy_phase_bench.py    (writes profiles/policy_phase_bench.json)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "model-based-pde-control_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

B, N, A = 256, 64, 4
LOW, HIGH = -2.0, 1.0


def replay(steps, nenv, episode, seed):
    from pdecontrol.mbrl.replay import ExperienceReplay
    from pdecontrol.mbrl.types import Sample
    rs = np.random.RandomState(seed)
    rp = ExperienceReplay()
    x = np.linspace(0, 2 * np.pi, N, endpoint=False)
    for t in range(steps // nenv):
        fields = rs.uniform(-1, 1, (nenv, 2, 1, 1)) * np.sin(x + rs.uniform(0, 6, (nenv, 2, 1, 1)))
        done = (t + 1) % episode == 0
        rp.add([Sample(fields[e, 0].astype(np.float32), rs.uniform(LOW, HIGH, (1, A)).astype(np.float32),
                       fields[e, 1].astype(np.float32), np.float32(-rs.uniform(0.01, 0.99)), False, done,
                       np.int32(t % episode + 1)) for e in range(nenv)])
    return rp


def datasets_for(imagined, real):
    from pdecontrol.surrogates.common.dataset import SubSeqDataset
    from pdegym.common.transforms import BatchTransform, ScaleTransform, SensorTransform, SampleTransform
    oscaling = ScaleTransform(batched=True, aggregate=True, frozen=False)
    oscaling.update(np.random.RandomState(5).uniform(-1.2, 1.2, (16, 1, N)).astype(np.float32))
    bounds = (np.full((1, 1, A), LOW, np.float32), np.full((1, 1, A), HIGH, np.float32))
    ascaling = ScaleTransform(bounds=bounds, aggregate=True, frozen=True, batched=True).Inverse
    replay_to_agent = SampleTransform(otransf=[oscaling, BatchTransform(SensorTransform(stride=1))], atransf=ascaling.Inverse)
    world_replay_to_agent = SampleTransform(atransf=ascaling.Inverse)
    make = lambda rp, stransf: SubSeqDataset(data=rp.data, length=1, stride=1, bootstrapping=False, stransf=stransf)
    return [make(replay(imagined, 32, 50, 1), world_replay_to_agent), make(replay(real, 8, 250, 2), replay_to_agent)]


def loader_for(datasets, updates):
    from torch.utils.data import ConcatDataset, DataLoader, RandomSampler
    from pdecontrol.surrogates.common.dataset import PDEDataLoader
    data = ConcatDataset(tuple(datasets))
    sampler = RandomSampler(data, replacement=True, num_samples=B * updates)
    return DataLoader(dataset=data, batch_size=B, shuffle=False, sampler=sampler, collate_fn=PDEDataLoader.sample_collate)


def timed(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--loader-updates", type=int, default=10)
    ap.add_argument("--imagined", type=int, default=32000)
    ap.add_argument("--real", type=int, default=4000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_phase_bench.json"))
    ap.add_argument("--profile-run", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    from sac_bench import agent_on
    from pdecontrol.mbrl import policy_phase as pp, replay_hip
    from pdecontrol.sac import sac_hip
    from pdecontrol.surrogates.common.dataset import DeviceSubSeqStore

    U = args.updates
    datasets = datasets_for(args.imagined, args.real)
    agents = {name: agent_on(dev) for name in ("loader", "update_many", "phase")}
    torch.manual_seed(1)
    if args.profile_run:
        pp.update_policy(agents["phase"], datasets, B, 20)
        pp.update_policy(agents["phase"], datasets, B, U)
        torch.cuda.synchronize()
        return

    # batches of (b): the phase's own samples, assembled on the device ahead of the timed windows
    plan = pp.PolicyBatchPlan(datasets, B, U)
    stores = [DeviceSubSeqStore(d.fields, dev) for d in datasets]
    stacked = list(pp.device_batches(plan, stores))

    def route_a():
        for batch in loader_for(datasets, args.loader_updates):
            agents["loader"].update(batch)

    routes = {"a_loader": route_a,
              "b_update_many": lambda: agents["update_many"].update_many(stacked),
              "c_phase": None}
    # warm-up: code objects, the captured graphs of (b) and (c), the allocator
    route_a()
    agents["update_many"].update_many(stacked[:10])
    pp.update_policy(agents["phase"], datasets, B, 10)
    torch.cuda.synchronize()

    ms = {"a_loader": [], "b_update_many": [], "c_phase_whole": [], "c_phase_updates": []}
    plan_ms, pack_ms, tiers = [], [], set()
    for _ in range(args.rounds):
        for name, call in routes.items():
            if name == "a_loader":
                ms[name].append(1e3 * timed(call)[0] / args.loader_updates)
            elif name == "b_update_many":
                ms[name].append(1e3 * timed(call)[0] / U)
            else:
                timings = {}
                whole, _ = timed(lambda: pp.update_policy(agents["phase"], datasets, B, U, timings=timings))
                ms["c_phase_whole"].append(1e3 * whole / U)
                ms["c_phase_updates"].append(1e3 * timings["updates_s"] / U)
                plan_ms.append(1e3 * timings["plan_s"])
                pack_ms.append(1e3 * timings["pack_s"])
                tiers.add(timings["tier"])
    assert tiers == {"kernel"}, tiers

    # rp_gather alone: device time per launch, events around U launches into the static buffers of the captured update
    tier = pp._KernelTier(plan, [pp._connector(d) for d in datasets], dev)
    graph = agents["phase"]._fused.graph_for((B, (1, A)))
    gather = lambda u: replay_hip.gather(sac_hip._stream(), tier.srcs, B, tier.rows.data_ptr() + u * B * 8, graph.obs,
                                         graph.actions, graph.nxtobs, graph.rewards, graph.terminated)
    for u in range(10):
        gather(u)
    gather_ms = []
    for _ in range(args.rounds):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for u in range(U):
            gather(u)
        end.record()
        torch.cuda.synchronize()
        gather_ms.append(start.elapsed_time(end) / U)

    med = lambda v: round(float(np.median(v)), 4)
    a, b, c, c_whole, g = med(ms["a_loader"]), med(ms["b_update_many"]), med(ms["c_phase_updates"]), med(ms["c_phase_whole"]), med(gather_ms)
    spread_b = round(max(ms["b_update_many"]) - min(ms["b_update_many"]), 4)
    allowed = round(b + g + spread_b, 4)
    rec = {"what": "policy-update phase, SAC agent (hidden 256, 64 observations, 4 actions, automatic entropy tuning, no "
                   "logger), B = 256: ms per update of (a) the reference's host loader feeding agent.update on the GPU, (b) "
                   "update_many over batches already on the device, (c) update_policy on the kernel tier; routes alternated "
                   "in one process, medians over the rounds; host clock around work ending in a device synchronisation",
           "device": torch.cuda.get_device_name(dev), "B": B, "updates_per_phase": U, "loader_updates_per_window": args.loader_updates,
           "rounds": args.rounds, "imagined_steps": int(len(datasets[0])), "real_steps": int(len(datasets[1])),
           "ms_per_update": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "a_loader_ms": a, "b_update_many_ms": b, "c_phase_updates_ms": c, "c_phase_whole_ms": c_whole,
           "c_plan_ms_per_phase": med(plan_ms), "c_pack_ms_per_phase": med(pack_ms),
           "c_updates_ms_per_phase": round(c * U, 3),
           "rp_gather_device_ms_per_launch": g, "rp_gather_device_ms_rounds": [round(x, 5) for x in gather_ms],
           "speedup_c_updates_vs_a": round(a / c, 1), "speedup_c_whole_vs_a": round(a / c_whole, 1),
           "b_spread_ms": spread_b, "c_allowed_ms": allowed, "c_within_floor_plus_gather_plus_spread": bool(c <= allowed),
           "c_over_allowed_ms": round(max(0.0, c - allowed), 4)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
