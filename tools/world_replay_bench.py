#!/usr/bin/env python3
"""Timings of whole controller iterations ``world_replay.resize -> imagine -> world_replay.extend -> update_policy`` on an
MI355X, with the imagined experience on the host and in HBM (pdecontrol/mbrl/device_replay.py).  Record only.

The workload joins those of tools/imagination_phase_bench.py and tools/policy_phase_bench.py: ``--envs`` (100) imagined
trajectories over ``--members`` (3) surrogates, N = 64, 4 actions, horizon ``--horizon`` (5), ``--rollouts`` (1 000) rollouts
per iteration, a ``world_replay`` of capacity ``--capacity`` (32 000) filled to its steady state before anything is timed,
``--real`` (4 000) real steps, B = 256, ``--updates`` (200) updates per iteration.  Two routes, alternated over ``--rounds``
rounds in one process, both warmed up, the host clock around work that ends in a device synchronisation:

  (a) host   written here only from calls the parent revision has: ``imagine()`` -> host ``ExperienceReplay.extend`` ->
             ``update_policy`` over two ``SubSeqDataset``s (which packs and uploads both replays).  ``--parent-only`` runs
             this route alone, so that the same file times it on the parent revision's tree in a process of its own;
             ``--parent-record FILE`` copies that process's figure into this record.
  (b) sink   ``imagine(sink=world_replay)`` -> ``world_replay.extend(staged)`` -> ``update_policy`` over the view and the
             real ``SubSeqDataset``.

Per round every route runs one untimed-inside iteration (the figure that is judged) and one with the ``timings`` hooks
(the split: every part then ends in a device synchronisation of its own).  Judged: (b)'s median lies below (a)'s minimum,
and the time saved is at least half of what (a)'s own split attributes to the imagined share of the pack, the replay build
and the copies back.

  --profile-run         warmed-up iterations of route (b) and nothing else: the program to put behind
                        ``rocprofv3 --kernel-trace --stats``
  --kernel-stats CSV    the kernel statistics of such a run: the rows of ``rp_append`` are copied into the record

Usage (repo root, on an MI355X):  python tools/world_replay_bench.py    (writes profiles/world_replay_bench.json)
"""
import argparse
import csv
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

B = 256
A_PARTS = ("reset_s", "steps_s", "copy_s", "build_s", "commit_s", "plan_s", "pack_s", "updates_s")
B_PARTS = ("reset_s", "steps_s", "append_s", "commit_s", "plan_s", "pack_s", "updates_s")


def timed(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


class Route:
    """One controller's world side: its own world, stack, agent and ``world_replay``."""

    def __init__(self, dev, args, with_sink):
        from imagination_phase_bench import scene
        from policy_phase_bench import A, HIGH, LOW, N, replay
        from pdecontrol.mbrl.replay import ExperienceReplay
        from pdecontrol.mbrl.worker import PDEEnvStack
        from pdecontrol.surrogates.common.dataset import SubSeqDataset
        from pdegym.common.transforms import BatchTransform, ScaleTransform, SensorTransform, SampleTransform
        self.args, self.with_sink = args, with_sink
        world, starting, stack, self.agent = scene(dev, args.envs, args.members, args.horizon)
        world.setup(starting)
        self.stack = PDEEnvStack(*stack)
        oscaling = ScaleTransform(batched=True, aggregate=True, frozen=False)
        oscaling.update(np.random.RandomState(5).uniform(-1.2, 1.2, (16, 1, N)).astype(np.float32))
        bounds = (np.full((1, 1, A), LOW, np.float32), np.full((1, 1, A), HIGH, np.float32))
        ascaling = ScaleTransform(bounds=bounds, aggregate=True, frozen=True, batched=True).Inverse
        to_agent = SampleTransform(otransf=[oscaling, BatchTransform(SensorTransform(stride=1))], atransf=ascaling.Inverse)
        self.world_to_agent = SampleTransform(atransf=ascaling.Inverse)
        self.make = lambda data, stransf: SubSeqDataset(data=data, length=1, stride=1, bootstrapping=False, stransf=stransf)
        self.real = self.make(replay(args.real, 8, 250, 2).data, to_agent)
        if with_sink:
            from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
            self.world_replay = DeviceExperienceReplay(args.capacity, device=dev)
        else:
            self.world_replay = ExperienceReplay(args.capacity)

    def iteration(self, timings=None, updates=None):
        from pdecontrol.mbrl import imagination_phase as ip, policy_phase as pp
        args, rp = self.args, self.world_replay
        clock = time.perf_counter
        rp.resize(args.capacity)
        sink = {"sink": rp} if self.with_sink else {}
        rollout = ip.imagine(self.agent, self.stack, args.rollouts, timings=timings, **sink)
        t0 = clock()
        rp.extend(rollout)
        if self.with_sink:
            imagined = rp.dataset(self.world_to_agent)
        else:
            imagined = self.make(rp.data, self.world_to_agent)
        if timings is not None:
            timings["commit_s"] = clock() - t0          # extend, resize and the dataset: host work only
        updates = args.updates if updates is None else updates
        if updates:
            pp.update_policy(self.agent, [imagined, self.real], B, updates, timings=timings)
        if timings is not None:
            assert timings["tier"] == "kernel", timings
        return rp.ntimesteps


def kernel_rows(path, name):
    with open(path, newline="") as f:
        return [row for row in csv.DictReader(f) if name in " ".join(str(v) for v in row.values())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--envs", type=int, default=100)
    ap.add_argument("--members", type=int, default=3)
    ap.add_argument("--horizon", type=int, default=5)
    ap.add_argument("--rollouts", type=int, default=1000)
    ap.add_argument("--capacity", type=int, default=32000)
    ap.add_argument("--real", type=int, default=4000)
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "world_replay_bench.json"))
    ap.add_argument("--parent-only", action="store_true")
    ap.add_argument("--parent-record", default=None)
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    np.random.seed(2)
    names = ("a_host",) if args.parent_only else ("b_sink",) if args.profile_run else ("a_host", "b_sink")
    routes = {name: Route(dev, args, name == "b_sink") for name in names}
    per_iteration = -(-args.rollouts // args.envs) * args.envs * args.horizon

    # fill every world_replay to its steady state (one iteration past the capacity), then warm the policy phase up
    fill = -(-args.capacity // max(args.rollouts * args.horizon, 1)) + 1
    for route in routes.values():
        for _ in range(fill):
            route.iteration(updates=0)
        route.iteration(updates=10)
        route.iteration()
        torch.cuda.synchronize()
    if args.profile_run:
        for _ in range(3):
            routes["b_sink"].iteration()
        torch.cuda.synchronize()
        return

    whole = {name: [] for name in routes}
    split = {name: {k: [] for k in (B_PARTS if name == "b_sink" else A_PARTS)} for name in routes}
    rows = {}
    for _ in range(args.rounds):
        for name, route in routes.items():
            seconds, rows[name] = timed(route.iteration)
            whole[name].append(1e3 * seconds)
        for name, route in routes.items():
            timings = {}
            route.iteration(timings=timings)
            for k in split[name]:
                split[name][k].append(1e3 * timings.get(k, 0.0))

    med = lambda v: round(float(np.median(v)), 3)
    rec = {"what": "controller iterations resize -> imagine -> extend -> update_policy: ms per iteration with the imagined "
                   "experience (a) in a host ExperienceReplay, packed and uploaded for every policy phase, and (b) in a "
                   "DeviceExperienceReplay written by rp_append and read in place; routes alternated in one process; host "
                   "clock around work ending in a device synchronisation; the splits come from separate iterations that "
                   "synchronise after each part",
           "device": torch.cuda.get_device_name(dev), "envs": args.envs, "members": args.members, "horizon": args.horizon,
           "rollouts": args.rollouts, "capacity": args.capacity, "real_steps": int(len(next(iter(routes.values())).real)),
           "B": B, "updates": args.updates, "rounds": args.rounds, "imagined_rows_per_iteration": per_iteration,
           "world_replay_rows": {k: int(v) for k, v in rows.items()}}
    for name in routes:
        rec[f"{name}_ms_per_iteration"] = [round(x, 3) for x in whole[name]]
        rec[f"{name}_median_ms"], rec[f"{name}_min_ms"], rec[f"{name}_max_ms"] = med(whole[name]), round(min(whole[name]), 3), round(max(whole[name]), 3)
        rec[f"{name}_split_ms"] = {k: med(v) for k, v in split[name].items()}
    if "b_sink" in routes:
        a, b = rec["a_host_median_ms"], rec["b_sink_median_ms"]
        parts = rec["a_host_split_ms"]
        imagined = rows["a_host"] / (rows["a_host"] + rec["real_steps"])
        attributed = parts["pack_s"] * imagined + parts["build_s"] + parts["copy_s"]
        rec.update({"slab_rows": int(routes["b_sink"].world_replay.rows),
                    "a_attributed_ms": {"imagined_share_of_rows": round(imagined, 4), "pack_share": round(parts["pack_s"] * imagined, 3),
                                        "build": parts["build_s"], "copy": parts["copy_s"], "sum": round(attributed, 3)},
                    "saved_ms": round(a - b, 3), "saved_over_attributed": round((a - b) / attributed, 3),
                    "ratio_a_over_b": round(a / b, 3),
                    "b_median_below_a_minimum": bool(b < rec["a_host_min_ms"]),
                    "saved_at_least_half_of_attributed": bool(a - b >= 0.5 * attributed)})
    if args.parent_record:
        with open(args.parent_record) as f:
            parent = json.loads(f.readline())
        rec["parent_process"] = {k: parent[k] for k in ("a_host_ms_per_iteration", "a_host_median_ms", "a_host_min_ms",
                                                        "a_host_max_ms", "a_host_split_ms")}
    if args.kernel_stats:
        rec["rp_append_kernel_stats"] = kernel_rows(args.kernel_stats, "rp_append")
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
