#!/usr/bin/env python3
"""Timings of the controller's warm-up phase (``learn()``: a ``RandomAgent`` for ``learning_starts`` real steps into the
real replay in HBM).  Record only: no ratio is fixed in advance.

The scene is tools/collection_phase_bench.py's: the controller's collection stack over a ``KSBatchedVecEnv`` in fast step
mode, a ``DeviceExperienceReplay`` on the same GPU as the sink, ``--learning-starts`` (20 000) steps per phase at ``--sizes``
(10x64, the reference's default ``--cpus``, and 1024x64).  Two routes, both warmed up twice, then alternated over
``--rounds`` rounds in one process, the host clock around work that ends in a device synchronisation:

  (a) loop      ``replay.extend(collect(worker, agent, stop, sink=replay))`` with a random agent that ``collect`` does not
                know (a local class): the per-step loop of ``Worker.rollout`` and the host replay staged into the sink --
                calls every earlier revision has, and what the warm-up cost there.
  (b) scripted  the same line with ``pdecontrol.mbrl.utils.RandomAgent``: per run of steps without a truncation one upload
                of the drawn actions, ``co_act_span``, the stepper launches, ``co_observe_span`` and ``ks_record_device``.

Both replays are unbounded: no phase evicts.  Each route keeps its own env, worker, action-space generator and replay, so
the episodes continue from phase to phase as the controller's would.

Usage (repo root, on an MI355X):  python tools/controller_warmup_bench.py    (writes profiles/controller_warmup_bench.json)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "model-based-pde-control_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from collection_phase_bench import scene, timed  # noqa: E402


class LocalRandomAgent:
    """``RandomAgent`` as ``collect`` met it before the scripted tier: a class it does not recognise."""

    def __init__(self, action_space):
        self.action_space = action_space

    def select_action(self, *args, **kwargs):
        return self.action_space.sample()


def route(dev, E, N, agent_cls, learning_starts):
    from pdecontrol.mbrl import collection_phase as cp
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    from pdecontrol.mbrl.worker import Worker
    stack, _, _ = scene(dev, E, N)
    worker = Worker(stack)
    worker._last_obs = stack.envs.reset(seed=1)
    worker._last_stored_obs = stack.ostore.obs.copy()[stack.ostore.mask]
    stack.world_wrapper.disable()
    space = stack.envs.action_space
    space.seed(7)
    agent, replay = agent_cls(space), DeviceExperienceReplay(device=dev)
    stop = lambda ts, _: ts >= learning_starts
    tiers = set()

    def phase():
        staged = cp.collect(worker, agent, stop, sink=replay)
        tiers.add((staged.tier, staged.host_steps))
        replay.extend(staged)
        return staged.ntimesteps

    return phase, tiers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--learning-starts", type=int, default=20000)
    ap.add_argument("--sizes", default="10x64,1024x64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "controller_warmup_bench.json"))
    args = ap.parse_args()
    from pdecontrol.mbrl import utils
    dev = torch.device("cuda", 0)
    report = {"device": torch.cuda.get_device_name(0), "learning_starts": args.learning_starts, "rounds": args.rounds, "sizes": {}}
    for size in args.sizes.split(","):
        E, N = (int(v) for v in size.split("x"))
        routes = {"a_loop": route(dev, E, N, LocalRandomAgent, args.learning_starts),
                  "b_scripted": route(dev, E, N, utils.RandomAgent, args.learning_starts)}
        for phase, _ in routes.values():                   # warm both up: allocations, the first launches
            phase()
            phase()
        seconds = {name: [] for name in routes}
        steps = {}
        for _ in range(args.rounds):                        # alternate in one process
            for name, (phase, _) in routes.items():
                t, n = timed(phase)
                seconds[name].append(t)
                steps[name] = n
        row = {}
        for name, (_, tiers) in routes.items():
            s = np.asarray(seconds[name])
            row[name] = {"median_s": round(float(np.median(s)), 5), "range_s": [round(float(s.min()), 5), round(float(s.max()), 5)],
                         "timesteps": int(steps[name]), "us_per_env_step": round(float(np.median(s)) / steps[name] * 1e6, 3),
                         "tier_and_host_steps": sorted(tiers)}
        assert {t for t, _ in routes["a_loop"][1]} == {"loop"} and {t for t, _ in routes["b_scripted"][1]} == {"kernel"}, row
        row["a_over_b"] = round(row["a_loop"]["median_s"] / row["b_scripted"]["median_s"], 2)
        report["sizes"][size] = row
        print(size, json.dumps(row))
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
