#!/usr/bin/env python3
"""Timings of the controller's real-env collection phase on an MI355X (pdecontrol/mbrl/collection_phase.py).  Record only.

The stack is the controller's collection stack (running observation scaling, sensors, world-model hook, action store,
frozen action scaling) over a ``KSBatchedVecEnv`` in fast step mode with the default ``Tmax`` (400 steps per episode) and
the default burn-in, at ``--sizes`` (1024x64 and 4096x256).  The agent is a SAC agent (hidden 256, no logger) on the same
GPU.  One phase is ``--steps`` (8) steps of all envs, with no truncation inside.  Two routes, alternated over ``--rounds``
rounds in one process after a warm-up of both, the host clock around work that ends in a device synchronisation:

  (a) loop    the per-step loop of ``Worker.rollout``, written here from calls every earlier revision has (the stack's
              ``step``, ``agent.select_action``, ``Sample.split`` + ``ExperienceReplay.add``, the stop test on the replay),
              so that ``--loop-only`` times the same route on a revision without the phase.  Its split into select_action /
              env step / wrappers / replay build comes from separate phases that synchronise after each part (the env step
              is the time inside ``KSBatchedVecEnv.step_wait``; the wrappers are the rest of ``envs.step``).
  (b) phase   ``collect`` on the kernel tier.

  --profile-run SIZE   one warmed-up phase of route (b) at one size and nothing else: the program to put behind
                       ``rocprofv3 --kernel-trace --stats``
  --kernel-trace CSV   ``*_kernel_trace.csv`` files of such runs ("1024x64=path,4096x256=path"): the median device time per
                       launch of the KS kernel, ``co_act`` and the two ``co_observe`` launches is read from them, and the
                       criterion (b) - ks <= 0.5 * ((a) - ks) is evaluated per size

Usage (repo root, on an MI355X):  python tools/collection_phase_bench.py    (writes profiles/collection_phase_bench.json)
"""
import argparse
import csv
import json
import os
import sys
import time
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "model-based-pde-control_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


class Box:
    def __init__(self, low, high, n):
        self.low, self.high = np.full((1, n), low, dtype=np.float32), np.full((1, n), high, dtype=np.float32)
        self.shape = (1, n)


def scene(dev, E, N):
    """(stack, agent) of the controller's collection phase (reference mbrl.py:146-175, 259-272)."""
    import pdegym  # noqa: F401
    from pdecontrol.mbrl.worker import PDEEnvStack
    from pdecontrol.mbrl.world.wrappers import BaseWorldVecEnvWrapper
    from pdecontrol.sac.sac import SAC
    from pdegym.common import transforms as T
    from pdegym.common import vec_wrappers as W
    from pdegym.kuramoto.batched import KSBatchedVecEnv
    env = KSBatchedVecEnv(E, dict(L=22.0 * N / 64, N=N), device=dev.index, step_mode="fast")
    oscaling = T.ScaleTransform(batched=True, aggregate=True, frozen=False)
    low = np.asarray(env.single_action_space.low)[np.newaxis, ...]
    high = np.asarray(env.single_action_space.high)[np.newaxis, ...]
    ascaling = T.ScaleTransform(bounds=(low, high), aggregate=True, frozen=True, batched=True).Inverse
    sensor = lambda: T.BatchTransform(T.SensorTransform(stride=1))
    ostore = W.StoreNObsVecWrapper(env, num_steps=1)
    envs = W.TransformObsWrapper(ostore, oscaling, frozen=False)
    envs = W.TransformObsWrapper(envs, sensor())
    world_wrapper = BaseWorldVecEnvWrapper(env=envs, surrogate=None, tstep=env.cfg_steps * env.dt)
    envs = W.TransformObsWrapper(world_wrapper, sensor())
    astore = W.StoreNActionsVecWrapper(envs, num_steps=1)
    envs = W.TransformActionWrapper(astore, ascaling, frozen=True)
    cfg = Namespace(gamma=0.99, tau=0.005, alpha=0.2, policy="Gaussian", target_update_interval=1,
                    automatic_entropy_tuning=False, cuda=False, device=dev, hidden_size=256, lr=3e-4)
    torch.manual_seed(0)
    agent = SAC(Box(-np.inf, np.inf, N), Box(-1.0, 1.0, 4), cfg, logger=None)
    return PDEEnvStack(envs=envs, ostore=ostore, astore=astore, world_wrapper=world_wrapper), agent, env


class Loop:
    """Route (a): ``Worker.rollout`` from calls every earlier revision has; keeps the last observation between phases."""

    def __init__(self, stack, agent, ks):
        self.stack, self.agent, self.ks = stack, agent, ks
        self.last = stack.envs.reset(seed=1)
        self.stored = stack.ostore.obs.copy()[stack.ostore.mask]

    def phase(self, steps, split=None):
        from pdecontrol.mbrl.replay import ExperienceReplay
        from pdecontrol.mbrl.types import Sample
        envs, ostore, astore = self.stack.envs, self.stack.ostore, self.stack.astore
        E = self.ks.num_envs
        clock, sync = time.perf_counter, torch.cuda.synchronize
        inner = [0.0]
        if split is not None:                        # the time inside the KS env's own step, the stepper's sync included
            plain = self.ks.step_wait

            def step_wait(**kw):
                t0 = clock()
                out = plain(**kw)
                inner[0] += clock() - t0
                return out

            self.ks.step_wait = step_wait
        replay = ExperienceReplay()
        t = clock()

        def lap(name):
            nonlocal t
            if split is not None:
                sync()
                split[name] = split.get(name, 0.0) + clock() - t
                t = clock()

        try:
            while not replay.ntimesteps >= steps * E:
                lap("replay_build")                  # the stop test re-counts every deque
                with torch.no_grad():
                    actions = self.agent.select_action(self.last)
                lap("select_action")
                self.last, rewards, terminated, truncated, infos = envs.step(actions)
                lap("env_step_and_wrappers")
                obs, self.stored = self.stored.copy(), ostore.obs.copy()[ostore.mask]
                nxtobs = self.stored.copy()
                assert "final_observation" not in infos, "a truncation inside the timed phase"
                sample = Sample(obs, astore.actions.copy()[astore.mask], nxtobs, rewards, terminated, truncated, infos["step"])
                replay.add(sample.split(axis=0))
                lap("replay_build")
        finally:
            if split is not None:
                del self.ks.step_wait
                split["env_step"] = split.get("env_step", 0.0) + inner[0]
                split["wrappers"] = split.get("wrappers", 0.0) + split.pop("env_step_and_wrappers") - inner[0]
        return replay


def timed(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def kernel_times(path):
    """{kernel family: median device microseconds per launch, launches} from a rocprofv3 ``*_kernel_trace.csv``.  The
    median leaves out the one long KS launch of the reset's burn-in."""
    want = {"ks": ("ks_rk4",), "co_act": ("co_act_span_kernel", "co_act_kernel"),
            "co_observe_extrema": ("co_span_extrema_kernel", "co_extrema_kernel"),
            "co_observe_scale": ("co_scale_kernel",), "sac_policy_forward": ("sac_policy_fwd",)}
    seen = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name", "")
            for key, needles in want.items():
                if any(n in name for n in needles):
                    seen.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
                    break
    return {k: {"launches": len(v), "us_per_launch": round(float(np.median(v)), 3),
                "range_us": [round(min(v), 3), round(max(v), 3)]} for k, v in seen.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--sizes", default="1024x64,4096x256")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collection_phase_bench.json"))
    ap.add_argument("--profile-run", default=None, metavar="SIZE")
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--loop-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    sizes = [tuple(int(v) for v in s.split("x")) for s in (args.profile_run or args.sizes).split(",")]
    if not args.loop_only:
        from pdecontrol.mbrl import collection_phase as cp
        from pdecontrol.mbrl.worker import Worker
    med = lambda v: round(float(np.median(v)), 4) if v else None

    def phase_b(worker, agent, E):
        replay = cp.collect(worker, agent, lambda ts, ep: ts >= args.steps * E)
        assert replay.tier == "kernel" and replay.host_steps == 0, (replay.tier, replay.tier_reason, replay.host_steps)
        return replay

    if args.profile_run:
        (E, N), = sizes
        stack, agent, _ = scene(dev, E, N)
        worker = Worker(stack)
        worker._last_obs = stack.envs.reset(seed=1)
        worker._last_stored_obs = stack.ostore.obs.copy()[stack.ostore.mask]
        for _ in range(3):
            phase_b(worker, agent, E)
        torch.cuda.synchronize()
        return

    stats = dict(kv.split("=") for kv in args.kernel_trace.split(",")) if args.kernel_trace else {}
    rec = {"what": "real-env collection phase: ms per phase and per step (one step of all envs) of (a) the per-step loop of "
                   "Worker.rollout over the wrapper stack and (b) collect on the kernel tier; routes alternated in one "
                   "process after a warm-up of both, medians and ranges over the rounds; host clock around work ending in a "
                   "device synchronisation; the split of (a) comes from separate phases that synchronise after each part; "
                   "device times per launch come from a separate rocprofv3 --kernel-trace --stats run of route (b)",
           "device": torch.cuda.get_device_name(dev), "steps_per_phase": args.steps, "rounds": args.rounds,
           "step_mode": "fast", "claims_from_code_reading_not_from_a_trace": [
               "no copy crosses the host inside a segment (the phase enqueues launches only between the uploads at a "
               "segment's start and the one copy back at its end)",
               "the kernel tier enqueues six launches per step (noise, policy forward, co_act, KS step, two of co_observe)"],
           "sizes": {}}
    for E, N in sizes:
        stack_a, agent_a, ks_a = scene(dev, E, N)
        loop = Loop(stack_a, agent_a, ks_a)
        if not args.loop_only:
            stack_b, agent_b, _ = scene(dev, E, N)
            worker = Worker(stack_b)
            worker._last_obs = stack_b.envs.reset(seed=1)
            worker._last_stored_obs = stack_b.ostore.obs.copy()[stack_b.ostore.mask]
        # warm-up: code objects, the allocator, pinned staging, clocks
        for _ in range(2):
            assert loop.phase(args.steps).ntimesteps == args.steps * E
            if not args.loop_only:
                assert phase_b(worker, agent_b, E).ntimesteps == args.steps * E
        ms, split = {"a_loop": [], "b_collect": []}, {}
        for _ in range(args.rounds):
            ms["a_loop"].append(1e3 * timed(lambda: loop.phase(args.steps))[0])
            if not args.loop_only:
                ms["b_collect"].append(1e3 * timed(lambda: phase_b(worker, agent_b, E))[0])
            parts = {}
            loop.phase(args.steps, split=parts)
            for k, v in parts.items():
                split.setdefault(k, []).append(1e3 * v / args.steps)
        a, b = med(ms["a_loop"]), med(ms["b_collect"])
        per_step = lambda v: None if v is None else round(v / args.steps, 4)
        size = {"envs": E, "N": N, "ms_per_phase": {k: [round(x, 3) for x in v] for k, v in ms.items()},
                "a_loop_ms_per_step": per_step(a), "b_collect_ms_per_step": per_step(b),
                "a_range_ms_per_step": [per_step(min(ms["a_loop"])), per_step(max(ms["a_loop"]))],
                "b_range_ms_per_step": [per_step(min(ms["b_collect"])), per_step(max(ms["b_collect"]))] if b else None,
                "a_split_ms_per_step": {k: med(v) for k, v in sorted(split.items())}}
        path = stats.get(f"{E}x{N}")
        if path:
            size["device_us_per_launch"] = kernel_times(path)
            ks = size["device_us_per_launch"].get("ks", {}).get("us_per_launch")
            if ks is not None and b is not None:
                ks_ms = ks / 1e3
                over_a, over_b = per_step(a) - ks_ms, per_step(b) - ks_ms
                size["criterion"] = {"ks_ms_per_step": round(ks_ms, 4), "a_minus_ks": round(over_a, 4), "b_minus_ks": round(over_b, 4),
                                     "bound": "b - ks <= 0.5 * (a - ks)", "holds": bool(over_b <= 0.5 * over_a)}
        rec["sizes"][f"{E}x{N}"] = size
        del loop
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
