#!/usr/bin/env python3
"""Timings of real-env collection over a ``BurgersBatchedVecEnv``.  Record only: no ratio is fixed in
advance.

Sizes: ``--sizes`` (10x512, the controller's default ``cpus`` at the BASELINE configs[4] grid, and 1024x512), 50 sub-steps
per step.  Every comparison is warmed up twice, then alternated over ``--rounds`` rounds in one process, the host clock
around work that ends in a device synchronisation; medians and ranges are reported.

  (i)  warm-up   a ``--learning-starts`` (2 000) step ``RandomAgent`` phase into a ``DeviceExperienceReplay``:
                 (a) ``replay.extend(worker.rollout(agent, stop))``, the per-step loop and the host replay uploaded, the only
                     route this env had;
                 (b) ``replay.extend(collect(worker, agent, stop, sink=replay))``: per run of steps without a truncation one
                     upload of the drawn actions, ``co_act_span``, ``bg_step_span``, ``co_observe_span`` and ``bg_record``.
                 Each route keeps its own env, worker, action-space generator and unbounded replay.
  (ii) C ABI     ``bg_step_span`` over ``--span`` (64) steps against as many ``bg_step`` launches writing the same trajectory
                 block, from the same state and action table (the outputs are compared once, byte for byte).

Usage (repo root, on an MI355X):  python tools/burgers_collect_bench.py    (writes profiles/burgers_collect_bench.json)
"""
import argparse
import ctypes
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

CFG_STEPS = 50


def timed(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def summary(seconds):
    s = np.asarray(seconds)
    return {"median_s": round(float(np.median(s)), 6), "range_s": [round(float(s.min()), 6), round(float(s.max()), 6)]}


def alternate(routes, rounds):
    """{name: seconds per round} of the calls of ``routes``, warmed up twice, then alternated."""
    for call in routes.values():
        call()
        call()
    seconds = {name: [] for name in routes}
    for _ in range(rounds):
        for name, call in routes.items():
            seconds[name].append(timed(call)[0])
    return seconds


# ----------------------------------------------------------------------------------------------------------------------
# (i) the warm-up phase
# ----------------------------------------------------------------------------------------------------------------------
def stack_over(env):
    """The controller's collection stack (reference mbrl.py:146-175, 259-272) over ``env``."""
    from pdecontrol.mbrl.worker import PDEEnvStack
    from pdecontrol.mbrl.world.wrappers import BaseWorldVecEnvWrapper
    from pdegym.common import transforms as T
    from pdegym.common import vec_wrappers as W
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
    return PDEEnvStack(envs=envs, ostore=ostore, astore=astore, world_wrapper=world_wrapper)


def warmup_route(dev, E, N, through_collect, learning_starts):
    from pdecontrol.mbrl import collection_phase as cp
    from pdecontrol.mbrl import utils
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    from pdecontrol.mbrl.worker import Worker
    from pdegym.burgers.burgers import BurgersBatchedVecEnv
    stack = stack_over(BurgersBatchedVecEnv(E, N=N, cfg_steps=CFG_STEPS, device=dev.index))
    worker = Worker(stack)
    worker._last_obs = stack.envs.reset(seed=1)
    worker._last_stored_obs = stack.ostore.obs.copy()[stack.ostore.mask]
    stack.world_wrapper.disable()
    space = stack.envs.action_space
    space.seed(7)
    agent, replay = utils.RandomAgent(space), DeviceExperienceReplay(device=dev)
    stop = lambda ts, _: ts >= learning_starts
    seen = {"tiers": set(), "timesteps": 0}

    def phase():
        if through_collect:
            got = cp.collect(worker, agent, stop, sink=replay)
            seen["tiers"].add((got.tier, got.host_steps))
        else:
            got = worker.rollout(agent, stop)
            seen["tiers"].add(("loop", got.ntimesteps // E))
        seen["timesteps"] = got.ntimesteps
        replay.extend(got)

    return phase, seen


def warmup(dev, E, N, rounds, learning_starts):
    routes = {"a_loop": warmup_route(dev, E, N, False, learning_starts), "b_kernel": warmup_route(dev, E, N, True, learning_starts)}
    seconds = alternate({name: phase for name, (phase, _) in routes.items()}, rounds)
    row = {}
    for name, (_, seen) in routes.items():
        row[name] = {**summary(seconds[name]), "timesteps": seen["timesteps"],
                     "us_per_env_step": round(float(np.median(seconds[name])) / seen["timesteps"] * 1e6, 3),
                     "tier_and_host_steps": sorted(seen["tiers"])}
    assert {t for t, _ in routes["b_kernel"][1]["tiers"]} == {"kernel"}, row
    row["a_over_b"] = round(row["a_loop"]["median_s"] / row["b_kernel"]["median_s"], 2)
    row["a_over_b_range"] = [round(min(seconds["a_loop"]) / max(seconds["b_kernel"]), 2),
                             round(max(seconds["a_loop"]) / min(seconds["b_kernel"]), 2)]
    return row


# ----------------------------------------------------------------------------------------------------------------------
# (ii) bg_step_span against T bg_step launches
# ----------------------------------------------------------------------------------------------------------------------
def span(dev, E, N, T, rounds, reps):
    from hipbind import ptr
    from pdegym.burgers import _hip
    from pdegym.burgers.burgers import BurgersBatchedVecEnv
    env = BurgersBatchedVecEnv(E, N=N, cfg_steps=CFG_STEPS, device=dev.index)
    env.reset(seed=3)
    lib, A = _hip.load(), len(env.Xi)
    u0 = env.u.clone()
    actions = torch.from_numpy(np.random.RandomState(5).uniform(-1, 1, (T, E, A)).astype(np.float32)).to(dev)
    out = {name: (torch.empty_like(u0), torch.zeros((T + 1, E, N), dtype=torch.float32, device=dev),
                  torch.zeros((T, E), dtype=torch.float64, device=dev), torch.zeros((T, E), dtype=torch.int32, device=dev))
           for name in ("launches", "span")}
    args = (env.dx, env.dt, env.nu, CFG_STEPS)
    stream = lambda: ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(dev.index))

    def launches():
        u, traj, ssq, status = out["launches"]
        for _ in range(reps):
            u.copy_(u0)
            st = stream()
            for t in range(T):
                _hip.check(lib.bg_step(st, ptr(u), ptr(actions[t]), ptr(env._F), A, E, N, *args, ptr(traj[t + 1]), ptr(ssq[t]),
                                       ptr(status[t])))

    def one_span():
        u, traj, ssq, status = out["span"]
        for _ in range(reps):
            u.copy_(u0)
            _hip.check(lib.bg_step_span(stream(), ptr(u), ptr(actions), ptr(env._F), A, E, N, T, env.dx, env.dt, env.nu, CFG_STEPS,
                                        ptr(traj), ptr(ssq), ptr(status)))

    seconds = alternate({"launches": launches, "span": one_span}, rounds)
    torch.cuda.synchronize()
    same = all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(out["launches"], out["span"]))
    finite = not bool(out["span"][3].any())
    row = {name: {**summary(np.asarray(s) / reps), "us_per_step": round(float(np.median(s)) / reps / T * 1e6, 3)}
           for name, s in seconds.items()}
    row.update(T=T, reps_per_timing=reps, outputs_identical=bool(same), finite=finite,
               launches_over_span=round(row["launches"]["median_s"] / row["span"]["median_s"], 3),
               launches_over_span_range=[round(min(seconds["launches"]) / max(seconds["span"]), 3),
                                         round(max(seconds["launches"]) / min(seconds["span"]), 3)])
    assert same and finite, row
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--learning-starts", type=int, default=2000)
    ap.add_argument("--span", type=int, default=64)
    ap.add_argument("--sizes", default="10x512,1024x512")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "burgers_collect_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    report = {"device": torch.cuda.get_device_name(0), "cfg_steps": CFG_STEPS, "learning_starts": args.learning_starts,
              "rounds": args.rounds, "sizes": {}}
    for size in args.sizes.split(","):
        E, N = (int(v) for v in size.split("x"))
        row = {"i_warmup": warmup(dev, E, N, args.rounds, args.learning_starts),
               "ii_span": span(dev, E, N, args.span, args.rounds, reps=200 if E <= 64 else 100)}
        report["sizes"][size] = row
        print(size, json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
