#!/usr/bin/env python3
"""Timings of the controller's imagined-rollout phase on an MI355X (pdecontrol/mbrl/imagination_phase.py).  Record only.

The world is a controller's: ``--envs`` (100) imagined trajectories over an ensemble of ``--members`` (3) autoregressive
ConvLSTM surrogates, N = 64, 4 actions, horizon ``--horizon`` (5), under the controller's five-wrapper action stack and
agent sensor; warm-up windows (tau = 3) come from a replay of synthetic episodes.  The agent is the SAC agent of
tools/sac_bench.py (hidden 256, no logger).  One phase is ``--rollouts`` (1 000) rollouts: 10 rounds of 5 steps.  Two
routes, alternated over ``--rounds`` rounds in one process, both warmed up, every window between two device
synchronisations:

  (a) loop    the per-step loop, written here from calls every earlier revision has (the stack's ``reset`` / ``step``,
              ``agent.select_action``, ``Sample.split`` + ``ExperienceReplay.add``), so that ``--loop-only`` times the same
              route on a revision without the phase.
  (b) phase   ``imagine``; its resets, steps, copies back and replay build are listed separately (each of the four then
              ends in a device synchronisation of its own, which the untimed phase does once per round).

The record says whether (b) beats (a) by more than (a)'s spread (max - min over the rounds).

  --profile-run   one warmed-up phase and nothing else: the program to put behind ``rocprofv3 --kernel-trace --stats``
  --loop-only     route (a) alone
  --objective dissipation   the env's dissipation reward (``objective=""``) in place of l2control; writes
                  profiles/imagination_phase_bench_dissipation.json.  The record then also holds
                  (p) parent   ``imagine`` as the revision before ``ro_settle_dissipation`` runs it under this objective:
                               the loop tier, ``Worker.rollout`` over the same stack.  It is timed by ``--parent-only``
                               in a process of its own, started before this one touches the GPU;
                  (c) l2control   the kernel tier of an l2control scene of the same shape, alternated with (b) in this
                               process, for information;
                  and the claim "(b) is faster than (p) by more than the two ranges together", met or missed.
  --parent-only   (p) alone: ``imagine`` with the kernel tier's recognition switched off in this process, so that the
                  call takes the loop tier whatever the objective; prints one JSON line

Usage (repo root, on an MI355X):  python tools/imagination_phase_bench.py    (writes profiles/imagination_phase_bench.json)
"""
import argparse
import gc
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "model-based-pde-control_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

TAU = 3


def scene(dev, envs, members, horizon, objective="l2control"):
    """(world, starting states, stack as (envs, ostore, astore), agent)"""
    import pdegym  # noqa: F401
    from sac_bench import agent_on
    from pdecontrol.architectures import KSAutoRegConvolutionalLSTM
    from pdecontrol.mbrl.replay import ExperienceReplay
    from pdecontrol.mbrl.types import Sample
    from pdecontrol.mbrl.world.world import WorldVecEnv
    from pdecontrol.surrogates.common import dataset as ds
    from pdecontrol.surrogates.surrogate import PDEEnsemble
    from pdecontrol.surrogates.training import PDETrainingModule
    from pdegym.common import transforms as T
    from pdegym.common import vec_wrappers as W
    from pdegym.kuramoto import KuramotoSivashinskyEnv
    # never stepped: forcing, spaces and the reward only (a falsy ``objective`` is what selects the dissipation reward)
    env = KuramotoSivashinskyEnv(**({"objective": ""} if objective == "dissipation" else {}))
    assert env.step_objective == objective
    N, tstep = env.N, env.cfg_steps * env.dt
    oscaling = T.ScaleTransform(bounds=(np.full((1, 1, 1), -3.0, np.float32), np.full((1, 1, 1), 3.0, np.float32)),
                                batched=True, aggregate=True, frozen=True)
    low, high = np.asarray(env.action_space.low)[np.newaxis, ...], np.asarray(env.action_space.high)[np.newaxis, ...]
    ascaling = T.ScaleTransform(bounds=(low, high), aggregate=True, frozen=True, batched=True).Inverse
    forcing = T.BatchTransform(env.forcing)
    lo, hi = np.squeeze(forcing(low), axis=0), np.squeeze(forcing(high), axis=0)
    pdescaling = T.BatchTransform(T.ScaleTransform(bounds=(lo, hi), scale=(-1, 1), aggregate=True, frozen=True))
    sensor = lambda: T.BatchTransform(T.SensorTransform(stride=1))
    agent_sensor, world_sensor = sensor(), sensor()
    replay_to_world = T.SampleTransform([oscaling, world_sensor], [forcing, pdescaling, world_sensor])

    rp, rs = ExperienceReplay(), np.random.RandomState(5)
    x = np.linspace(0, 2 * np.pi, N, endpoint=False)
    for ep_len in (40,) * 8:
        phase = rs.uniform(0, 6)
        for t in range(ep_len):
            mk = lambda tt: (np.sin(x + phase + 0.3 * tt) + 0.5 * np.cos(2 * x - 0.2 * tt)).astype(np.float32)[None, :]
            rp.add([Sample(mk(t), rs.uniform(-1, 1, (1, 4)).astype(np.float32), mk(t + 1), np.float32(-1.0), False,
                           t == ep_len - 1, np.int32(t + 1))])
    modules = []
    for seed in range(members):
        torch.manual_seed(seed)
        f = KSAutoRegConvolutionalLSTM()
        sur = f.surrogate(delta=tstep, dscaling=None, tau=TAU, **f.model())
        modules.append(PDETrainingModule(surrogate=sur, loss=torch.nn.MSELoss(reduction="none"), tstep=tstep, delta=tstep,
                                         tau=TAU, tbtt=10).to(dev))
    world = WorldVecEnv(surrogate=PDEEnsemble(modules, num_elites=members), observation_space=env.observation_space,
                        action_space=env.action_space, max_episode_steps=env.max_episode_steps,
                        stransf=replay_to_world.Inverse, reward_func=env.reward_func, num_envs=envs, horizon=horizon,
                        tstep=tstep, batched_reward_func=env.batched_reward_func)
    starting = ds.StartingStateDataset(data=rp.data, length=TAU, stride=1, bootstrapping=False, stransf=replay_to_world)
    ostore = W.StoreNObsVecWrapper(world, num_steps=1)
    stack = W.TransformObsWrapper(ostore, agent_sensor)
    stack = W.TransformActionWrapper(stack, world_sensor)
    stack = W.TransformActionWrapper(stack, pdescaling, frozen=True)
    stack = W.TransformActionWrapper(stack, forcing, frozen=True)
    stack = W.TransformActionWrapper(stack, ascaling, frozen=True)
    astore = W.StoreNActionsVecWrapper(stack, num_steps=1)
    return world, starting, (astore, ostore, astore), agent_on(dev, auto=False)


def loop_phase(agent, stack, num_rollouts):
    """Route (a): a fresh worker's rollout until ``num_rollouts`` episodes have stopped."""
    from pdecontrol.mbrl.replay import ExperienceReplay
    from pdecontrol.mbrl.types import Sample
    envs, ostore, astore = stack
    replay = ExperienceReplay()
    last = envs.reset()
    stored = ostore.obs.copy()[ostore.mask]
    while replay.nstopped < num_rollouts:
        with torch.no_grad():
            actions = agent.select_action(last)
        last, rewards, terminated, truncated, infos = envs.step(actions)
        obs, stored = stored.copy(), ostore.obs.copy()[ostore.mask]
        nxtobs = stored.copy()
        if "final_observation" in infos:
            index = infos["_final_observation"]
            nxtobs[index] = ostore.finals[index].copy()[ostore.mask[index]]
        sample = Sample(obs, astore.actions.copy()[astore.mask], nxtobs, rewards, terminated, truncated, infos["step"])
        replay.add(sample.split(axis=0))
    return replay


_GC = {"start": 0.0, "ms": 0.0}


def _watch_gc(phase, info):
    """Host time Python's cyclic collector takes (``gc.callbacks``): a phase builds thousands of deques, and a full
    collection that lands inside a timed window shows as a round tens of ms longer than its neighbours."""
    if phase == "start":
        _GC["start"] = time.perf_counter()
    else:
        _GC["ms"] += 1e3 * (time.perf_counter() - _GC["start"])


gc.callbacks.append(_watch_gc)


def timed(call):
    """(seconds, result); ``timed.gc_ms`` is the collector's share of the window (recorded, not subtracted)."""
    torch.cuda.synchronize()
    _GC["ms"] = 0.0
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    timed.gc_ms = round(_GC["ms"], 3)
    return seconds, out


def parent_only(args, dev):
    """(p): ms per phase of ``imagine`` on the loop tier, warmed up, one JSON line."""
    from pdecontrol.mbrl import imagination_phase as ip
    from pdecontrol.mbrl.worker import PDEEnvStack
    ip._kernel_tier = lambda agent, stack: (None, None)      # what the revision before ro_settle_dissipation decides
    world, starting, stack, agent = scene(dev, args.envs, args.members, args.horizon, args.objective)
    world.setup(starting)
    torch.manual_seed(1)
    np.random.seed(2)
    stack = PDEEnvStack(*stack)
    steps = ip.imagine(agent, stack, args.rollouts).ntimesteps // args.envs
    ip.imagine(agent, stack, args.rollouts)
    ms, gc_ms = [], []
    for _ in range(args.rounds):
        timings = {}
        ms.append(1e3 * timed(lambda: ip.imagine(agent, stack, args.rollouts, timings=timings))[0])
        gc_ms.append(timed.gc_ms)
        assert timings["tier"] == "loop", timings
    print(json.dumps({"objective": args.objective, "steps_per_phase": int(steps), "parent_ms_per_phase": [round(x, 3) for x in ms],
                      "parent_gc_ms_in_window": gc_ms}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--envs", type=int, default=100)
    ap.add_argument("--members", type=int, default=3)
    ap.add_argument("--horizon", type=int, default=5)
    ap.add_argument("--rollouts", type=int, default=1000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--objective", choices=("l2control", "dissipation"), default="l2control")
    ap.add_argument("--parent-only", action="store_true")
    args = ap.parse_args()
    diss = args.objective == "dissipation"
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "imagination_phase_bench_dissipation.json" if diss else "imagination_phase_bench.json")
    parent = None
    if diss and not (args.parent_only or args.profile_run or args.loop_only):
        # (p) in a process of its own, before this one opens the GPU
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-only", "--objective", args.objective] +
                               [f"--{k}={getattr(args, k)}" for k in ("rounds", "envs", "members", "horizon", "rollouts")],
                               check=True, capture_output=True, text=True)
        parent = json.loads(child.stdout.strip().splitlines()[-1])
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    if args.parent_only:
        return parent_only(args, dev)
    if not args.loop_only:
        from pdecontrol.mbrl import imagination_phase as ip
        from pdecontrol.mbrl.worker import PDEEnvStack

    scenes = {name: scene(dev, args.envs, args.members, args.horizon, args.objective) for name in ("a_loop", "b_phase")}
    if parent is not None:
        scenes["c_l2control"] = scene(dev, args.envs, args.members, args.horizon)
    for world, starting, _, _ in scenes.values():
        world.setup(starting)
    torch.manual_seed(1)
    np.random.seed(2)
    world_a, _, stack_a, agent_a = scenes["a_loop"]
    world_b, _, stack_b, agent_b = scenes["b_phase"]
    route_a = lambda: loop_phase(agent_a, stack_a, args.rollouts)
    if args.profile_run:
        stack = PDEEnvStack(*stack_b)
        ip.imagine(agent_b, stack, args.rollouts)
        ip.imagine(agent_b, stack, args.rollouts)
        torch.cuda.synchronize()
        return

    # warm-up: code objects, the captured graphs of the world and of the imagined step, the allocator
    steps = route_a().ntimesteps // args.envs
    ms = {"a_loop_phase": [], "b_phase_whole": []}
    split = {k: [] for k in ("reset_s", "steps_s", "copy_s", "build_s")}
    split_c = {k: [] for k in split}
    gc_ms = {k: [] for k in ("a_loop_phase", "b_phase_whole", "c_l2control_phase_whole")}
    if not args.loop_only:
        stack = PDEEnvStack(*stack_b)
        assert ip.imagine(agent_b, stack, args.rollouts).ntimesteps == steps * args.envs
    if "c_l2control" in scenes:
        _, _, stack_c, agent_c = scenes["c_l2control"]
        stack_c = PDEEnvStack(*stack_c)
        ms["c_l2control_phase_whole"] = []
        assert ip.imagine(agent_c, stack_c, args.rollouts).ntimesteps == steps * args.envs
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        ms["a_loop_phase"].append(1e3 * timed(route_a)[0])
        gc_ms["a_loop_phase"].append(timed.gc_ms)
        if args.loop_only:
            continue
        whole, _ = timed(lambda: ip.imagine(agent_b, stack, args.rollouts))       # untimed inside: one sync per round
        ms["b_phase_whole"].append(1e3 * whole)
        gc_ms["b_phase_whole"].append(timed.gc_ms)
        timings = {}
        ip.imagine(agent_b, stack, args.rollouts, timings=timings)
        assert timings["tier"] == "kernel", timings
        for k in split:
            split[k].append(1e3 * timings[k])
        if "c_l2control" in scenes:
            ms["c_l2control_phase_whole"].append(1e3 * timed(lambda: ip.imagine(agent_c, stack_c, args.rollouts))[0])
            gc_ms["c_l2control_phase_whole"].append(timed.gc_ms)
            timings = {}
            ip.imagine(agent_c, stack_c, args.rollouts, timings=timings)
            assert timings["tier"] == "kernel", timings
            for k in split_c:
                split_c[k].append(1e3 * timings[k])

    med = lambda v: round(float(np.median(v)), 4) if v else None
    spread = lambda v: round(max(v) - min(v), 4) if v else None
    a, b = med(ms["a_loop_phase"]), med(ms["b_phase_whole"])
    rec = {"objective": args.objective,
           "what": "imagined-rollout phase: ms per phase and per imagined step (one step of all envs) of (a) the per-step "
                   "loop over the wrapper stack and (b) imagine on the kernel tier; routes alternated in one process, medians "
                   "over the rounds; host clock around work ending in a device synchronisation; the split of (b) comes from "
                   "separate phases that synchronise after each part",
           "device": torch.cuda.get_device_name(dev), "envs": args.envs, "members": args.members, "horizon": args.horizon,
           "rollouts": args.rollouts, "steps_per_phase": int(steps), "rounds": args.rounds,
           "ms_per_phase": {k: [round(x, 3) for x in v] for k, v in ms.items()},
           "gc_ms_in_window": {k: v for k, v in gc_ms.items() if v},
           "a_loop_ms_per_phase": a, "a_loop_ms_per_step": None if a is None else round(a / steps, 4),
           "a_spread_ms_per_phase": spread(ms["a_loop_phase"]),
           "b_phase_ms_per_phase": b, "b_phase_ms_per_step": None if b is None else round(b / steps, 4),
           "b_spread_ms_per_phase": spread(ms["b_phase_whole"]),
           "b_split_ms_per_phase": {k: med(v) for k, v in split.items()},
           "b_steps_ms_per_step": None if not split["steps_s"] else round(med(split["steps_s"]) / steps, 4)}
    if b is not None:
        rec["speedup_b_vs_a"] = round(a / b, 2)
        rec["b_beats_a_by_more_than_a_spread"] = bool(a - b > rec["a_spread_ms_per_phase"])
    if parent is not None:
        assert parent["steps_per_phase"] == steps
        p, c = parent["parent_ms_per_phase"], ms["c_l2control_phase_whole"]
        rec["parent_what"] = ("(p) imagine as the revision before ro_settle_dissipation runs it under this objective (the loop "
                              "tier, Worker.rollout), in a process of its own before this one; (c) the kernel tier of an "
                              "l2control scene of the same shape, alternated with (b), for information")
        rec.update({"p_parent_ms_per_phase_rounds": p, "p_parent_gc_ms_in_window": parent.get("parent_gc_ms_in_window"), "p_parent_ms_per_phase": med(p), "p_parent_ms_per_step": round(med(p) / steps, 4),
                    "p_range_ms_per_phase": [min(p), max(p)], "b_range_ms_per_phase": [round(min(ms["b_phase_whole"]), 3),
                                                                                      round(max(ms["b_phase_whole"]), 3)],
                    "speedup_b_vs_parent": round(med(p) / b, 2),
                    "b_faster_than_parent_by_more_than_both_ranges": bool(med(p) - b > spread(p) + spread(ms["b_phase_whole"])),
                    "c_l2control_ms_per_phase": med(c), "c_l2control_ms_per_step": round(med(c) / steps, 4),
                    "c_range_ms_per_phase": [round(min(c), 3), round(max(c), 3)],
                    "c_steps_ms_per_step": round(med(split_c["steps_s"]) / steps, 4)})
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
