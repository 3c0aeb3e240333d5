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

Usage (repo root, on an MI355X):  python tools/imagination_phase_bench.py    (writes profiles/imagination_phase_bench.json)
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

TAU = 3


def scene(dev, envs, members, horizon):
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
    env = KuramotoSivashinskyEnv()                 # never stepped: forcing, spaces and the reward only
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


def timed(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--envs", type=int, default=100)
    ap.add_argument("--members", type=int, default=3)
    ap.add_argument("--horizon", type=int, default=5)
    ap.add_argument("--rollouts", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imagination_phase_bench.json"))
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--loop-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    if not args.loop_only:
        from pdecontrol.mbrl import imagination_phase as ip
        from pdecontrol.mbrl.worker import PDEEnvStack

    scenes = {name: scene(dev, args.envs, args.members, args.horizon) for name in ("a_loop", "b_phase")}
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
    if not args.loop_only:
        stack = PDEEnvStack(*stack_b)
        assert ip.imagine(agent_b, stack, args.rollouts).ntimesteps == steps * args.envs
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        ms["a_loop_phase"].append(1e3 * timed(route_a)[0])
        if args.loop_only:
            continue
        whole, _ = timed(lambda: ip.imagine(agent_b, stack, args.rollouts))       # untimed inside: one sync per round
        ms["b_phase_whole"].append(1e3 * whole)
        timings = {}
        ip.imagine(agent_b, stack, args.rollouts, timings=timings)
        assert timings["tier"] == "kernel", timings
        for k in split:
            split[k].append(1e3 * timings[k])

    med = lambda v: round(float(np.median(v)), 4) if v else None
    spread = lambda v: round(max(v) - min(v), 4) if v else None
    a, b = med(ms["a_loop_phase"]), med(ms["b_phase_whole"])
    rec = {"what": "imagined-rollout phase: ms per phase and per imagined step (one step of all envs) of (a) the per-step "
                   "loop over the wrapper stack and (b) imagine on the kernel tier; routes alternated in one process, medians "
                   "over the rounds; host clock around work ending in a device synchronisation; the split of (b) comes from "
                   "separate phases that synchronise after each part",
           "device": torch.cuda.get_device_name(dev), "envs": args.envs, "members": args.members, "horizon": args.horizon,
           "rollouts": args.rollouts, "steps_per_phase": int(steps), "rounds": args.rounds,
           "ms_per_phase": {k: [round(x, 3) for x in v] for k, v in ms.items()},
           "a_loop_ms_per_phase": a, "a_loop_ms_per_step": None if a is None else round(a / steps, 4),
           "a_spread_ms_per_phase": spread(ms["a_loop_phase"]),
           "b_phase_ms_per_phase": b, "b_phase_ms_per_step": None if b is None else round(b / steps, 4),
           "b_spread_ms_per_phase": spread(ms["b_phase_whole"]),
           "b_split_ms_per_phase": {k: med(v) for k, v in split.items()},
           "b_steps_ms_per_step": None if not split["steps_s"] else round(med(split["steps_s"]) / steps, 4)}
    if b is not None:
        rec["speedup_b_vs_a"] = round(a / b, 2)
        rec["b_beats_a_by_more_than_a_spread"] = bool(a - b > rec["a_spread_ms_per_phase"])
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
