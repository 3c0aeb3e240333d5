#!/usr/bin/env python3
"""Timings of the imagined-rollout phase over the Burgers / FNO world.  Record only: no ratio is fixed in
advance.

Configuration: N = 512, ``--envs`` (100) imagined trajectories, ``--members`` (3) seeded ``FNOAutoRegSurrogate`` members,
horizon ``--horizon`` (5), ``--phase-rounds`` (10) rounds per phase, ``--phases-per-timing`` (4) phases per timed window
(a single phase takes tens of ms; seconds are reported per phase), the controller's wrapper stack with the forcing at
full width and an agent sensor of stride 4 (128 observation columns, a width of the fused SAC kernels).  Every comparison
is warmed up twice, then alternated over ``--rounds`` rounds in one process, the host clock around work that ends in a
device synchronisation; medians and ranges are reported.

  (i)  phase   (a) the loop tier, ``Worker(stack).rollout`` (the world itself is device-resident);
               (b) the kernel tier with ``PDECONTROL_FNO_SELECT=0``: every member's ``fno_forward``, ``ro_settle`` over all;
               (c) the kernel tier with ``fno_forward_select``: one evaluation per env.
               Each route keeps its own world, stack, agent and captured graphs.
  (ii) C ABI   ``--members`` ``fno_forward`` launches against one ``fno_forward_select`` at B = 100 and B = 1024 (the
               picked rows are compared once, byte for byte).

Usage (repo root, on an MI355X):  python tools/burgers_imagination_bench.py   (writes profiles/burgers_imagination_bench.json)
"""
import argparse
import ctypes
import gc
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

N, TAU, STRIDE, CFG_STEPS = 512, 3, 4, 50


def timed(call):
    gc.collect()                 # a phase builds thousands of deques: their collection stays outside the timed window
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


def beats(seconds, fast, slow):
    """Whether ``fast``'s median is below ``slow``'s by more than the two ranges together."""
    f, s = np.asarray(seconds[fast]), np.asarray(seconds[slow])
    return bool(np.median(s) - np.median(f) > (f.max() - f.min()) + (s.max() - s.min()))


# ----------------------------------------------------------------------------------------------------------------------
# (i) the phase
# ----------------------------------------------------------------------------------------------------------------------
def scene(dev, envs, members, horizon, objective="l2control"):
    """(world, starting states, PDEEnvStack, agent) over a real ``BurgersBatchedVecEnv`` as the reward owner."""
    from pdecontrol.architectures.fno import BurgersFNO
    from pdecontrol.mbrl.replay import ExperienceReplay
    from pdecontrol.mbrl.types import Sample
    from pdecontrol.mbrl.worker import PDEEnvStack
    from pdecontrol.mbrl.world.world import WorldVecEnv
    from pdecontrol.sac.sac import SAC
    from pdecontrol.surrogates.common import dataset as ds
    from pdecontrol.surrogates.surrogate import PDEEnsemble
    from pdecontrol.surrogates.training import PDETrainingModule
    from pdegym.burgers.burgers import BurgersBatchedVecEnv
    from pdegym.common import transforms as T
    from pdegym.common import vec_wrappers as W
    env = BurgersBatchedVecEnv(envs, N=N, cfg_steps=CFG_STEPS, device=dev.index, objective=objective)   # never stepped
    tstep = env.cfg_steps * env.dt
    oscaling = T.ScaleTransform(bounds=(np.full((1, 1, 1), -3.0, np.float32), np.full((1, 1, 1), 3.0, np.float32)),
                                batched=True, aggregate=True, frozen=True)
    low = np.asarray(env.single_action_space.low)[np.newaxis, ...]
    high = np.asarray(env.single_action_space.high)[np.newaxis, ...]
    ascaling = T.ScaleTransform(bounds=(low, high), aggregate=True, frozen=True, batched=True).Inverse
    forcing = T.BatchTransform(env.forcing)
    lo, hi = np.squeeze(forcing(low), axis=0), np.squeeze(forcing(high), axis=0)
    pdescaling = T.BatchTransform(T.ScaleTransform(bounds=(lo, hi), scale=(-1, 1), aggregate=True, frozen=True))
    agent_sensor = T.BatchTransform(T.SensorTransform(stride=STRIDE))
    world_sensor = T.BatchTransform(T.SensorTransform(stride=1))
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
        f = BurgersFNO()
        sur = f.surrogate(delta=tstep, dscaling=None, tau=TAU, **f.model())
        modules.append(PDETrainingModule(surrogate=sur, loss=torch.nn.MSELoss(reduction="none"), tstep=tstep, delta=tstep,
                                         tau=TAU, tbtt=10).to(dev))
    world = WorldVecEnv(surrogate=PDEEnsemble(modules, num_elites=members), observation_space=env.single_observation_space,
                        action_space=env.single_action_space, max_episode_steps=env.max_episode_steps,
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
    O = len(range(STRIDE // 2, N, STRIDE))
    box = lambda lo_, hi_, n: Namespace(low=np.full((1, n), lo_, np.float32), high=np.full((1, n), hi_, np.float32), shape=(1, n))
    cfg = Namespace(gamma=0.99, tau=0.005, alpha=0.2, policy="Gaussian", target_update_interval=1,
                    automatic_entropy_tuning=False, cuda=False, device=dev, hidden_size=256, lr=3e-4)
    torch.manual_seed(0)
    agent = SAC(box(-np.inf, np.inf, O), box(-1.0, 1.0, 4), cfg, logger=None)
    return world, starting, PDEEnvStack(envs=astore, ostore=ostore, astore=astore, world_wrapper=None), agent


def phase_route(dev, args, route):
    from pdecontrol.mbrl import imagination_phase as ip
    from pdecontrol.mbrl.worker import Worker
    world, starting, stack, agent = scene(dev, args.envs, args.members, args.horizon)
    world.setup(starting)
    rollouts = args.phase_rounds * args.envs
    seen = {"tiers": set(), "timesteps": 0, "select": set()}

    def phase():
        for _ in range(args.phases_per_timing):
            one_phase()

    def one_phase():
        if route == "a_loop":
            got = Worker(stack).rollout(agent, lambda ts, eps: eps >= rollouts)
            seen["tiers"].add("loop")
        else:
            os.environ["PDECONTROL_FNO_SELECT"] = "0" if route == "b_generic" else "1"
            timings = {}
            try:
                got = ip.imagine(agent, stack, rollouts, timings=timings)
            finally:
                os.environ.pop("PDECONTROL_FNO_SELECT", None)
            seen["tiers"].add(timings["tier"])
            seen["select"].add(bool(world._imagination.select))
        seen["timesteps"] = got.ntimesteps

    return phase, seen


def phases(dev, args):
    names = ("a_loop", "b_generic", "c_select")
    routes = {name: phase_route(dev, args, name) for name in names}
    seconds = alternate({name: phase for name, (phase, _) in routes.items()}, args.rounds)
    row = {}
    seconds = {name: list(np.asarray(s) / args.phases_per_timing) for name, s in seconds.items()}     # per phase
    for name, (_, seen) in routes.items():
        steps = seen["timesteps"] // args.envs
        row[name] = {**summary(seconds[name]), "timesteps": seen["timesteps"], "steps_per_phase": steps,
                     "us_per_step": round(float(np.median(seconds[name])) / steps * 1e6, 3), "tiers": sorted(seen["tiers"])}
    assert routes["b_generic"][1]["tiers"] == routes["c_select"][1]["tiers"] == {"kernel"}, row
    assert routes["b_generic"][1]["select"] == {False} and routes["c_select"][1]["select"] == {True}, row
    steps = row["c_select"]["steps_per_phase"]
    row["b_minus_c_us_per_step"] = round((row["b_generic"]["median_s"] - row["c_select"]["median_s"]) / steps * 1e6, 3)
    row["b_over_c"] = round(row["b_generic"]["median_s"] / row["c_select"]["median_s"], 3)
    row["b_over_c_range"] = [round(min(seconds["b_generic"]) / max(seconds["c_select"]), 3),
                             round(max(seconds["b_generic"]) / min(seconds["c_select"]), 3)]
    row["a_over_c"] = round(row["a_loop"]["median_s"] / row["c_select"]["median_s"], 3)
    row["select_beats_generic_by_more_than_both_ranges"] = beats(seconds, "c_select", "b_generic")
    return row


# ----------------------------------------------------------------------------------------------------------------------
# (ii) members x fno_forward against one fno_forward_select
# ----------------------------------------------------------------------------------------------------------------------
def c_abi(dev, B, members, rounds, reps):
    from pdecontrol.architectures.fno import FNO1d
    from pdecontrol.surrogates import fno_hip
    lib = fno_hip.load()
    rs = np.random.RandomState(B)
    x = np.linspace(0, 2 * np.pi, N, endpoint=False)
    rows = lambda: torch.from_numpy(np.stack([np.sin(x + rs.uniform(0, 6)) + 0.5 * np.cos(2 * x + rs.uniform(0, 6))
                                              for _ in range(B)]).astype(np.float32)).to(dev)
    u, act = rows(), rows()
    structs, keep = [], []
    for m in range(members):
        torch.manual_seed(100 + m)
        w, ps = fno_hip._weights_struct(fno_hip.parameters_of(FNO1d().to(dev)))
        structs.append(w)
        keep.append(ps)
    cscale, cshift = [0.05 * (1 + 0.1 * m) for m in range(members)], [0.01 * m for m in range(members)]
    chosen = torch.from_numpy(rs.randint(0, members, (1, B)).astype(np.int32)).to(dev)
    outs = [torch.empty((B, N), device=dev) for _ in range(members)]
    delta, picked = torch.empty((B, N), device=dev), torch.empty((B, N), device=dev)
    ws = (fno_hip.FnoWeights * members)(*structs)
    a = fno_hip.FnoSelectArgs(ws, (ctypes.c_float * members)(*cscale), (ctypes.c_float * members)(*cshift), members,
                              chosen.data_ptr(), None, 1, u.data_ptr(), act.data_ptr(), picked.data_ptr())

    def forwards():
        st = fno_hip._stream()
        for _ in range(reps):
            for m in range(members):
                fno_hip._check(lib.fno_forward(st, ctypes.byref(structs[m]), 32, 16, 4, N, B, B, fno_hip._ptr(u), 0, N,
                                               fno_hip._ptr(act), 0, N, cscale[m], cshift[m], fno_hip._ptr(delta),
                                               fno_hip._ptr(outs[m]), None, None, 0, 0))

    def select():
        st = fno_hip._stream()
        for _ in range(reps):
            fno_hip.forward_select(st, N, B, a)

    seconds = alternate({"forwards": forwards, "select": select}, rounds)
    torch.cuda.synchronize()
    want = torch.stack(outs)[chosen[0].long(), torch.arange(B, device=dev)]
    same = want.cpu().numpy().tobytes() == picked.cpu().numpy().tobytes()
    row = {name: {**summary(np.asarray(s) / reps), "us_per_step": round(float(np.median(s)) / reps * 1e6, 3)}
           for name, s in seconds.items()}
    row.update(members=members, reps_per_timing=reps, rows_identical=bool(same),
               forwards_over_select=round(row["forwards"]["median_s"] / row["select"]["median_s"], 3),
               forwards_over_select_range=[round(min(seconds["forwards"]) / max(seconds["select"]), 3),
                                           round(max(seconds["forwards"]) / min(seconds["select"]), 3)])
    assert same, row
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--envs", type=int, default=100)
    ap.add_argument("--members", type=int, default=3)
    ap.add_argument("--horizon", type=int, default=5)
    ap.add_argument("--phase-rounds", type=int, default=10)
    ap.add_argument("--phases-per-timing", type=int, default=4)
    ap.add_argument("--batches", default="100,1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "burgers_imagination_bench.json"))
    args = ap.parse_args()
    assert args.rounds >= 7, "at least 7 alternated rounds"
    dev = torch.device("cuda", 0)
    report = {"device": torch.cuda.get_device_name(0), "N": N, "envs": args.envs, "members": args.members,
              "horizon": args.horizon, "rounds_per_phase": args.phase_rounds, "agent_sensor_stride": STRIDE,
              "rounds": args.rounds, "phases_per_timing": args.phases_per_timing}
    report["i_phase"] = phases(dev, args)
    print("phase", json.dumps(report["i_phase"]), flush=True)
    report["ii_c_abi"] = {}
    for B in (int(v) for v in args.batches.split(",")):
        report["ii_c_abi"][f"B{B}"] = c_abi(dev, B, args.members, args.rounds, reps=100 if B <= 128 else 40)
        print(f"B{B}", json.dumps(report["ii_c_abi"][f"B{B}"]), flush=True)
    select_default = report["i_phase"]["select_beats_generic_by_more_than_both_ranges"]
    report["default_route"] = "select" if select_default else "generic"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
