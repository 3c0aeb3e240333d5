#!/usr/bin/env python3
"""Timings of the Burgers objectives.  Record only: nothing here chooses a route.

  (i)  stepper   ``bg_step_objective`` under the dissipation objective against ``bg_step`` of the same build, at
                 8192 x 512 and 1024 x 64 with 50 sub-steps per launch and four actuators, on the smooth initial
                 condition of the env.  One process; both legs are warmed up for ``--warmup`` seconds (until the clocks
                 settle), then alternated over ``--rounds`` (7) rounds, hipEvent pairs around ``--reps`` launches; medians
                 and ranges of the ms per launch are reported.
  (ii) phase     one imagined-rollout phase of 50 steps (100 envs x 3 FNO members, N = 512; the scene of
                 tools/burgers_imagination_bench.py) on the kernel tier under each objective: ``ro_settle`` against
                 ``ro_settle_burgers_dissipation`` at the end of the captured step.  Warmed up twice, alternated over the
                 same number of rounds, the host clock around a phase that ends in a device synchronisation.

Usage (repo root, on an MI355X):  python tools/burgers_objective_bench.py   (writes profiles/burgers_objective_bench.json)
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

CASES = [(8192, 512), (1024, 64)]
SUBSTEPS = 50


def stepper(E, N, rounds, reps, warmup):
    from hipbind import ptr
    from pdegym.burgers import _hip
    from pdegym.burgers.burgers import BurgersBatchedVecEnv, _stream
    env = BurgersBatchedVecEnv(E, N=N, cfg_steps=SUBSTEPS, device=0)
    lib = env._lib
    env.reset(seed=3)
    u0 = env.u.clone()
    actions = torch.from_numpy(np.random.RandomState(1).uniform(-1, 1, (E, 4)).astype(np.float32)).to(env.device)
    ssq = torch.zeros(E, dtype=torch.float64, device=env.device)
    status = torch.zeros(E, dtype=torch.int32, device=env.device)
    head = (ptr(env.u), ptr(actions), ptr(env._F), 4, E, N, env.dx, env.dt, env.nu, SUBSTEPS, None, ptr(ssq), ptr(status))

    def l2control():
        _hip.check(lib.bg_step(_stream(env.device), *head))

    def dissipation():
        _hip.check_objective(lib.bg_step_objective(_stream(env.device), *head, _hip.OBJECTIVES["dissipation"]))

    legs = {"bg_step": l2control, "bg_step_objective_dissipation": dissipation}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warmup:
        for call in legs.values():
            for _ in range(reps):
                call()
        torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(rounds):
        for name, call in legs.items():
            env.u.copy_(u0)                          # every timed window starts from the same state
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                call()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / reps)
    assert int(status.sum()) == 0, "non-finite state"
    row = {"num_envs": E, "N": N, "substeps": SUBSTEPS, "reps_per_window": reps}
    for name, v in ms.items():
        row[name] = {"median_ms": round(float(np.median(v)), 5), "range_ms": [round(min(v), 5), round(max(v), 5)]}
    a, b = np.asarray(ms["bg_step_objective_dissipation"]), np.asarray(ms["bg_step"])
    row["dissipation_over_l2control"] = round(float(np.median(a) / np.median(b)), 4)
    row["ratio_range"] = [round(float(a.min() / b.max()), 4), round(float(a.max() / b.min()), 4)]
    return row


def phases(rounds, envs=100, members=3, horizon=50):
    import burgers_imagination_bench as ib
    from pdecontrol.mbrl import imagination_phase as ip
    dev = torch.device("cuda", 0)
    routes, seen = {}, {}
    for objective in ("l2control", "dissipation"):
        world, starting, stack, agent = ib.scene(dev, envs, members, horizon, objective=objective)
        world.setup(starting)

        def phase(stack=stack, agent=agent, objective=objective):
            timings = {}
            got = ip.imagine(agent, stack, envs, timings=timings)
            seen[objective] = (timings["tier"], got.ntimesteps)

        routes[objective] = phase
    seconds = ib.alternate(routes, rounds)
    row = {"num_envs": envs, "members": members, "N": ib.N, "steps": horizon}
    for objective, s in seconds.items():
        assert seen[objective] == ("kernel", envs * horizon), seen
        row[objective] = ib.summary(s)
    row["dissipation_over_l2control"] = round(row["dissipation"]["median_s"] / row["l2control"]["median_s"], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "burgers_objective_bench.json"))
    args = ap.parse_args()
    out = {"tool": "burgers_objective_bench", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "stepper": [stepper(E, N, args.rounds, args.reps, args.warmup) for E, N in CASES],
           "imagination_phase": phases(args.rounds)}
    text = json.dumps(out, indent=1)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
