#!/usr/bin/env python3
"""Timings of the real-env collection phase with the real replay kept in HBM.  Record only.

The scene is tools/collection_phase_bench.py's: the controller's collection stack over a ``KSBatchedVecEnv`` in fast step
mode, a SAC agent (hidden 256) on the same GPU, phases of ``--steps`` (8) steps of all envs without a truncation, at
``--sizes`` (1024x64 and 4096x256).  Two routes, both warmed up twice, then alternated over ``--rounds`` rounds in one
process, the host clock around work that ends in a device synchronisation:

  (a) host   ``collect`` without a sink, then ``replay.extend`` on a host ``ExperienceReplay``: calls the revision before
             the sink has, so that ``--host-only`` times the same route there, in a process of its own.
  (b) sink   ``collect(sink=replay)`` then ``replay.extend`` on a ``DeviceExperienceReplay``.

Both replays are unbounded: no phase evicts.  Route (b) is also run in phases that synchronise after each part
(``b_split``: the reservation, the write-back of the host state, the commit; the rest is the enqueue of the steps and of
``ks_record_device``, the tail copies and the wait for them).

  --profile-run SIZE   one warmed-up phase of route (b) at one size and nothing else: the program to put behind
                       ``rocprofv3 --kernel-trace --stats``
  --kernel-trace CSV   ``*_kernel_trace.csv`` files of such runs ("1024x64=path,4096x256=path"): the median device time per
                       launch of the KS kernel and of ``ks_record_device`` is read from them and the criterion
                       (b) - ks <= 0.5 * ((a) - ks) is evaluated per size against (a)'s median and its minimum
  --readers            also time, without a criterion, ``update_policy``'s pack lap over a real replay of 4 000 steps
                       (a view against the packed host replay) and the store of ``world.setup``'s starting states (the
                       window store against the pack)

Usage (repo root, on an MI355X):  python tools/real_replay_bench.py    (writes profiles/real_replay_bench.json)
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "model-based-pde-control_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from collection_phase_bench import scene, timed  # noqa: E402


def kernel_times(path):
    want = {"ks": ("ks_rk4",), "ks_record_device": ("ks_record_kernel",)}
    seen = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name", "")
            for key, needles in want.items():
                if any(n in name for n in needles):
                    seen.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: {"launches": len(v), "us_per_launch": round(float(np.median(v)), 3),
                "range_us": [round(min(v), 3), round(max(v), 3)]} for k, v in seen.items()}


def primed_worker(dev, E, N):
    from pdecontrol.mbrl.worker import Worker
    stack, agent, _ = scene(dev, E, N)
    worker = Worker(stack)
    worker._last_obs = stack.envs.reset(seed=1)
    worker._last_stored_obs = stack.ostore.obs.copy()[stack.ostore.mask]
    return worker, agent


def split_phase(cp, worker, agent, stop, sink, out):
    """One phase of route (b) with a synchronisation after each part; the parts' seconds go to the empty dict ``out``."""
    clock, sync = time.perf_counter, torch.cuda.synchronize

    def wrap(owner, name, key):
        plain = getattr(owner, name)

        def timed_part(*args, **kwargs):
            sync()
            t0 = clock()
            result = plain(*args, **kwargs)
            sync()
            out[key] = out.get(key, 0.0) + clock() - t0
            return result

        setattr(owner, name, timed_part)
        return lambda: setattr(owner, name, plain)

    undo = [wrap(cp._SinkPhase, "reserve", "staging"), wrap(cp, "_restore", "write_back")]
    try:
        sync()
        t0 = clock()
        staged = cp.collect(worker, agent, stop, sink=sink)
        sync()
        total = clock() - t0
    finally:
        for u in undo:
            u()
    t0 = clock()
    sink.extend(staged)
    sync()
    out["commit"] = out.get("commit", 0.0) + clock() - t0
    out["enqueue_tail_copies_and_wait"] = total - out.get("staging", 0.0) - out.get("write_back", 0.0)


def readers(dev, real_steps=4000):
    """``update_policy``'s pack lap and the store of the world's starting states, over the slabs and over the pack."""
    import _policy_phase_scenario as pp_sc
    from pdecontrol.mbrl import policy_phase as pp
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    from pdecontrol.mbrl.replay import ExperienceReplay
    from pdecontrol.mbrl.world.world import _DeviceStartingStates
    from pdecontrol.surrogates.common.dataset import StartingStateDataset, SubSeqDataset
    import _sac_models as sm
    build_agent = lambda dev: sm.build(256, obs_dim=64, act_dim=4, seed=0, device=str(dev))
    rollout = pp_sc.scripted_replay(64, 4, 1, real_steps // 4, {e: tuple(range(100, real_steps, 100)) for e in range(4)})
    host, sink = ExperienceReplay(), DeviceExperienceReplay(device=dev)
    host.extend(rollout)
    sink.extend(rollout)
    _, to_agent = pp_sc.controller_connectors(4, width=64)
    out = {"real_steps": host.ntimesteps, "update_policy_pack_ms": {}, "starting_states_store_ms": {}}
    for name, make in (("packed", lambda: SubSeqDataset(data=host.data, length=1, stride=1, bootstrapping=False, stransf=to_agent)),
                       ("view", lambda: sink.dataset(to_agent))):
        laps = []
        for _ in range(4):
            agent, timings = build_agent(dev), {}
            pp.update_policy(agent, [make()], 256, 2, timings=timings)
            laps.append(1e3 * timings["pack_s"])
        out["update_policy_pack_ms"][name] = {"first": round(laps[0], 3), "median_of_the_rest": round(float(np.median(laps[1:])), 3),
                                              "tier": timings["tier"]}
    for name, data in (("packed", host.data), ("window_store", None)):
        laps = []
        for i in range(4):
            if data is None:
                sink._window_store = None                  # a new state of the replay: the map is built and uploaded again
            starting = StartingStateDataset(data=sink.data if data is None else data, length=3, stride=1, bootstrapping=False)
            laps.append(1e3 * timed(lambda: _DeviceStartingStates(starting, dev, 64).next_batch())[0])
        out["starting_states_store_ms"][name] = {"first": round(laps[0], 3), "median_of_the_rest": round(float(np.median(laps[1:])), 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--sizes", default="1024x64,4096x256")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "real_replay_bench.json"))
    ap.add_argument("--profile-run", default=None, metavar="SIZE")
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--readers", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    from pdecontrol.mbrl import collection_phase as cp
    from pdecontrol.mbrl.replay import ExperienceReplay
    sizes = [tuple(int(v) for v in s.split("x")) for s in (args.profile_run or args.sizes).split(",")]
    med = lambda v: round(float(np.median(v)), 4) if v else None
    per_step = lambda v: None if v is None else round(v / args.steps, 4)

    def phase_a(worker, agent, E, replay):
        rollout = cp.collect(worker, agent, lambda ts, ep: ts >= args.steps * E)
        assert rollout.tier == "kernel" and rollout.host_steps == 0, (rollout.tier, rollout.tier_reason, rollout.host_steps)
        replay.extend(rollout)

    def phase_b(worker, agent, E, sink):
        staged = cp.collect(worker, agent, lambda ts, ep: ts >= args.steps * E, sink=sink)
        assert staged.tier == "kernel" and staged.host_steps == 0, (staged.tier, staged.tier_reason, staged.host_steps)
        sink.extend(staged)

    if not args.host_only:
        from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    if args.profile_run:
        (E, N), = sizes
        worker, agent = primed_worker(dev, E, N)
        sink = DeviceExperienceReplay(device=dev, rows=4 * args.steps * E)
        for _ in range(3):
            phase_b(worker, agent, E, sink)
        torch.cuda.synchronize()
        return

    stats = dict(kv.split("=") for kv in args.kernel_trace.split(",")) if args.kernel_trace else {}
    rec = {"what": "real-env collection phase with its commit to the real replay: ms per phase and per step (one step of all "
                   "envs) of (a) collect without a sink + extend on a host ExperienceReplay and (b) collect(sink=) + extend on "
                   "a DeviceExperienceReplay; routes alternated in one process after a warm-up of both, medians and ranges "
                   "over the rounds; host clock around work ending in a device synchronisation; device times per launch come "
                   "from a separate rocprofv3 --kernel-trace --stats run of route (b)",
           "device": torch.cuda.get_device_name(dev), "steps_per_phase": args.steps, "rounds": args.rounds, "step_mode": "fast",
           "host_only": bool(args.host_only), "claims_from_code_reading_not_from_a_trace": [
               "no sample crosses to the host between ks_step_device and rp_gather on route (b) (the tail copies carry one "
               "observation row and one action row per env, the policy's observation, the bounds and the status)",
               "route (b) adds one launch (ks_record_device) and one upload (dst and steps) per segment"],
           "sizes": {}}
    for E, N in sizes:
        worker_a, agent_a = primed_worker(dev, E, N)
        host = ExperienceReplay()
        if not args.host_only:
            worker_b, agent_b = primed_worker(dev, E, N)
            sink = DeviceExperienceReplay(device=dev, rows=(4 + 2 * args.rounds) * args.steps * E)
        for _ in range(2):                               # warm-up: code objects, the allocator, pinned staging, clocks
            phase_a(worker_a, agent_a, E, host)
            if not args.host_only:
                phase_b(worker_b, agent_b, E, sink)
        ms, split = {"a_host": [], "b_sink": []}, {}
        for _ in range(args.rounds):
            ms["a_host"].append(1e3 * timed(lambda: phase_a(worker_a, agent_a, E, host))[0])
            if not args.host_only:
                ms["b_sink"].append(1e3 * timed(lambda: phase_b(worker_b, agent_b, E, sink))[0])
                parts = {}
                split_phase(cp, worker_b, agent_b, lambda ts, ep: ts >= args.steps * E, sink, parts)
                for k, v in parts.items():
                    split.setdefault(k, []).append(1e3 * v / args.steps)
        a, b = med(ms["a_host"]), med(ms["b_sink"])
        size = {"envs": E, "N": N, "ms_per_phase": {k: [round(x, 3) for x in v] for k, v in ms.items()},
                "a_host_ms_per_step": per_step(a), "b_sink_ms_per_step": per_step(b),
                "a_range_ms_per_step": [per_step(min(ms["a_host"])), per_step(max(ms["a_host"]))],
                "b_range_ms_per_step": [per_step(min(ms["b_sink"])), per_step(max(ms["b_sink"]))] if b else None,
                "b_split_ms_per_step": {k: med(v) for k, v in sorted(split.items())}}
        path = stats.get(f"{E}x{N}")
        if path:
            size["device_us_per_launch"] = kernel_times(path)
            ks = size["device_us_per_launch"].get("ks", {}).get("us_per_launch")
            if ks is not None and b is not None:
                ks_ms = ks / 1e3
                over_b = per_step(b) - ks_ms
                size["criterion"] = {"ks_ms_per_step": round(ks_ms, 4), "b_minus_ks": round(over_b, 4), "bound": "b - ks <= 0.5 * (a - ks)"}
                for label, value in (("median", per_step(a)), ("minimum", per_step(min(ms["a_host"])))):
                    over_a = value - ks_ms
                    size["criterion"][f"a_{label}_minus_ks"] = round(over_a, 4)
                    size["criterion"][f"holds_against_a_{label}"] = bool(over_b <= 0.5 * over_a)
        rec["sizes"][f"{E}x{N}"] = size
    if args.readers and not args.host_only:
        rec["readers_no_criterion"] = readers(dev)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
