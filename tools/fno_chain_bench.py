#!/usr/bin/env python3
"""Timings of the one-launch free-running FNO rollout (``fno_forward_chain``) and of the surrogate-update phase over an FNO
member on an MI355X.

  (a) rollout   ``module._full_rollout`` under ``no_grad`` for a ``BurgersFNO`` with seeded random weights, tau = 5, with
                ``PDECONTROL_FNO_CHAIN=1`` (the teacher-forced ``fno_forward`` launch, then one ``fno_forward_chain``) and with
                ``PDECONTROL_FNO_CHAIN=0`` (one ``fno_forward`` per free-running step), at N = 512, B = 128, T = 35 (the
                Burgers test phase's batch) and at N = 512, B = 64, T = 20.
                Judged: the chain is the default only if at BOTH shapes its median is below the per-step route's by more
                than the two ranges added together, a range leaving out any single round above twice its route's median.
  (b) phase     ``update_surrogate`` on the kernel tier and with ``tier="loop"`` for a ``BurgersFNO`` member over a device
                replay of 4 000 rows (40 scripted episodes of 100 steps, N = 512, the controller's connector), windows of
                20 steps in batches of 64: ``--epochs`` epochs (training and validation) per call, the phase's own ``timings``
                (a device synchronisation at every lap) per training step and per validation epoch.  Recorded, not judged.

One process; two warm-up calls of every route (they capture the graphs), then the routes alternated over ``--rounds``
rounds, one call a round; the host clock around a device synchronisation; every round, the median and the range.

Usage (repo root, on an MI355X):  python tools/fno_chain_bench.py --out profiles/fno_chain_bench.json
"""
import argparse
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

N, TAU = 512, 5
SHAPES = ((128, 35), (64, 20))
EPISODES, EPISODE_STEPS, WINDOW, BATCH = 40, 100, 20, 64


def connector(env):
    """The controller's connector (pdecontrol/mbrl/mbrl.py, setup_transforms) with fixed observation bounds."""
    from pdegym.common import transforms as tr
    oscaling = tr.ScaleTransform(bounds=(np.full((1, 1, 1), -3.0, np.float32), np.full((1, 1, 1), 3.0, np.float32)),
                                 batched=True, aggregate=True, frozen=True)
    forcing = tr.BatchTransform(env.forcing)
    low = np.asarray(env.single_action_space.low)[np.newaxis, ...]
    high = np.asarray(env.single_action_space.high)[np.newaxis, ...]
    lo, hi = np.squeeze(forcing(low), axis=0), np.squeeze(forcing(high), axis=0)
    pdescaling = tr.BatchTransform(tr.ScaleTransform(bounds=(lo, hi), scale=(-1, 1), aggregate=True, frozen=True))
    sensor = tr.BatchTransform(tr.SensorTransform(stride=1))
    return tr.SampleTransform([oscaling, sensor], [forcing, pdescaling, sensor])


def member(env, stransf, dev, seed=0):
    """A ``BurgersFNO`` training module as the controller builds it: delta statistics in a ``Normalize`` that the
    surrogate's ``dscaling`` and the module's ``undscaling`` share."""
    from pdecontrol.architectures.fno import BurgersFNO
    from pdecontrol.surrogates.training import PDETrainingModule
    from pdegym.common import transforms as tr
    torch.manual_seed(seed)
    norm = tr.Normalize(aggregate=True, batched=True)
    norm.mean, norm.var, norm.count = torch.full((1, 1, 1), 0.01), torch.full((1, 1, 1), 0.5), 100
    und = tr.BatchTransform(norm)
    tstep = env.cfg_steps * env.dt
    f = BurgersFNO()
    sur = f.surrogate(delta=tstep, dscaling=und.Inverse, tau=TAU, **f.model())
    return PDETrainingModule(surrogate=sur, loss=torch.nn.MSELoss(reduction="none"), tstep=tstep, delta=tstep, undscaling=und,
                             env=env, stransf=stransf, tau=TAU, tbtt=10).to(dev)


def batch(stransf, b, t, dev):
    g = torch.Generator().manual_seed(b + t)
    x = torch.linspace(0, 2 * np.pi, N + 1)[:-1]
    raw = sum(torch.rand(b * t, 1, 1, generator=g) / (k + 1) * torch.sin((k + 1) * x + 6 * torch.rand(b * t, 1, 1, generator=g))
              for k in range(4))
    raw_actions = 2 * torch.rand(b * t, 1, 4, generator=g) - 1
    return (stransf.otransf(raw).reshape(b, t, 1, N).to(dev), stransf.atransf(raw_actions).reshape(b, t, 1, N).to(dev))


def device_replay(dev):
    """40 scripted episodes of 100 steps (a smooth travelling field, uniform actions) in a ``DeviceExperienceReplay``."""
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    from pdecontrol.mbrl.replay import ExperienceReplay
    from pdecontrol.mbrl.types import Sample
    rs = np.random.RandomState(3)
    x = np.linspace(0, 2 * np.pi, N, endpoint=False)
    host = ExperienceReplay()
    for _ in range(EPISODES):
        phase, amp = rs.uniform(0, 6), rs.uniform(0.5, 1.5)
        t = np.arange(EPISODE_STEPS + 1)[:, None]
        field = (amp * np.sin(x[None, :] + phase + 0.03 * t) + 0.5 * np.cos(2 * x[None, :] - 0.02 * t)).astype(np.float32)[:, None, :]
        acts = rs.uniform(-1, 1, (EPISODE_STEPS, 1, 4)).astype(np.float32)
        for k in range(EPISODE_STEPS):
            host.add([Sample(field[k], acts[k], field[k + 1], np.float32(-1.0), False, k == EPISODE_STEPS - 1, np.int32(k + 1))])
    sink = DeviceExperienceReplay(device=dev)
    sink.extend(host)
    return sink


def timed(call):
    """ms of one call between two device synchronisations, on the host clock."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def summary(values):
    med = float(np.median(values))
    kept = [v for v in values if v <= 2 * med]
    # the range leaves out a single round above twice the median (reported beside it, as DESIGN 4.26 reports its outliers)
    if len(values) - len(kept) > 1:
        kept = list(values)
    return {"rounds": [round(v, 4) for v in values], "median": round(med, 4), "min": round(min(values), 4),
            "max": round(max(values), 4), "range_without_one_outlier": round(max(kept) - min(kept), 4),
            "outliers": [round(v, 4) for v in values if v not in kept]}


def alternate(routes, rounds):
    for call in routes.values():
        for _ in range(2):                                              # two warm-up calls each
            call()
    out = {name: [] for name in routes}
    for _ in range(rounds):
        for name, call in routes.items():
            out[name].append(call())
    return out


def bench_rollout(module, stransf, dev, rounds):
    rec = {}
    for b, t in SHAPES:
        states, actions = batch(stransf, b, t, dev)

        def route(switch):
            def call():
                os.environ["PDECONTROL_FNO_CHAIN"] = switch

                def run():
                    with torch.no_grad():
                        module._full_rollout(states, actions)
                try:
                    return timed(run)
                finally:
                    os.environ.pop("PDECONTROL_FNO_CHAIN", None)
            return call

        ms = alternate({"chain": route("1"), "per_step": route("0")}, rounds)
        row = {name: summary(v) for name, v in ms.items()}
        gain = row["per_step"]["median"] - row["chain"]["median"]
        noise = row["per_step"]["range_without_one_outlier"] + row["chain"]["range_without_one_outlier"]
        row["gain_ms"], row["ranges_added_ms"], row["chain_wins"] = round(gain, 4), round(noise, 4), bool(gain > noise)
        # the two routes computed the same bytes
        os.environ["PDECONTROL_FNO_CHAIN"] = "0"
        with torch.no_grad():
            want = module._full_rollout(states, actions)
        os.environ["PDECONTROL_FNO_CHAIN"] = "1"
        with torch.no_grad():
            got = module._full_rollout(states, actions)
        os.environ.pop("PDECONTROL_FNO_CHAIN", None)
        row["same_bytes"] = bool(torch.equal(got.outputs, want.outputs) and torch.equal(got.deltas, want.deltas))
        rec[f"N{N}_B{b}_T{t}"] = row
    rec["chain_is_the_default"] = all(row["chain_wins"] for row in rec.values())
    return rec


def bench_phase(env, stransf, dev, rounds, epochs):
    from pdecontrol.mbrl.surrogate_phase import FitState, update_surrogate
    from pdecontrol.surrogates.common.datamodule import PDEDataModule
    from pdecontrol.surrogates.common.schedulers import StepScheduler
    sink = device_replay(dev)
    keys = list(sink.episodes)
    cut = int(0.8 * len(keys))

    def route(tier):
        module, fit = member(env, stransf, dev, seed=1), FitState()
        dm = PDEDataModule(data=sink.data, train=keys[:cut], val=keys[cut:], bootstrapping=True, stransf=stransf, tau=TAU,
                           batch_size=BATCH, device_data=dev,
                           curriculum=StepScheduler(steptype="epoch", steps=[], values=[WINDOW - TAU]))

        def call():
            np.random.seed(11)
            timings = {}
            before = fit.global_step
            update_surrogate(module, dm, fit, max_steps=10 ** 6, min_steps=0, patience=10 ** 6, max_epochs=epochs, timings=timings,
                             **({} if tier is None else {"tier": tier}))
            assert timings["tier"] == ("kernel" if tier is None else "loop"), (timings, fit.tier_reason)
            timings["steps"] = fit.global_step - before
            return timings
        return call

    raw = alternate({"kernel": route(None), "loop": route("loop")}, rounds)
    rec = {"rows": int(sink.ntimesteps), "window": WINDOW, "batch": BATCH, "epochs_per_call": epochs,
           "training_steps_per_call": sorted({c["steps"] for calls in raw.values() for c in calls})}
    for name, calls in raw.items():
        rec[name] = {"train_ms_per_step": summary([1e3 * c["train_s"] / c["steps"] for c in calls]),
                     "validation_ms_per_epoch": summary([1e3 * c["validation_s"] / epochs for c in calls]),
                     "plan_ms_per_call": summary([1e3 * c["plan_s"] for c in calls])}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--skip-phase", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    from pdegym.burgers import BurgersBatchedVecEnv
    env = BurgersBatchedVecEnv(1, N=N, device=dev.index)
    stransf = connector(env)
    rec = {"what": "fno_forward_chain against one fno_forward per free-running step (module._full_rollout under no_grad, BurgersFNO, "
                   "tau = 5), and update_surrogate over an FNO member on its kernel tier against tier='loop'; ms; two warm-up "
                   "calls a route, routes alternated, host clock around a device synchronisation; every round, the median, "
                   "the range", "rounds": args.rounds, "device": torch.cuda.get_device_name(dev)}
    rec["rollout"] = bench_rollout(member(env, stransf, dev), stransf, dev, args.rounds)
    if not args.skip_phase:
        rec["update_surrogate"] = bench_phase(env, stransf, dev, args.rounds, args.epochs)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
