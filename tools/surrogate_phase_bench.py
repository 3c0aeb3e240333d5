#!/usr/bin/env python3
"""Timings of the controller's surrogate-update phase on an MI355X (pdecontrol/mbrl/surrogate_phase.py).  Record only.

Per grid width (N = 64 and N = 256): B = 64, T = 20 (tau 5 + 15), a real replay of ``--real`` (4 000) steps in episodes of
250 held in the slabs of a ``DeviceExperienceReplay``, the controller's connector (observation scaling, Gaussian forcing,
forcing scaling), hop-1 bootstrapped windows.  One process; both routes are warmed twice, then alternated over
``--rounds`` (5) rounds; every window is a host clock around work that ends in a device synchronisation; medians and
ranges are recorded.

  (a) trainer   calls the parent commit already has: the shim ``Trainer.fit`` over ``PDEDataModule(device_data=...)`` with
                a ``graphed=True`` module, ``--steps`` (200) steps.  ``--parent-only`` times this route alone, so that it
                can be run on the parent's tree in a process of its own.
  (b) phase     ``update_surrogate`` on the kernel tier for ``--steps`` steps: its plan and training seconds (``timings``);
                its validation epochs are timed separately.  200 steps do not fit in one epoch of this replay, so the
                call runs ``min_steps = max_steps = --steps`` over several epochs instead of ``max_epochs=1``, and the
                plan seconds also hold the ``val_dataloader()`` build of every epoch: work route (a), which never
                validates, has none of.  It is left in (b), which makes the criterion harder for (b), not easier.
  step         the captured TBPTT step's own time: back-to-back replays of the same graph, in the same process.

Criterion, at both widths:  (b) - step <= 0.5 * ((a) - step)  per training step, against (a)'s median and against its
minimum.  The record says whether it holds; a miss is reported as a miss.

Recorded without a criterion: one validation epoch through ``sur_val_loss`` against the torch ops of ``validation_step``
(both behind the same gather and rollout).

  --profile-run   one warmed-up phase and nothing else: the program to put behind ``rocprofv3 --kernel-trace --stats``
                  for the kernel times of ``sur_gather_windows`` and ``sur_val_loss``

Usage (repo root, on an MI355X):  python tools/surrogate_phase_bench.py    (writes profiles/surrogate_phase_bench.json)
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

B, TAU, HORIZON, A = 64, 5, 15, 4
DEV = "cuda"


def scene(N, real, graphed):
    """(module, datamodule factory) of one width: a fresh datamodule per window, the replay and the module shared."""
    from pdecontrol.architectures import KSAutoRegConvolutionalLSTM, KSAutoRegConvolutionalLSTMN
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    from pdecontrol.mbrl.replay import ExperienceReplay
    from pdecontrol.mbrl.types import Sample
    from pdecontrol.surrogates.common.datamodule import PDEDataModule
    from pdecontrol.surrogates.common.schedulers import ConstantLengthScheduler
    from pdecontrol.surrogates.training import PDETrainingModule
    from pdegym.common import transforms as T
    from pdegym.kuramoto import KuramotoSivashinskyEnv
    env = KuramotoSivashinskyEnv() if N == 64 else KuramotoSivashinskyEnv(L=88.0, N=N)
    tstep = env.cfg_steps * env.dt
    low, high = np.asarray(env.action_space.low)[None], np.asarray(env.action_space.high)[None]
    oscaling = T.ScaleTransform(bounds=(np.full((1, 1, 1), -3.0, np.float32), np.full((1, 1, 1), 3.0, np.float32)),
                                batched=True, aggregate=True, frozen=True)
    forcing = T.BatchTransform(env.forcing)
    lo, hi = np.squeeze(forcing(low), axis=0), np.squeeze(forcing(high), axis=0)
    pdescaling = T.BatchTransform(T.ScaleTransform(bounds=(lo, hi), scale=(-1, 1), aggregate=True, frozen=True))
    sensor = T.BatchTransform(T.SensorTransform(stride=1))
    stransf = T.SampleTransform([oscaling, sensor], [forcing, pdescaling, sensor])

    rs = np.random.RandomState(1)
    host = ExperienceReplay()
    x = np.linspace(0, 2 * np.pi, N, endpoint=False)
    for t in range(real):
        k, phase = t % 250, 0.37 * (t // 250)
        field = lambda kk: (np.sin(x + phase + 0.05 * kk) + 0.5 * np.cos(2 * x - 0.03 * kk)).astype(np.float32)[None, :]
        host.add([Sample(field(k), rs.uniform(-1, 1, (1, A)).astype(np.float32), field(k + 1), np.float32(-1.0), False,
                         k == 249, np.int32(k + 1))])
    sink = DeviceExperienceReplay(device=DEV)
    sink.extend(host)
    keys = list(sink.episodes)
    nval = max(1, len(keys) // 8)

    torch.manual_seed(0)
    norm = T.Normalize(aggregate=True, batched=True)
    norm.mean, norm.var, norm.count = torch.full((1, 1, 1), 0.01), torch.full((1, 1, 1), 0.5), 100
    und = T.BatchTransform(norm)
    f = KSAutoRegConvolutionalLSTM() if N == 64 else KSAutoRegConvolutionalLSTMN()
    sur = f.surrogate(delta=tstep, dscaling=und.Inverse, tau=TAU, **f.model(N=N))
    module = PDETrainingModule(surrogate=sur, loss=torch.nn.MSELoss(reduction="none"), tstep=tstep, delta=tstep, undscaling=und,
                               stransf=stransf, tau=TAU, tbtt=10, graphed=graphed).to(DEV)

    def datamodule():
        return PDEDataModule(data=sink.data, train=keys[:-nval], val=keys[-nval:], bootstrapping=True, stransf=stransf,
                             curriculum=ConstantLengthScheduler(length=HORIZON), tau=TAU, stride=1, batch_size=B,
                             device_data=DEV)
    return module, datamodule


def timed(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def spread(values):
    return {"median": float(np.median(values)), "min": float(np.min(values)), "max": float(np.max(values)),
            "values": [float(v) for v in values]}


def measure(N, args):
    from pdecontrol._compat.lightning import pl
    rec = {"N": N, "B": B, "T": TAU + HORIZON, "steps": args.steps, "real": args.real}
    trainer_module, trainer_dm = scene(N, args.real, graphed=True)

    def route_a():
        np.random.seed(0)
        trainer = pl.Trainer(max_steps=args.steps, max_epochs=10 ** 6)
        trainer.fit(trainer_module, datamodule=trainer_dm())
        assert trainer.global_step == args.steps
        return None

    if args.parent_only:
        for _ in range(2):
            route_a()
        rec["trainer_ms_per_step"] = spread([1e3 * timed(route_a)[0] / args.steps for _ in range(args.rounds)])
        return rec

    from pdecontrol.mbrl import surrogate_phase as sp
    phase_module, phase_dm = scene(N, args.real, graphed=False)

    def route_b():
        np.random.seed(0)
        timings, fit = {}, sp.FitState()
        sp.update_surrogate(phase_module, phase_dm(), fit, max_steps=args.steps, min_steps=args.steps, patience=10 ** 9,
                            timings=timings)
        assert timings["tier"] == "kernel" and fit.global_step == args.steps, (timings, fit.tier_reason)
        timings["epochs"] = len(fit.history)
        return timings

    if args.profile_run:
        for _ in range(2):
            route_b()
        return rec
    for _ in range(2):
        route_a()
        route_b()
    a, b, val = [], [], []
    for _ in range(args.rounds):
        a.append(1e3 * timed(route_a)[0] / args.steps)
        t = route_b()
        b.append(1e3 * (t["train_s"] + t["plan_s"]) / args.steps)
        val.append(1e3 * t["validation_s"] / t["epochs"])
    rec["trainer_ms_per_step"], rec["phase_ms_per_step"] = spread(a), spread(b)
    rec["phase_validation_epoch_ms"] = spread(val)

    # the captured step's own time: the graph of the full batch shape, replayed back to back
    steps = [s for key, s in phase_module.__dict__["_graphed_steps"].items() if key[0][0] == B]
    step = steps[0]
    snapshot = [p.detach().clone() for p in phase_module.surrogate.parameters()]
    own = []
    for _ in range(args.rounds):
        own.append(1e3 * timed(lambda: [step.g_main.replay() for _ in range(args.steps)])[0] / args.steps)
    with torch.no_grad():
        for p, s in zip(phase_module.surrogate.parameters(), snapshot):
            p.copy_(s)
    rec["captured_step_ms"] = spread(own)

    step_ms = rec["captured_step_ms"]["median"]
    for against in ("median", "min"):
        lhs, rhs = rec["phase_ms_per_step"]["median"] - step_ms, 0.5 * (rec["trainer_ms_per_step"][against] - step_ms)
        rec[f"criterion_against_{against}"] = {"phase_minus_step_ms": lhs, "half_trainer_minus_step_ms": rhs, "holds": bool(lhs <= rhs)}

    # one validation epoch: sur_val_loss against the torch ops of validation_step, behind the same gather and rollout
    dm = phase_dm()
    dm.trainer = sp.FitState()
    tier, reason = sp._pick_tier(phase_module, dm)
    assert tier is not None, reason
    np.random.seed(0)
    loader = dm.val_dataloader()
    routes = {"sur_val_loss": lambda: sp._validate_kernel(phase_module, tier, loader, B)}
    real_route = phase_module._fused_validation_loss

    def torch_ops():
        phase_module._fused_validation_loss = lambda *a, **k: None
        try:
            return sp._validate_kernel(phase_module, tier, loader, B)
        finally:
            phase_module._fused_validation_loss = real_route
    routes["torch_ops"] = torch_ops
    for name, call in routes.items():
        for _ in range(2):
            call()
        rec[f"validation_epoch_{name}_ms"] = spread([1e3 * timed(call)[0] for _ in range(args.rounds)])
    rec["validation_batches"] = (len(loader.dataset) + B - 1) // B
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--real", type=int, default=4000)
    ap.add_argument("--widths", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--parent-only", action="store_true")
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("PDECONTROL_PIPELINED", "1")      # both routes replay the same schedule
    assert torch.cuda.is_available(), "needs a GPU"
    rec = {"device": torch.cuda.get_device_name(0), "pipelined": os.environ["PDECONTROL_PIPELINED"],
           "widths": [measure(N, args) for N in args.widths]}
    if args.profile_run:
        return
    name = "surrogate_phase_bench_parent.json" if args.parent_only else "surrogate_phase_bench.json"
    out = args.out or os.path.join(ROOT, "profiles", name)
    line = json.dumps(rec)
    print(line)
    with open(out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
