#!/usr/bin/env python3
"""Timings of one fold of the offline surrogate evaluation on an MI355X (pdecontrol/surrogates/evaluation/evaluate.py;
DESIGN.md 4.21).  Record only.

The fold is the published configuration (runscripts/offline.sh of the reference), ``--epochs`` (10) epochs per timed call:
N = 64, 100 episodes of 400 steps, 4 actions, 5 folds with 20 % of the training episodes held out for validation (64
training episodes), batch 64, tau = 10, target length 30 (windows of 40 steps), gradient_clip_val 0.5, the N = 64 ConvLSTM
factory.  The dataset is synthetic (smooth travelling fields, seeded) so that the same program runs on the parent's tree;
it is packed into HBM once per datamodule, for both routes alike.  Two routes, both warmed up, alternated over
``--rounds`` (5) rounds in one process, each on a module and a ``FitState`` of its own:

  (a) unfrozen   the four fitted ``Normalize`` scalings left unfrozen, the state in which ``recognition.world_connector``
                 refuses the connector: ``update_surrogate`` runs its loop tier (device batches assembled with
                 index_select and the torch transforms, ``fused_step``, ``validation_step``'s torch ops).  This is the
                 route the parent commit has.  ``--parent-only`` times it alone, so that it can be run on the parent's
                 tree in a process of its own.
  (b) frozen     the scalings frozen, as ``fit_scalings`` leaves them: the kernel tier (``sur_gather_windows`` into the
                 captured TBPTT step, ``sur_val_loss``).

Per route and round: ms per training step (``timings["train_s"]`` over the steps of the call), ms of validation per
epoch, ms of planning per epoch.  The rule of DESIGN.md 4.1: (b) is faster where its median per training step lies below
(a)'s by more than three times the larger of the two spreads (max - min over the rounds); the record says whether it does.

Without ``--parent-only`` two more records, without a criterion: ``fit_scalings`` on its kernel tier against its host tier
(numpy arrays, as the reference holds them) on the fold's 64 training episodes, and ``generate_dataset`` of 100 episodes of
the default env against its ``tier="loop"``.

Usage (repo root, on an MI355X):  python tools/offline_eval_bench.py    (writes profiles/offline_eval_bench.json)
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

N, A, EPISODES, STEPS = 64, 4, 100, 400
TAU, TARGET, BATCH, CLIP, DELTA = 10, 30, 64, 0.5, 0.25


def dataset(seed=0):
    """obs, actions, nxt [E, T, 1, .] fp32: travelling fields around 0.5, uniform actions."""
    rs = np.random.RandomState(seed)
    x = np.linspace(0, 2 * np.pi, N, endpoint=False)
    t = np.arange(STEPS + 1)[None, :, None]
    phase, amp = rs.uniform(0, 6, (EPISODES, 1, 1)), rs.uniform(0.5, 1.5, (EPISODES, 1, 1))
    field = (0.5 + amp * np.sin(x[None, None, :] + phase + 0.05 * t) + 0.5 * np.cos(2 * x[None, None, :] - 0.03 * t)).astype(np.float32)
    actions = rs.uniform(-1, 1, (EPISODES, STEPS, 1, A)).astype(np.float32)
    return field[:, :-1, None, :], actions, field[:, 1:, None, :]


def split():
    """Fold 0 of the published split: KFold(5, shuffle, seed 0) written out, then the 80 / 20 cut by position."""
    order = np.arange(EPISODES)
    np.random.RandomState(0).shuffle(order)
    test = np.sort(order[:EPISODES // 5])
    train = np.setdiff1d(np.arange(EPISODES), test)
    cut = int(np.ceil(0.8 * len(train)))
    return train[:cut], train[cut:], test


def fitted_scalings(env, obs, actions, nxt, train):
    """The reference's fit (evaluate.py:86-112) on torch CPU tensors: classes both trees have."""
    from pdegym.common.transforms import BatchTransform, Normalize, Operation, SampleTransform
    flat = lambda f: torch.from_numpy(f[train].reshape(-1, 1, f.shape[-1]))
    o, a, x = flat(obs), flat(actions), flat(nxt)
    oscaling, ascaling, pdescaling, undscaling = (Normalize(aggregate=True, batched=True) for _ in range(4))
    forcing = BatchTransform(env.forcing)
    oscaling.update(o)
    ascaling.update(a)
    pdescaling.update(forcing(a))
    undscaling.update((oscaling(x) - oscaling(o)) / DELTA)
    return (oscaling, ascaling, pdescaling, undscaling), SampleTransform(oscaling, Operation([forcing, pdescaling]))


def route(env, fields, splits, frozen, dev):
    """(module, datamodule, FitState) of one route: scalings of its own, frozen or not."""
    from pdecontrol.architectures import KSAutoRegConvolutionalLSTM
    from pdecontrol.mbrl.surrogate_phase import FitState
    from pdecontrol.mbrl.types import Sample
    from pdecontrol.surrogates.common.datamodule import PDEDataModule
    from pdecontrol.surrogates.common.schedulers import ConstantLengthScheduler
    from pdecontrol.surrogates.training import PDETrainingModule
    from pdegym.common.transforms import BatchTransform
    obs, actions, nxt = fields
    train, val, test = splits
    scalings, stransf = fitted_scalings(env, obs, actions, nxt, train)
    for s in scalings:
        s.frozen = frozen
    und = BatchTransform(scalings[3])
    torch.manual_seed(0)
    f = KSAutoRegConvolutionalLSTM()
    surrogate = f.surrogate(**f.model(), delta=DELTA, dscaling=und.Inverse)
    module = PDETrainingModule(surrogate=surrogate, loss=torch.nn.MSELoss(reduction="none"), env=env, stransf=stransf, tstep=DELTA,
                               delta=DELTA, undscaling=und, tau=TAU, tbtt=1000000).to(dev)
    rewards = np.zeros((EPISODES, STEPS), np.float32)
    flags = np.zeros((EPISODES, STEPS), bool)
    steps = np.tile(np.arange(STEPS, dtype=np.int32), (EPISODES, 1))
    as_dict = lambda f: {e: f[e] for e in range(EPISODES)}              # episode -> column: what a replay's fields look like
    data = Sample(*(as_dict(f) for f in (obs, actions, nxt, rewards, flags, flags, steps)))
    dm = PDEDataModule(data=data, train=[int(i) for i in train], val=[int(i) for i in val], test=[int(i) for i in test],
                       stransf=stransf, curriculum=ConstantLengthScheduler(length=TARGET), tau=TAU, batch_size=BATCH,
                       target_length=TARGET, device_data=dev)
    return module, dm, FitState()


def run(module, dm, fit, epochs):
    from pdecontrol.mbrl.surrogate_phase import update_surrogate
    timings, before = {}, fit.global_step
    update_surrogate(module, dm, fit, max_steps=2 ** 62, min_steps=0, patience=10 ** 6, max_epochs=epochs, gradient_clip_val=CLIP,
                     timings=timings)
    steps = fit.global_step - before
    return {"tier": timings["tier"], "steps": steps, "train_ms_per_step": 1e3 * timings["train_s"] / steps,
            "validation_ms_per_epoch": 1e3 * timings["validation_s"] / epochs, "plan_ms_per_epoch": 1e3 * timings["plan_s"] / epochs}


def timed(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--parent-only", action="store_true")
    ap.add_argument("--generate-episodes", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    from pdegym.kuramoto import KuramotoSivashinskyEnv
    env = KuramotoSivashinskyEnv(device=0)
    fields, splits = dataset(), split()
    np.random.seed(0)
    names = ("a_unfrozen",) if args.parent_only else ("a_unfrozen", "b_frozen")
    routes = {name: route(env, fields, splits, name == "b_frozen", dev) for name in names}
    for name in names:                                       # warm-up: code objects, the captured steps, the packs
        run(*routes[name], 1)
    rounds = {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:
            rounds[name].append(run(*routes[name], args.epochs))
    med = lambda v: round(float(np.median(v)), 4)
    rec = {"what": "one fold of the offline evaluation at the published configuration (N = 64, 100 episodes of 400 steps, batch 64, "
                   "tau 10, target 30, clip 0.5), a few epochs: ms per training step, of validation per epoch and of planning per "
                   "epoch of update_surrogate with the scalings unfrozen (loop tier, the parent's route) and frozen (kernel tier); "
                   "routes alternated in one process, medians and spreads (max - min) over the rounds; host clock around work "
                   "ending in a device synchronisation",
           "device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "epochs_per_call": args.epochs,
           "steps_per_call": rounds[names[0]][0]["steps"], "parent_only": bool(args.parent_only)}
    for name in names:
        rec[name] = {"tier": sorted({r["tier"] for r in rounds[name]})}
        for key in ("train_ms_per_step", "validation_ms_per_epoch", "plan_ms_per_epoch"):
            values = [r[key] for r in rounds[name]]
            rec[name][key] = {"median": med(values), "spread": round(max(values) - min(values), 4), "rounds": [round(v, 4) for v in values]}
    if not args.parent_only:
        a, b = rec["a_unfrozen"]["train_ms_per_step"], rec["b_frozen"]["train_ms_per_step"]
        margin = 3 * max(a["spread"], b["spread"])
        rec["ab_rule"] = {"a_median_ms": a["median"], "b_median_ms": b["median"], "three_times_the_larger_spread_ms": round(margin, 4),
                          "b_faster_by_the_rule": bool(a["median"] - b["median"] > margin),
                          "ratio_a_over_b": round(a["median"] / b["median"], 3)}
        assert rec["a_unfrozen"]["tier"] == ["loop"] and rec["b_frozen"]["tier"] == ["kernel"], (rec["a_unfrozen"], rec["b_frozen"])

        from pdecontrol.surrogates.evaluation import evaluate as ev
        from pdecontrol.surrogates.evaluation.generate import generate_dataset
        device_fields = [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in fields]
        ev.fit_scalings(device_fields, splits[0], env.forcing, DELTA)                      # warm-up
        fit_ms = {"kernel": [], "host": []}
        for _ in range(args.rounds):
            ms, fit = timed(lambda: ev.fit_scalings(device_fields, splits[0], env.forcing, DELTA))
            assert fit.tier == "kernel"
            fit_ms["kernel"].append(ms)
            ms, fit = timed(lambda: ev.fit_scalings(fields, splits[0], env.forcing, DELTA))
            assert fit.tier == "host"
            fit_ms["host"].append(ms)
        rec["fit_scalings_ms"] = {k: {"median": med(v), "spread": round(max(v) - min(v), 4)} for k, v in fit_ms.items()}
        rec["fit_scalings_rows"] = int(len(splits[0]) * STEPS)

        E = args.generate_episodes
        generate_dataset("KuramotoSivashinskyEnv-v0", 2, device="cuda", seed=0)            # warm-up (two envs)
        gen = {}
        for tier in (None, "loop"):
            ms, data = timed(lambda: generate_dataset("KuramotoSivashinskyEnv-v0", E, device="cuda", seed=0, tier=tier))
            gen[data.tier] = round(ms, 1)
        rec["generate_dataset_ms"] = dict(gen, episodes=E, steps_per_episode=int(data.tensors[0].shape[1]),
                                          note="one run each; both include the reset burn-in and the autoreset burn-in of every env")
    line = json.dumps(rec)
    print(line)
    out = args.out or os.path.join(ROOT, "profiles", "offline_eval_bench_parent.json" if args.parent_only else "offline_eval_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
