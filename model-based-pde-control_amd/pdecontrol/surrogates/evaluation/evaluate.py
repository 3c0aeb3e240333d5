"""The offline k-fold evaluation of a surrogate (reference ``pdecontrol/surrogates/evaluation/evaluate.py``, driven by
``runscripts/offline.sh``): per fold the four scaling transforms are fitted on the training episodes, the surrogate is
trained with early stopping on the validation episodes and tested on the held-out ones.

    python -m pdecontrol.surrogates.evaluation.evaluate --env_id KuramotoSivashinskyEnv-v0 --data KSattractor.pl \\
        --factory KSAutoRegConvolutionalLSTM --splits 5 --total 0.9 --val 0.2 --target_length 30 --device cuda \\
        --training '{"tbtt": 1000000, "tau": 10, "batch_size": 64, "patience": 50}' \\
        --trainer '{"max_epochs": 250, "gradient_clip_val": 0.5}' --output offline-run

The reference's flags keep their names and defaults; ``--project``, ``--offline`` and ``--factory_module`` are accepted and
unused (there is no wandb here; the published script passes the last), ``--device`` is new.  No Lightning, wandb, gym
registry lookups beyond ``gym.make``, plotting or pandas: a fold is

    fit_scalings -> update_surrogate (pdecontrol/mbrl/surrogate_phase.py) -> test_surrogate (surrogates/test_phase.py)

and with ``--device cuda`` it stays in HBM from the fit to the test tables: the dataset goes up once,
``rpn_moments`` and ``rpd_moments`` (csrc/replay.hip) fit the scalings from it in place, the fitted scalings are FROZEN
-- the reference never updates them after the fit -- which is what lets ``recognition.world_connector`` reduce the
connector to affine coefficients, so that training gathers its windows with ``sur_gather_windows`` into the captured
TBPTT step, validation takes ``sur_val_loss`` and the test runs ``ks_eval_rows_device``.

Per fold ``main`` writes ``fold<k>.json`` (configuration, tiers, validation history, test scalars, seconds) and
``fold<k>.npz`` (per-step test tables, the kept test sequences, ``hsteploss`` per epoch) under ``--output``, and with
``--store`` ``fold<k>_model.pt`` (the surrogate's state dict and the four scalings).
"""
import argparse
import json
import math
import os
import sys
import time
from typing import Any, NamedTuple, Optional

import numpy as np
import torch

from pdecontrol.mbrl.recognition import Unrecognized, field_map, forcing_matrix, is_forcing, notice
from pdecontrol.mbrl.types import Sample
from pdecontrol.surrogates.common.dataset import DeviceSubSeqStore
from pdegym.common.transforms import BatchTransform, Normalize, Operation, SampleTransform

UNBOUNDED_STEPS = 2 ** 62        # ``max_steps`` of a trainer config that sets none: the epochs and the patience end the fit
DEFAULT_PATIENCE = 3             # EarlyStopping's own default, for a training config without "patience"
DEFAULT_MAX_EPOCHS = 1000        # pl.Trainer's, where neither max_epochs nor max_steps is given


# ----------------------------------------------------------------------------------------------------------------------
# folds
# ----------------------------------------------------------------------------------------------------------------------
def _kfold_rule(n, splits, seed):
    """``KFold(splits, shuffle=True, random_state=seed).split(arange(n))`` written out: one
    ``RandomState(seed).shuffle(arange(n))``, consecutive blocks of ``n // k`` items (one more in the first ``n % k``),
    each block sorted as the test fold and its sorted complement as the train fold."""
    n, splits = int(n), int(splits)
    if splits < 2 or splits > n:
        raise ValueError(f"{splits} folds of {n} episodes: 2 ... {n} are possible")
    order = np.arange(n)
    np.random.RandomState(seed).shuffle(order)
    sizes = np.full(splits, n // splits, dtype=np.int64)
    sizes[:n % splits] += 1
    folds, start = [], 0
    for size in sizes:
        mask = np.zeros(n, dtype=bool)
        mask[order[start:start + size]] = True
        folds.append((np.nonzero(~mask)[0], np.nonzero(mask)[0]))
        start += size
    return folds


def kfold_indices(n, splits, seed):
    """[(train indices, test indices)] of the reference's ``KFold(splits, shuffle=True, random_state=seed)`` over ``n``
    items: sklearn's where it is importable, else the same draw (``_kfold_rule``)."""
    try:
        from sklearn.model_selection import KFold
    except ImportError:
        return _kfold_rule(n, splits, seed)
    return [(np.asarray(train), np.asarray(test)) for train, test in KFold(int(splits), shuffle=True, random_state=seed).split(np.arange(int(n)))]


def fold_split(train_idx, val):
    """(train, validation) of a fold's train indices, cut by position: the first ``ceil((1 - val) * len)`` train."""
    size = math.ceil((1.0 - val) * len(train_idx))
    return train_idx[:size], train_idx[size:]


def total_count(total, n):
    """Episodes of ``n`` the ``--total`` fraction keeps: ``ceil(total * n)``."""
    return math.ceil(total * n)


# ----------------------------------------------------------------------------------------------------------------------
# the numpy twin of rpn_moments
# ----------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fp32 fma of fp32 arrays in numpy: the product of two fp32 values is exact in fp64; the fp64 sum is rounded to odd
    (its rounding error, from TwoSum, says whether it was inexact), so that the rounding to fp32 that follows is the one
    rounding of the exact a * b + c."""
    p, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    bits = s.view(np.int64)
    odd = (err != 0) & ((bits & 1) == 0) & np.isfinite(s) & (s != 0)
    away = np.where((err > 0) == (s > 0), 1, -1)             # the magnitude grows when the error has the sum's sign
    return np.where(odd, (bits + np.where(odd, away, 0)).view(np.float64), s).astype(np.float32)


def forced_numpy(actions, F):
    """``row_ops.h``'s ``forcing_col`` for every column: [..., A] x [A, N] -> [..., N], one rounded fp32 product and then
    one fp32 fma per further actuator in index order."""
    a, F = np.asarray(actions, dtype=np.float32), np.asarray(F, dtype=np.float32)
    acc = (a[..., 0:1] * F[0]).astype(np.float32)
    for m in range(1, F.shape[0]):
        acc = _fma32(np.broadcast_to(a[..., m:m + 1], acc.shape), np.broadcast_to(F[m], acc.shape), acc)
    return acc


def field_moments_numpy(obs, actions, F, rows=None):
    """(sums, stats) of ``rpn_moments`` (include/replay/fit.h) in numpy, the kernel's contract: ``obs`` [R, (1,) N] and
    ``actions`` [R, (1,) A] fp32, ``F`` [A, N] or None, ``rows`` the listed rows (None: all, in order).  Per field --
    observations, actions and, with ``F``, the forced actions ``forced_numpy`` -- the fp64 sums of v and v * v per
    column and over all columns, and the two-pass fp64 mean and ``ddof=1`` variance (NaN below two values); laid out as
    the kernel lays them out, each field's columns followed by its total.  A row outside ``[0, R)`` makes everything
    NaN."""
    from pdecontrol.mbrl.delta_phase import moments_numpy
    obs, actions = np.asarray(obs, dtype=np.float32), np.asarray(actions, dtype=np.float32)
    obs, actions = obs.reshape(obs.shape[0], obs.shape[-1]), actions.reshape(actions.shape[0], actions.shape[-1])
    rows = np.arange(obs.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64)
    inside = (rows >= 0) & (rows < obs.shape[0])
    rows = np.where(inside, rows, 0)
    fields = [obs[rows], actions[rows]]
    if F is not None:
        fields.append(forced_numpy(actions[rows], F))
    parts = [moments_numpy(f) for f in fields]
    sums, stats = (np.concatenate([p[i] for p in parts], axis=1) for i in range(2))
    if not inside.all():
        sums[:], stats[:] = np.nan, np.nan
    return sums, stats


# ----------------------------------------------------------------------------------------------------------------------
# the scaling fits
# ----------------------------------------------------------------------------------------------------------------------
class FittedScalings(NamedTuple):
    """What ``fit_scalings`` returns: the four fitted, frozen ``Normalize(aggregate=True, batched=True)``, the connector
    built from them, the tier that fitted them ("kernel" or "host") and, on the host tier of a CUDA dataset, why."""
    oscaling: Normalize
    ascaling: Normalize
    pdescaling: Normalize
    undscaling: Normalize
    stransf: SampleTransform
    tier: str
    tier_reason: Optional[str] = None


def _flat(field):
    """[E, T, 1, W] as its [E * T, 1, W] view."""
    return field.reshape((field.shape[0] * field.shape[1],) + tuple(field.shape[2:]))


def _fit_host(obs, actions, nxtobs, train_idx, forcing, delta, oscaling, ascaling, pdescaling, undscaling):
    """The reference's lines (evaluate.py:96-112) on whatever the fields are (numpy arrays, or tensors on any device)."""
    index = train_idx if isinstance(obs, np.ndarray) else torch.as_tensor(train_idx, device=obs.device)
    obs, actions, nxtobs = _flat(obs[index]), _flat(actions[index]), _flat(nxtobs[index])
    # update observation and action scaling
    oscaling.update(obs)
    ascaling.update(actions)
    pdescaling.update(forcing(actions))
    # scale changes between state transitions
    deltas = oscaling(nxtobs) - oscaling(obs)
    undscaling.update(deltas / delta)


def _fit_kernel(obs, actions, nxtobs, train_idx, forcing, delta, oscaling, ascaling, pdescaling, undscaling):
    """One ``rpn_moments`` call for three of the fits, then ``rpd_moments`` with the fitted observation scaling's
    coefficients for the fourth; every batch statistic goes into its ``Normalize`` through ``merge`` with the row count
    as ``n_new``, which is what ``update`` passes.  Nothing of rows x N elements is allocated: the row list, the two
    workspaces and four small output tensors are all."""
    import hipbind
    from pdecontrol.mbrl import replay_hip
    replay_hip.load()
    device = obs.device
    E, T, _, N = (int(v) for v in obs.shape)
    A = int(actions.shape[-1])
    F = forcing_matrix(is_forcing(forcing))
    if tuple(F.shape) != (A, N):
        raise Unrecognized(f"a forcing matrix of shape {tuple(F.shape)} for {A} actuators and {N} columns")
    slabs = tuple(_flat(f) for f in (obs, actions, nxtobs))
    if any(f.dtype != torch.float32 or not f.is_contiguous() for f in slabs):
        raise Unrecognized("fields that are not contiguous fp32")
    episodes = torch.as_tensor(np.asarray(train_idx, dtype=np.int64)).to(device)
    rows = (episodes[:, None] * T + torch.arange(T, dtype=torch.int64, device=device)[None, :]).reshape(-1)
    n = int(rows.numel())
    need = replay_hip.fit_workspace_doubles(N, A, True, n), replay_hip.delta_workspace_doubles(N, n)
    if min(need) < 1:
        raise Unrecognized(f"{n} rows of {N} observation and {A} action columns (1 ... {replay_hip.MAX_OBS_DIM} and 1 ... "
                           f"{replay_hip.MAX_ACT_DIM} are supported)")
    offsets, ld = replay_hip.fit_layout(N, A, True)
    workspace = torch.empty(max(need), dtype=torch.float64, device=device)
    sums = torch.empty((2, ld), dtype=torch.float64, device=device)
    stats = torch.empty((2, ld), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        replay_hip.fit_moments(hipbind.stream(), slabs[0], slabs[1], F.to(device), rows, n, 0, workspace, sums, stats)
        for scaling, first, width in ((oscaling, offsets[0], N), (ascaling, offsets[1], A), (pdescaling, offsets[2], N)):
            total = first + width                               # the field's aggregate follows its columns
            scaling.merge(stats[0, total:total + 1].reshape(1, 1, 1), stats[1, total:total + 1].reshape(1, 1, 1), n)
        oscaling.frozen = True                                  # fitted: from here on it is the affine map rpd_moments takes
        coef = field_map(oscaling, N, normalize=True).coef.to(device)
        dsums = torch.empty((2, N + 1), dtype=torch.float64, device=device)
        dstats = torch.empty((2, N + 1), dtype=torch.float32, device=device)
        replay_hip.delta_moments(hipbind.stream(), slabs[0], slabs[2], 0, 1, coef, rows, n, delta, 0, workspace, dsums, dstats)
        undscaling.merge(dstats[0, N:N + 1].reshape(1, 1, 1), dstats[1, N:N + 1].reshape(1, 1, 1), n)


def fit_scalings(data, train_idx, forcing, delta, device=None, untransformed=False):
    """The four scalings of a fold, fitted on the episodes ``train_idx`` of ``data`` (the seven fields ``[E, T, ...]``,
    numpy arrays or tensors), and the connector built from them: ``SampleTransform(oscaling, Operation([forcing,
    pdescaling]))``, or with ``untransformed`` ``SampleTransform(oscaling, ascaling)``.  ``forcing``: the env's
    ``GaussianForcing``, bare or in a ``BatchTransform``; ``delta``: ``cfg_steps * dt``; ``device``: where tensor fields
    are moved before the fit (None: where they are).

    Kernel tier: fields that are CUDA tensors and a ``GaussianForcing`` -- ``rpn_moments`` and ``rpd_moments`` read the
    training rows in place (``_fit_kernel``).  Host tier: the reference's lines, on numpy arrays or on tensors of any
    device.  Both tiers end by freezing the four scalings; the reference never updates them after the fit."""
    fields = tuple(data)
    obs, actions, nxtobs = fields[0], fields[1], fields[2]
    if device is not None and not isinstance(obs, np.ndarray):
        obs, actions, nxtobs = (f.to(device) for f in (obs, actions, nxtobs))
    if not isinstance(forcing, BatchTransform):
        forcing = BatchTransform(forcing)
    scalings = tuple(Normalize(aggregate=True, batched=True) for _ in range(4))
    oscaling, ascaling, pdescaling, undscaling = scalings
    train_idx = np.asarray(train_idx, dtype=np.int64)
    args = (obs, actions, nxtobs, train_idx, forcing, delta) + scalings
    tier, reason = "host", None
    if isinstance(obs, torch.Tensor) and obs.is_cuda:
        try:
            if is_forcing(forcing) is None:
                raise Unrecognized(f"a {type(forcing.transform).__name__} in place of the GaussianForcing")
            _fit_kernel(*args)
            tier = "kernel"
        except Unrecognized as e:
            reason = str(e)
            notice("the scalings of the offline evaluation are fitted on the host tier: %s", reason)
            for scaling in scalings:
                scaling.frozen = False
                scaling.reset()
    if tier == "host":
        _fit_host(*args)
    for scaling in scalings:
        scaling.frozen = True
    atransf = ascaling if untransformed else Operation([forcing, pdescaling])
    return FittedScalings(oscaling, ascaling, pdescaling, undscaling, SampleTransform(oscaling, atransf), tier, reason)


# ----------------------------------------------------------------------------------------------------------------------
# a dataset in HBM where the datamodule expects a replay's fields
# ----------------------------------------------------------------------------------------------------------------------
_PACKED = (torch.float32, torch.float32, torch.float32, torch.float32, torch.bool, torch.bool, torch.int32)


class EpisodeField:
    """One field ``[E, T, ...]`` of a device dataset as the datamodule reads a replay's: ``field[e]`` is episode e's
    column, ``tensors`` are all seven fields, and ``window_store(device)`` is the ``DeviceSubSeqStore`` over their
    ``[E * T, ...]`` views where they live (episode e is rows e T ... e T + T - 1: nothing is packed or copied)."""

    def __init__(self, tensors, index):
        self.tensors, self._index = tensors, index

    def keys(self):
        return range(int(self.tensors[0].shape[0]))

    def __len__(self):
        return int(self.tensors[0].shape[0])

    def __getitem__(self, episode):
        return self.tensors[self._index][int(episode)]

    def window_store(self, device):
        from pdecontrol.mbrl.device_replay import _same_device
        if not _same_device(device, self.tensors[0].device):
            return None
        E, T = (int(v) for v in self.tensors[0].shape[:2])
        return DeviceSubSeqStore.over([_flat(t) for t in self.tensors], {e: e * T for e in range(E)}, E * T)


def device_fields(data, device):
    """The seven fields of ``data`` on ``device``, in the dtypes a packed replay has (``steps`` int32), as a ``Sample`` the
    datamodule takes with ``device_data=device``."""
    tensors = tuple(torch.as_tensor(f).to(device=device, dtype=dt).contiguous() for f, dt in zip(data, _PACKED))
    return Sample(*(EpisodeField(tensors, i) for i in range(len(tensors))))


# ----------------------------------------------------------------------------------------------------------------------
# one fold
# ----------------------------------------------------------------------------------------------------------------------
class FoldReport(NamedTuple):
    """What ``evaluate_fold`` returns: the validation ``history`` of ``update_surrogate`` (one dict per epoch), the last
    epoch's "Val. Loss", the test ``EpochReport``, the training seconds, the tiers of the fit of the scalings, of the
    training and of the test, the trained module and the fitted scalings."""
    history: list
    val_loss: float
    test: Any
    training_seconds: float
    tiers: dict
    module: Any
    scalings: FittedScalings


def merged_config(factory, factory_name, sections, loss, target_length):
    """The reference's config dict: the factory's defaults overridden by the JSON flags, ``target_length`` among the
    training keys."""
    training = dict(sections["training"], target_length=target_length)
    merged = {name: {**getattr(factory.defaults, name), **value} for name, value in dict(sections, training=training).items()}
    return {"factory": factory_name, **merged, "loss": loss}


def build_module(env, factory, config, scalings, device):
    """The factory's surrogate in a ``PDETrainingModule`` on ``device``, as the reference builds it (evaluate.py:147-164):
    the surrogate's ``dscaling`` and the module's ``undscaling`` are the two directions of one ``BatchTransform`` view
    of the fitted ``undscaling`` -- the view the controller uses, so ``hipops.undscale_constants`` takes it."""
    from pdecontrol.surrogates.phyloss import phyloss
    from pdecontrol.surrogates.training import PDETrainingModule
    from pdecontrol.surrogates.utils import ignore_extra_keywords
    scenario = env.scenario
    delta = scenario["cfg_steps"] * scenario["dt"]
    # the kernel tier leaves the statistics on the device; the captured training step reads those of ``undscaling`` as
    # host scalars while it is being captured, where a copy from the device is not allowed: keep them on the host, as
    # the controller does after its delta phase
    und = scalings.undscaling
    if isinstance(und.mean, torch.Tensor) and und.mean.is_cuda:
        und.mean, und.var = und.mean.cpu(), und.var.cpu()
    undscaling = BatchTransform(und)
    loss = ignore_extra_keywords(getattr(phyloss, config["loss"]))(**scenario, reduction="none")
    model = factory.model(**config["model"])
    surrogate = factory.surrogate(**model, **config["surrogate"], delta=delta, dscaling=undscaling.Inverse)
    module = PDETrainingModule(surrogate=surrogate, loss=loss, env=env, stransf=scalings.stransf, tstep=delta, delta=delta,
                               undscaling=undscaling, **config["training"])
    return module.to(device)


def build_datamodule(fields, train_idx, val_idx, test_idx, stransf, config, target_length, device_data=None):
    """The reference's ``PDEDataModule`` (evaluate.py:191-201) under ``ConstantLengthScheduler(target_length)``;
    ``fields``: ``device_fields`` with ``device_data``, else the seven numpy arrays."""
    from pdecontrol.surrogates.common.datamodule import PDEDataModule
    from pdecontrol.surrogates.common.schedulers import ConstantLengthScheduler
    as_list = lambda index: [int(i) for i in np.asarray(index).reshape(-1)]
    return PDEDataModule(data=fields, train=as_list(train_idx), val=as_list(val_idx), test=as_list(test_idx), stransf=stransf,
                         curriculum=ConstantLengthScheduler(length=target_length), device_data=device_data,
                         **{"target_length": target_length, **config["training"]})


def evaluate_fold(data, train_idx, val_idx, test_idx, env, factory, config, *, target_length=30, untransformed=False, device=None,
                  tier=None):
    """One fold: the scalings fitted on ``train_idx``, ``build_module``, ``build_datamodule``, ``update_surrogate`` with
    the trainer section's ``max_steps`` (unbounded without one), ``max_epochs`` and ``gradient_clip_val`` and the
    training section's ``patience``, then ``test_surrogate``.  ``data``: the dataset's seven ``[E, T, ...]`` fields;
    ``env``: the (unwrapped) ``KuramotoSivashinskyEnv``; ``config``: ``merged_config``'s dict; ``device``: None / CPU keeps
    the host loaders of the reference, a CUDA device keeps the fold in HBM.  ``tier="loop"`` forces ``update_surrogate``'s
    loop tier."""
    from pdecontrol.mbrl.surrogate_phase import FitState, update_surrogate
    from pdecontrol.surrogates.test_phase import test_surrogate
    device = torch.empty(0, device="cpu" if device is None else device).device
    on_gpu = device.type == "cuda"
    scenario = env.scenario
    delta = scenario["cfg_steps"] * scenario["dt"]
    fields = device_fields(data, device) if on_gpu else Sample(*(np.asarray(f) for f in data))
    raw = fields.obs.tensors if on_gpu else tuple(fields)
    scalings = fit_scalings(raw, train_idx, BatchTransform(env.forcing), delta, untransformed=untransformed)
    module = build_module(env, factory, config, scalings, device)
    datamodule = build_datamodule(fields, train_idx, val_idx, test_idx, scalings.stransf, config, target_length,
                                  device_data=device if on_gpu else None)
    trainer = config["trainer"]
    max_epochs = trainer.get("max_epochs")
    if max_epochs is None and (trainer.get("max_steps") is None or int(trainer["max_steps"]) < 0):
        max_epochs = DEFAULT_MAX_EPOCHS
    fit = FitState()
    start = time.time()
    max_steps = trainer.get("max_steps")
    if max_steps is None or int(max_steps) < 0:                  # pl.Trainer: -1 (its default) is no limit on the steps
        max_steps = UNBOUNDED_STEPS
    value = update_surrogate(module, datamodule, fit, max_steps=max_steps, min_steps=0,
                             patience=config["training"].get("patience", DEFAULT_PATIENCE), max_epochs=max_epochs,
                             gradient_clip_val=trainer.get("gradient_clip_val"), tier=tier)
    if on_gpu:
        torch.cuda.synchronize(device)
    seconds = time.time() - start
    report = test_surrogate(module, datamodule)
    tiers = {"fit": scalings.tier, "training": fit.tier, "training_reason": fit.tier_reason, "test": report.tier}
    return FoldReport(fit.history, value, report, seconds, tiers, module, scalings)


# ----------------------------------------------------------------------------------------------------------------------
# command line
# ----------------------------------------------------------------------------------------------------------------------
def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--project", type=str)
    parser.add_argument("--env_id", type=str)
    parser.add_argument("--factory", type=str)
    parser.add_argument("--factory_module", type=str)
    parser.add_argument("--untransformed", action="store_true")
    parser.add_argument("--data", type=str)
    parser.add_argument("--target_length", type=int, default=30)
    parser.add_argument("--splits", type=int, default=5)
    parser.add_argument("--total", type=float, default=1.0)
    parser.add_argument("--val", type=float, default=0.2)
    parser.add_argument("--loss", type=str, default="MSELoss")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--offline", action="store_true")
    parser.add_argument("--store", action="store_true")
    parser.add_argument("--output", type=str, default=None)
    parser.add_argument("--model", type=str, default="{}")
    parser.add_argument("--surrogate", type=str, default="{}")
    parser.add_argument("--training", type=str, default="{}")
    parser.add_argument("--curriculum", type=str, default="{}")
    parser.add_argument("--trainer", type=str, default="{}")
    parser.add_argument("--device", type=str, default="cpu")
    return parser


def _fold_files(directory, fold, config, result, indices):
    """fold<k>.json and fold<k>.npz of one fold; returns the JSON's dict."""
    train_idx, val_idx, test_idx = indices
    test = result.test
    summary = {
        "fold": fold, "config": config, "tiers": result.tiers, "Training Time": result.training_seconds,
        "Val. Loss": result.val_loss, "epochs": len(result.history),
        "train": [int(i) for i in train_idx], "val": [int(i) for i in val_idx], "test": [int(i) for i in test_idx],
        "history": [{k: v for k, v in row.items() if k != "hsteploss"} for row in result.history],
        "test_scalars": test.scalars, "test_batches": test.batches, "test_samples": test.samples,
    }
    with open(os.path.join(directory, f"fold{fold}.json"), "w") as out:
        json.dump(summary, out, default=float, indent=1)
    arrays = {f"table/{name}": value for name, value in test.tables.items()}
    arrays.update(states=test.states, outputs=test.outputs, actions=test.actions,
                  hsteploss=np.asarray([row["hsteploss"] for row in result.history], dtype=np.float32))
    np.savez(os.path.join(directory, f"fold{fold}.npz"), **arrays)
    return summary


def main(argv=None, make_env=None):
    """The fold loop of the reference's script: one seeding of torch and numpy before the first fold, the folds of
    ``kfold_indices`` over the first ``ceil(total * len(data))`` episodes, per fold ``fold_split`` and ``evaluate_fold``.
    ``make_env()`` replaces ``gym.make(env_id, config={"device": ...})`` (tests: a short-episode env)."""
    from pdecontrol import architectures
    from pdecontrol.mbrl.mbrl import RunLog
    args = build_parser().parse_args(argv)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    device = torch.empty(0, device=args.device).device
    if make_env is None:
        from pdegym._gym import gym
        ordinal = device.index if device.type == "cuda" else -1
        make_env = lambda: gym.make(args.env_id, config={"device": ordinal})
    env = make_env().unwrapped
    data = torch.load(args.data, weights_only=False)
    fields = tuple(data.tensors)
    if device.type == "cuda":
        fields = tuple(t.to(device) for t in fields)             # the dataset's one trip to the device, for every fold
    log = RunLog(args.output or "pdecontrol-offline")
    os.makedirs(log.dir, exist_ok=True)
    sections = {name: json.loads(getattr(args, name)) for name in ("model", "surrogate", "training", "curriculum", "trainer")}
    folds = kfold_indices(total_count(args.total, len(data)), args.splits, args.seed)
    for fold, (train_idx, test_idx) in enumerate(folds):
        train_idx, val_idx = fold_split(train_idx, args.val)
        factory = getattr(architectures, args.factory)()
        config = merged_config(factory, args.factory, sections, args.loss, args.target_length)
        result = evaluate_fold(fields, train_idx, val_idx, test_idx, env, factory, config, target_length=args.target_length,
                               untransformed=args.untransformed, device=device)
        summary = _fold_files(log.dir, fold, config, result, (train_idx, val_idx, test_idx))
        log({k: v for k, v in summary.items() if k not in ("config", "history", "train", "val", "test")})
        if args.store:
            checkpoint = {"state_dict": result.module.surrogate.state_dict()}
            checkpoint.update({name: getattr(result.scalings, name) for name in ("oscaling", "ascaling", "pdescaling", "undscaling")})
            torch.save(checkpoint, os.path.join(log.dir, f"fold{fold}_model.pt"))
    with open(os.path.join(log.dir, "history.jsonl"), "w") as out:
        for row in log.history:
            out.write(json.dumps(row, default=float) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
