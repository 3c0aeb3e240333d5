"""The controller's surrogate-update phase (reference ``update_surrogate``, pdecontrol/mbrl/mbrl.py:568-595):
``reset_trainer`` + ``trainer.fit(module, datamodule)`` + ``logged_metrics["Val. Loss"]`` of one ensemble member, as one
call that needs no pytorch-lightning.

Two tiers.  The kernel tier keeps the phase in HBM: per loader one ``locate_many`` and one upload of the windows' first
rows; per training step one ``sur_gather_windows`` launch straight into the static buffers of the captured TBPTT step
(``GraphedTBPTTStep``) and one replay; per validation batch one gather into time-major storage, the fused rollout on its
``[B, T, 1, N]`` view (for an FNO with ``PDECONTROL_FNO_CHAIN=1``: the teacher-forced launch and one
``fno_forward_chain``) and one ``sur_val_loss`` launch into the epoch's device accumulator; per validation epoch one small
device-to-host copy, the only synchronisation besides graph capture.
The loop tier runs the same rule over the datamodule's own loaders, for everything the kernel tier does not take, and
says so once per reason (``recognition.notice``).
"""
import math
import time

import numpy as np
import torch

from pdecontrol.mbrl.recognition import Unrecognized, notice, same_device, world_connector
from pdecontrol.surrogates.graph_step import clip_value

METRICS = ("Val. Loss", "Val. Scaled Loss", "Val. Delta Loss")


class FitState:
    """What persists across the calls of one member's trainer: ``global_step``, ``current_epoch``, the early stopping's
    ``best_score`` and ``wait_count``, the optimizer of the loop tier, and ``history`` (one dict per validation epoch:
    the three validation metrics, ``hsteploss``, ``epoch`` and ``global_step``).  It doubles as the
    ``datamodule.trainer`` the curriculum reads."""

    def __init__(self):
        self.global_step = 0
        self.current_epoch = 0
        self.best_score = math.inf
        self.wait_count = 0
        self.history = []
        self.optimizers = self.schedulers = None
        self.tier = self.tier_reason = None


# ----------------------------------------------------------------------------------------------------------------------
# tiers
# ----------------------------------------------------------------------------------------------------------------------
def _single_process():
    dist = torch.distributed
    return not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)


def _fused_step_ok(module):
    """``fused_step`` takes this module: on CUDA, nothing frozen (the captured step trains every parameter)."""
    frozen = getattr(module, "_frozen_parameters", None)
    return module.device.type == "cuda" and callable(getattr(module, "fused_step", None)) and callable(frozen) and not frozen()


def _fno_refusal(surrogate, n, na):
    """Why the kernel tier does not take the FNO ``surrogate`` over gathered state rows of ``n`` and action rows of ``na``
    columns, or None: the whole-network kernels' geometry and an affine ``dscaling`` (``fno_hip.world_supported``), and an
    action field on the state's grid."""
    from pdecontrol.surrogates import fno_hip
    if not fno_hip.world_supported(surrogate, n):
        return (f"an FNO the whole-network kernels do not take at a state row of {n} points (width {fno_hip.WIDTH}, "
                f"{fno_hip.MODES} modes, {fno_hip.LAYERS} layers, a power of two in [64, 512] points, an affine dscaling)")
    if na != n:
        return f"an action row of {na} columns beside a state row of {n}: the FNO reads the action field at every grid point"
    return None


class _KernelTier:
    """The gather of one call: the store's fields, the recognised connector, the uploaded tables."""

    def __init__(self, module, datamodule):
        from pdecontrol.surrogates import hipops, ops
        from pdecontrol.surrogates.common.dataset import device_store
        from pdecontrol.surrogates.surrogate import AutoRegPDESurrogate
        from pdecontrol.architectures.fno import FNOAutoRegSurrogate
        device = module.device
        if device.type != "cuda":
            raise Unrecognized("a module that is not on a GPU")
        if not ops.fused_enabled():
            raise Unrecognized("the fused kernels switched off")
        if not all(callable(getattr(module, name, None)) for name in ("graphed_step_for", "_frozen_parameters", "_full_rollout",
                                                                          "_fused_validation_loss")):
            raise Unrecognized(f"a {type(module).__name__} without the captured TBPTT step of PDETrainingModule")
        surrogate = getattr(module, "surrogate", None)
        fno = isinstance(surrogate, FNOAutoRegSurrogate)
        if fno:
            pass        # the whole-network FNO kernels: their geometry is checked below, at the gather's row widths
        elif hipops.fused_latent_supported(surrogate):
            # the latent ConvLSTM: the captured decoded-mode step, on the conditions of PDETrainingModule._latent_training_step
            constants = getattr(module, "_latent_constants", None)
            if not callable(constants) or constants() is None:
                raise Unrecognized(f"a latent {type(surrogate).__name__} whose loss or delta scalings the decoded-mode kernels "
                                   f"do not take")
        elif not isinstance(surrogate, AutoRegPDESurrogate) or not hipops.fused_supported(surrogate):
            raise Unrecognized(f"a {type(surrogate).__name__} the fused TBPTT step does not implement")
        if module._frozen_parameters():
            raise Unrecognized("a partly frozen surrogate")
        if not _single_process():
            raise Unrecognized("more than one process")
        if datamodule.device_data is None or not same_device(device, datamodule.device_data):
            raise Unrecognized("a datamodule without device_data on the module's device")
        if datamodule._store is None:
            datamodule._store = device_store(datamodule.data, datamodule.device_data)
        store = datamodule._store
        replay = getattr(store, "replay", None)
        if replay is not None:                       # the slabs of a device-resident replay, read through its row map
            store._fresh()
            fields, rowmap = replay.tensors, store.rowmap
        else:
            fields, rowmap = store.tensors, None
        obs, actions = fields[0], fields[1]
        if obs.dim() != 3 or obs.shape[1] != 1 or actions.dim() != 3 or actions.shape[1] != 1:
            raise Unrecognized(f"fields of shape {tuple(obs.shape[1:])} and {tuple(actions.shape[1:])} (one channel each)")
        obs_map, act_maps = world_connector(datamodule.stransf, obs.shape[2], actions.shape[2])
        if fno:
            reason = _fno_refusal(surrogate, obs_map.width, act_maps[2].width)
            if reason is not None:
                raise Unrecognized(reason)
        self.gather = hipops.WindowGather(obs, actions, rowmap, store.total, obs_map, act_maps)
        reason = self.gather.refused()
        if reason is not None:
            raise Unrecognized(reason)
        self.store, self.device = store, device
        self.widths = (obs_map.width, act_maps[2].width)
        # the phase asks for sur_val_loss over the FNO rollout's time-major storage; validation_step on its own does not
        self.loss_keywords = {"fno": True} if fno else {}
        self._val_buffers = {}

    def plan(self, loader):
        """(first rows of every item on the device, number of items, window length) of a loader of the datamodule."""
        dataset = loader.dataset
        n = int(len(dataset))
        keys, offsets = dataset.locate_many(np.arange(n))
        first = np.asarray([self.store.starts[k] for k in keys], dtype=np.int64) + offsets
        return torch.from_numpy(np.ascontiguousarray(first)).to(self.device, non_blocking=True), n, int(dataset.length)

    def shapes(self, b, l):
        return (b, l, 1, self.widths[0]), (b, l, 1, self.widths[1])

    def val_buffers(self, b, l):
        """[B, T, 1, N] views of time-major storage, one pair per batch shape."""
        key = (b, l)
        if key not in self._val_buffers:
            tm = lambda shape: torch.zeros((shape[1], shape[0]) + shape[2:], device=self.device).transpose(0, 1)
            self._val_buffers[key] = tuple(tm(s) for s in self.shapes(b, l))
        return self._val_buffers[key]


def _pick_tier(module, datamodule):
    try:
        return _KernelTier(module, datamodule), None
    except Unrecognized as e:
        return None, str(e)


# ----------------------------------------------------------------------------------------------------------------------
# validation epochs
# ----------------------------------------------------------------------------------------------------------------------
class _EpochMeter:
    """Sample-weighted sums of an epoch's validation metrics, kept where the module lives; ``result()`` is the epoch's
    one copy to the host."""

    def __init__(self):
        self.sums, self.hstep, self.count = None, None, 0

    def add(self, out, logged, b):
        scalar = lambda v: torch.as_tensor(v, dtype=torch.float32, device=out["loss"].device).reshape(())
        nan = float("nan")
        row = torch.stack([scalar(out["loss"]), scalar(logged.get(METRICS[1], nan)), scalar(logged.get(METRICS[2], nan))]) * b
        hstep = out["hsteploss"].detach().to(torch.float32) * b
        self.sums = row if self.sums is None else self.sums + row
        self.hstep = hstep if self.hstep is None else self.hstep + hstep
        self.count += b

    def result(self):
        if self.count == 0:
            return {name: float("nan") for name in METRICS} | {"hsteploss": np.zeros(0, np.float32)}
        flat = (torch.cat((self.sums, self.hstep)) / self.count).cpu().numpy()
        return {name: float(flat[i]) for i, name in enumerate(METRICS)} | {"hsteploss": flat[3:].copy()}


def _validate_loop(module, loader):
    meter = _EpochMeter()
    with torch.no_grad():
        for bidx, batch in enumerate(loader):
            if hasattr(module, "logged"):
                for name in METRICS[1:]:
                    module.logged.pop(name, None)
            out = module.validation_step(batch, bidx)
            meter.add(out, getattr(module, "logged", {}), int(batch[0].shape[0]))
    return meter.result()


def _validate_kernel(module, tier, loader, batch_size):
    """Per batch one gather into time-major storage, the fused rollout on its [B, T, 1, N] view and one ``sur_val_loss``
    launch that adds the batch's error sums to the epoch's device accumulator; the epoch's metrics are then one copy to
    the host and a division by counts the host knows.  A batch ``sur_val_loss`` does not take (the module's conditions,
    ``PDETrainingModule._fused_validation_loss``) goes through ``validation_step``'s torch ops into the meter."""
    meter = _EpochMeter()
    first, n, l = tier.plan(loader)
    accum, fused_samples = torch.zeros(3 + l, dtype=torch.float64, device=tier.device), 0
    with torch.no_grad():
        for bidx, i0 in enumerate(range(0, n, batch_size)):
            b = min(batch_size, n - i0)
            states, actions = tier.val_buffers(b, l)
            tier.gather(first, i0, b, l, states, actions)
            fused = module._fused_validation_loss(module._full_rollout(states, actions), states, accum=accum, outputs=False,
                                                  **tier.loss_keywords)
            if fused is not None:
                fused_samples += b
                continue
            out = module.validation_step((states, actions), bidx)
            meter.add(out, getattr(module, "logged", {}), b)
    if fused_samples == 0:
        return meter.result()
    sums, width = accum.cpu().numpy(), tier.widths[0]
    counts = np.asarray([l, l, l - 1], np.float64) * fused_samples * width
    metrics = {name: float(sums[i] / counts[i]) for i, name in enumerate(METRICS)}
    metrics["hsteploss"] = (sums[3:] / (fused_samples * width)).astype(np.float32)
    if meter.count:                           # an epoch that mixed both routes: the sample-weighted mean of the two
        other, total = meter.result(), fused_samples + meter.count
        for name in METRICS:
            metrics[name] = (metrics[name] * fused_samples + other[name] * meter.count) / total
        metrics["hsteploss"] = (metrics["hsteploss"] * fused_samples + other["hsteploss"] * meter.count) / total
    return metrics


# ----------------------------------------------------------------------------------------------------------------------
# training epochs
# ----------------------------------------------------------------------------------------------------------------------
def _captured_lr(module, fit):
    """The learning rate of the captured step: ``StepLR(step_size, lr_gamma)`` over the trainer's epochs in closed form
    (None, the module's own, for the default ``lr_gamma`` of 1)."""
    if module.lr_gamma == 1.0:
        return None
    return module.lr * module.lr_gamma ** (fit.current_epoch // module.step_size)


def _train_loop(module, fit, loader, target, fused, clip=None):
    """One epoch over the datamodule's loader; True when the step target cut it."""
    clipped = {} if clip is None else {"clip": clip}        # without a clip: the calls as they have always been
    module.train()
    if not fused and fit.optimizers is None:
        optimizers, schedulers = module.configure_optimizers()
        fit.optimizers, fit.schedulers = list(optimizers), [s["scheduler"] for s in schedulers]
    for bidx, batch in enumerate(loader):
        if fit.global_step >= target:
            return True
        if fused:
            module.fused_step(batch, lr=_captured_lr(module, fit), **clipped)
        else:                                   # the shim's closure order: training_step -> zero_grad -> backward -> step
            opt = fit.optimizers[0]
            out = module.training_step(batch, bidx)
            opt.zero_grad(set_to_none=True)
            out["loss"].backward()
            if clip is not None:
                torch.nn.utils.clip_grad_norm_(module.surrogate.parameters(), clip)
            opt.step()
        fit.global_step += 1
    if not fused:
        for s in fit.schedulers:
            s.step()
    return fit.global_step >= target


def _train_kernel(module, tier, fit, loader, target, batch_size, clip=None):
    module.train()
    first, n, l = tier.plan(loader)
    lr = _captured_lr(module, fit)
    clipped = {} if clip is None else {"clip": clip}
    for i0 in range(0, n, batch_size):
        if fit.global_step >= target:
            return True
        b = min(batch_size, n - i0)
        step = module.graphed_step_for(*tier.shapes(b, l), lr=lr, **clipped)   # captured on first use; keeps the valid() check
        tier.gather(first, i0, b, l, step.states, step.actions)
        step.step(lr=lr)
        fit.global_step += 1
    return fit.global_step >= target


# ----------------------------------------------------------------------------------------------------------------------
# the phase
# ----------------------------------------------------------------------------------------------------------------------
def update_surrogate(module, datamodule, fit, *, max_steps, min_steps, patience, max_epochs=None, timings=None, tier=None,
                     gradient_clip_val=None):
    """Fits ``module`` on ``datamodule`` and returns the last epoch's "Val. Loss" as a float: ``reset_trainer`` +
    ``trainer.fit`` + ``logged_metrics["Val. Loss"]`` of the reference (mbrl.py:568-595), with ``fit`` (a ``FitState``)
    in the trainer's place.  The rule below is this repository's reading of that fit loop; it is unpinned against
    pytorch-lightning itself, the same status as the Trainer shim.

    - **On entry:** `wait_count = 0`; the targets are `global_step + max_steps` and `global_step + min_steps`;
      `best_score` is kept from earlier calls.
    - **Per epoch, training:** call `datamodule.train_dataloader()`. It builds its `SubSeqDataset`, so the bootstrap
      `np.random.randint` draw and the curriculum lookup happen exactly as in the loop. Train over its batches in order,
      and stop mid-epoch when the step target is reached.
    - **Per training step, clipping:** with `gradient_clip_val` > 0 (the trainer's key; `None` or <= 0 is none) the
      gradient of all the surrogate's parameters is scaled to that norm between backward and the optimizer step
      (`clip_grad_norm_`), on every route: inside the captured step on the kernel tier and under `fused_step`, by
      torch in the closure order.
    - **Per epoch, validation:** call `datamodule.val_dataloader()`. Its epoch "Val. Loss" is the sample-weighted mean
      over batches.
    - **Early stopping** (mode min, min_delta 0):
      - a strictly smaller value sets `best_score` and zeroes `wait_count`; anything else increments it;
      - `wait_count >= patience` or a non-finite value asks to stop.
    - **Fit ends** when:
      - the step target is reached; or
      - a stop was asked and `global_step` >= the min target; or
      - `max_epochs` epochs have run.
    - **Returns** the last epoch's "Val. Loss" as a float. `fit.history` keeps every epoch's three validation metrics
      and `hsteploss`.

    Every training epoch is followed by its validation epoch, the one the step target cut included, and
    ``current_epoch`` advances after the validation, so both loaders of an epoch see the same ``current_epoch``.  Training
    epochs run under ``module.train()``, validation epochs under ``module.eval()`` and ``no_grad``.  The learning rate
    follows ``configure_optimizers``' ``StepLR`` over ``fit.current_epoch``.

    The kernel tier applies when the module is on CUDA, the fused kernels are enabled, ``fused_step`` accepts the module
    (the fused TBPTT architecture, the latent ConvLSTM under ``PDETrainingModule._latent_constants``, or an
    ``FNOAutoRegSurrogate`` that ``fno_hip.world_supported`` takes at the gather's state width, with an action row as wide
    as the state row; nothing frozen),
    there is a single process, the datamodule has ``device_data`` on that
    device, ``recognition.world_connector`` recognises ``datamodule.stransf`` and ``sur_gather_windows`` does not refuse
    the geometry.  Everything else runs on the loop tier over the datamodule's own loaders: ``fused_step`` on CUDA where
    the module allows it, else ``training_step -> zero_grad -> backward -> step`` with the optimizer of
    ``configure_optimizers`` kept on ``fit``; validation through ``module.validation_step`` under ``no_grad``.

    ``tier="loop"`` forces the loop tier (the controller's ``phase_tiers="loop"``): the datamodule's own loaders, which
    with ``device_data`` yield device batches, and ``fused_step`` where the module allows it.

    ``timings`` (tools/surrogate_phase_bench.py) is an optional dict that receives the host seconds of the plan
    (dataloaders, ``locate_many``, uploads), of training and of validation, and the tier that ran; on a CUDA module each
    lap then ends in a device synchronisation, which the phase otherwise does only for an epoch's validation metrics."""
    clock = time.perf_counter
    cuda = module.device.type == "cuda"

    def lap(name, t0):
        if timings is not None:
            if cuda:
                torch.cuda.synchronize(module.device)
            timings[name] = timings.get(name, 0.0) + clock() - t0
        return clock()

    fit.wait_count = 0
    target, min_target = fit.global_step + int(max_steps), fit.global_step + int(min_steps)
    datamodule.trainer = fit
    if tier not in (None, "loop"):
        raise ValueError(f"tier is {tier!r}: None or 'loop'")
    clip = clip_value(gradient_clip_val)
    tier, reason = (None, "the loop tier was asked for") if tier == "loop" else _pick_tier(module, datamodule)
    fit.tier, fit.tier_reason = ("kernel", None) if tier is not None else ("loop", reason)
    if tier is None:
        notice("the surrogate-update phase runs on its loop tier: %s", reason, expected=not cuda)
    fused = tier is None and cuda and _single_process() and _fused_step_ok(module)
    batch_size = int(datamodule.batch_size)
    epochs, value = 0, float("nan")
    while True:
        t = clock()
        loader = datamodule.train_dataloader()
        t = lap("plan_s", t)
        if tier is not None:
            cut = _train_kernel(module, tier, fit, loader, target, batch_size, clip)
        else:
            cut = _train_loop(module, fit, loader, target, fused, clip)
        t = lap("train_s", t)
        loader = datamodule.val_dataloader()
        t = lap("plan_s", t)
        module.eval()                            # as a trainer's validation loop does; every training epoch sets train()
        metrics = _validate_kernel(module, tier, loader, batch_size) if tier is not None else _validate_loop(module, loader)
        lap("validation_s", t)
        value = metrics[METRICS[0]]
        fit.history.append(dict(metrics, epoch=fit.current_epoch, global_step=fit.global_step))
        if value < fit.best_score:
            fit.best_score, fit.wait_count = value, 0
        else:
            fit.wait_count += 1
        stop = fit.wait_count >= patience or not math.isfinite(value)
        fit.current_epoch += 1
        epochs += 1
        if cut or (stop and fit.global_step >= min_target) or (max_epochs is not None and epochs >= max_epochs):
            break
    if timings is not None:
        timings["tier"] = fit.tier
    return float(value)
