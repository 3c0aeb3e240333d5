"""The surrogate test phase: what ``trainer.test(module, datamodule)`` with ``EvalLogCallback`` computes in the reference's
offline evaluation (pdecontrol/surrogates/evaluation/evaluate.py; pdecontrol/callbacks.py:84-138), as one call that needs
no Lightning, wandb or pandas.

``test_surrogate`` walks the test dataloader with the module in eval mode under ``no_grad``, takes the batch-size-weighted
mean of every metric of ``PDETrainingModule.test_step`` over the batches and keeps the first ``nstore`` sequences of
states, outputs and actions.  Two tiers:

  * "kernel" -- the conditions of ``test_step``'s kernel tier (CUDA fp32 ``[B, T, 1, N]`` batches, a
    ``KuramotoSivashinskyEnv``, a recognised inverse observation chain, the fused switch on).  A batch is the rollout plus
    ``ks_eval_rows_device`` and ``ks_eval_fold_device``, the second adding ``B`` times its tables to one device
    accumulator; the epoch is one copy of ``1 + 25 T`` doubles plus the kept sequences.
  * "torch" -- the loop over ``test_step``'s host lines, as the reference runs it.

The tier is chosen on the first batch (``tier=None``) or forced (``tier="torch"`` / ``tier="kernel"``).
"""
from dataclasses import dataclass
from typing import Dict

import numpy as np
import torch


@dataclass
class EpochReport:
    """What ``EvalLogCallback.on_test_epoch_end`` logs and stores: ``scalars`` (wandb.log), ``tables`` (the "Time Table",
    name -> ``[T]``), and the first ``nstore`` sequences (test.npz)."""
    scalars: Dict[str, float]
    tables: Dict[str, np.ndarray]
    states: np.ndarray
    outputs: np.ndarray
    actions: np.ndarray
    batches: int
    samples: int
    tier: str


def test_surrogate(module, datamodule=None, dataloaders=None, nstore=20, tier=None):
    """One test epoch of ``module`` (a ``PDETrainingModule``) over ``dataloaders`` or ``datamodule.test_dataloader()``;
    returns an ``EpochReport``.  Every batch of an epoch must have the same number of steps ``T``: the per-step tables of
    batches with different ``T`` have no weighted mean (ValueError)."""
    if tier not in (None, "kernel", "torch"):
        raise ValueError(f"tier must be None, 'kernel' or 'torch', not {tier!r}")
    if dataloaders is None:
        if datamodule is None:
            raise ValueError("test_surrogate needs a datamodule or dataloaders")
        dataloaders = datamodule.test_dataloader()
    device = module.device
    was_training = module.training
    module.eval()
    try:
        with torch.no_grad():
            return _epoch(module, dataloaders, device, int(nstore), tier)
    finally:
        module.train(was_training)


def _epoch(module, loader, device, nstore, tier):
    steps, batches, samples = None, 0, 0
    accum = None                        # kernel tier: the device accumulator; torch tier: name -> fp64 host sums
    kept = {"states": [], "outputs": [], "actions": []}
    n_kept = 0
    for bidx, batch in enumerate(loader):
        states, actions = (v.to(device) for v in batch[:2])
        bsize = states.shape[0]
        if steps is None:
            steps = states.shape[1]
        elif states.shape[1] != steps:
            raise ValueError(f"batch {bidx} has {states.shape[1]} steps, the batches before it {steps}: the batches of a "
                             f"test epoch must share T")
        need = min(bsize, max(nstore - n_kept, 0))
        out = None
        if tier != "torch":
            out = module._full_rollout(states, actions)
            plan = module._test_kernel_plan(states, out)
            if plan is None and (tier == "kernel" or batches):
                raise RuntimeError(f"batch {bidx} cannot run on the kernel tier of test_step (the log says why)")
            tier = "torch" if plan is None else "kernel"
        if tier == "kernel":
            import kspde
            if accum is None:
                accum = torch.zeros(1 + kspde.EVAL_TABLES * steps, dtype=torch.float64, device=device)
            _, truth, pred = module._test_metrics_device(states, actions, out, plan, accum=accum, keep=need > 0)
            module.last_test_tier = "kernel"
            fields = {"states": truth, "outputs": pred, "actions": actions} if need else {}
        else:
            out = module._full_rollout(states, actions) if out is None else out
            data = module._test_step_host(states, actions, out)
            module.last_test_tier = "torch"
            fields = {name: data.pop(name) for name in tuple(kept)}
            accum = {} if accum is None else accum
            for name, value in data.items():
                accum[name] = accum.get(name, 0.0) + bsize * np.asarray(value, dtype=np.float64)
        if need:
            for name, value in fields.items():
                kept[name].append(value[:need].detach().clone() if isinstance(value, torch.Tensor) else value[:need])
            n_kept += need
        batches += 1
        samples += bsize
    if not batches:
        raise ValueError("the test dataloader yielded no batch")
    if tier == "kernel":
        named = module._named_tables(accum.cpu().numpy() / samples, steps)      # the epoch's one copy of the metrics
        kept = {name: [v.cpu().numpy() for v in values] for name, values in kept.items()}
    else:
        named = {name: value / samples for name, value in accum.items()}
    scalars = {name: float(value) for name, value in named.items() if np.ndim(value) == 0}
    tables = {name: np.asarray(value) for name, value in named.items() if np.ndim(value) > 0}
    cat = lambda values: np.concatenate(values) if values else np.empty((0,), dtype=np.float32)
    return EpochReport(scalars=scalars, tables=tables, states=cat(kept["states"]), outputs=cat(kept["outputs"]),
                      actions=cat(kept["actions"]), batches=batches, samples=samples, tier=tier)
