"""Builders and helpers of the gradient-contract tests (tests/test_surrogate_grad_contracts_gpu.py).

The modules are the ones the fused-path tests use (``_build`` of test_surrogate_fused_gpu.py, ``_fno_pair`` of
test_fno.py): non-trivial LayerNorm affine parameters and biases, and a ``dscaling`` that is either the identity or the
inverse of a scalar ``Normalize`` (the affine form the controller fits).  They are built on the CPU in fp32; a test takes
its fp64 reference with ``copy.deepcopy(module).double()`` BEFORE the first fused call (the fused packs hang on the
surrogate) and moves the original to the GPU."""
import copy

import numpy as np
import torch


def ks_module(N=64, scaled=True, seed=0):
    """PDETrainingModule around a KSAutoRegConvolutionalLSTM surrogate at grid width N (delta = tstep = 0.25, tau = 5,
    tbtt = 10), CPU fp32."""
    from pdecontrol.architectures import KSAutoRegConvolutionalLSTMN
    from pdecontrol.surrogates.training import PDETrainingModule
    from pdegym.common.transforms import BatchTransform, Normalize
    torch.manual_seed(seed)
    und = None
    if scaled:
        norm = Normalize(aggregate=True, batched=True)
        norm.mean, norm.var, norm.count = torch.full((1, 1, 1), 0.01), torch.full((1, 1, 1), 0.5), 100
        und = BatchTransform(norm)
    f = KSAutoRegConvolutionalLSTMN()
    s = f.surrogate(delta=0.25, dscaling=None if und is None else und.Inverse, tau=5, **f.model(N=N))
    m = PDETrainingModule(surrogate=s, loss=torch.nn.MSELoss(reduction="none"), tstep=0.25, delta=0.25,
                          undscaling=und, tau=5, tbtt=10)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in m.surrogate.named_parameters():
            if "norm" in name or name.endswith(".bias"):
                p.add_(0.3 * torch.randn(p.shape, generator=g))
    return m


def fno_module(scaled=True, seed=0):
    """PDETrainingModule around the Burgers FNO surrogate (width 32, 16 modes, 4 layers; delta = tstep = 0.05, tau = 5,
    tbtt = 10), CPU fp32.  The FNO's parameters do not depend on the grid width."""
    from pdecontrol.architectures import BurgersFNO
    from pdecontrol.surrogates.training import PDETrainingModule
    from pdegym.common.transforms import BatchTransform, Normalize
    und = None
    if scaled:
        norm = Normalize(aggregate=True, batched=True)
        norm.mean, norm.var, norm.count = torch.full((1, 1, 1), 0.02), torch.full((1, 1, 1), 0.3), 50
        und = BatchTransform(norm)
    torch.manual_seed(seed)
    f = BurgersFNO()
    s = f.surrogate(delta=0.05, dscaling=None if und is None else und.Inverse, tau=5, **f.model())
    return PDETrainingModule(surrogate=s, loss=torch.nn.MSELoss(reduction="none"), tstep=0.05, delta=0.05,
                             undscaling=und, tau=5, tbtt=10)


def reference_and_device(module, dev):
    """(fp64 CPU copy, the module itself on ``dev``): the copy is taken before anything ran on the GPU."""
    ref = copy.deepcopy(module).double()
    return ref, module.to(dev)


def grid(K, kind, delta):
    """(times, targets) of a rollout with K internal steps.  ``every``: one action and one reported target per step.
    ``skip``: the integer rule of ``action_and_target_indices`` re-uses an action (the second time point is 2 delta) and
    the targets repeat, skip and reorder steps."""
    if kind == "every":
        times, pick = delta * torch.arange(K), list(range(K))
    else:
        times = delta * torch.tensor([0.0] + [float(k) for k in range(2, K)]) if K >= 3 else delta * torch.arange(K)
        pick = [K - 1, 0, K - 1, K // 2]
    targets = delta * (torch.tensor(pick, dtype=torch.float64) + 1)
    return times, targets


def rollout_tensors(rollout, kind):
    """The tensors a rollout returns, by name: KS -- outputs, deltas, outlatents and both hidden tensors; FNO -- outputs
    and deltas."""
    out = {"outputs": rollout.outputs, "deltas": rollout.deltas}
    if kind == "ks":
        out["outlatents"] = rollout.outlatents
        out["hidden_h"], out["hidden_c"] = rollout.hidden
    return out


def weighted_loss(tensors, weights):
    """sum over every returned tensor of <tensor, fixed random weights> (weights are fp64 CPU tensors)."""
    total = 0
    for name, t in tensors.items():
        total = total + (t * weights[name].to(device=t.device, dtype=t.dtype)).sum()
    return total


def loss_weights(tensors, seed):
    g = torch.Generator().manual_seed(seed)
    return {name: torch.randn(tuple(t.shape), generator=g, dtype=torch.float64) for name, t in tensors.items()}


def assert_close(got, ref, rtol, atol_scale, msg=""):
    """Element-wise closeness with an absolute floor of ``atol_scale * max(1, max|ref|)``."""
    got, ref = got.detach().cpu().double().numpy(), ref.detach().cpu().double().numpy()
    assert got.shape == ref.shape, (msg, got.shape, ref.shape)
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol_scale * max(1.0, float(np.abs(ref).max())), err_msg=msg)


def trainable_grads(module):
    """{name: gradient} of every parameter that requires grad.  An undefined gradient counts as zero: autograd leaves it
    undefined where no path reaches the parameter (H0 when the first step is teacher forced), a fused backward may write
    zeros; a zero gradient where the other side has a non-zero one fails the comparison."""
    out = {}
    for name, p in module.named_parameters():
        if p.requires_grad:
            g = torch.zeros_like(p) if p.grad is None else p.grad
            out[name] = g.detach().cpu().double().numpy()
    return out


def frozen_without_grad(module):
    """Asserts that no parameter with requires_grad=False carries a .grad."""
    bad = [name for name, p in module.named_parameters() if not p.requires_grad and p.grad is not None]
    assert not bad, f"frozen parameters received a .grad: {bad[:6]}{' ...' if len(bad) > 6 else ''}"
