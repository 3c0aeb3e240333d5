"""``BurgersPhyPDELoss`` on the Burgers kernels (C ABI: include/burgers_hip.h ``bg_phyloss_*``; kernels: csrc/burgers.hip):
the element-wise loss in ONE launch and its gradient in ONE launch, instead of about 25 small torch kernels per
sub-step and direction.  ``_PhyLossFn`` is an ordinary autograd node: it launches on the current stream, allocates
through torch only and never synchronises with the host, so it can be captured in a hipGraph."""
import torch

from hipbind import ptr as _ptr, stream as _stream
from pdecontrol.surrogates import ops

WIDTHS = (64, 128, 256, 512, 1024)


def load():
    from pdegym.burgers import _hip
    return _hip.load()            # raises when the library has not been built: no silent fallback


def _check(rc):
    from pdegym.burgers import _hip
    _hip.check(rc)


def unsupported(augmented):
    """None when the kernels compute the loss of ``augmented``, else the reason."""
    if augmented.dtype != torch.float32:
        return f"physics loss on {str(augmented.dtype).replace('torch.', '')} input (the kernels are fp32)"
    if augmented.dim() != 4 or augmented.shape[2] != 1:
        return f"physics loss on input of shape {tuple(augmented.shape)} (the kernels take [B, T, 1, N])"
    if augmented.shape[-1] not in WIDTHS:
        return f"physics loss at N = {augmented.shape[-1]} (the kernels take N in {WIDTHS})"
    if augmented.shape[0] * augmented.shape[1] == 0:
        return "physics loss on an empty batch"
    return None


def use_kernels(augmented):
    """True when the loss of this tensor runs on the HIP kernels: any fp32 CUDA tensor [B, T, 1, N] of a supported width
    unless opted out (``ops.fused(False)`` / ``PDECONTROL_FUSED=0``).  What the kernels refuse runs the torch spelling on
    PyTorch-ROCm kernels, announced once per reason."""
    if not (augmented.is_cuda and ops.fused_enabled()):
        return False
    reason = unsupported(augmented)
    if reason is None:
        load()
        return True
    if reason not in ops._NOTIFIED:
        ops._NOTIFIED.add(reason)
        ops._LOG.warning("the fused HIP kernels do not implement the %s: it runs on plain PyTorch-ROCm kernels", reason)
    return False


class _PhyLossFn(torch.autograd.Function):
    """Element-wise loss [B, T, 1, N] of ``augmented``.  Saved for backward (only when the input needs a gradient):
    the input, ``diff = augmented - target`` and, for ``substeps > 1``, the state before every sub-step but the first."""

    @staticmethod
    def forward(ctx, augmented, dx, dt, nu, substeps):
        lib = load()
        a = augmented.contiguous()
        B, T, _, N = a.shape
        need = ctx.needs_input_grad[0]          # (grad mode is off inside forward: ask the node)
        loss = torch.empty_like(a)
        diff = torch.empty_like(a) if need else None
        n_states = B * (T - 1) * (substeps - 1) * N if need else 0
        states = torch.empty(n_states, device=a.device, dtype=torch.float32) if n_states else None
        _check(lib.bg_phyloss_forward(_stream(), _ptr(a), B, T, N, dx, dt, nu, substeps, _ptr(loss), _ptr(diff), _ptr(states),
                                      n_states))
        if need:
            ctx.save_for_backward(a, diff, *(() if states is None else (states,)))
            ctx.meta = (dx, dt, nu, substeps)
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        lib = load()
        a, diff, *rest = ctx.saved_tensors
        states = rest[0] if rest else None
        dx, dt, nu, substeps = ctx.meta
        B, T, _, N = a.shape
        g = g_loss.contiguous()                 # (the gradient of a mean arrives as an expanded scalar)
        grad = torch.empty_like(a)
        _check(lib.bg_phyloss_backward(_stream(), _ptr(a), _ptr(diff), _ptr(g), _ptr(states),
                                       0 if states is None else states.numel(), B, T, N, dx, dt, nu, substeps, _ptr(grad)))
        return grad, None, None, None, None


def burgers_phyloss(augmented, dx, dt, nu, substeps=1):
    """The element-wise physics loss of fp32 CUDA ``augmented`` [B, T, 1, N] (``unsupported(augmented) is None``)."""
    if not torch.is_grad_enabled():     # the node's needs_input_grad ignores no_grad: detach, so that nothing is saved
        augmented = augmented.detach()
    return _PhyLossFn.apply(augmented, float(dx), float(dt), float(nu), int(substeps))
