"""Helpers of the SAC agent under the reference's names (pdecontrol/sac/utils.py): target-network updates and two
log-density utilities."""
import math

import torch


def create_log_gaussian(mean, log_std, t):
    """Log-density of ``t`` under the reference's diagonal Gaussian form: the quadratic term is ``(0.5 (t - mean) / std)^2``
    (the 0.5 inside the square, as the reference has it), summed over the last axis."""
    scaled = 0.5 * (t - mean) / (log_std.exp())
    quadratic = -(scaled.pow(2))
    width = mean.shape[-1]
    return quadratic.sum(dim=-1) - log_std.sum(dim=-1) - 0.5 * (width * math.log(2 * math.pi))


def logsumexp(inputs, dim=None, keepdim=False):
    """Max-shifted log-sum-exp; ``dim=None`` flattens first."""
    if dim is None:
        inputs, dim = inputs.view(-1), 0
    top, _ = torch.max(inputs, dim=dim, keepdim=True)
    out = top + (inputs - top).exp().sum(dim=dim, keepdim=True).log()
    return out if keepdim else out.squeeze(dim)


def soft_update(target, source, tau):
    """Polyak average ``target <- (1 - tau) target + tau source``, parameter by parameter."""
    for dst, src in zip(target.parameters(), source.parameters()):
        dst.data.copy_(dst.data * (1.0 - tau) + src.data * tau)


def hard_update(target, source):
    """``target <- source``, parameter by parameter."""
    for dst, src in zip(target.parameters(), source.parameters()):
        dst.data.copy_(src.data)
