"""Builders of the delay-surrogate tests (tests/test_delay_surrogate_host.py, tests/test_delay_surrogate_gpu.py)."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden():
    """(delay_golden.npz, b8 states [8, 20, 1, 64], b8 actions [8, 20, 1, 4], surrogate_golden.npz): the delay fixture reuses
    the surrogate fixture's states and the latent fixture's 4-actuator actions."""
    shared, latent = np.load(os.path.join(GOLDEN, "surrogate_golden.npz")), np.load(os.path.join(GOLDEN, "latent_golden.npz"))
    return (np.load(os.path.join(GOLDEN, "delay_golden.npz")), torch.from_numpy(shared["b8_states"]),
            torch.from_numpy(latent["lstm_actions"]), shared)


def build(scaled=False, seed=0, perturb=False, delay=None):
    """(surrogate, PDETrainingModule) of KSDelayCNNSurrogateFactory on the CPU in fp32, as the fixture: delta = tstep = 0.25,
    tau = 5, tbtt = 10, MSELoss(reduction="none").  ``perturb``: non-trivial LayerNorm affine parameters and biases.
    ``delay``: rebuild the transition with another window length (a layout the kernels refuse)."""
    import _latent_models as lm
    import pdecontrol.architectures as arch
    from pdecontrol.surrogates.training import PDETrainingModule
    from pdecontrol.surrogates.transition import DelayTransitionModel
    from pdecontrol.surrogates.models.fcnn import LinearBlock
    und, dsc = lm.normalize_pair() if scaled else (None, None)
    torch.manual_seed(seed)
    f = arch.KSDelayCNNSurrogateFactory()
    model = f.model()
    if delay is not None:
        fwd = torch.nn.Sequential(LinearBlock(12 * delay, 8, 12, 8, activation=torch.nn.ELU),
                                  LinearBlock(12, 8, 8, 8, activation=torch.nn.ELU),
                                  LinearBlock(8, 8, 8, 8, activation=torch.nn.Tanh))
        model["transition_model"] = DelayTransitionModel(8, 8, 4, 8, fwd_model=fwd, delay=delay)
    sur = f.surrogate(delta=0.25, dscaling=dsc, tau=5, **model)
    module = PDETrainingModule(surrogate=sur, loss=torch.nn.MSELoss(reduction="none"), tstep=0.25, delta=0.25,
                               undscaling=und, tau=5, tbtt=10)
    if perturb:
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for name, p in sur.named_parameters():
                if "norm" in name or name.endswith(".bias"):
                    p.add_(0.3 * torch.randn(p.shape, generator=g))
    return sur, module


def stored(g, prefix, name, value):
    """Compare ``value`` with the fixture's record of it: the full tensor, or fp64 sum, sum of squares and every 97th element."""
    v = np.asarray(value)
    if f"{prefix}/{name}" in g.files:
        np.testing.assert_array_equal(v, g[f"{prefix}/{name}"], err_msg=name)
        return
    v64 = v.astype(np.float64)
    assert v64.sum() == g[f"{prefix}sum/{name}"] and (v64 * v64).sum() == g[f"{prefix}sq/{name}"], name
    np.testing.assert_array_equal(v.reshape(-1)[::97], g[f"{prefix}pick/{name}"], err_msg=name)


def recorded(g, prefix):
    """Names of the tensors the fixture records under ``prefix``."""
    out = set()
    for k in g.files:
        head, _, name = k.partition("/")
        if head in (prefix, prefix + "pick"):
            out.add(name)
    return out
