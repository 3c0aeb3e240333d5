"""Builders of the latent-surrogate tests (tests/test_latent_surrogate_host.py, tests/test_latent_surrogate_gpu.py)."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden():
    """(latent_golden.npz, surrogate_golden.npz): the latent fixture shares its batch and true deltas with the second."""
    return np.load(os.path.join(GOLDEN, "latent_golden.npz")), np.load(os.path.join(GOLDEN, "surrogate_golden.npz"))


def normalize_pair(mean=0.01, var=0.5, count=100):
    """(undscaling, dscaling): a Normalize with scalar statistics and its inverse, as the controller builds them."""
    from pdegym.common.transforms import BatchTransform, Normalize
    norm = Normalize(aggregate=True, batched=True)
    norm.mean, norm.var, norm.count = torch.full((1, 1, 1), mean), torch.full((1, 1, 1), var), count
    und = BatchTransform(norm)
    return und, und.Inverse


def build(factory="KSLatentConvolutionalLSTM", N=None, scaled=False, seed=0, perturb=False):
    """(surrogate, PDETrainingModule) of a latent factory on the CPU in fp32: delta = tstep = 0.25, tau = 5, tbtt = 10,
    MSELoss(reduction="none"), seeded as the fixture.  ``perturb``: non-trivial LayerNorm affine parameters and biases
    (as tests/_grad_contract_models.py does for the autoregressive model)."""
    import pdecontrol.architectures as arch
    from pdecontrol.surrogates.training import PDETrainingModule
    und, dsc = normalize_pair() if scaled else (None, None)
    torch.manual_seed(seed)
    f = getattr(arch, factory)()
    model = f.model() if N is None else f.model(N=N)
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
