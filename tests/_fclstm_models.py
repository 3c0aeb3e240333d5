"""Builders of the fully-connected LSTM surrogate tests (tests/test_fclstm_surrogate_host.py,
tests/test_fclstm_surrogate_gpu.py): both factories, KSAutoRegFullyConnectedLSTM and KSLatentLSTM."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FACTORIES = ("KSAutoRegFullyConnectedLSTM", "KSLatentLSTM")


def golden():
    """(fclstm_golden.npz, latent_golden.npz, b8 states [8, 20, 1, 64], b8 actions [8, 20, 1, 4]): the autoregressive
    factory's fixture, the latent factory's (``lstm_*``), and the batch both were recorded on (the states of
    surrogate_golden.npz, the 4-actuator actions of latent_golden.npz)."""
    shared, latent = np.load(os.path.join(GOLDEN, "surrogate_golden.npz")), np.load(os.path.join(GOLDEN, "latent_golden.npz"))
    return (np.load(os.path.join(GOLDEN, "fclstm_golden.npz")), latent, torch.from_numpy(shared["b8_states"]),
            torch.from_numpy(latent["lstm_actions"]))


def build(factory="KSAutoRegFullyConnectedLSTM", scaled=False, seed=0, perturb=False, ssize=None, activation=None):
    """(surrogate, PDETrainingModule) of a factory on the CPU in fp32, as the fixtures: delta = tstep = 0.25, tau = 5,
    tbtt = 10, MSELoss(reduction="none").  ``perturb`` moves every bias (the LSTM's and the Linear layers').  ``ssize`` /
    ``activation`` rebuild the tree with another latent width / hidden activation: layouts the kernels refuse."""
    import _latent_models as lm
    import pdecontrol.architectures as arch
    from pdecontrol.surrogates.models.fcnn import LinearBlock
    from pdecontrol.surrogates.training import PDETrainingModule
    from pdecontrol.surrogates.transition import LSTMTransitionModel
    und, dsc = lm.normalize_pair() if scaled else (None, None)
    torch.manual_seed(seed)
    f = getattr(arch, factory)()
    model = f.model()
    if ssize is not None or activation is not None:
        w = 16 if ssize is None else ssize
        act = (torch.nn.SiLU if factory == FACTORIES[0] else torch.nn.ELU) if activation is None else activation
        last = torch.nn.Tanh if factory == FACTORIES[0] else torch.nn.Identity
        model["state_encoder"] = torch.nn.Sequential(LinearBlock(1, 64, 1, 32, activation=act),
                                                     LinearBlock(1, 32, 1, w, activation=act))
        model["state_decoder"] = torch.nn.Sequential(LinearBlock(1, w, 1, 32, activation=act),
                                                     LinearBlock(1, 32, 1, 64, activation=last))
        model["transition_model"] = LSTMTransitionModel(schannels=1, ssize=w, achannels=1, asize=4)
    sur = f.surrogate(delta=0.25, dscaling=dsc, tau=5, **model)
    module = PDETrainingModule(surrogate=sur, loss=torch.nn.MSELoss(reduction="none"), tstep=0.25, delta=0.25,
                               undscaling=und, tau=5, tbtt=10)
    if perturb:
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for name, p in sur.named_parameters():
                if ".bias" in name:            # Linear: .bias; nn.LSTM: .bias_ih_l0, .bias_hh_l0
                    p.add_(0.3 * torch.randn(p.shape, generator=g))
    return sur, module
