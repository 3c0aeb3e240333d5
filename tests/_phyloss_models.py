"""Shared pieces of tests/test_phyloss_host.py and tests/test_phyloss_gpu.py."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "phyloss_golden.npz")
TAGS = ("n512", "n128", "t1", "t2")
#: the keys of pdegym.burgers' ``scenario`` at its defaults (BurgersBatchedVecEnv.scenario), as the controller passes them
SCENARIO = {"cfg_steps": 50, "L": 2 * np.pi, "N": 512, "dx": 2 * np.pi / 512, "Tmax": 10.0, "dt": 1e-3, "nu": 0.01,
            "Xi": [0, 0.25, 0.5, 0.75], "objective": "l2control"}


def golden():
    return np.load(GOLDEN)


def smooth_fields(B, T, N, seed, dtype=torch.float64, amp=1.0):
    """[B, T, 1, N]: per (b, t) a sum of four sines with seeded amplitudes and phases (NOT a solver trajectory: on one the
    loss is pure cancellation and a relative bound says nothing)."""
    rs = np.random.RandomState(seed)
    x = np.linspace(0, 2 * np.pi, N, endpoint=False)
    amps, phases = rs.uniform(-1, 1, (B * T, 4, 1)), rs.uniform(0, 6, (B * T, 4, 1))
    rows = (amps * np.sin(np.arange(1, 5)[None, :, None] * x[None, None, :] + phases)).sum(1) * amp
    return torch.from_numpy(rows.reshape(B, T, 1, N)).to(dtype)


def weights_like(t, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(t.shape, generator=g, dtype=torch.float64) * 2 - 1).to(t.dtype)


def burgers_loss(N, substeps=1, reduction="none", dt=None, nu=0.02):
    """The loss at the parameters tests/test_burgers.py steps the kernel with (dt small enough for stability at 1024)."""
    from pdecontrol.surrogates.phyloss import phyloss
    dt = (5e-4 if N < 1024 else 1e-4) if dt is None else dt
    return phyloss.BurgersPhyPDELoss(dx=2 * np.pi / N, dt=dt, nu=nu, reduction=reduction, substeps=substeps)


def fno_module(loss, training_mode="decoded", device="cpu", seed=0, **model):
    from pdecontrol.architectures import BurgersFNO
    from pdecontrol.surrogates.training import PDETrainingModule
    torch.manual_seed(seed)
    f = BurgersFNO()
    extra = {} if training_mode is None else {"training_mode": training_mode}
    s = f.surrogate(delta=0.05, dscaling=None, tau=5, **extra, **f.model(**model))
    return PDETrainingModule(surrogate=s, loss=loss, tstep=0.05, delta=0.05, tau=5, tbtt=10).to(device)
