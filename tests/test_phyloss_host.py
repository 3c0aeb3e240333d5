"""The Burgers physics-informed loss (pdecontrol/surrogates/phyloss) on the CPU: the reference's import path and names,
bit parity of the torch spelling with the reference class's recorded outputs (tests/golden/phyloss_golden.npz, written by
tools/gen_phyloss_golden.py), the ``substeps`` extension, and the FNO surrogate trained on decoded states."""
import numpy as np
import pytest
import torch

import _phyloss_models as pm


def test_reference_import_path_names_and_constructor_call():
    from pdecontrol.surrogates.phyloss import phyloss          # the reference's line (mbrl.py:38)
    from pdecontrol.surrogates.utils import ignore_extra_keywords
    assert phyloss.MSELoss is torch.nn.MSELoss
    for name in ("MSELoss", "PhyPDELoss", "BurgersPhyPDELoss"):
        assert isinstance(getattr(phyloss, name), type), name
    assert issubclass(phyloss.BurgersPhyPDELoss, phyloss.PhyPDELoss)
    loss = ignore_extra_keywords(phyloss.BurgersPhyPDELoss)(**pm.SCENARIO, reduction="none")    # mbrl.py:213-216
    assert (loss.dx, loss.dt, loss.nu) == (pm.SCENARIO["dx"], pm.SCENARIO["dt"], pm.SCENARIO["nu"])
    assert loss.substeps == 1 and loss.criterion.reduction == "none"
    assert ignore_extra_keywords(phyloss.MSELoss)(**pm.SCENARIO, reduction="none").reduction == "none"

    class _Sur:
        psteps = 50

    class _Mod:
        surrogate = _Sur()
    loss.check(pm.SCENARIO, _Mod())
    with pytest.raises(AssertionError):
        loss.check(dict(pm.SCENARIO, cfg_steps=49), _Mod())
    with pytest.raises(ValueError):
        phyloss.BurgersPhyPDELoss(dx=0.1, dt=1e-3, nu=0.01, substeps=0)


@pytest.mark.parametrize("tag", pm.TAGS)
def test_cpu_fp32_is_bit_equal_to_the_reference_class(tag):
    from pdecontrol.surrogates.phyloss import phyloss
    g = pm.golden()
    dx, dt, nu = (float(v) for v in g[f"{tag}_params"])
    u = torch.from_numpy(g[f"{tag}_u"]).requires_grad_(True)
    loss = phyloss.BurgersPhyPDELoss(dx=dx, dt=dt, nu=nu, reduction="none")(u, "ignored", also="ignored")
    assert loss.dtype == torch.float32 and loss.shape == u.shape
    assert np.array_equal(loss.detach().numpy(), g[f"{tag}_loss_none"])
    (torch.from_numpy(g[f"{tag}_weights"]) * loss).sum().backward()
    assert np.array_equal(u.grad.numpy(), g[f"{tag}_grad"])
    with torch.no_grad():
        mean = phyloss.BurgersPhyPDELoss(dx=dx, dt=dt, nu=nu, reduction="mean")(u)
    assert np.array_equal(mean.numpy(), g[f"{tag}_loss_mean"])
    # slot 0 is compared with the LAST slice (the reference's choice), not with a predecessor
    a = u.detach()
    assert np.array_equal(loss.detach()[:, 0].numpy(), ((a[:, 0] - a[:, -1]) ** 2).numpy())


def test_substeps_chain_phyevolve_and_default_is_one():
    g = pm.golden()
    dx, dt, nu = (float(v) for v in g["n128_params"])
    from pdecontrol.surrogates.phyloss import phyloss
    u = torch.from_numpy(g["n128_u"])
    base = phyloss.BurgersPhyPDELoss(dx=dx, dt=dt, nu=nu)
    assert torch.equal(phyloss.BurgersPhyPDELoss(dx=dx, dt=dt, nu=nu, substeps=1)(u), base(u))
    for S in (2, 5):
        evolved = u
        for _ in range(S):
            evolved = base.phyevolve(evolved)
        target = torch.cat((u[:, -1:], evolved[:, :-1]), dim=1)
        got = phyloss.BurgersPhyPDELoss(dx=dx, dt=dt, nu=nu, substeps=S)(u)
        assert torch.equal(got, (u - target) ** 2), S
        assert not torch.equal(got, base(u))
    # fp64 input runs the same spelling at its own precision
    u64 = u.double()
    ref = phyloss.BurgersPhyPDELoss(dx=dx, dt=dt, nu=nu, substeps=3)
    l64 = ref(u64)
    assert l64.dtype == torch.float64
    np.testing.assert_allclose(ref(u).numpy(), l64.numpy(), rtol=0, atol=1e-5 * float(l64.max()))


def test_fno_trains_on_decoded_states_with_the_physics_loss_on_cpu():
    from pdecontrol.architectures import BurgersFNO
    f = BurgersFNO()
    assert f.surrogate(delta=0.05, **f.model()).training_mode == "delta"
    assert pm.fno_module(torch.nn.MSELoss(reduction="none"), training_mode=None).training_mode == "delta"
    with pytest.raises(ValueError):
        f.surrogate(delta=0.05, training_mode="latent", **f.model())
    loss = pm.burgers_loss(64, substeps=2)
    m = pm.fno_module(loss, width=16, modes=8, layers=2)
    assert m.training_mode == "decoded" and m.surrogate.training_mode == "decoded"
    st, ac = pm.smooth_fields(4, 12, 64, 5, torch.float32), pm.smooth_fields(4, 12, 64, 6, torch.float32)
    out = m.training_step((st, ac), 0)
    out["loss"].backward()
    assert torch.isfinite(out["loss"])
    with torch.no_grad():
        spelled = loss(torch.cat((st[:, :1], out["outputs"][:, :-1]), dim=1), st).mean()
    assert torch.equal(out["loss"].detach(), spelled)
    for name, p in m.surrogate.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, name


def test_entry_points_validate_on_the_host():
    """Refusals come back as a negative status with a message, before anything is launched (so this needs no GPU)."""
    import ctypes
    from pdegym.burgers import _hip
    lib = _hip.load()
    one = ctypes.c_void_p(64)
    fwd = lambda B, T, N, S, diff, states, n: lib.bg_phyloss_forward(None, one, B, T, N, 0.1, 1e-3, 0.01, S, one, diff, states, n)
    bwd = lambda B, T, N, S, states, n: lib.bg_phyloss_backward(None, one, one, one, states, n, B, T, N, 0.1, 1e-3, 0.01, S, one)
    assert lib.bg_phyloss_forward(None, None, 1, 1, 64, 0.1, 1e-3, 0.01, 1, None, None, None, 0) == -1
    assert b"bad argument" in lib.bg_last_error()
    assert fwd(2, 3, 96, 1, None, None, 0) == -4 and b"96" in lib.bg_last_error()
    assert fwd(2, 3, 2048, 1, None, None, 0) == -4 and b"supported sizes" in lib.bg_last_error()
    assert fwd(2, 3, 64, 0, None, None, 0) == -1                              # substeps < 1
    assert fwd(0, 3, 64, 1, None, None, 0) == -1
    assert fwd(2, 3, 64, 4, one, None, 0) == -3                               # a gradient at substeps > 1 needs the state store
    need = 2 * 2 * 3 * 64
    assert fwd(2, 3, 64, 4, one, one, need - 1) == -3 and str(need).encode() in lib.bg_last_error()
    assert bwd(2, 3, 64, 4, None, 0) == -3 and bwd(2, 3, 64, 4, one, need - 1) == -3
    assert bwd(2, 3, 100, 1, None, 0) == -4
