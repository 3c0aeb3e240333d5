"""The latent-space surrogate (LatentAutoRegPDESurrogate) on an MI355X: the KSLatentConvolutionalLSTM layout runs on the
fused kernels (hipops.fused_latent_rollout: two encoder launches + sur_latent_chunk_forward / _backward), every other
latent architecture on plain PyTorch-ROCm kernels.

Each fused case is compared with the same module on the CPU in fp64 (the plain torch spelling), with the bars of
tests/test_surrogate_grad_contracts_gpu.py: forward values rtol 2e-4 / atol 2e-5 of the tensor's scale, every gradient
within GRAD_TOL of its own scale (``check_grads``), the decoder's first bias in front of SiLU + LayerNorm within 2e-3 (the
same decoder, the same cancellation as in the autoregressive model).  The loss is a fixed random weighted sum over every
tensor the rollout returns -- outputs, the deltas of all K steps, inlatents, outlatents and both hidden tensors -- so the
gradient of each reaches every input."""
import numpy as np
import pytest
import torch

import _grad_contract_models as gm
import _latent_models as lm
from conftest import check_grads

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FWD = dict(rtol=2e-4, atol_scale=2e-5)
NOISY_BIAS, NOISY_BIAS_TOL = "state_decoder.model.block_l0.deconvolution.bias", 2e-3


def _tensors(ro):
    return {"outputs": ro.outputs, "deltas": ro.deltas, "inlatents": ro.inlatents, "outlatents": ro.outlatents,
            "hidden_h": ro.hidden[0], "hidden_c": ro.hidden[1]}


def _pair(N, scaled, seed=0):
    """(fp64 CPU reference surrogate, fp32 GPU surrogate): the copy is taken before anything ran on the GPU."""
    import copy
    factory = "KSLatentConvolutionalLSTM" if N == 64 else "KSLatentConvolutionalLSTMN"
    sur, module = lm.build(factory, N=None if N == 64 else N, scaled=scaled, seed=seed, perturb=True)
    ref = copy.deepcopy(module).double()
    return ref, module.to(DEV)


_CACHE = {}


def _cached_pair(N, scaled):
    if (N, scaled) not in _CACHE:
        _CACHE[(N, scaled)] = _pair(N, scaled)
    return _CACHE[(N, scaled)]


def _inputs(B, S, A, N, seed, amp=1.0):
    g = torch.Generator().manual_seed(seed)
    st = (torch.rand(B, S, 1, N, generator=g, dtype=torch.float64) * 2 - 1) * amp
    ac = torch.rand(B, A, 1, N, generator=g, dtype=torch.float64) * 2 - 1
    return st, ac


def _count_calls(monkeypatch, module, name):
    calls = []
    orig = getattr(module, name)
    monkeypatch.setattr(module, name, lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    return calls


def _clear(*modules):
    for m in modules:
        for p in m.parameters():
            p.grad = None


# (N, S, K, B, hidden carried, Normalize dscaling, target grid): every N, S, K, B, hidden and scaling value, each with
# several of the others
ROLLOUT_CASES = [
    (64, 1, 1, 1, False, False, "every"), (64, 5, 10, 4, True, True, "every"), (64, 5, 15, 64, False, True, "skip"),
    (64, 1, 10, 1, True, False, "skip"), (64, 5, 1, 4, False, False, "every"), (64, 1, 15, 4, True, True, "every"),
    (128, 1, 10, 64, True, False, "every"), (128, 5, 15, 1, False, True, "every"), (128, 5, 10, 4, True, False, "skip"),
    (128, 1, 1, 4, False, True, "every"),
    (256, 5, 10, 4, False, False, "every"), (256, 1, 15, 1, True, True, "skip"), (256, 5, 15, 64, True, False, "every"),
    (256, 1, 1, 64, False, True, "every"),
]


@pytest.mark.parametrize("N,S,K,B,with_hidden,scaled,kind", ROLLOUT_CASES,
                         ids=[f"N{c[0]}-S{c[1]}-K{c[2]}-B{c[3]}-{'hidden' if c[4] else 'H0C0'}-{'affine' if c[5] else 'identity'}-{c[6]}"
                              for c in ROLLOUT_CASES])
def test_latent_rollout_forward_and_gradients(N, S, K, B, with_hidden, scaled, kind, monkeypatch):
    from pdecontrol.surrogates import hipops
    ref, gpu = _cached_pair(N, scaled)
    sur_ref, sur_gpu = ref.surrogate, gpu.surrogate
    _clear(sur_ref, sur_gpu)
    times, targets = gm.grid(K, kind, sur_ref.delta)
    seed = N * 1000 + S * 100 + K * 10 + B
    st, ac = _inputs(B, S, len(times), N, seed)
    hidden_ref = hidden_gpu = None
    if with_hidden:
        g = torch.Generator().manual_seed(seed + 7)
        shape = (B,) + tuple(sur_ref.transition_model.H0.shape)
        h = (0.5 * torch.randn(shape, generator=g, dtype=torch.float64), 0.5 * torch.randn(shape, generator=g, dtype=torch.float64))
        hidden_ref = tuple(t.clone().requires_grad_(True) for t in h)
        hidden_gpu = tuple(t.to(DEV, torch.float32).requires_grad_(True) for t in h)
    calls = _count_calls(monkeypatch, hipops, "fused_latent_rollout")
    for sur in (sur_ref, sur_gpu):    # hidden = None: the initial state H0 / C0 is trainable in this case
        sur.transition_model.H0.requires_grad_(not with_hidden)
        sur.transition_model.C0.requires_grad_(not with_hidden)
    try:
        st_r, ac_r = st.clone().requires_grad_(True), ac.clone().requires_grad_(True)
        st_g, ac_g = st.to(DEV, torch.float32).requires_grad_(True), ac.to(DEV, torch.float32).requires_grad_(True)
        ro_ref = sur_ref.rollout(st_r, ac_r, times, targets, hidden=hidden_ref)
        ro_gpu = sur_gpu.rollout(st_g, ac_g, times, targets, hidden=hidden_gpu)
        assert calls, "the latent ConvLSTM must run on hipops.fused_latent_rollout"
        assert ro_gpu.deltas.shape[1] == K, "deltas cover every internal step"
        weights = gm.loss_weights(_tensors(ro_ref), seed)
        gm.weighted_loss(_tensors(ro_ref), weights).backward()
        gm.weighted_loss(_tensors(ro_gpu), weights).backward()
        torch.cuda.synchronize(DEV)
        label = f"latent rollout N={N} S={S} K={K} B={B} hidden={with_hidden} scaled={scaled} {kind}"
        want = _tensors(ro_ref)
        for name, got in _tensors(ro_gpu).items():
            gm.assert_close(got, want[name], FWD["rtol"], FWD["atol_scale"], msg=f"{label}: {name}")
        grad = lambda t: (torch.zeros_like(t) if t.grad is None else t.grad).detach().cpu().double().numpy()
        got_in = {"input.states": grad(st_g), "input.actions": grad(ac_g)}
        want_in = {"input.states": grad(st_r), "input.actions": grad(ac_r)}
        if with_hidden:
            for j, tag in enumerate(("h", "c")):
                got_in[f"input.hidden_{tag}"], want_in[f"input.hidden_{tag}"] = grad(hidden_gpu[j]), grad(hidden_ref[j])
        check_grads(label + " inputs", got_in, want_in.__getitem__)
        ref_grads, gpu_grads = gm.trainable_grads(sur_ref), gm.trainable_grads(sur_gpu)
        noisy = {k: gpu_grads.pop(k) for k in [NOISY_BIAS] if k in gpu_grads}
        check_grads(label + " parameters", gpu_grads, ref_grads.__getitem__)
        check_grads(label + " decoder bias in front of LayerNorm", noisy, ref_grads.__getitem__, tol=NOISY_BIAS_TOL)
        gm.frozen_without_grad(sur_gpu)
    finally:
        for sur in (sur_ref, sur_gpu):
            sur.transition_model.H0.requires_grad_(False)
            sur.transition_model.C0.requires_grad_(False)
            _clear(sur)


def test_no_grad_inference_saves_nothing(monkeypatch):
    from pdecontrol.surrogates import hipops
    ref, gpu = _pair(64, True, seed=6)
    times, targets = gm.grid(6, "every", ref.surrogate.delta)
    st, ac = _inputs(4, 2, len(times), 64, 21)
    saved = _count_calls(monkeypatch, hipops, "_saved_buffer")
    calls = _count_calls(monkeypatch, hipops, "fused_latent_rollout")
    with torch.no_grad():
        ro = gpu.surrogate.rollout(st.float().to(DEV), ac.float().to(DEV), times, targets)
        ro_ref = ref.surrogate.rollout(st, ac, times, targets)
    assert calls and not saved, "no-grad inference must run the fused forward without a saved buffer"
    want = _tensors(ro_ref)
    for name, got in _tensors(ro).items():
        gm.assert_close(got, want[name], FWD["rtol"], FWD["atol_scale"], msg=f"no-grad: {name}")
    assert all(p.grad is None for p in gpu.surrogate.parameters())


def test_frozen_submodule_over_two_optimizer_steps(monkeypatch):
    from pdecontrol.surrogates import hipops
    ref, gpu = _pair(64, True, seed=4)
    for m in (ref, gpu):
        m.surrogate.state_encoder.requires_grad_(False)
    lr = gpu.lr
    ref_opt = torch.optim.Adam([p for p in ref.surrogate.parameters() if p.requires_grad], lr=lr)
    opt = gpu.configure_optimizers()[0][0]
    assert isinstance(opt, torch.optim.Adam) and not isinstance(opt, hipops.PackAdam)
    start = {n: p.detach().clone() for n, p in gpu.surrogate.named_parameters()}
    st, ac = _inputs(4, 13, 13, 64, 5, amp=0.8)
    calls = _count_calls(monkeypatch, hipops, "fused_latent_rollout")
    for it in range(2):
        out_ref = ref.training_step((st, ac), it)
        out_ref["loss"].backward()
        out = gpu.training_step((st.float().to(DEV), ac.float().to(DEV)), it)
        out["loss"].backward()
        torch.cuda.synchronize(DEV)
        rel = abs(float(out["loss"].detach()) - float(out_ref["loss"].detach())) / abs(float(out_ref["loss"].detach()))
        assert rel < 1e-5, (it, rel)
        gm.frozen_without_grad(gpu.surrogate)
        ref_grads = gm.trainable_grads(ref.surrogate)
        check_grads(f"frozen latent state encoder, step {it}", gm.trainable_grads(gpu.surrogate), ref_grads.__getitem__)
        ref_opt.step()
        opt.step()
        ref_opt.zero_grad(set_to_none=True)
        opt.zero_grad(set_to_none=True)
    assert len(calls) == 4, "two TBPTT chunks per step, both on the fused latent rollout"
    ref_params = dict(ref.surrogate.named_parameters())
    for name, p in gpu.surrogate.named_parameters():
        if not p.requires_grad:
            assert torch.equal(p.detach(), start[name]), f"frozen parameter {name} moved"
            continue
        err = float((p.detach().cpu().double() - ref_params[name].detach()).abs().max())
        assert err <= 2 * lr, f"{name}: {err:.3e} from the fp64 reference after 2 Adam steps"


@pytest.mark.parametrize("scaled", [False, True], ids=["identity", "affine"])
def test_training_step_matches_reference_fixture(scaled, monkeypatch):
    """training_step at the fixture's batch (N = 64, B = 8, T = 20) against the reference's recorded loss and gradients."""
    from pdecontrol.surrogates import hipops
    g, shared = lm.golden()
    sur, module = lm.build(scaled=scaled)
    module = module.to(DEV)
    calls = _count_calls(monkeypatch, hipops, "fused_latent_rollout")
    batch = (torch.from_numpy(shared["b8_states"]).to(DEV), torch.from_numpy(shared["b8_actions"]).to(DEV))
    out = module.training_step(batch, 0)
    out["loss"].backward()
    torch.cuda.synchronize(DEV)
    assert calls
    ref_loss = float(g["nz_loss" if scaled else "id_loss"])
    assert abs(float(out["loss"].detach()) - ref_loss) / abs(ref_loss) < 1e-5
    np.testing.assert_allclose(out["outputs"].cpu().numpy(), g["id_outputs"], rtol=2e-4,
                               atol=2e-5 * max(1.0, float(np.abs(g["id_outputs"]).max())))
    grads = {k: p.grad.detach().cpu().double().numpy() for k, p in module.surrogate.named_parameters() if p.grad is not None}
    assert sorted(grads) == sorted(k[8:] for k in g.files if k.startswith("id_grad/"))
    check_grads(f"latent training_step vs reference fixture scaled={scaled}", grads, lambda k: g["id_grad/" + k])


def test_fully_connected_latent_lstm_runs_on_plain_kernels(caplog):
    import logging
    from pdecontrol.surrogates import hipops, ops
    assert ops.fused_enabled()
    _, cpu = lm.build("KSLatentLSTM")
    _, gpu = lm.build("KSLatentLSTM")
    gpu = gpu.to(DEV)
    assert not hipops.fused_latent_supported(gpu.surrogate)
    g, shared = lm.golden()
    s, a = torch.from_numpy(shared["b8_states"]), torch.from_numpy(g["lstm_actions"])
    with caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        out = gpu.training_step((s.to(DEV), a.to(DEV)), 0)
    assert any("plain PyTorch-ROCm" in r.message and "KSLatentConvolutionalLSTM" in r.message for r in caplog.records) or \
        "LatentAutoRegPDESurrogate/LSTMTransitionModel" in ops._NOTIFIED
    out["loss"].backward()
    ref = cpu.training_step((s, a), 0)
    ref["loss"].backward()
    torch.cuda.synchronize(DEV)
    np.testing.assert_allclose(float(out["loss"].detach()), float(ref["loss"].detach()), rtol=1e-5)
    ref_grads = {k: p.grad.double().numpy() for k, p in cpu.surrogate.named_parameters() if p.grad is not None}
    check_grads("KSLatentLSTM on plain PyTorch-ROCm", {k: p.grad.cpu().double().numpy() for k, p in gpu.surrogate.named_parameters()
                                                        if p.grad is not None}, ref_grads.__getitem__)


def test_latent_ensemble_steps_world_env_like_cpu():
    """A PDEEnsemble of three latent members drives WorldVecEnv (the generic world path: the device-resident path is for
    the autoregressive layout only) for five steps, on the fused kernels and on the CPU."""
    import _world_scenario as sc
    from test_world_env import namespace
    from pdecontrol.architectures import KSLatentConvolutionalLSTM
    from pdecontrol.surrogates import hipops
    from pdecontrol.surrogates.surrogate import PDEEnsemble
    from pdecontrol.surrogates.training import PDETrainingModule

    def run(device):
        M = namespace()
        M.factory_cls = KSLatentConvolutionalLSTM

        def three(modules, num_elites):
            torch.manual_seed(2)
            f, m0 = KSLatentConvolutionalLSTM(), modules[0]
            sur = f.surrogate(delta=m0.delta, dscaling=None, tau=m0.tau, **f.model())
            third = PDETrainingModule(surrogate=sur, loss=torch.nn.MSELoss(reduction="none"), tstep=m0.tstep, delta=m0.delta,
                                      tau=m0.tau, tbtt=10).to(device)
            return PDEEnsemble(modules + [third], num_elites=3)

        M.Ensemble = three
        return sc.run(M, device=device)

    calls = []
    orig = hipops.fused_latent_rollout
    hipops.fused_latent_rollout = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        got = run(DEV)
    finally:
        hipops.fused_latent_rollout = orig
    assert len(calls) >= 3 * 5, "every member's imagined step must run on the fused latent rollout"
    assert not sc.run.last_world._use_device_path()
    want = run("cpu")
    assert sorted(got) == sorted(want)
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.dtype.kind == "f":
            np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5, err_msg=k)
        else:
            np.testing.assert_array_equal(a, b, err_msg=k)
