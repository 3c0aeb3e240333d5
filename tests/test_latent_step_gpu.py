"""The captured optimizer step of the latent ConvLSTM surrogate on an MI355X (``hipops.fused_latent_tbptt_train`` behind
``PDETrainingModule._latent_training_step``, replayed by ``GraphedTBPTTStep``): T = 13 at tbtt = 5, tau = 2 is three chunks
(5 + 5 + 3), so the pass crosses two chunk boundaries and ends on a ragged chunk.

Against the same module on the CPU in fp64 with the bounds of tests/test_latent_surrogate_gpu.py (loss 1e-5 relative, every
gradient under ``check_grads``, the decoder's first bias in front of SiLU + LayerNorm within 2e-3, parameters within 2 lr after
two Adam steps); a replay against the same pass launched eagerly and two fresh steps against each other bit for bit; the clip
with the bound tests/test_surrogate_clip_gpu.py holds ``grad_norm`` to; and the re-capture after a re-fit of the delta
statistics."""
import copy

import numpy as np
import pytest
import torch

import _grad_contract_models as gm
import _latent_models as lm
import _surrogate_phase_scenario as psc
from conftest import check_grads

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
T, TAU, TBTT = 13, 2, 5
NOISY_BIAS, NOISY_BIAS_TOL = "state_decoder.model.block_l0.deconvolution.bias", 2e-3


def _module(N, seed=0, scaled=True):
    factory = "KSLatentConvolutionalLSTM" if N == 64 else "KSLatentConvolutionalLSTMN"
    _, module = lm.build(factory, N=None if N == 64 else N, scaled=scaled, seed=seed, perturb=True)
    module.tau, module.tbtt = TAU, TBTT
    return module


def _batch(B, N, seed, amp=0.8):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(B, T, 1, N, generator=g, dtype=torch.float64) * 2 - 1) * amp,
            torch.rand(B, T, 1, N, generator=g, dtype=torch.float64) * 2 - 1)


def _gpu(batch):
    return tuple(t.float().to(DEV) for t in batch)


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _state(module):
    """Parameters and the packs' Adam state (moments, step counters) as bytes."""
    params, adam = psc.optimizer_state(module)
    return [a.tobytes() for a in params + adam]


def _grad_norm(module):
    grads = [p.grad.detach().double().reshape(-1) for p in module.surrogate.parameters() if p.grad is not None]
    return float(torch.linalg.vector_norm(torch.cat(grads)))


def _last_step(module):
    return module.__dict__["_last_graphed_step"]


@pytest.mark.parametrize("N,B", [(64, 1), (64, 4), (256, 4)])
def test_captured_latent_step_against_the_fp64_reference(N, B):
    module = _module(N)
    ref = copy.deepcopy(module).double()
    gpu = module.to(DEV)
    lr = gpu.lr
    ref_opt = torch.optim.Adam([p for p in ref.surrogate.parameters() if p.requires_grad], lr=lr)
    batch = _batch(B, N, 100 * N + B)
    for it in range(2):
        out_ref = ref.training_step(batch, it)
        out_ref["loss"].backward()
        out = gpu.fused_step(_gpu(batch))
        torch.cuda.synchronize(DEV)
        step = _last_step(gpu)
        assert step.used_latent and step.adam_in_flush and step.opt is None, "the latent module takes the captured kernel step"
        assert not step.autotune or not step.used_pipelined, "one schedule: nothing to tune"
        want = float(out_ref["loss"].detach())
        rel = abs(float(out["loss"]) - want) / abs(want)
        assert rel < 1e-5, (it, rel)
        assert out["hsteploss"].shape == (T,) and float(out["hsteploss"][0]) == 0.0
        for key in ("outputs", "outdeltas", "deltas", "hsteploss"):
            assert tuple(out[key].shape) == tuple(out_ref[key].shape), key
            gm.assert_close(out[key], out_ref[key], 2e-4, 2e-5, msg=f"{key} at step {it}")
        ref_grads = gm.trainable_grads(ref.surrogate)
        grads = {k: v for k, v in gm.trainable_grads(gpu.surrogate).items() if k in ref_grads}
        noisy = {k: grads.pop(k) for k in [NOISY_BIAS] if k in grads}
        label = f"captured latent step N={N} B={B} step {it}"
        check_grads(label, grads, ref_grads.__getitem__)
        check_grads(label + " decoder bias in front of LayerNorm", noisy, ref_grads.__getitem__, tol=NOISY_BIAS_TOL)
        ref_opt.step()
        ref_opt.zero_grad(set_to_none=True)
    assert gpu.surrogate._fused_packs.adam_step_count() == 2
    ref_params = dict(ref.surrogate.named_parameters())
    for name, p in gpu.surrogate.named_parameters():
        err = float((p.detach().cpu().double() - ref_params[name].detach()).abs().max())
        assert err <= 2 * lr, f"{name}: {err:.3e} from the fp64 reference after 2 Adam steps"


def test_replay_equals_the_eager_launches_and_a_second_fresh_step():
    from pdecontrol.surrogates import hipops
    batches = [_gpu(_batch(4, 64, 7 + k)) for k in range(2)]
    captured = []
    for _ in range(2):                                   # two fresh modules, two captured steps each
        m = _module(64, seed=3).to(DEV)
        outs = [{k: _bits(v) for k, v in m.fused_step(b).items()} for b in batches]
        torch.cuda.synchronize(DEV)
        captured.append((outs, _state(m)))
    assert captured[0][1] == captured[1][1], "two fresh steps from the same start differ"
    for a, b in zip(captured[0][0], captured[1][0]):
        assert a == b, "two fresh steps return different results"
    # the same pass launched eagerly, with the Adam descriptors lent to the packs as the capture lends them
    m = _module(64, seed=3).to(DEV)
    packs = hipops.packs_for(m.surrogate, 64, 4)
    desc = packs.adam_descriptors(m.lr, (0.9, 0.999), 1e-8)
    eager = []
    for b in batches:
        packs.lend_adam(desc)
        try:
            out = m._latent_training_step(b)
        finally:
            packs.disable_adam()
        assert out is not None
        eager.append({k: _bits(v) for k, v in out.items()})
    torch.cuda.synchronize(DEV)
    for k, (a, b) in enumerate(zip(captured[0][0], eager)):
        assert sorted(a) == sorted(b)
        for key in a:
            assert a[key] == b[key], f"step {k}: {key} of the replay differs from the eager launches"
    assert _state(m) == captured[0][1], "parameters or Adam state of the replay differ from the eager launches"


def test_clip_inside_the_captured_latent_step():
    batch = _gpu(_batch(4, 64, 11))
    plain, huge, clipped = (_module(64, seed=2).to(DEV) for _ in range(3))
    plain.fused_step(batch)
    huge.fused_step(batch, clip=1e30)
    clipped.fused_step(batch, clip=0.5)
    torch.cuda.synchronize(DEV)
    step = _last_step(huge)
    free = float(step.grad_norm[0])
    assert step.clip == 1e30 and step.adam_in_flush and np.isfinite(free) and free > 0
    assert abs(_grad_norm(huge) - free) <= 1e-6 * free
    assert _state(huge) == _state(plain), "a bound nothing reaches must leave the unclipped step"
    step = _last_step(clipped)
    assert step.clip == 0.5 and step.adam_in_flush and step.grad_norm is clipped.surrogate._fused_packs.grad_norm
    n, g = float(step.grad_norm[0]), _grad_norm(clipped)
    assert n == free, "the norm before clipping is the unclipped step's"
    if n > 0.5:
        assert g <= 0.5 * (1 + 1e-6), (n, g)
        assert _state(clipped) != _state(plain)
    else:
        assert abs(g - n) <= 1e-6 * n, (n, g)


def test_refitted_delta_statistics_recapture_the_step():
    m = _module(64, seed=1).to(DEV)
    batch = _gpu(_batch(4, 64, 13))
    m.fused_step(batch)
    step = _last_step(m)
    assert step.valid() and m.graphed_step_for(batch[0].shape, batch[1].shape) is step
    norm = m.undscaling.transform
    norm.reset()
    norm.update(torch.linspace(-0.6, 0.9, 64).reshape(64, 1, 1))
    assert not step.valid()
    out = m.fused_step(batch)
    torch.cuda.synchronize(DEV)
    again = _last_step(m)
    assert again is not step and again.valid() and again.used_latent and again.adam_in_flush
    assert m.surrogate._fused_packs.adam_step_count() == 2, "the re-captured step continues the same Adam state"
    # the re-captured launches carry the new constants: the reported true deltas are the new scaling of the states' differences
    want = m.undscaling(torch.diff(batch[0], dim=1) / m.delta)
    assert torch.equal(out["deltas"], want) or torch.allclose(out["deltas"], want, rtol=1e-6, atol=1e-6)
