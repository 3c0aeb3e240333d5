"""The delay-embedding surrogate ablation (KSDelayCNNSurrogateFactory) on the CPU: registry, seeded initial weights, rollout
and training_step against the reference's recorded values (tests/golden/delay_golden.npz, written by
tools/gen_delay_golden.py), bit for bit; the re-encoding the free-running delay step reads; the routing predicates; and
the host-side answers of libdelay_hip.so."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _delay_models as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "model-based-pde-control_amd", "lib", "libdelay_hip.so")


@pytest.fixture(scope="module")
def fx():
    return dm.golden()


def _training_step(scaled, fx):
    g, s8, a8, _ = fx
    sur, module = dm.build(scaled=scaled)
    res = module.training_step((s8, a8), 0)
    res["loss"].backward()
    return sur, module, res


def test_delay_factory_is_registered():
    import pdecontrol.architectures as arch
    from pdecontrol.surrogates.surrogate import AutoRegPDESurrogate
    from pdecontrol.surrogates.transition import DelayTransitionModel
    f = getattr(arch, "KSDelayCNNSurrogateFactory")()
    model = f.model(N=256, L=88.0)      # the scenario keywords are ignored, as in the reference
    assert set(model) == {"state_encoder", "state_decoder", "action_encoder", "transition_model"}
    assert isinstance(model["transition_model"], DelayTransitionModel) and model["transition_model"].delay == 3
    assert isinstance(f.surrogate(delta=0.25, **model), AutoRegPDESurrogate)
    for name in ("KSAutoRegConvolutionalLSTM", "KSAutoRegFullyConnectedLSTM", "KSLatentConvolutionalLSTM", "KSLatentLSTM"):
        assert hasattr(arch, name)


def test_seeded_build_matches_reference_state_dict(fx):
    g = fx[0]
    sur, _ = dm.build()
    sd = sur.state_dict()
    assert sorted(sd) == sorted(dm.recorded(g, "sd"))
    for k, v in sd.items():
        dm.stored(g, "sd", k, v.numpy())
    assert sum(p.numel() for p in sur.parameters()) == 39830


@pytest.mark.parametrize("scaled", [False, True], ids=["identity", "normalize"])
def test_training_step_matches_reference_bitwise(scaled, fx):
    g, _, _, shared = fx
    tag = "nz_" if scaled else "id_"
    sur, module, res = _training_step(scaled, fx)
    assert module.training_mode == "delta"
    assert res["loss"].item() == g[tag + "loss"]
    for key in ("hsteploss", "outputs", "outdeltas"):
        np.testing.assert_array_equal(res[key].numpy(), g[tag + key], err_msg=key)
    np.testing.assert_array_equal(res["deltas"].numpy(), shared["b8n_deltas" if scaled else "b8_deltas"])
    names = [k for k, p in sur.named_parameters() if p.grad is not None]
    assert sorted(names) == sorted(dm.recorded(g, tag + "grad"))
    for k, p in sur.named_parameters():
        dm.stored(g, tag + "grad", k, p.grad.numpy())


def test_two_call_rollout_matches_reference_bitwise(fx):
    g, s8, a8, _ = fx
    sur, _ = dm.build()
    times, targets = 0.25 * torch.arange(10), 0.25 * (torch.arange(10) + 1)
    with torch.no_grad():
        r1 = sur.rollout(states=s8[:1, :5], actions=a8[:1, :10], times=times, targets=targets, hidden=None)
        given = tuple(h.clone() for h in r1.hidden)
        r2 = sur.rollout(states=r1.outputs[:, -1, None], actions=a8[:1, 10:], times=times, targets=targets, hidden=r1.hidden)
    for h, h0 in zip(r1.hidden, given):
        assert torch.equal(h, h0), "a context passed in must not be written to"
    for tag, r in (("ro1_", r1), ("ro2_", r2)):
        for name in ("outputs", "deltas", "inlatents", "outlatents"):
            np.testing.assert_array_equal(getattr(r, name).numpy(), g[tag + name], err_msg=tag + name)
        np.testing.assert_array_equal(r.hidden[0].numpy(), g[tag + "S"])
        np.testing.assert_array_equal(r.hidden[1].numpy(), g[tag + "A"])


def test_caller_hidden_is_not_written():
    from pdecontrol.surrogates.transition import DelayTransitionModel
    sur, _ = dm.build()
    tm = sur.transition_model
    g = torch.Generator().manual_seed(3)
    hidden = (torch.randn(2, 3, 8, 8, generator=g), torch.randn(2, 3, 4, 8, generator=g))
    keep = tuple(h.clone() for h in hidden)
    s, a = torch.randn(2, 1, 8, 8, generator=g), torch.randn(2, 1, 4, 8, generator=g)
    for fn in (tm.teacherforcing, tm.transition):
        out, new = fn(states=s, actions=a, hidden=hidden)
        assert all(torch.equal(h, k) for h, k in zip(hidden, keep))
        assert torch.equal(new[0][:, :2], hidden[0][:, 1:]) and torch.equal(new[0][:, 2], s[:, 0])
        assert torch.equal(new[1][:, :2], hidden[1][:, 1:]) and torch.equal(new[1][:, 2], a[:, 0])
    assert DelayTransitionModel.reads_free_running_state
    zero = tm._context(s.double(), None)
    assert zero[0].dtype == torch.float64 and zero[0].device == s.device and not zero[0].any()


def test_free_running_steps_read_the_reencoded_prediction(fx, monkeypatch):
    """tbptt_forward keeps the re-encoding on for the delay model: every free-running step appends the encoding of the
    previous prediction.  With it off (the ConvLSTM rule), inlast would stay the first given state's encoding and the
    loss would differ."""
    from pdecontrol.surrogates.transition import DelayTransitionModel, TransitionModel
    g, s8, a8, _ = fx
    sur, module = dm.build()
    assert not TransitionModel.reads_free_running_state
    seen = []
    orig = DelayTransitionModel.transition

    def spy(self, states, actions, hidden=None, **kw):
        seen.append(states.detach().clone())
        return orig(self, states, actions, hidden=hidden, **kw)

    monkeypatch.setattr(DelayTransitionModel, "transition", spy)
    steps = []
    orig_rollout = type(sur).rollout

    def spy_rollout(self, *a, **k):
        ro = orig_rollout(self, *a, **k)
        steps.append(ro)
        return ro

    monkeypatch.setattr(type(sur), "rollout", spy_rollout)
    with torch.no_grad():
        res = module.training_step((s8, a8), 0)
    assert len(seen) == (10 - 5) + (10 - 1)      # chunk 1 starts from one seed state
    assert res["loss"].item() == g["id_loss"]
    # chunk 0: free-running step k (k >= 5) reads encode(output_{k-1})
    enc = sur.state_encoder
    outs = steps[0].outputs
    for i, k in enumerate(range(5, 10)):
        assert torch.equal(seen[i], enc(outs[:, k - 1:k])), k
    # with the ConvLSTM rule (re-encoding off) the step differs
    monkeypatch.setattr(DelayTransitionModel, "reads_free_running_state", False)
    sur2, module2 = dm.build()
    with torch.no_grad():
        res2 = module2.training_step((s8, a8), 0)
    assert res2["loss"].item() != g["id_loss"]


def test_fused_routing_predicates():
    from pdecontrol.surrogates import delay_hip, hipops, ops
    sur, _ = dm.build()
    assert delay_hip.fused_delay_supported(sur)
    assert not hipops.fused_supported(sur) and not hipops.fused_latent_supported(sur)
    refused, _ = dm.build(delay=2)
    assert not delay_hip.fused_delay_supported(refused)
    assert ops.is_delay(sur) and ops.is_delay(refused)
    assert not ops.use_fused_delay_for(sur, torch.zeros(2)) and not ops.use_fused_for(sur, torch.zeros(2))
    import _grad_contract_models as gm
    autoreg = gm.ks_module(64, False).surrogate
    assert not delay_hip.fused_delay_supported(autoreg) and not ops.is_delay(autoreg)
    sur.state_decoder.model.block_l0.layernorm = None
    assert not delay_hip.fused_delay_supported(sur)


def test_library_exports_every_header_function():
    """load() types every row of the binding's table (a missing export raises); that the table is the header's:
    tests/test_capi_symbols.py.  Then the host-side answers and refusals."""
    from pdecontrol.surrogates import delay_hip
    if not os.path.exists(LIB):
        pytest.skip("libdelay_hip.so not built")
    lib = delay_hip.load()   # loads without a GPU
    assert lib.dly_param_count() == 39830
    assert lib.dly_supported(64, 3, 8, 8, 4, 8, 4, 39830) == 0
    assert lib.dly_supported(64, 2, 8, 8, 4, 8, 4, 39830) < 0 and b"delay" in lib.dly_last_error()
    assert lib.dly_supported(128, 3, 8, 8, 4, 8, 4, 39830) < 0
    assert lib.dly_workspace_floats(64) == 64 * 39830
    null, fake = None, ctypes.c_void_p(16)     # never dereferenced: refused on the host
    assert lib.dly_forward(null, fake, 0, 1, 1, fake, fake, null, null, 0.25, 1.0, 0.0, fake, fake, fake, fake, fake, fake) < 0
    assert b"dly_forward" in lib.dly_last_error()
    assert lib.dly_backward(null, fake, 1, 1, 1, fake, fake, null, null, fake, fake, 0.25, 1.0, null, null, null, null, null,
                            null, null, null, null, null, fake, null) < 0
    assert b"workspace" in lib.dly_last_error()
