"""The fully-connected LSTM baselines without a GPU: layout recognition (fclstm_hip.fused_fc_supported), the opt-in switch
(ops.enable_fused_fc / ops.fused_fc / PDECONTROL_FUSED_FC), the host side of the sur_fc_* C ABI (sizes, refusals), and
this repo's CPU modules against the reference's recorded training steps (tests/golden/fclstm_golden.npz for
KSAutoRegFullyConnectedLSTM, ``lstm_*`` of latent_golden.npz for KSLatentLSTM)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _fclstm_models as fm
from conftest import PKG, ROOT, check_grads

LIB = os.path.join(PKG, "lib", "libsurrogate_hip.so")


def test_layout_recognition_accepts_both_factories_and_nothing_else():
    import _delay_models as dm
    import _latent_models as lm
    import _grad_contract_models as gm
    from pdecontrol.surrogates import fclstm_hip
    for factory in fm.FACTORIES:
        for scaled in (False, True):
            sur, _ = fm.build(factory, scaled=scaled)
            assert fclstm_hip.fused_fc_supported(sur), factory
            assert sum(p.numel() for p in fclstm_hip._kernel_parameters(sur)) == fclstm_hip.NPARAM == 6672
            assert [n for n, p in sur.named_parameters() if not p.requires_grad] == ["transition_model.H0", "transition_model.C0"]
        assert not fclstm_hip.fused_fc_supported(fm.build(factory, ssize=8)[0]), factory
        assert not fclstm_hip.fused_fc_supported(fm.build(factory, activation=torch.nn.LeakyReLU)[0]), factory
    # the answer is kept on the surrogate: a copy and an edited tree are examined again
    import copy
    sur, _ = fm.build()
    assert fclstm_hip.fused_fc_supported(sur) and fclstm_hip.fused_fc_supported(sur)
    twin = copy.deepcopy(sur)
    assert fclstm_hip.fused_fc_supported(twin)
    twin.state_decoder.model[0].activation = torch.nn.Tanh()
    assert not fclstm_hip.fused_fc_supported(twin) and fclstm_hip.fused_fc_supported(sur)
    twin.state_decoder.model[0].activation = torch.nn.SiLU()
    twin.transition_model.lstm = torch.nn.LSTM(4, 16, batch_first=True, bias=False)
    assert not fclstm_hip.fused_fc_supported(twin)
    assert "_fc_layout" not in sur.state_dict() and fclstm_hip.fused_fc_supported(copy.deepcopy(sur).double())
    assert not fclstm_hip.fused_fc_supported(gm.ks_module().surrogate)                       # autoregressive ConvLSTM
    assert not fclstm_hip.fused_fc_supported(lm.build("KSLatentConvolutionalLSTM")[0])       # latent ConvLSTM
    assert not fclstm_hip.fused_fc_supported(dm.build()[0])                                  # delay model


def test_flat_vector_order_is_named_parameters_without_the_frozen_state():
    from pdecontrol.surrogates import fclstm_hip
    sur, _ = fm.build()
    names = [n for n, _ in sur.named_parameters() if not n.endswith((".H0", ".C0"))]
    assert names == ["state_encoder.model.0.linear.weight", "state_encoder.model.0.linear.bias",
                     "state_encoder.model.1.linear.weight", "state_encoder.model.1.linear.bias",
                     "state_decoder.model.0.linear.weight", "state_decoder.model.0.linear.bias",
                     "state_decoder.model.1.linear.weight", "state_decoder.model.1.linear.bias",
                     "transition_model.lstm.weight_ih_l0", "transition_model.lstm.weight_hh_l0",
                     "transition_model.lstm.bias_ih_l0", "transition_model.lstm.bias_hh_l0"]
    params = dict(sur.named_parameters())
    assert all(a is params[n] for a, n in zip(fclstm_hip._kernel_parameters(sur), names))


def test_switch_is_off_by_default_and_the_context_manager_restores_it():
    from pdecontrol.surrogates import ops
    assert "PDECONTROL_FUSED_FC" in os.environ or not ops.fused_fc_enabled()
    before = ops.fused_fc_enabled()
    with ops.fused_fc(True):
        assert ops.fused_fc_enabled()
        with ops.fused_fc(False):
            assert not ops.fused_fc_enabled()
        assert ops.fused_fc_enabled()
    assert ops.fused_fc_enabled() == before
    ops.enable_fused_fc(True)
    assert ops.fused_fc_enabled()
    ops.reset_fused()
    assert ops.fused_fc_enabled() == before
    # a CPU tensor never takes the kernels, switch or not, and nothing is loaded or logged for it
    sur, _ = fm.build()
    with ops.fused_fc(True):
        assert not ops.use_fused_fc_for(sur, torch.zeros(2, 1, 1, 64))


@pytest.mark.parametrize("value,expect", [(None, False), ("1", True), ("0", False)])
def test_environment_variable_is_read_at_import(value, expect):
    env = {k: v for k, v in os.environ.items() if k != "PDECONTROL_FUSED_FC"}
    if value is not None:
        env["PDECONTROL_FUSED_FC"] = value
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {PKG!r}]\n"
            "from pdecontrol.surrogates import ops\n"
            "print(int(ops.fused_fc_enabled()), int(ops.fused_enabled()))")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout.split()
    assert out == [str(int(expect)), "1"]


needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libsurrogate_hip.so not built (run __graft_entry__.build())")


@needs_lib
def test_sizes_are_exact_and_the_library_loads_without_a_gpu():
    from pdecontrol.surrogates import hipops
    lib = hipops.load()
    assert lib.sur_fc_param_count() == 6672
    for b, k in ((1, 1), (64, 10)):
        assert lib.sur_fc_saved_floats(b, k) == 256 * b * k
        assert lib.sur_fc_workspace_floats(b, k) == 304 * b * k
    assert lib.sur_fc_saved_floats(0, 4) == 0 and lib.sur_fc_workspace_floats(4, -1) == 0
    assert lib.sur_fc_supported(64, 32, 16, 32, 4, 0, 0, 6672) == 0
    assert lib.sur_fc_supported(64, 32, 16, 32, 4, 1, 1, 6672) == 0
    for args in ((128, 32, 16, 32, 4, 0, 0, 6672), (64, 32, 8, 32, 4, 0, 0, 6672), (64, 32, 16, 32, 8, 0, 0, 6672),
                 (64, 32, 16, 32, 4, 2, 0, 6672), (64, 32, 16, 32, 4, 0, 5, 6672), (64, 32, 16, 32, 4, 0, 0, 6704)):
        assert lib.sur_fc_supported(*args) == -4, args
        assert b"sur_fc_supported" in lib.sur_last_error()


@needs_lib
def test_abi_rejects_bad_arguments_before_touching_the_device():
    """NULL required pointers, non-positive sizes and unknown codes: a negative status and the entry point's own name in
    sur_last_error(), with no HIP call (this machine may have no GPU)."""
    from pdecontrol.surrogates import hipops
    lib = hipops.load()
    p = ctypes.c_void_p(256)     # never dereferenced: every refusal happens before the launch
    null = None

    def forward(params=p, form=0, act=0, B=2, S=1, K=1, states=p, actions=p, outputs=p, deltas=p, outl=p, h=p, c=p):
        return lib.sur_fc_forward(null, params, form, act, B, S, K, states, actions, null, null, 0.25, 1.0, 0.0, outputs,
                                  deltas, null, outl, h, c, null)

    def backward(params=p, form=0, act=0, B=2, S=1, K=1, states=p, actions=p, saved=p, work=p):
        return lib.sur_fc_backward(null, params, form, act, B, S, K, states, actions, null, saved, 0.25, 1.0, null, null,
                                   null, null, null, null, null, null, null, null, null, work)

    bad_forward = [dict(params=null), dict(states=null), dict(actions=null), dict(outputs=null), dict(outl=null),
                   dict(h=null), dict(c=null), dict(deltas=null), dict(B=0), dict(S=0), dict(K=-1), dict(form=2),
                   dict(act=-1), dict(act=2)]
    for kw in bad_forward:
        assert forward(**kw) == -1, kw
        assert b"sur_fc_forward" in lib.sur_last_error(), kw
    bad_backward = [dict(params=null), dict(states=null), dict(actions=null), dict(saved=null), dict(work=null), dict(B=0),
                    dict(S=-3), dict(K=0), dict(form=-1), dict(act=7)]
    for kw in bad_backward:
        assert backward(**kw) == -1, kw
        assert b"sur_fc_backward" in lib.sur_last_error(), kw


def _fixture_step(factory, scaled):
    g, latent, s8, a8 = fm.golden()
    sur, module = fm.build(factory, scaled=scaled)
    out = module.training_step((s8, a8), 0)
    out["loss"].backward()
    grads = {k: p.grad.double().numpy() for k, p in sur.named_parameters() if p.grad is not None}
    return g, latent, out, grads


@pytest.mark.parametrize("scaled", [False, True], ids=["identity", "normalize"])
def test_cpu_autoregressive_module_reproduces_the_reference_fixture(scaled):
    g, _, out, grads = _fixture_step("KSAutoRegFullyConnectedLSTM", scaled)
    tag = "nz_" if scaled else "id_"
    ref_loss = float(g[tag + "loss"])
    assert abs(float(out["loss"].detach()) - ref_loss) / abs(ref_loss) < 1e-6
    np.testing.assert_allclose(out["hsteploss"].detach().numpy(), g[tag + "hsteploss"], rtol=1e-5)
    np.testing.assert_allclose(out["outputs"].detach().numpy(), g[tag + "outputs"], rtol=2e-4,
                               atol=2e-5 * max(1.0, float(np.abs(g[tag + "outputs"]).max())))
    recorded = {k[len(tag + "grad/"):] for k in g.files if k.startswith(tag + "grad/")}
    assert recorded == set(grads) and len(recorded) == 12
    check_grads(f"FC-LSTM CPU vs fixture scaled={scaled}", grads, lambda k: g[f"{tag}grad/{k}"])


def test_cpu_latent_module_reproduces_the_reference_fixture():
    _, latent, out, grads = _fixture_step("KSLatentLSTM", False)
    ref_loss = float(latent["lstm_loss"])
    assert abs(float(out["loss"].detach()) - ref_loss) / abs(ref_loss) < 1e-6
    np.testing.assert_allclose(out["hsteploss"].detach().numpy(), latent["lstm_hsteploss"], rtol=1e-5)
    recorded = {k[len("lstm_grad/"):] for k in latent.files if k.startswith("lstm_grad/")}
    assert recorded == set(grads) and len(recorded) == 12
    check_grads("latent FC-LSTM CPU vs fixture", grads, lambda k: latent[f"lstm_grad/{k}"])
