"""The fully-connected LSTM baselines (KSAutoRegFullyConnectedLSTM, KSLatentLSTM) on an MI355X with the opt-in switch on:
the whole rollout on csrc/sur_fclstm.hip (fclstm_hip.fused_fc_rollout: sur_fc_forward, and sur_fc_backward under
autograd); with the switch off, overridden, or for a layout / input the kernels refuse, plain PyTorch-ROCm kernels with
the notices as before.

Each fused case is compared with the same module on the CPU in fp64, with the bars of tests/test_delay_surrogate_gpu.py:
forward values rtol 2e-4 / atol 2e-5 of the tensor's scale, every gradient within GRAD_TOL of its own scale
(``check_grads``).  The loss is a fixed random weighted sum over every tensor the rollout returns -- outputs, deltas,
outlatents, both hidden tensors and the inlatents when there are any -- so its gradient reaches every input.  Every case
also measures what fp32 PyTorch on the CPU loses against the same fp64 module and appends both figures to
fclstm_parity_observed.jsonl next to the gradient parity log (profiles/fclstm_parity_observed.json is that file of one run)."""
import copy
import json
import logging
import os

import numpy as np
import pytest
import torch

import _fclstm_models as fm
import _grad_contract_models as gm
from conftest import GRAD_LOG, check_grads

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FWD = dict(rtol=2e-4, atol_scale=2e-5)
OBSERVED = os.path.join(os.path.dirname(GRAD_LOG), "fclstm_parity_observed.jsonl")


@pytest.fixture(autouse=True)
def _switch_on():
    """Every test here runs with the FC-LSTM kernels switched on unless it switches them off itself."""
    from pdecontrol.surrogates import ops
    with ops.fused_fc(True):
        yield


def _tensors(ro):
    out = {"outputs": ro.outputs, "deltas": ro.deltas, "outlatents": ro.outlatents, "hidden_h": ro.hidden[0],
           "hidden_c": ro.hidden[1]}
    if ro.inlatents is not None:
        out["inlatents"] = ro.inlatents
    return out


def _pair(factory, scaled, seed=0, **kw):
    """(fp64 CPU copy, fp32 CPU module, the module on the GPU), biases perturbed."""
    _, module = fm.build(factory, scaled=scaled, seed=seed, perturb=True, **kw)
    return copy.deepcopy(module).double(), module, copy.deepcopy(module).to(DEV)


_CACHE = {}


def _cached_pair(factory, scaled):
    if (factory, scaled) not in _CACHE:
        _CACHE[factory, scaled] = _pair(factory, scaled)
    return _CACHE[factory, scaled]


def _inputs(B, S, A, seed, amp=1.0):
    g = torch.Generator().manual_seed(seed)
    st = (torch.rand(B, S, 1, 64, generator=g, dtype=torch.float64) * 2 - 1) * amp
    ac = torch.rand(B, A, 1, 4, generator=g, dtype=torch.float64) * 2 - 1
    return st, ac


def _hidden(B, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.5 * torch.randn(1, B, 16, generator=g, dtype=torch.float64),
            0.5 * torch.randn(1, B, 16, generator=g, dtype=torch.float64))


class _Counting:
    """A stand-in for the loaded library that counts sur_fc_forward / sur_fc_backward calls."""

    def __init__(self, lib):
        self.lib, self.calls = lib, {"sur_fc_forward": 0, "sur_fc_backward": 0}

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name not in self.calls:
            return fn

        def counted(*a):
            self.calls[name] += 1
            return fn(*a)
        return counted


@pytest.fixture
def counting(monkeypatch):
    from pdecontrol.surrogates import fclstm_hip
    c = _Counting(fclstm_hip.load())
    monkeypatch.setattr(fclstm_hip, "load", lambda: c)
    return c.calls


def _clear(*modules):
    for m in modules:
        for p in m.parameters():
            p.grad = None


def _plain_notices(caplog):
    return [r for r in caplog.records if "plain PyTorch-ROCm" in r.message]


def _grad(t):
    return (torch.zeros_like(t) if t.grad is None else t.grad).detach().cpu().double().numpy()


def _scale_err(got, ref):
    """max |got - ref| over the tensor's scale max(1, max |ref|): the figure of the forward bar's absolute floor."""
    got, ref = got.detach().cpu().double().numpy(), ref.detach().cpu().double().numpy()
    return float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max()))


def _grad_err(got, ref):
    """max over tensors of max |g - g_ref| / max |g_ref| (check_grads's figure)."""
    worst = 0.0
    for name, g in got.items():
        scale = float(np.abs(ref[name]).max())
        worst = max(worst, float(np.abs(g - ref[name]).max()) / scale if scale > 0 else float(np.abs(g).max()))
    return worst


def _run(sur, st, ac, times, targets, hidden, weights):
    """One rollout and the backward of the weighted loss; returns the rollout."""
    _clear(sur)
    ro = sur.rollout(st, ac, times, targets, hidden=hidden)
    gm.weighted_loss(_tensors(ro), weights).backward()
    return ro


# (B, given, steps, hidden carried, Normalize dscaling, grid)
ROLLOUT_CASES = [
    (1, 1, 1, False, False, "every"), (7, 3, 3, True, True, "every"), (64, 5, 10, False, True, "every"),
    (300, 1, 20, True, False, "every"), (1, 5, 10, True, False, "every"), (7, 1, 20, False, True, "every"),
    (64, 1, 1, True, True, "every"), (300, 3, 3, False, False, "every"), (7, 5, 10, True, True, "skip"),
    (5, 6, 4, False, True, "every"),
]


@pytest.mark.parametrize("factory", fm.FACTORIES)
@pytest.mark.parametrize("B,S,K,with_hidden,scaled,kind", ROLLOUT_CASES,
                         ids=[f"B{c[0]}-S{c[1]}-K{c[2]}-{'hidden' if c[3] else 'zero'}-{'affine' if c[4] else 'identity'}-{c[5]}"
                              for c in ROLLOUT_CASES])
def test_fc_rollout_forward_and_gradients(factory, B, S, K, with_hidden, scaled, kind, counting, caplog):
    ref, cpu32, gpu = _cached_pair(factory, scaled)
    sur_ref, sur_cpu, sur_gpu = ref.surrogate, cpu32.surrogate, gpu.surrogate
    times, targets = gm.grid(K, kind, sur_ref.delta)
    seed = S * 100 + K * 10 + B
    st, ac = _inputs(B, S, len(times), seed)
    h = _hidden(B, seed + 7) if with_hidden else None

    def leaves(device, dtype):
        mk = lambda t: t.to(device, dtype).clone().requires_grad_(True)
        return mk(st), mk(ac), (None if h is None else tuple(mk(t) for t in h))

    in_ref, in_cpu, in_gpu = leaves("cpu", torch.float64), leaves("cpu", torch.float32), leaves(DEV, torch.float32)
    ro_ref = sur_ref.rollout(in_ref[0], in_ref[1], times, targets, hidden=in_ref[2])
    weights = gm.loss_weights(_tensors(ro_ref), seed)
    _clear(sur_ref)
    gm.weighted_loss(_tensors(ro_ref), weights).backward()
    ro_cpu = _run(sur_cpu, in_cpu[0], in_cpu[1], times, targets, in_cpu[2], weights)     # fp32 PyTorch on the CPU: the yardstick
    assert counting["sur_fc_forward"] == 0
    with caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        ro_gpu = _run(sur_gpu, in_gpu[0], in_gpu[1], times, targets, in_gpu[2], weights)
    torch.cuda.synchronize(DEV)
    assert counting == {"sur_fc_forward": 1, "sur_fc_backward": 1}, counting
    assert not _plain_notices(caplog)

    label = f"{factory} rollout B={B} S={S} K={K} hidden={with_hidden} scaled={scaled} {kind}"
    want = _tensors(ro_ref)
    assert set(_tensors(ro_gpu)) == set(want)

    def input_grads(leaf):
        out = {"input.states": _grad(leaf[0]), "input.actions": _grad(leaf[1])}
        if leaf[2] is not None:
            out["input.h_in"], out["input.c_in"] = _grad(leaf[2][0]), _grad(leaf[2][1])
        return out

    grads = {who: {**input_grads(leaf), **gm.trainable_grads(sur)}
             for who, leaf, sur in (("ref", in_ref, sur_ref), ("cpu", in_cpu, sur_cpu), ("gpu", in_gpu, sur_gpu))}
    rec = {"case": label,
           "forward_err_of_scale": {"kernels": max(_scale_err(t, want[n]) for n, t in _tensors(ro_gpu).items()),
                                    "fp32_cpu": max(_scale_err(t, want[n]) for n, t in _tensors(ro_cpu).items())},
           "gradient_err_of_scale": {"kernels": _grad_err(grads["gpu"], grads["ref"]),
                                     "fp32_cpu": _grad_err(grads["cpu"], grads["ref"])}}
    print("fclstm parity", json.dumps(rec))
    try:
        os.makedirs(os.path.dirname(OBSERVED), exist_ok=True)
        with open(OBSERVED, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass

    for name, got in _tensors(ro_gpu).items():
        gm.assert_close(got, want[name], FWD["rtol"], FWD["atol_scale"], msg=f"{label}: {name}")
    check_grads(label + " inputs", input_grads(in_gpu), input_grads(in_ref).__getitem__)
    check_grads(label + " parameters", gm.trainable_grads(sur_gpu), gm.trainable_grads(sur_ref).__getitem__)
    if with_hidden:
        assert not np.any(_grad(in_gpu[2][0])), "the first step is teacher forced: no path from the incoming H"
        for j in range(2):
            assert torch.equal(in_gpu[2][j].detach().cpu(), h[j].float()), "the given hidden tensors are not written"
    _clear(sur_ref, sur_cpu, sur_gpu)


@pytest.mark.parametrize("factory,tag", [("KSAutoRegFullyConnectedLSTM", "id_"), ("KSAutoRegFullyConnectedLSTM", "nz_"),
                                         ("KSLatentLSTM", "lstm_")])
def test_training_step_matches_fixture_and_fp64(factory, tag, counting, caplog, monkeypatch):
    from pdecontrol.surrogates import fclstm_hip
    g, latent, s8, a8 = fm.golden()
    fixture = latent if tag == "lstm_" else g
    _, module = fm.build(factory, scaled=tag == "nz_")
    ref = copy.deepcopy(module).double()
    module = module.to(DEV)
    rollouts, rollout = [], fclstm_hip.fused_fc_rollout
    monkeypatch.setattr(fclstm_hip, "fused_fc_rollout", lambda *a: (rollouts.append(rollout(*a)), rollouts[-1])[1])
    with caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        out = module.training_step((s8.to(DEV), a8.to(DEV)), 0)
    out["loss"].backward()
    torch.cuda.synchronize(DEV)
    assert counting == {"sur_fc_forward": 2, "sur_fc_backward": 2}, counting
    assert not _plain_notices(caplog)
    assert len(rollouts) == 2
    if factory == "KSAutoRegFullyConnectedLSTM":
        assert all(r.inlatents is None for r in rollouts), "the training module switches the re-encoding off"
        assert module.surrogate.reencode_predictions
    ref_loss = float(fixture[tag + "loss"])
    assert abs(float(out["loss"].detach()) - ref_loss) / abs(ref_loss) < 1e-5
    out_ref = ref.training_step((s8.double(), a8.double()), 0)
    out_ref["loss"].backward()
    want = fixture[tag + "outputs"] if tag + "outputs" in fixture.files else out_ref["outputs"].detach().numpy()
    np.testing.assert_allclose(out["outputs"].detach().cpu().numpy(), want, rtol=2e-4,
                               atol=2e-5 * max(1.0, float(np.abs(want).max())))
    grads = {k: p.grad.detach().cpu().double().numpy() for k, p in module.surrogate.named_parameters() if p.grad is not None}
    assert len(grads) == 12
    check_grads(f"{factory} training_step vs fixture {tag}", grads, lambda k: fixture[f"{tag}grad/{k}"])
    check_grads(f"{factory} training_step vs fp64 {tag}", gm.trainable_grads(module.surrogate),
                gm.trainable_grads(ref.surrogate).__getitem__)


@pytest.mark.parametrize("factory", fm.FACTORIES)
def test_two_backward_runs_are_bit_identical(factory):
    _, _, gpu = _pair(factory, False, seed=3)
    times, targets = gm.grid(10, "every", 0.25)
    st, ac = _inputs(64, 5, 10, 11)
    st, ac = st.float().to(DEV), ac.float().to(DEV)
    runs = []
    for _ in range(2):
        _clear(gpu.surrogate)
        ro = gpu.surrogate.rollout(st, ac, times, targets)
        (ro.outputs.square().sum() + ro.outlatents.sum() + ro.hidden[1].sum()).backward()
        torch.cuda.synchronize(DEV)
        runs.append({k: p.grad.clone() for k, p in gpu.surrogate.named_parameters() if p.requires_grad})
    assert len(runs[0]) == 12
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
        assert runs[0][k].abs().max() > 0, k


def _plain_run(factory, caplog, **build_kw):
    """Two rollouts on the GPU, compared with the fp64 CPU module; returns the notices they logged."""
    from pdecontrol.surrogates import ops
    ops._NOTIFIED.clear()
    dtype = build_kw.pop("dtype", torch.float32)
    times, targets = gm.grid(6, "every", 0.25)
    st, ac = _inputs(4, 2, 6, 5)
    sur_cpu, _ = fm.build(factory, seed=2, **build_kw)
    sur_gpu = copy.deepcopy(sur_cpu).to(DEV, dtype)
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        for _ in range(2):
            ro = sur_gpu.rollout(st.to(DEV, dtype), ac.to(DEV, dtype), times, targets)
    ro_ref = sur_cpu.double().rollout(st, ac, times, targets)
    for name, got in _tensors(ro).items():
        gm.assert_close(got, _tensors(ro_ref)[name], FWD["rtol"], FWD["atol_scale"], msg=f"{factory} {build_kw}: {name}")
    return _plain_notices(caplog)


@pytest.mark.parametrize("factory", fm.FACTORIES)
def test_switch_off_is_the_plain_path_with_the_notice_as_before(factory, counting, caplog):
    from pdecontrol.surrogates import ops
    with ops.fused_fc(False):
        notices = _plain_run(factory, caplog)
    assert len(notices) == 1 and "is not the architecture the fused HIP kernels implement" in notices[0].message
    assert "LSTMTransitionModel" in notices[0].message
    assert counting == {"sur_fc_forward": 0, "sur_fc_backward": 0}


@pytest.mark.parametrize("factory", fm.FACTORIES)
def test_the_plain_path_opt_out_overrides_the_switch(factory, counting, caplog):
    from pdecontrol.surrogates import ops
    assert ops.fused_fc_enabled()
    with ops.fused(False):
        notices = _plain_run(factory, caplog)
    assert not notices                       # the explicit opt-out announces nothing, as before
    assert counting == {"sur_fc_forward": 0, "sur_fc_backward": 0}


@pytest.mark.parametrize("factory", fm.FACTORIES)
@pytest.mark.parametrize("what,kw", [("ssize=8", dict(ssize=8)), ("fp64", dict(dtype=torch.float64))])
def test_refused_layout_and_fp64_take_torch_with_one_notice(factory, what, kw, counting, caplog):
    notices = _plain_run(factory, caplog, **kw)
    assert len(notices) == 1, (what, [r.message for r in caplog.records])
    assert counting == {"sur_fc_forward": 0, "sur_fc_backward": 0}


@pytest.mark.parametrize("factory", fm.FACTORIES)
def test_no_grad_keeps_nothing_for_backward(factory, counting, monkeypatch):
    _, _, gpu = _pair(factory, True, seed=6)
    times, targets = gm.grid(6, "every", 0.25)
    st, ac = _inputs(4, 2, 6, 21)
    saved = []
    orig = torch.autograd.function.FunctionCtx.save_for_backward
    monkeypatch.setattr(torch.autograd.function.FunctionCtx, "save_for_backward",
                        lambda self, *t: (saved.append(len(t)), orig(self, *t))[1])
    with torch.no_grad():
        ro = gpu.surrogate.rollout(st.float().to(DEV), ac.float().to(DEV), times, targets)
    torch.cuda.synchronize(DEV)
    assert counting == {"sur_fc_forward": 1, "sur_fc_backward": 0} and ro.outputs.grad_fn is None
    assert not saved, "save_for_backward must not be called under no_grad"
    assert all(p.grad is None for p in gpu.surrogate.parameters())
    assert torch.isfinite(ro.outputs).all()


@pytest.mark.parametrize("factory", fm.FACTORIES)
def test_frozen_decoder_gets_no_grad(factory, counting):
    ref, _, gpu = _pair(factory, False, seed=4)
    for m in (ref, gpu):
        m.surrogate.state_decoder.requires_grad_(False)
    st, ac = _inputs(4, 13, 13, 5, amp=0.8)
    out_ref = ref.training_step((st, ac), 0)
    out_ref["loss"].backward()
    out = gpu.training_step((st.float().to(DEV), ac.float().to(DEV)), 0)
    out["loss"].backward()
    torch.cuda.synchronize(DEV)
    assert counting == {"sur_fc_forward": 2, "sur_fc_backward": 2}
    gm.frozen_without_grad(gpu.surrogate)
    assert all(p.grad is None for p in gpu.surrogate.state_decoder.parameters())
    assert sum(p.grad is not None for p in gpu.surrogate.parameters()) == 8
    check_grads(f"{factory} frozen decoder", gm.trainable_grads(gpu.surrogate), gm.trainable_grads(ref.surrogate).__getitem__)


@pytest.mark.parametrize("factory", fm.FACTORIES)
def test_no_grad_rollout_replays_bit_identical_under_graph_capture(factory):
    _, _, gpu = _pair(factory, False, seed=8)
    times, targets = gm.grid(10, "every", 0.25)
    st, ac = _inputs(16, 5, 10, 3)
    st, ac = st.float().to(DEV), ac.float().to(DEV)
    with torch.no_grad():
        eager = gpu.surrogate.rollout(st, ac, times, targets)
        torch.cuda.synchronize(DEV)
        s = torch.cuda.Stream(DEV)
        s.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(s):
            gpu.surrogate.rollout(st, ac, times, targets)     # warm-up on the capture stream
        torch.cuda.current_stream(DEV).wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            captured = gpu.surrogate.rollout(st, ac, times, targets)
        graph.replay()
        torch.cuda.synchronize(DEV)
    for name, got in _tensors(captured).items():
        assert torch.equal(got, _tensors(eager)[name]), name


@pytest.mark.parametrize("factory", fm.FACTORIES)
def test_ensemble_step_from_a_carried_hidden_state_matches_the_cpu(factory, counting):
    """What WorldVecEnv.step asks of the ensemble: three members, 100 rows, one step from a carried hidden state."""
    from pdecontrol.surrogates.surrogate import PDEEnsemble
    members_cpu = [fm.build(factory, seed=seed, perturb=True)[1] for seed in range(3)]
    members_gpu = [copy.deepcopy(m).to(DEV) for m in members_cpu]
    st, ac = _inputs(100, 1, 1, 17)
    times, targets = torch.zeros(1), torch.full((1,), 0.25)
    hidden = [_hidden(100, 30 + j) for j in range(3)]
    outs = []
    for members, dev, dtype in ((members_cpu, "cpu", torch.float64), (members_gpu, DEV, torch.float32)):
        ens = PDEEnsemble([m.double() if dtype is torch.float64 else m for m in members], num_elites=3)
        hid = [tuple(t.to(dev, dtype) for t in h) for h in hidden]
        torch.manual_seed(5)
        np.random.seed(5)
        with torch.no_grad():
            outs.append(ens.rollout(st.to(dev, dtype), ac.to(dev, dtype), times, targets, hidden=hid))
    torch.cuda.synchronize(DEV)
    assert counting == {"sur_fc_forward": 3, "sur_fc_backward": 0}
    gm.assert_close(outs[1].outputs, outs[0].outputs, FWD["rtol"], FWD["atol_scale"], msg="elite choice or member outputs")
    for (h_cpu, c_cpu), (h_gpu, c_gpu) in zip(outs[0].hidden, outs[1].hidden):
        assert h_gpu.shape == (1, 100, 16) and c_gpu.shape == (1, 100, 16)
        gm.assert_close(h_gpu, h_cpu, FWD["rtol"], FWD["atol_scale"], msg="carried H")
        gm.assert_close(c_gpu, c_cpu, FWD["rtol"], FWD["atol_scale"], msg="carried C")
