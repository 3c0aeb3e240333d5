"""The delay-embedding surrogate (KSDelayCNNSurrogateFactory) on an MI355X: the whole rollout on csrc/delay.hip
(delay_hip.fused_delay_rollout: dly_forward, and dly_backward under autograd), any other delay layout and fp64 input on
plain PyTorch-ROCm kernels with one notice.

Each fused case is compared with the same module on the CPU in fp64, with the bars of tests/test_latent_surrogate_gpu.py:
forward values rtol 2e-4 / atol 2e-5 of the tensor's scale, every gradient within GRAD_TOL of its own scale
(``check_grads``).  The loss is a fixed random weighted sum over every tensor the rollout returns -- outputs, deltas,
inlatents, outlatents and both context tensors -- so its gradient reaches every input."""
import copy
import logging

import numpy as np
import pytest
import torch

import _delay_models as dm
import _grad_contract_models as gm
from conftest import check_grads

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FWD = dict(rtol=2e-4, atol_scale=2e-5)


def _tensors(ro):
    return {"outputs": ro.outputs, "deltas": ro.deltas, "inlatents": ro.inlatents, "outlatents": ro.outlatents,
            "context_s": ro.hidden[0], "context_a": ro.hidden[1]}


def _pair(scaled, seed=0, **kw):
    sur, module = dm.build(scaled=scaled, seed=seed, perturb=True, **kw)
    ref = copy.deepcopy(module).double()
    return ref, module.to(DEV)


_CACHE = {}


def _cached_pair(scaled):
    if scaled not in _CACHE:
        _CACHE[scaled] = _pair(scaled)
    return _CACHE[scaled]


def _inputs(B, S, A, seed, amp=1.0):
    g = torch.Generator().manual_seed(seed)
    st = (torch.rand(B, S, 1, 64, generator=g, dtype=torch.float64) * 2 - 1) * amp
    ac = torch.rand(B, A, 1, 4, generator=g, dtype=torch.float64) * 2 - 1
    return st, ac


class _Counting:
    """A stand-in for the loaded library that counts dly_forward / dly_backward calls."""

    def __init__(self, lib):
        self.lib, self.calls = lib, {"dly_forward": 0, "dly_backward": 0}

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
    from pdecontrol.surrogates import delay_hip
    c = _Counting(delay_hip.load())
    monkeypatch.setattr(delay_hip, "load", lambda: c)
    return c.calls


def _clear(*modules):
    for m in modules:
        for p in m.parameters():
            p.grad = None


def _hidden(B, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.5 * torch.randn(B, 3, 8, 8, generator=g, dtype=torch.float64),
            0.5 * torch.randn(B, 3, 4, 8, generator=g, dtype=torch.float64))


# (B, given, steps, hidden carried, Normalize dscaling, grid)
ROLLOUT_CASES = [
    (1, 1, 1, False, False, "every"), (7, 3, 3, True, True, "every"), (64, 5, 10, False, True, "every"),
    (300, 1, 20, True, False, "every"), (1, 5, 10, True, False, "every"), (7, 1, 20, False, True, "every"),
    (64, 1, 1, True, True, "every"), (300, 3, 3, False, False, "every"), (7, 5, 10, True, True, "skip"),
    (5, 6, 4, False, True, "every"), (7, 1, 2, True, False, "every"),
]


@pytest.mark.parametrize("B,S,K,with_hidden,scaled,kind", ROLLOUT_CASES,
                         ids=[f"B{c[0]}-S{c[1]}-K{c[2]}-{'hidden' if c[3] else 'zero'}-{'affine' if c[4] else 'identity'}-{c[5]}"
                              for c in ROLLOUT_CASES])
def test_delay_rollout_forward_and_gradients(B, S, K, with_hidden, scaled, kind, counting, caplog):
    ref, gpu = _cached_pair(scaled)
    sur_ref, sur_gpu = ref.surrogate, gpu.surrogate
    _clear(sur_ref, sur_gpu)
    times, targets = gm.grid(K, kind, sur_ref.delta)
    seed = S * 100 + K * 10 + B
    st, ac = _inputs(B, S, len(times), seed)
    hidden_ref = hidden_gpu = None
    if with_hidden:
        h = _hidden(B, seed + 7)
        hidden_ref = tuple(t.clone().requires_grad_(True) for t in h)
        hidden_gpu = tuple(t.to(DEV, torch.float32).requires_grad_(True) for t in h)
    st_r, ac_r = st.clone().requires_grad_(True), ac.clone().requires_grad_(True)
    st_g, ac_g = st.to(DEV, torch.float32).requires_grad_(True), ac.to(DEV, torch.float32).requires_grad_(True)
    with caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        ro_ref = sur_ref.rollout(st_r, ac_r, times, targets, hidden=hidden_ref)
        ro_gpu = sur_gpu.rollout(st_g, ac_g, times, targets, hidden=hidden_gpu)
    assert counting["dly_forward"] == 1, "the delay model must run on dly_forward"
    assert not [r for r in caplog.records if "plain PyTorch-ROCm" in r.message]
    weights = gm.loss_weights(_tensors(ro_ref), seed)
    gm.weighted_loss(_tensors(ro_ref), weights).backward()
    gm.weighted_loss(_tensors(ro_gpu), weights).backward()
    torch.cuda.synchronize(DEV)
    assert counting["dly_backward"] == 1
    label = f"delay rollout B={B} S={S} K={K} hidden={with_hidden} scaled={scaled} {kind}"
    want = _tensors(ro_ref)
    for name, got in _tensors(ro_gpu).items():
        gm.assert_close(got, want[name], FWD["rtol"], FWD["atol_scale"], msg=f"{label}: {name}")
    grad = lambda t: (torch.zeros_like(t) if t.grad is None else t.grad).detach().cpu().double().numpy()
    got_in = {"input.states": grad(st_g), "input.actions": grad(ac_g)}
    want_in = {"input.states": grad(st_r), "input.actions": grad(ac_r)}
    if with_hidden:
        for j, tag in enumerate(("s", "a")):
            got_in[f"input.context_{tag}"], want_in[f"input.context_{tag}"] = grad(hidden_gpu[j]), grad(hidden_ref[j])
    check_grads(label + " inputs", got_in, want_in.__getitem__)
    check_grads(label + " parameters", gm.trainable_grads(sur_gpu), gm.trainable_grads(sur_ref).__getitem__)
    if with_hidden:
        assert torch.equal(hidden_gpu[0].detach().cpu(), h[0].float()), "the given context is not written"
    _clear(sur_ref, sur_gpu)


@pytest.mark.parametrize("scaled", [False, True], ids=["identity", "normalize"])
def test_training_step_matches_fixture_and_fp64(scaled, counting, caplog):
    g, s8, a8, _ = dm.golden()
    tag = "nz_" if scaled else "id_"
    sur, module = dm.build(scaled=scaled)
    ref = copy.deepcopy(module).double()
    module = module.to(DEV)
    with caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        out = module.training_step((s8.to(DEV), a8.to(DEV)), 0)
    out["loss"].backward()
    torch.cuda.synchronize(DEV)
    assert counting["dly_forward"] == 2 and counting["dly_backward"] == 2, counting
    assert not [r for r in caplog.records if "plain PyTorch-ROCm" in r.message]
    ref_loss = float(g[tag + "loss"])
    assert abs(float(out["loss"].detach()) - ref_loss) / abs(ref_loss) < 1e-5
    np.testing.assert_allclose(out["outputs"].cpu().numpy(), g[tag + "outputs"], rtol=2e-4,
                               atol=2e-5 * max(1.0, float(np.abs(g[tag + "outputs"]).max())))
    grads = {k: p.grad.detach().cpu().double().numpy() for k, p in module.surrogate.named_parameters()}
    full = {k: v for k, v in grads.items() if f"{tag}grad/{k}" in g.files}
    check_grads(f"delay training_step vs fixture scaled={scaled}", full, lambda k: g[f"{tag}grad/{k}"])
    out_ref = ref.training_step((s8.double(), a8.double()), 0)
    out_ref["loss"].backward()
    check_grads(f"delay training_step vs fp64 scaled={scaled}", grads, gm.trainable_grads(ref.surrogate).__getitem__)


def test_two_backward_runs_are_bit_identical():
    ref, gpu = _pair(False, seed=3)
    times, targets = gm.grid(10, "every", 0.25)
    st, ac = _inputs(64, 5, 10, 11)
    st, ac = st.float().to(DEV), ac.float().to(DEV)
    runs = []
    for _ in range(2):
        _clear(gpu.surrogate)
        ro = gpu.surrogate.rollout(st, ac, times, targets)
        (ro.outputs.square().sum() + ro.outlatents.sum()).backward()
        torch.cuda.synchronize(DEV)
        runs.append({k: p.grad.clone() for k, p in gpu.surrogate.named_parameters()})
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_refused_layout_and_fp64_take_torch_with_one_notice(counting, caplog):
    from pdecontrol.surrogates import ops
    times, targets = gm.grid(6, "every", 0.25)
    st, ac = _inputs(4, 2, 6, 5)
    for what, kw, dtype in (("delay=2", dict(delay=2), torch.float32), ("fp64", {}, torch.float64)):
        ops._NOTIFIED.clear()
        sur_cpu, _ = dm.build(seed=2, **kw)
        sur_gpu = copy.deepcopy(sur_cpu).to(DEV, dtype)
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
            for _ in range(2):
                ro = sur_gpu.rollout(st.to(DEV, dtype), ac.to(DEV, dtype), times, targets)
        notices = [r for r in caplog.records if "plain PyTorch-ROCm" in r.message]
        assert len(notices) == 1, (what, [r.message for r in caplog.records])
        ro_ref = sur_cpu.double().rollout(st, ac, times, targets)
        for name, got in _tensors(ro).items():
            gm.assert_close(got, _tensors(ro_ref)[name], FWD["rtol"], FWD["atol_scale"], msg=f"{what}: {name}")
    assert counting["dly_forward"] == 0


def test_plain_path_switch_runs_on_cuda():
    from pdecontrol.surrogates import ops
    times, targets = gm.grid(8, "every", 0.25)
    st, ac = _inputs(4, 3, 8, 9)
    sur_cpu, _ = dm.build(seed=1)
    sur_gpu = copy.deepcopy(sur_cpu).to(DEV)
    with ops.fused(False):
        ro = sur_gpu.rollout(st.float().to(DEV), ac.float().to(DEV), times, targets)
    ro_ref = sur_cpu.double().rollout(st, ac, times, targets)
    for name, got in _tensors(ro).items():
        gm.assert_close(got, _tensors(ro_ref)[name], FWD["rtol"], FWD["atol_scale"], msg=name)


def test_no_grad_keeps_nothing_for_backward(counting, monkeypatch):
    from pdecontrol.surrogates import delay_hip
    _, gpu = _pair(True, seed=6)
    times, targets = gm.grid(6, "every", 0.25)
    st, ac = _inputs(4, 2, 6, 21)
    saved = []
    orig = torch.autograd.function.FunctionCtx.save_for_backward
    monkeypatch.setattr(torch.autograd.function.FunctionCtx, "save_for_backward",
                        lambda self, *t: (saved.append(len(t)), orig(self, *t))[1])
    with torch.no_grad():
        ro = gpu.surrogate.rollout(st.float().to(DEV), ac.float().to(DEV), times, targets)
    assert counting["dly_forward"] == 1 and ro.outputs.grad_fn is None
    assert all(p.grad is None for p in gpu.surrogate.parameters())
    assert delay_hip.load().dly_workspace_floats(4) > 0   # the workspace only exists inside dly_backward's call


def test_frozen_submodule_gets_no_grad(counting):
    ref, gpu = _pair(False, seed=4)
    for m in (ref, gpu):
        m.surrogate.action_encoder.requires_grad_(False)
    st, ac = _inputs(4, 13, 13, 5, amp=0.8)
    out_ref = ref.training_step((st, ac), 0)
    out_ref["loss"].backward()
    out = gpu.training_step((st.float().to(DEV), ac.float().to(DEV)), 0)
    out["loss"].backward()
    torch.cuda.synchronize(DEV)
    assert counting["dly_backward"] == 2
    gm.frozen_without_grad(gpu.surrogate)
    assert all(p.grad is None for p in gpu.surrogate.action_encoder.parameters())
    check_grads("frozen delay action encoder", gm.trainable_grads(gpu.surrogate), gm.trainable_grads(ref.surrogate).__getitem__)


def test_no_grad_rollout_replays_bit_identical_under_graph_capture():
    _, gpu = _pair(False, seed=8)
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
