"""The Burgers physics-informed loss on an MI355X: forward and adjoint on csrc/burgers.hip (one launch each), and the FNO
surrogate trained through it on the whole-network kernels.

Every comparison is against this repository's CPU module in fp64, which tests/test_phyloss_host.py ties bit for bit to the
reference class.  Tolerances are the project's own: forward rtol 2e-4 with atol 2e-5 of the tensor's maximum
(tests/test_delay_surrogate_gpu.py), gradients within GRAD_TOL of the tensor's scale (``check_grads``).  For orientation,
the reference's fp32 CPU arithmetic against fp64 on such fields: forward 1.4e-7 / 2.5e-7 of scale at 1 / 50 sub-steps,
gradient 0.8e-7 / 1.3e-7.  The observed maxima are appended to phyloss_parity_observed.jsonl next to conftest's gradient
parity log (tools/phyloss_bench.py --parity collects them into profiles/phyloss_parity_observed.json)."""
import copy
import json
import logging
import os

import numpy as np
import pytest
import torch

import _phyloss_models as pm
from conftest import GRAD_LOG, check_grads

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FWD = dict(rtol=2e-4, atol_scale=2e-5)
OBSERVED = os.path.join(os.path.dirname(GRAD_LOG), "phyloss_parity_observed.jsonl")


def _record(**rec):
    print("phyloss parity", json.dumps(rec))
    try:
        os.makedirs(os.path.dirname(OBSERVED), exist_ok=True)
        with open(OBSERVED, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


def _scaled_error(got, ref):
    got, ref = got.detach().cpu().double().numpy(), ref.detach().cpu().double().numpy()
    scale = float(np.abs(ref).max())
    return float(np.abs(got - ref).max()) / scale if scale > 0 else float(np.abs(got).max())


def _assert_forward(got, ref, msg):
    got_n, ref_n = got.detach().cpu().double().numpy(), ref.detach().cpu().double().numpy()
    assert got_n.shape == ref_n.shape, (msg, got_n.shape, ref_n.shape)
    np.testing.assert_allclose(got_n, ref_n, rtol=FWD["rtol"], atol=FWD["atol_scale"] * float(np.abs(ref_n).max()), err_msg=msg)


class _Counting:
    """A stand-in for the loaded library that counts bg_phyloss_forward / bg_phyloss_backward calls and keeps their
    arguments."""

    def __init__(self, lib):
        self.lib, self.calls, self.args = lib, {"bg_phyloss_forward": 0, "bg_phyloss_backward": 0}, {}

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name not in self.calls:
            return fn

        def counted(*a):
            self.calls[name] += 1
            self.args[name] = a
            return fn(*a)
        return counted


@pytest.fixture
def counting(monkeypatch):
    from pdecontrol.surrogates.phyloss import phyloss_hip
    c = _Counting(phyloss_hip.load())
    monkeypatch.setattr(phyloss_hip, "load", lambda: c)
    return c


def _reference(loss, u64, weights):
    """Element-wise loss and d sum(weights * loss) / d input of the CPU module in fp64."""
    u = u64.clone().requires_grad_(True)
    out = loss(u)
    (weights * out).sum().backward()
    return out.detach(), u.grad


# a row count that is not a multiple of the four waves per workgroup is included on purpose: (1, 1), (1, 2), (3, 7)
SHAPES = [(1, 1), (1, 2), (3, 7), (64, 20)]


@pytest.mark.parametrize("S", [1, 2, 50])
@pytest.mark.parametrize("B,T", SHAPES, ids=[f"B{b}-T{t}" for b, t in SHAPES])
@pytest.mark.parametrize("N", [64, 128, 256, 512, 1024])
def test_forward_and_input_gradient_against_cpu_fp64(N, B, T, S, counting, caplog):
    loss = pm.burgers_loss(N, substeps=S)
    u64 = pm.smooth_fields(B, T, N, seed=N + 7 * B + T + S)
    w64 = pm.weights_like(u64, seed=N + S)
    ref, gref = _reference(loss, u64, w64)
    u = u64.float().to(DEV).requires_grad_(True)
    with caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        got = loss(u)
        (w64.float().to(DEV) * got).sum().backward()
    torch.cuda.synchronize(DEV)
    assert counting.calls == {"bg_phyloss_forward": 1, "bg_phyloss_backward": 1}
    assert not [r for r in caplog.records if "plain PyTorch-ROCm" in r.message]
    assert got.shape == u.shape and got.dtype == torch.float32
    _record(case=f"N{N}-B{B}-T{T}-S{S}", forward=_scaled_error(got, ref), gradient=_scaled_error(u.grad, gref),
            forward_atol_scale=FWD["atol_scale"], gradient_tol=2e-4)
    _assert_forward(got, ref, "element-wise loss")
    check_grads(f"physics loss input gradient (N={N}, B={B}, T={T}, substeps={S})", {"augmented": u.grad.cpu().numpy()},
                {"augmented": gref.numpy()}.__getitem__)


@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
def test_non_contiguous_input_and_reductions(reduction, counting):
    N, B, T, S = 256, 5, 6, 3
    loss = pm.burgers_loss(N, substeps=S, reduction=reduction)
    base64 = pm.smooth_fields(T, B, N, seed=3)                       # [T, B, 1, N]; the input is its transpose
    u64 = base64.transpose(0, 1)
    w64 = pm.weights_like(loss(u64), seed=4)
    ref, gref = _reference(loss, u64, w64)
    base = base64.float().to(DEV).requires_grad_(True)
    u = base.transpose(0, 1)
    assert not u.is_contiguous()
    got = loss(u)
    (w64.float().to(DEV) * got).sum().backward()
    torch.cuda.synchronize(DEV)
    assert counting.calls == {"bg_phyloss_forward": 1, "bg_phyloss_backward": 1}
    assert got.shape == ref.shape
    _record(case=f"noncontiguous-{reduction}", forward=_scaled_error(got, ref),
            gradient=_scaled_error(base.grad.transpose(0, 1), gref), forward_atol_scale=FWD["atol_scale"], gradient_tol=2e-4)
    _assert_forward(got, ref, f"loss, reduction={reduction}")
    check_grads(f"physics loss, non-contiguous input, reduction={reduction}",
                {"augmented": base.grad.transpose(0, 1).cpu().numpy()}, {"augmented": gref.numpy()}.__getitem__)


def test_nothing_saved_without_a_gradient_and_backward_is_deterministic(counting):
    loss = pm.burgers_loss(512, substeps=4)
    u = pm.smooth_fields(6, 5, 512, seed=11, dtype=torch.float32).to(DEV)
    with torch.no_grad():
        quiet = loss(u.clone().requires_grad_(True))
    assert quiet.grad_fn is None
    diff, states = counting.args["bg_phyloss_forward"][10:12]
    assert diff is None and states is None, "no_grad: nothing may be written for the adjoint"
    detached = loss(u)
    assert detached.grad_fn is None and counting.args["bg_phyloss_forward"][10] is None
    assert counting.calls == {"bg_phyloss_forward": 2, "bg_phyloss_backward": 0}
    w = pm.weights_like(u.cpu(), seed=12).to(DEV)
    grads = []
    for _ in range(2):
        x = u.clone().requires_grad_(True)
        out = loss(x)
        assert torch.equal(out, quiet)
        (w * out).sum().backward()
        grads.append(x.grad)
    torch.cuda.synchronize(DEV)
    assert counting.args["bg_phyloss_forward"][10] is not None and counting.args["bg_phyloss_forward"][11] is not None
    assert torch.equal(grads[0], grads[1]), "two backward runs must be bit-identical"


def test_what_the_kernels_refuse_runs_the_torch_spelling_with_one_notice(counting, caplog):
    from pdecontrol.surrogates import ops
    cases = (("fp64 input", 128, torch.float64, True, 1), ("N = 96", 96, torch.float32, True, 1),
             ("ops.fused(False)", 128, torch.float32, False, 0))
    for what, N, dtype, fused, n_notices in cases:
        ops._NOTIFIED.clear()
        caplog.clear()
        loss = pm.burgers_loss(N, substeps=2)
        u64 = pm.smooth_fields(3, 4, N, seed=N)
        w64 = pm.weights_like(u64, seed=1)
        ref, gref = _reference(loss, u64, w64)
        u = u64.to(DEV, dtype).requires_grad_(True)
        with caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"), ops.fused(fused):
            for _ in range(2):
                got = loss(u)
            (w64.to(DEV, dtype) * got).sum().backward()
        notices = [r for r in caplog.records if "plain PyTorch-ROCm" in r.message]
        assert len(notices) == n_notices, (what, [r.message for r in caplog.records])
        assert counting.calls == {"bg_phyloss_forward": 0, "bg_phyloss_backward": 0}, what
        _assert_forward(got, ref, what)
        check_grads(f"physics loss torch spelling on the GPU ({what})", {"augmented": u.grad.cpu().numpy()},
                    {"augmented": gref.numpy()}.__getitem__)


def test_loss_of_an_env_trajectory_vanishes_at_cfg_steps_substeps():
    """A property tying the loss to the env: with ``substeps = cfg_steps`` the loss of a zero-action trajectory is at
    rounding level, with ``cfg_steps - 1`` it is one missing sub-step (fp64 on the CPU: 3.8e-15 against 9.4e-7).  The bound
    1e-3 on the ratio sits five orders above rounding and three below a real off-by-one."""
    from pdecontrol.surrogates.phyloss import phyloss
    from pdegym.burgers import make_vec
    env = make_vec(6)
    assert env.N == 512 and env.cfg_steps == 50
    env.reset(seed=5)
    frames = [env.u.clone()]
    for _ in range(5):
        frames.append(env.step_torch(None)[0].clone())
    traj = torch.stack(frames, dim=1).unsqueeze(2)                       # [E, T, 1, N]
    sc = env.scenario
    mean = {}
    for S in (sc["cfg_steps"], sc["cfg_steps"] - 1):
        out = phyloss.BurgersPhyPDELoss(dx=sc["dx"], dt=sc["dt"], nu=sc["nu"], substeps=S)(traj)
        mean[S] = float(out[:, 1:].double().mean())
    print("env consistency", mean)
    assert mean[49] > 0 and mean[50] <= 1e-3 * mean[49], mean


@pytest.mark.parametrize("S", [1, 50])
def test_fno_decoded_mode_with_the_physics_loss_on_the_whole_network_kernels(S, counting, caplog):
    from pdecontrol.surrogates import fno_hip
    N, B, T = 512, 8, 20
    loss = pm.burgers_loss(N, substeps=S, dt=1e-3, nu=0.01)
    gpu = pm.fno_module(loss)
    ref = copy.deepcopy(gpu).double()
    gpu = gpu.to(DEV)
    assert gpu.training_mode == "decoded" and fno_hip.supported(gpu.surrogate.model, N)
    st, ac = pm.smooth_fields(B, T, N, seed=21), pm.smooth_fields(B, T, N, seed=22)
    r = ref.training_step((st, ac), 0)
    r["loss"].backward()
    calls = []
    orig = fno_hip._FNOTBPTTFn.apply
    fno_hip._FNOTBPTTFn.apply = lambda *a: (calls.append(1), orig(*a))[1]
    try:
        with caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
            out = gpu.training_step((st.float().to(DEV), ac.float().to(DEV)), 0)
    finally:
        fno_hip._FNOTBPTTFn.apply = orig
    out["loss"].backward()
    torch.cuda.synchronize(DEV)
    assert len(calls) == 1, "the TBPTT pass must run on the whole-network kernels, as one autograd node"
    assert not [x for x in caplog.records if "plain PyTorch-ROCm" in x.message]
    assert counting.calls == {"bg_phyloss_forward": 1, "bg_phyloss_backward": 1}
    rel = abs(float(out["loss"].detach()) - float(r["loss"].detach())) / abs(float(r["loss"].detach()))
    _record(case=f"fno-decoded-S{S}", loss_rel=rel, loss_tol=1e-5)
    grads = {k: p.grad for k, p in gpu.surrogate.named_parameters()}
    assert all(g is not None and float(g.abs().max()) > 0 for g in grads.values()), "never a silent zero"
    assert rel < 1e-5, rel
    check_grads(f"FNO decoded mode + physics loss vs CPU fp64 (substeps={S})", {k: g.cpu().numpy() for k, g in grads.items()},
                dict((k, p.grad.numpy()) for k, p in ref.surrogate.named_parameters()).__getitem__)


def test_fno_delta_mode_keeps_its_launch_sequence(monkeypatch):
    """Delta mode with MSELoss hands the TBPTT node no gradient on its outputs: the library calls of forward + backward are
    the ones of the node's own launch plan, nothing added for the decoded path."""
    from pdecontrol.surrogates import fno_hip
    N, B, T = 512, 8, 20
    gpu = pm.fno_module(torch.nn.MSELoss(reduction="none"), training_mode="delta").to(DEV)
    names = []
    lib = fno_hip.load()

    class _Log:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name in ("fno_row_width", "fno_last_error"):
                return fn
            return lambda *a: (names.append(name), fn(*a))[1]
    monkeypatch.setattr(fno_hip, "load", lambda: _Log())
    seen = []
    orig = fno_hip._FNOTBPTTFn.backward
    monkeypatch.setattr(fno_hip._FNOTBPTTFn, "backward",
                        staticmethod(lambda ctx, gd, go: (seen.append((gd is not None, go is not None)), orig(ctx, gd, go))[1]))
    st, ac = pm.smooth_fields(B, T, N, seed=23, dtype=torch.float32).to(DEV), pm.smooth_fields(B, T, N, seed=24, dtype=torch.float32).to(DEV)
    out = gpu.training_step((st, ac), 0)
    out["loss"].backward()
    torch.cuda.synchronize(DEV)
    assert seen == [(True, False)]
    # two chunks of 10: chunk 0 = one teacher-forced launch (5 steps) + 5 free-running, chunk 1 = 1 + 9
    assert names == ["fno_forward"] * 16 + ["fno_backward"] * 16 + ["fno_reduce_rows", "fno_spec_wgrad"], names


def test_forward_and_backward_replay_bit_identical_under_graph_capture():
    loss = pm.burgers_loss(512, substeps=5)
    u = pm.smooth_fields(16, 10, 512, seed=31, dtype=torch.float32).to(DEV)
    w = pm.weights_like(u.cpu(), seed=32).to(DEV)

    from pdecontrol.surrogates.graph_step import capture_graph

    def run(x):
        out = loss(x)
        (grad,) = torch.autograd.grad((w * out).sum(), x)
        return out.detach(), grad
    x = u.clone().requires_grad_(True)
    eager = run(x)
    torch.cuda.synchronize(DEV)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        run(x)                                  # warm-up on the capture stream
    torch.cuda.current_stream(DEV).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    # the project's capture helper: synchronises, and keeps Python's cyclic collector off during the capture (it must not
    # free GPU objects of earlier tests while the stream is capturing)
    captured = capture_graph(graph, lambda: run(x), s)
    graph.replay()
    torch.cuda.synchronize(DEV)
    for name, got, want in zip(("loss", "gradient"), captured, eager):
        assert torch.equal(got, want), name
