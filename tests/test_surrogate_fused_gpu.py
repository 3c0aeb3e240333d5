"""Fused HIP surrogate kernels (libsurrogate_hip.so) against the plain torch path on the same GPU,
and the fused TBPTT step against the golden tensors from the reference (loss within 1e-5 rel)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _build(dev, scaled=True, N=64, seed=0):
    from pdecontrol.architectures import KSAutoRegConvolutionalLSTMN
    from pdecontrol.surrogates.training import PDETrainingModule
    from pdegym.common.transforms import BatchTransform, Normalize
    torch.manual_seed(seed)
    und = None
    if scaled:
        norm = Normalize(aggregate=True, batched=True)
        norm.mean, norm.var, norm.count = torch.full((1, 1, 1), 0.01), torch.full((1, 1, 1), 0.5), 100
        und = BatchTransform(norm)
    f = KSAutoRegConvolutionalLSTMN()
    s = f.surrogate(delta=0.25, dscaling=None if und is None else und.Inverse, tau=5, **f.model(N=N))
    m = PDETrainingModule(surrogate=s, loss=torch.nn.MSELoss(reduction="none"), tstep=0.25, delta=0.25,
                          undscaling=und, tau=5, tbtt=10)
    # non-trivial LayerNorm affine parameters and biases so every gradient path is exercised
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in m.surrogate.named_parameters():
            if "norm" in name or name.endswith(".bias"):
                p.add_(0.3 * torch.randn(p.shape, generator=g))
    return m.to(dev)


def _grads(module):
    return {k: p.grad.detach().clone() for k, p in module.surrogate.named_parameters() if p.grad is not None}


def _zero(module):
    for p in module.surrogate.parameters():
        if p.grad is not None:
            p.grad.zero_()


def _close(a, b, rtol=2e-4, atol_scale=2e-5, msg=""):
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol_scale * max(1.0, np.abs(b).max()), err_msg=msg)


@pytest.mark.parametrize("which", ["state_encoder", "action_encoder"])
@pytest.mark.parametrize("N", [64, 128, 256])
def test_fused_encoder_forward_backward(dev, which, N):
    from pdecontrol.surrogates import hipops
    m = _build(dev, N=N)
    enc = getattr(m.surrogate, which).model
    g = torch.Generator().manual_seed(5)
    x = torch.randn(7, 1, N, generator=g).to(dev).requires_grad_(True)
    up = torch.randn(7, enc.block_l2.conv3x3_l1.out_channels, N // 4, generator=g).to(dev)
    z_ref = enc(x)
    z_ref.backward(up)
    ref_g, dx_ref = _grads(m), x.grad.clone()
    _zero(m)
    x.grad = None
    packs = hipops.packs_for(m.surrogate, N, 7)
    pack = packs.state_enc if which == "state_encoder" else packs.action_enc
    z = hipops.encode(x, pack, packs)
    _close(z, z_ref, msg="forward")
    z.backward(up)
    _close(x.grad, dx_ref, msg="dx")
    got = _grads(m)
    for k, v in ref_g.items():
        if k.startswith(which):
            _close(got[k], v, atol_scale=8e-5, msg=k)


@pytest.mark.parametrize("N", [64, 128, 256])
@pytest.mark.parametrize("K,S", [(1, 1), (4, 2), (3, 1), (5, 5)])
def test_fused_chunk_forward_backward(dev, N, K, S):
    """K rollout steps (S teacher forced) -- cell chain, parallel decoders, integration -- vs the same steps composed
    from torch modules, with upstream gradients on every output (h_all, c_all, d_all, out_all)."""
    from pdecontrol.surrogates import hipops
    m = _build(dev, N=N)
    sur = m.surrogate
    hq, B = N // 4, 5
    g = torch.Generator().manual_seed(7)
    mk = lambda *shape: torch.randn(*shape, generator=g).to(dev).requires_grad_(True)
    xlat_t, lstates_t, c0, h0 = mk(K, B, 4, hq), mk(S, B, 16, hq), mk(B, 16, hq), mk(B, 16, hq)
    states_t = torch.randn(S, B, 1, N, generator=g).to(dev)
    ups = [torch.randn(K, B, 16, hq, generator=g).to(dev), torch.randn(K, B, 16, hq, generator=g).to(dev),
           torch.randn(K, B, 1, N, generator=g).to(dev), torch.randn(K, B, 1, N, generator=g).to(dev)]

    def torch_chunk():
        H, C, out = h0, c0, None
        hs, cs, ds, outs = [], [], [], []
        for k in range(K):
            h_in = lstates_t[k] if k < S else H
            base = states_t[k] if k < S else out
            H, C = sur.transition_model.cnnlstmcell(xlat_t[k], h_in, C)
            d = sur.state_decoder.model(H)
            out = base + sur.delta * sur.dscaling(d)
            hs.append(H), cs.append(C), ds.append(d), outs.append(out)
        return torch.stack(hs), torch.stack(cs), torch.stack(ds), torch.stack(outs)

    leaves = (xlat_t, lstates_t, c0)
    outs_ref = torch_chunk()
    torch.autograd.backward(outs_ref, ups)
    ref_g = _grads(m)
    ref_in = [t.grad.clone() for t in leaves]
    _zero(m)
    for t in leaves + (h0,):
        t.grad = None
    packs = hipops.packs_for(sur, N, B)
    outs = hipops.rollout_chunk(xlat_t, lstates_t, states_t, h0, c0, packs)
    for name, a, b in zip(("h_all", "c_all", "d_all", "out_all"), outs, outs_ref):
        _close(a, b, msg=name)
    torch.autograd.backward(outs, ups)
    for name, t, r in zip(("dxlat", "dlstates", "dc0"), leaves, ref_in):
        _close(t.grad, r, msg=name)
    assert h0.grad is None or float(h0.grad.abs().max()) == 0.0  # S >= 1: h0 never enters the arithmetic
    got = _grads(m)
    for k, v in ref_g.items():
        if k.startswith(("transition_model", "state_decoder")):
            # parameter gradients are long fp32 sums (space x time) with cancellation: summation order
            # (MFMA k-order vs MIOpen) moves them by a few 1e-5 of the tensor's scale
            _close(got[k], v, atol_scale=8e-5, msg=k)


def test_fused_training_step_matches_unfused_and_golden(dev, sur_golden):
    from pdecontrol.surrogates import ops
    g = sur_golden
    s, a = torch.from_numpy(g["b8_states"]).to(dev), torch.from_numpy(g["b8_actions"]).to(dev)
    try:
        for scaled, tag in ((False, "b8"), (True, "b8n")):
            from test_surrogate_gpu import _module
            m = _module(dev, scaled)
            ops.enable_fused(True)
            _zero(m)
            res = m.training_step((s, a), 0)
            res["loss"].backward()
            rel = abs(res["loss"].item() - g[f"{tag}_loss"]) / abs(g[f"{tag}_loss"])
            assert rel < 1e-5, rel
            np.testing.assert_allclose(res["outputs"].cpu().numpy(), g[f"{tag}_outputs"], rtol=1e-3, atol=1e-4)
            np.testing.assert_allclose(res["outdeltas"].cpu().numpy(), g[f"{tag}_outdeltas"], rtol=1e-3, atol=1e-4)
            from conftest import check_grads
            check_grads(f"n64 {tag} fused vs golden (fused_gpu suite)",
                        {k: p.grad.detach().cpu().numpy() for k, p in m.surrogate.named_parameters() if p.requires_grad},
                        lambda k: g[f"{tag}_grad/" + k])
    finally:
        ops.reset_fused()


def test_fused_hip_graph_training_matches_unfused(dev):
    from pdecontrol.surrogates import ops
    from pdecontrol.surrogates.bench_tbptt import build_module, synthetic_batch
    from pdecontrol.surrogates.graph_step import GraphedTBPTTStep
    batch = synthetic_batch(B=16, device=dev)
    with ops.fused(False):
        plain = GraphedTBPTTStep(build_module(dev), tuple(batch[0].shape))
        l_plain = [float(plain.step(*batch)["loss"].detach()) for _ in range(4)]
    try:
        ops.enable_fused(True)
        fused = GraphedTBPTTStep(build_module(dev), tuple(batch[0].shape))
        l_fused = [float(fused.step(*batch)["loss"].detach()) for _ in range(4)]
    finally:
        ops.reset_fused()
    np.testing.assert_allclose(l_fused, l_plain, rtol=3e-5)
    assert l_fused[-1] < l_fused[0]


def test_ensemble_parallel_step_equals_member_by_member(dev):
    """Three ensemble members stepped side by side on their own streams == stepped one after the other
    (the reference's order, mbrl.py:408): same graphs, deterministic reductions -> bit-identical."""
    from pdecontrol.surrogates import ops
    from pdecontrol.surrogates.bench_tbptt import build_module, synthetic_batch
    from pdecontrol.surrogates.ensemble_step import EnsembleTBPTTStep
    from pdecontrol.surrogates.graph_step import GraphedTBPTTStep
    batches = []
    for i in range(3):
        s, a = synthetic_batch(B=16, device=dev)
        batches.append((s.roll(i, 0) * (1 - 0.1 * i), a.roll(i, 1)))
    try:
        ops.enable_fused(True)
        seq_losses, seq_params = [], []
        for i in range(3):
            # pipelined=False: the launch structure of an ensemble member (a member runs on a forked stream of the
            # ensemble capture and cannot fork again, so it keeps every chunk's backward in the same launches)
            g = GraphedTBPTTStep(build_module(dev, seed=i), tuple(batches[i][0].shape), pipelined=False)
            g.step(*batches[i])
            seq_losses.append([float(g.step()["loss"].detach()) for _ in range(3)])
            seq_params.append(torch.cat([p.detach().reshape(-1) for p in g.module.surrogate.parameters()]).clone())
        ens = EnsembleTBPTTStep([build_module(dev, seed=i) for i in range(3)], tuple(batches[0][0].shape))
        ens.step(batches)
        ens_losses = [[] for _ in range(3)]
        for _ in range(3):
            res = ens.step()
            torch.cuda.synchronize(dev)
            for i, r in enumerate(res):
                ens_losses[i].append(float(r["loss"].detach()))
        for i, g in enumerate(ens.members):
            flat = torch.cat([p.detach().reshape(-1) for p in g.module.surrogate.parameters()])
            assert torch.equal(flat, seq_params[i]), f"member {i} parameters differ"
        assert ens_losses == seq_losses
        assert len({l[0] for l in ens_losses}) == 3  # members really are different models / batches
    finally:
        ops.reset_fused()


@pytest.mark.parametrize("N", [64, 128, 256])
def test_encoder_saved_activations_backward_matches_recompute(dev, N, monkeypatch):
    """Encoder backward fed with the forward's saved intermediates (one residual block per launch) against the
    whole-encoder kernel that recomputes them: same forward, gradients equal up to summation grouping.  For the 1-2-4-4
    action encoder this is also the one-wave-per-sample VALU blocks (csrc/sur_narrow.h ``nr_*``: the per-block launches
    route it there) against the MFMA gather-GEMM blocks of the whole-encoder kernel, at three widths."""
    from pdecontrol.surrogates import hipops, ops
    g = torch.Generator().manual_seed(3)
    states = (torch.rand(8, 20, 1, N, generator=g) * 2 - 1).to(dev)
    actions = (torch.rand(8, 20, 1, N, generator=g) * 2 - 1).to(dev)
    grads, losses = [], []
    try:
        ops.enable_fused(True)
        for save in (True, False):
            monkeypatch.setattr(hipops, "SAVE_ACTIVATIONS", save)
            m = _build(dev, N=N)
            out = m.training_step((states, actions), 0)
            out["loss"].backward()
            torch.cuda.synchronize()
            grads.append(_grads(m))
            losses.append(float(out["loss"].detach()))
            if save:
                f = hipops.load().sur_chunk_saved_floats(__import__("ctypes").byref(m.surrogate._fused_packs.chunk.c))
                assert f > 0, "saved-activation path not available for this geometry"
    finally:
        ops.reset_fused()
    assert losses[0] == losses[1]
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 20
    for k in grads[0]:
        _close(grads[0][k], grads[1][k], rtol=2e-4, atol_scale=2e-5, msg=k)


@pytest.mark.parametrize("scaled", [True, False])
def test_fused_delta_loss_matches_torch_ops(dev, scaled):
    """sur_tbptt_delta_loss (loss, per-step loss, logged statistics, true deltas, gradient) against the torch-op
    spelling of training.py:100-121 on the same fused rollout."""
    from pdecontrol.surrogates import hipops, ops
    g = torch.Generator().manual_seed(11)
    states = (torch.rand(16, 20, 1, 64, generator=g) * 2 - 1).to(dev)
    actions = (torch.rand(16, 20, 1, 64, generator=g) * 2 - 1).to(dev)
    res = {}
    try:
        ops.enable_fused(True)
        for mode in ("fused_loss", "torch_loss"):
            m = _build(dev, scaled=scaled)
            if mode == "torch_loss":
                m._fused_delta_loss = lambda rollouts, states: None
            out = m.training_step((states, actions), 0)
            out["loss"].backward()
            torch.cuda.synchronize()
            res[mode] = (out, dict(m.logged), _grads(m))
    finally:
        ops.reset_fused()
    (of, lf, gf), (ot, lt, gt) = res["fused_loss"], res["torch_loss"]
    assert of["loss"].shape == ot["loss"].shape == ()
    np.testing.assert_allclose(float(of["loss"].detach()), float(ot["loss"].detach()), rtol=2e-6)
    np.testing.assert_allclose(of["hsteploss"].cpu().numpy(), ot["hsteploss"].cpu().numpy(), rtol=2e-6)
    assert torch.equal(of["deltas"], ot["deltas"])          # same fp32 expression, element by element
    assert torch.equal(of["outdeltas"], ot["outdeltas"]) and torch.equal(of["outputs"], ot["outputs"])
    for name in ("Train Loss", "Train Mean Delta Output", "Train Std. Delta Output", "Train Mean Delta", "Train Std. Delta"):
        np.testing.assert_allclose(float(lf[name]), float(lt[name]), rtol=1e-5, atol=1e-7, err_msg=name)
    for k in gt:
        _close(gf[k], gt[k], rtol=1e-5, atol_scale=1e-6, msg=k)


def test_graphed_step_leaves_eager_backward_untouched(dev):
    """The Adam update lives only in the captured launches: an eager backward through the same surrogate afterwards
    accumulates plain gradients and does not move the parameters."""
    from pdecontrol.surrogates import ops
    from pdecontrol.surrogates.bench_tbptt import build_module, synthetic_batch
    from pdecontrol.surrogates.graph_step import GraphedTBPTTStep
    batch = synthetic_batch(B=8, device=dev)
    try:
        ops.enable_fused(True)
        m = build_module(dev)
        g = GraphedTBPTTStep(m, tuple(batch[0].shape))
        assert g.adam_in_flush
        g.step(*batch)
        torch.cuda.synchronize(dev)
        before = torch.cat([p.detach().reshape(-1) for p in m.surrogate.parameters()]).clone()
        for p in m.surrogate.parameters():
            if p.grad is not None:
                p.grad.zero_()
        m.training_step(batch, 0)["loss"].backward()
        torch.cuda.synchronize(dev)
        after = torch.cat([p.detach().reshape(-1) for p in m.surrogate.parameters()])
        assert torch.equal(before, after), "eager backward must not apply an optimizer step"
        assert any(float(p.grad.abs().max()) > 0 for p in m.surrogate.parameters() if p.grad is not None)
        g.step()                                   # and the graph still steps
        torch.cuda.synchronize(dev)
        stepped = torch.cat([p.detach().reshape(-1) for p in m.surrogate.parameters()])
        assert not torch.equal(stepped, after)
    finally:
        ops.reset_fused()


def test_adam_inside_the_flush_launch_matches_torch_adam(dev):
    """Three graph-replayed optimizer steps (Adam applied by the gradient-reduction launch) against three eager steps
    with torch.optim.Adam on the same fused kernels.  The two schedules sum the per-workgroup gradient rows in different
    orders (pipelined chunks + folded rows vs one launch set), so a gradient element differs by up to GRAD_TOL = 2e-4 of
    its tensor's scale (conftest.check_grads); Adam's update lr * m / (sqrt(v) + eps) is homogeneous of degree 0 in the
    gradients, so that relative noise passes straight into the update: <= lr * GRAD_TOL per step, 3 steps."""
    from pdecontrol.surrogates import ops
    from pdecontrol.surrogates.bench_tbptt import build_module, synthetic_batch
    from pdecontrol.surrogates.graph_step import GraphedTBPTTStep
    batch = synthetic_batch(B=8, device=dev)
    try:
        ops.enable_fused(True)
        ref = build_module(dev)
        opt = torch.optim.Adam(ref.surrogate.parameters(), lr=ref.lr)
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            ref.training_step(batch, 0)["loss"].backward()
            opt.step()
        m = build_module(dev)
        g = GraphedTBPTTStep(m, tuple(batch[0].shape))
        assert g.adam_in_flush
        g.step(*batch)
        g.step()
        g.step()
        torch.cuda.synchronize(dev)
        for (name, p), q in zip(m.surrogate.named_parameters(), ref.surrogate.parameters()):
            np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().cpu().numpy(), rtol=2e-5, atol=3 * ref.lr * 2e-4,
                                       err_msg=name)
    finally:
        ops.reset_fused()


@pytest.mark.parametrize("T", [12, 25, 45])
def test_fused_tbptt_other_chunkings(dev, T):
    """Sequence lengths other than the benchmark's: T = 12 -> chunks of 10 + 2, T = 25 -> 10 + 10 + 5 (all chunks in
    the same backward launches), T = 45 -> five chunks (more than sur_chunks_backward takes: one launch set per chunk
    on side streams).  Fused step against the plain torch path on the same GPU."""
    from pdecontrol.surrogates import ops
    g = torch.Generator().manual_seed(T)
    states = (torch.rand(6, T, 1, 64, generator=g) * 2 - 1).to(dev)
    actions = (torch.rand(6, T, 1, 64, generator=g) * 2 - 1).to(dev)
    res = {}
    try:
        for fused in (False, True):
            ops.enable_fused(fused)
            m = _build(dev)
            out = m.training_step((states, actions), 0)
            out["loss"].backward()
            torch.cuda.synchronize(dev)
            res[fused] = (out, _grads(m))
    finally:
        ops.reset_fused()
    (ot, gt), (of, gf) = res[False], res[True]
    np.testing.assert_allclose(float(of["loss"].detach()), float(ot["loss"].detach()), rtol=1e-5)
    _close(of["outputs"], ot["outputs"], rtol=1e-3, atol_scale=1e-4, msg="outputs")
    _close(of["hsteploss"], ot["hsteploss"], rtol=1e-4, atol_scale=1e-6, msg="hsteploss")
    assert gf.keys() == gt.keys()
    from conftest import check_grads
    check_grads(f"fused vs plain torch kernels, same device (T={T})",
                {k: v.detach().cpu().numpy() for k, v in gf.items()}, lambda k: gt[k].detach().cpu().numpy(),
                tol=2e-3)   # B = 6 random sequences, both sides fp32 on the GPU: observed <= 3.5e-4 (decoder bias behind a LayerNorm)


@pytest.mark.parametrize("N", [64, 256])
def test_accumulators_in_partial_rows_give_the_same_gradients(dev, N, monkeypatch):
    """The backward kernels keep their gradient accumulators in LDS when they fit (LDS-typed pointers: the GL = true
    instantiations of dec_bwd / cell_wgrad / enc_block_bwd) and accumulate straight into the workgroup's partial row otherwise
    (GL = false).  Every supported geometry fits, so SUR_ACCUMULATE_IN_ROWS=1 forces the second form: the sums are taken in the
    same order, the gradients must be IDENTICAL."""
    from pdecontrol.surrogates import ops
    g = torch.Generator().manual_seed(11)
    states = (torch.rand(8, 20, 1, N, generator=g) * 2 - 1).to(dev)
    actions = (torch.rand(8, 20, 1, N, generator=g) * 2 - 1).to(dev)
    grads, losses = [], []
    try:
        ops.enable_fused(True)
        for force in ("0", "1"):
            monkeypatch.setenv("SUR_ACCUMULATE_IN_ROWS", force)
            m = _build(dev, N=N)
            out = m.training_step((states, actions), 0)
            out["loss"].backward()
            torch.cuda.synchronize(dev)
            grads.append(_grads(m))
            losses.append(float(out["loss"].detach()))
    finally:
        ops.reset_fused()
    assert losses[0] == losses[1]
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 20
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k


def test_fused_training_step_at_a_third_grid_width(dev):
    """N = 128 (between the two benchmark sizes): the shape-specialised primitives -- narrow action-encoder blocks, parity-
    sorted transposed convolutions, single-channel layers as one tile -- at widths 64 / 32 / 128.  Fused step against the
    plain torch path on the same GPU."""
    from pdecontrol.surrogates import ops
    N = 128
    g = torch.Generator().manual_seed(N)
    states = (torch.rand(5, 20, 1, N, generator=g) * 2 - 1).to(dev)
    actions = (torch.rand(5, 20, 1, N, generator=g) * 2 - 1).to(dev)
    res = {}
    try:
        for fused in (False, True):
            ops.enable_fused(fused)
            m = _build(dev, N=N)
            if fused:
                assert ops.use_fused_for(m.surrogate, states), "the fused path must take this geometry"
            out = m.training_step((states, actions), 0)
            out["loss"].backward()
            torch.cuda.synchronize(dev)
            res[fused] = (out, _grads(m))
    finally:
        ops.reset_fused()
    (ot, gt), (of, gf) = res[False], res[True]
    np.testing.assert_allclose(float(of["loss"].detach()), float(ot["loss"].detach()), rtol=1e-5)
    _close(of["outputs"], ot["outputs"], rtol=1e-3, atol_scale=1e-4, msg="outputs")
    assert gf.keys() == gt.keys()
    from conftest import check_grads
    check_grads(f"fused vs plain torch kernels, same device (N={N})",
                {k: v.detach().cpu().numpy() for k, v in gf.items()}, lambda k: gt[k].detach().cpu().numpy(), tol=2e-3)


@pytest.mark.parametrize("N", [96, 192, 512])
def test_grid_widths_the_fused_layernorm_cannot_reduce_are_refused(dev, N, caplog):
    """The fused LayerNorm reduces rows of 16, 32 or k * 64 <= 256 values: N = 96 / 192 give rows of 24 / 48 / 96, N = 512 rows of
    512.  (Before the check N = 96 normalised 64 of 96 values: loss off by 5e-4, silently.)  The library refuses the geometry
    -- every launch returns -4 -- and the module runs such a surrogate on the torch kernels with ONE logged notice, like an
    architecture the kernels do not cover: same loss as with the fused path switched off."""
    import ctypes
    import logging
    from pdecontrol.surrogates import hipops, ops
    g = torch.Generator().manual_seed(N)
    states = (torch.rand(3, 12, 1, N, generator=g) * 2 - 1).to(dev)
    actions = (torch.rand(3, 12, 1, N, generator=g) * 2 - 1).to(dev)
    losses = {}
    try:
        for fused in (False, True):
            ops.enable_fused(fused)
            m = _build(dev, N=N)
            if fused:
                with caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
                    assert not ops.use_fused_for(m.surrogate, states)
                    assert not ops.use_fused_for(m.surrogate, states)
                reason = hipops.geometry_unsupported(m.surrogate, N)
                assert reason and "LayerNorm" in reason
                assert sum("grid width" in r.getMessage() for r in caplog.records) <= 1   # once per reason (module-level memory)
                packs = hipops.FusedPacks(m.surrogate, N, 3)       # a caller that goes to the C ABI anyway is turned away there
                x = torch.zeros(3, 1, N, device=dev)
                z = torch.zeros(3, packs.state_enc.c.c[3], N // 4, device=dev)
                rc = hipops.load().sur_encoder_forward(None, ctypes.byref(packs.state_enc.c), x.data_ptr(), 3, z.data_ptr(), None)
                msg = hipops.load().sur_last_error()
                assert rc == -4 and (b"LayerNorm" in msg or (N == 512 and b"LDS" in msg)), msg   # 512: the encoder's rows fit, its LDS does not
            out = m.training_step((states, actions), 0)
            out["loss"].backward()
            torch.cuda.synchronize(dev)
            losses[fused] = float(out["loss"].detach())
    finally:
        ops.reset_fused()
    assert losses[True] == losses[False]


def test_pack_adam_matches_torch_adam_and_lightning_closure_order(dev):
    """configure_optimizers() on a GPU hands out PackAdam (one launch over the packs' flat moments).  Five eager steps in
    pytorch-lightning's order (training_step -> zero_grad(set_to_none) -> backward -> step) against torch.optim.Adam on
    the same kernels; a StepLR-style learning-rate change in between must reach the device scalar."""
    from pdecontrol.surrogates import hipops
    from pdecontrol.surrogates.bench_tbptt import build_module, synthetic_batch
    batch = synthetic_batch(B=8, device=dev)
    ref, m = build_module(dev), build_module(dev)
    opt_ref = torch.optim.Adam(ref.surrogate.parameters(), lr=ref.lr)
    opt = m.configure_optimizers()[0][0]
    assert isinstance(opt, hipops.PackAdam)
    for k in range(5):
        if k == 3:
            for o in (opt_ref, opt):
                o.param_groups[0]["lr"] = 2.5e-4
        for mod, o in ((ref, opt_ref), (m, opt)):
            out = mod.training_step(batch, 0)
            o.zero_grad(set_to_none=True)
            out["loss"].backward()
            o.step()
    torch.cuda.synchronize(dev)
    assert m.surrogate._fused_packs.adam_step_count() == 5
    for (name, p), q in zip(m.surrogate.named_parameters(), ref.surrogate.parameters()):
        # atol: Adam's update lr * m / sqrt(v) turns a 1-ulp difference of a near-zero gradient into O(1e-4) of a step
        # (lr = 1e-3, five steps: parameters move by up to 5e-3)
        np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().cpu().numpy(), rtol=2e-5, atol=1e-6, err_msg=name)
    sd = opt.state_dict()
    assert sd["packs"][2]["step"] == 5 and sd["param_groups"][0]["lr"] == 2.5e-4


def test_pack_adam_state_restored_before_the_first_forward(dev):
    """A checkpoint is loaded before the packs exist (Lightning restores optimizer states before the first batch): the
    moments and the step counter must survive and the continued run must equal the uninterrupted one."""
    from pdecontrol.surrogates import hipops
    from pdecontrol.surrogates.bench_tbptt import build_module, synthetic_batch
    batch = synthetic_batch(B=8, device=dev)

    def steps(mod, opt, n):
        for _ in range(n):
            out = mod.training_step(batch, 0)
            opt.zero_grad(set_to_none=True)
            out["loss"].backward()
            opt.step()

    a = build_module(dev)
    opt_a = a.configure_optimizers()[0][0]
    steps(a, opt_a, 3)
    weights = {k: v.detach().clone() for k, v in a.surrogate.state_dict().items()}
    saved = opt_a.state_dict()
    steps(a, opt_a, 2)                                      # the uninterrupted run: 5 steps
    b = build_module(dev, seed=123)
    b.surrogate.load_state_dict(weights)
    opt_b = b.configure_optimizers()[0][0]
    assert isinstance(opt_b, hipops.PackAdam) and getattr(b.surrogate, "_fused_packs", None) is None
    opt_b.load_state_dict(saved)                            # no packs yet
    steps(b, opt_b, 2)
    torch.cuda.synchronize(dev)
    assert b.surrogate._fused_packs.adam_step_count() == 5
    for (name, p), q in zip(b.surrogate.named_parameters(), a.surrogate.parameters()):
        np.testing.assert_array_equal(p.detach().cpu().numpy(), q.detach().cpu().numpy(), err_msg=name)


def test_fully_connected_lstm_factory_trains_on_cuda_under_the_defaults(dev, caplog):
    """The reference also ships KSAutoRegFullyConnectedLSTM (architectures/autoreg.py) and trains it on the GPU as it is.
    The fused kernels do not implement it: under the DEFAULT settings it must run (plain PyTorch-ROCm kernels, one logged
    notice) -- rollout, training_step, backward, optimizer step -- and agree with the CPU."""
    import logging
    from pdecontrol.architectures import KSAutoRegFullyConnectedLSTM
    from pdecontrol.surrogates import hipops, ops
    from pdecontrol.surrogates.training import PDETrainingModule
    assert ops.fused_enabled()

    def build(device):
        torch.manual_seed(0)
        f = KSAutoRegFullyConnectedLSTM()
        sur = f.surrogate(delta=0.25, dscaling=None, tau=5, **f.model())
        return PDETrainingModule(surrogate=sur, loss=torch.nn.MSELoss(reduction="none"), tstep=0.25, delta=0.25, tau=5,
                                 tbtt=10).to(device)

    g = torch.Generator().manual_seed(1)
    # this ablation consumes the raw 4 actuator values, not the forcing field
    s, a = torch.rand(4, 20, 1, 64, generator=g) * 2 - 1, torch.rand(4, 20, 1, 4, generator=g) * 2 - 1
    cpu, gpu = build("cpu"), build(dev)
    assert not hipops.fused_supported(gpu.surrogate)
    with caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        out = gpu.training_step((s.to(dev), a.to(dev)), 0)
    assert any("plain PyTorch-ROCm" in r.message for r in caplog.records)
    opt = gpu.configure_optimizers()[0][0]
    assert not isinstance(opt, hipops.PackAdam)
    opt.zero_grad(set_to_none=True)
    out["loss"].backward()
    opt.step()
    ref = cpu.training_step((s, a), 0)
    np.testing.assert_allclose(float(out["loss"].detach()), float(ref["loss"].detach()), rtol=1e-5)
    times = 0.25 * torch.arange(10)
    r = gpu.surrogate.rollout(states=s[:, :5].to(dev), actions=a[:, :10].to(dev), times=times, targets=times + 0.25)
    assert r.outputs.shape == (4, 10, 1, 64) and torch.isfinite(r.outputs).all()
