"""The surrogate-update phase on the GPU: ``sur_gather_windows`` against its numpy twin bit for bit, and the phase's
kernel tier against a hand-written loop (tests/_surrogate_phase_scenario.py)."""
import itertools

import numpy as np
import pytest
import torch

import _surrogate_phase_scenario as sc

pytestmark = pytest.mark.gpu

PAD = 37                                      # floats of fill pattern before and after each output


def _dev(array, off):
    """``array`` on the device in a buffer of its own, its base ``off`` floats (4 * off bytes) past a 16-byte boundary."""
    if array is None:
        return None
    t = torch.as_tensor(array)
    flat = torch.empty(t.numel() + 4, dtype=t.dtype, device="cuda")
    assert flat.data_ptr() % 16 == 0
    out = flat[off:off + t.numel()].view(t.shape)
    out.copy_(t)
    return out


def _maps_on(c, off):
    """The case's maps with their tables on the device at base offset ``off`` (``WindowGather`` keeps device tables)."""
    fm = lambda m: sc.FieldMap(m.start, m.stride, m.width, _dev(m.coef, off))
    act_in, F, act_out = c.act_maps
    return fm(c.obs_map), (fm(act_in), _dev(F, off), fm(act_out))


def _output(B, L, W, time_major, off):
    """(the flat fill-patterned buffer, its [B, L, W] view, the bool mask of the floats the view covers)."""
    flat = torch.full((2 * PAD + B * L * W + 4,), sc.FILL, dtype=torch.float32, device="cuda")
    base = PAD + (-PAD % 4) + off
    strides = (W, B * W, 1) if time_major else (L * W, W, 1)
    view = flat.as_strided((B, L, W), strides, base)
    mask = np.zeros(flat.numel(), bool)
    mask[base:base + B * L * W] = True
    return flat, view, mask


def run_gather(c, time_major, off, first=None):
    """One launch of the case; asserts the fill pattern around both outputs and returns (states, actions) as numpy."""
    from pdecontrol.surrogates import hipops
    obs_map, act_maps = _maps_on(c, off)
    gather = hipops.WindowGather(_dev(c.obs, off), _dev(c.actions, off), _dev(c.rowmap, 0), c.total, obs_map, act_maps)
    assert gather.refused() is None, gather.refused()
    first = torch.as_tensor(np.concatenate(([-99], c.first if first is None else first)), device="cuda")   # offset 1: base + 8
    sflat, sview, smask = _output(c.B, c.L, obs_map.width, time_major, off)
    aflat, aview, amask = _output(c.B, c.L, act_maps[2].width, time_major, off)
    gather(first, 1, c.B, c.L, sview, aview)
    torch.cuda.synchronize()
    for flat, mask in ((sflat, smask), (aflat, amask)):
        assert np.all(flat.cpu().numpy()[~mask] == np.float32(sc.FILL)), "the fill pattern around an output changed"
    return sview.cpu().numpy(), aview.cpu().numpy()


def same_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (what, float(np.nanmax(np.abs(got - want))))


# the axes of the matrix that are not a size: sensor stride, sensor start, coefficients, row map, layout, base alignment
OTHER = list(itertools.product((1, 2), (0, 1), (False, True), (False, True), (False, True), (0, 1)))
SIZES = list(itertools.product((64, 98, 256), (1, 4, 16), (1, 5, 64), (1, 6, 25)))


@pytest.mark.parametrize("forcing", (True, False), ids=("forcing", "noforcing"))
@pytest.mark.parametrize("N", (64, 98, 256))
def test_gather_matches_the_twin_over_every_size(N, forcing):
    """Every (N, A, B, L) of the matrix with and without forcing, against the twin bit for bit.  The six other axes (64
    combinations) ride along in rotation: the 27 sizes of one N take 27 consecutive combinations, offset per (N, forcing),
    so the six runs of this test walk through all 64 at least twice; their full cross is the next test."""
    k0 = 27 * ((64, 98, 256).index(N) * 2 + int(forcing))
    for i, (_, A, B, L) in enumerate(s for s in SIZES if s[0] == N):
        stride, start, coefs, permuted, time_major, off = OTHER[(k0 + i) % len(OTHER)]
        c = sc.gather_case(1000 + k0 + i, N, A, B, L, forcing, stride, start, coefs, permuted)
        states, actions = run_gather(c, time_major, off)
        want_s, want_a = sc.case_twin(c)
        what = (N, A, B, L, forcing, stride, start, coefs, permuted, time_major, off)
        same_bits(states, want_s, ("states",) + what)
        same_bits(actions, want_a, ("actions",) + what)


@pytest.mark.parametrize("forcing", (True, False), ids=("forcing", "noforcing"))
@pytest.mark.parametrize("N,A,B,L", ((64, 4, 5, 6), (98, 16, 5, 6), (64, 1, 2, 3), (98, 1, 2, 3)))
def test_gather_matches_the_twin_over_every_path(N, A, B, L, forcing):
    """The full cross of sensor stride and start, coefficients, row map, output layout and base alignment at one size
    whose widths are multiples of four (the float4 path is taken exactly where the host decides so) and one where they
    are not."""
    for k, (stride, start, coefs, permuted, time_major, off) in enumerate(OTHER):
        c = sc.gather_case(2000 + k, N, A, B, L, forcing, stride, start, coefs, permuted)
        states, actions = run_gather(c, time_major, off)
        want_s, want_a = sc.case_twin(c)
        what = (N, A, B, L, forcing, stride, start, coefs, permuted, time_major, off)
        same_bits(states, want_s, ("states",) + what)
        same_bits(actions, want_a, ("actions",) + what)


@pytest.mark.parametrize("permuted", (False, True), ids=("packed", "rowmap"))
def test_gather_poisons_rows_outside_the_replay(permuted):
    """Windows that start before the replay, run past its end or lie wholly outside: NaN rows for exactly the steps
    outside [0, total), every other row as the twin has it, the surroundings untouched."""
    c = sc.gather_case(7, 64, 4, 5, 6, True, 1, 0, True, permuted)
    first = np.asarray([-3, c.total - 2, 4, c.total + 50, -(2 ** 40)], np.int64)
    for time_major, off in itertools.product((False, True), (0, 1)):
        states, actions = run_gather(c, time_major, off, first=first)
        want_s, want_a = sc.case_twin(c, first=first)
        assert np.isnan(want_s[0, :3]).all() and not np.isnan(want_s[0, 3:]).any() and not np.isnan(want_s[2]).any()
        assert np.isnan(want_s[1, 2:]).all() and np.isnan(want_s[3]).all() and np.isnan(want_a[4]).all()
        same_bits(states, want_s, ("states", time_major, off))
        same_bits(actions, want_a, ("actions", time_major, off))


@pytest.mark.parametrize("forcing", (True, False), ids=("forcing", "noforcing"))
def test_gather_with_a_sensor_start_that_is_a_multiple_of_four(forcing):
    """Stride 1 and start 4 at N = 64: widths of 60, so the float4 path runs with a non-zero ``obs_start`` / ``act_start``
    wherever the bases are aligned (base offset 0), and the scalar path with the same sensor at base offset 1."""
    others = itertools.product((False, True), (False, True), (False, True), (0, 1))
    for k, (coefs, permuted, time_major, off) in enumerate(others):
        c = sc.gather_case(3000 + k, 64, 4, 5, 6, forcing, 1, 4, coefs, permuted)
        assert c.obs_map.start == 4 and c.obs_map.width == 60 and (not forcing or c.act_maps[2].start == 4)
        states, actions = run_gather(c, time_major, off)
        want_s, want_a = sc.case_twin(c)
        what = (forcing, coefs, permuted, time_major, off)
        same_bits(states, want_s, ("states",) + what)
        same_bits(actions, want_a, ("actions",) + what)


def test_gather_poisons_rows_the_rowmap_sends_outside_the_slabs():
    """Logical rows inside [0, total) whose ``rowmap`` entry is below 0, at ``rows`` or far beyond it: NaN rows for exactly
    those steps, every other row as the twin has it, the surroundings untouched."""
    c = sc.gather_case(8, 64, 4, 5, 6, True, 1, 0, True, True)
    c.rowmap = c.rowmap.copy()
    bad = {int(c.first[0]) + 1: -1, int(c.first[2]): c.rows, int(c.first[4]) + 5: c.rows + 2 ** 33}
    for logical, physical in bad.items():
        c.rowmap[logical] = physical
    want_s, want_a = sc.case_twin(c)
    assert np.isnan(want_s[0, 1]).all() and np.isnan(want_s[2, 0]).all() and np.isnan(want_a[4, 5]).all()
    assert not np.isnan(want_s).all(axis=-1).all()
    for time_major, off in itertools.product((False, True), (0, 1)):
        states, actions = run_gather(c, time_major, off)
        same_bits(states, want_s, ("states", time_major, off))
        same_bits(actions, want_a, ("actions", time_major, off))


# ----------------------------------------------------------------------------------------------------------------------
# sur_val_loss
# ----------------------------------------------------------------------------------------------------------------------
LOSS_RTOL, HSTEP_RTOL = 1e-5, 1e-4            # the sibling kernel's tolerances (tests/test_surrogate_gpu.py)
_SCENES = {}


def scene(N=64):
    """(namespace, env, the controller's transforms, a training module on the GPU) per grid width, built once."""
    if N not in _SCENES:
        import _rollout_scenario as rsc
        M = rsc.repo_namespace()
        env = M.Env() if N == 64 else M.Env(L=88.0, N=N)
        tf = rsc.transforms(M, env)
        _SCENES[N] = (M, env, tf, sc.training_module(M, env, tf, "cuda", N=N))
    return _SCENES[N]


def _rollout_inputs(module, B, T, N, seed):
    """A batch in the scaled range and the fused rollout's time-major predictions for it."""
    rs = np.random.RandomState(seed)
    x = np.linspace(0, 2 * np.pi, N, endpoint=False)
    t = np.arange(T)[None, :, None]
    phase = rs.uniform(0, 6, (B, 1, 1))
    states = (0.3 * np.sin(x[None, None, :] + phase + 0.3 * t) + 0.1 * np.cos(2 * x[None, None, :] - 0.2 * t))
    states = torch.from_numpy(states.astype(np.float32)[:, :, None, :]).cuda()
    actions = torch.from_numpy(rs.uniform(-1, 1, (B, T, 1, N)).astype(np.float32)).cuda()
    with torch.no_grad():
        out = module._full_rollout(states, actions)
    out_all, d_all = out.outputs.transpose(0, 1), out.deltas.transpose(0, 1)
    assert out_all.is_contiguous() and d_all.is_contiguous(), "the fused rollout keeps its time-major storage"
    return states, actions, out, out_all, d_all


@pytest.mark.parametrize("N", (64, 256))
@pytest.mark.parametrize("T", (2, 6, 25))
@pytest.mark.parametrize("B", (1, 3, 64))
def test_val_loss_against_fp64_and_the_torch_ops(B, T, N, monkeypatch):
    from pdecontrol.surrogates import hipops
    M, env, tf, module = scene(N)
    states, actions, out, out_all, d_all = _rollout_inputs(module, B, T, N, seed=B * 100 + T)
    consts = hipops.undscale_constants(module.undscaling)
    inv = module._inverse_scaling(N, states.device)
    assert consts is not None and inv is not None and inv is not False

    def run(accum):
        with torch.no_grad():
            res = module._fused_validation_loss(out, states, accum=accum)
        assert res is not None, "validation_step must route this configuration to sur_val_loss"
        torch.cuda.synchronize()
        return [None if r is None else r.cpu().numpy() for r in res]

    acc = torch.zeros(3 + T, dtype=torch.float64, device="cuda")
    loss, hstep, scalars, deltas, decoded = run(acc)
    want = sc.val_loss_fp64(states.cpu().numpy(), out_all.cpu().numpy(), d_all.cpu().numpy(), module.delta, consts[0], consts[1],
                            inv.cpu().numpy())
    print(f"B={B} T={T} N={N}: loss {loss} / fp64 {want['loss']}, scaled {scalars[0]} / {want['scaled']}, delta {scalars[1]} / "
          f"{want['delta']}, max hstep rel {np.max(np.abs(hstep[1:] - want['hsteploss'][1:]) / want['hsteploss'][1:])}")
    assert abs(loss - want["loss"]) <= LOSS_RTOL * want["loss"]
    assert abs(scalars[0] - want["scaled"]) <= LOSS_RTOL * want["scaled"]
    assert abs(scalars[1] - want["delta"]) <= LOSS_RTOL * want["delta"]
    np.testing.assert_allclose(hstep, want["hsteploss"], rtol=HSTEP_RTOL, atol=0)
    assert hstep[0] == 0.0
    np.testing.assert_allclose(acc.cpu().numpy(), want["sums"], rtol=HSTEP_RTOL, atol=0)
    np.testing.assert_allclose(deltas, want["deltas"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(decoded, want["decoded"], rtol=1e-5, atol=1e-5)
    # `decoded` is the inverse scaling in its four separately rounded fp32 steps: the bits of FieldMap.apply_numpy
    dec_in = np.concatenate((states.cpu().numpy()[:, :1], out_all.cpu().numpy().transpose(1, 0, 2, 3)[:, :-1]), axis=1)
    want_dec = sc.FieldMap(0, 1, N, inv.cpu()).apply_numpy(dec_in)
    assert decoded.shape == want_dec.shape and decoded.tobytes() == want_dec.tobytes(), \
        float(np.max(np.abs(decoded - want_dec)))

    # the torch ops of validation_step on the same device, over the same rollout
    fused_step = module.validation_step((states, actions), 0)
    fused_logged = {k: float(v) for k, v in module.logged.items() if k.startswith("Val.")}
    monkeypatch.setattr(module, "_fused_validation_loss", lambda *a, **k: None)
    with torch.no_grad():
        torch_step = module.validation_step((states, actions), 0)
    torch_logged = {k: float(v) for k, v in module.logged.items() if k.startswith("Val.")}
    monkeypatch.undo()
    print("fused", fused_logged, "torch", torch_logged)
    assert set(fused_step) == set(torch_step)
    for name in ("Val. Loss", "Val. Scaled Loss", "Val. Delta Loss"):
        assert abs(fused_logged[name] - torch_logged[name]) <= LOSS_RTOL * abs(torch_logged[name]), name
    assert abs(float(fused_step["loss"]) - float(torch_step["loss"])) <= LOSS_RTOL * float(torch_step["loss"])
    np.testing.assert_allclose(fused_step["hsteploss"].cpu().numpy(), torch_step["hsteploss"].cpu().numpy(), rtol=HSTEP_RTOL)
    for name in ("outputs", "states", "outdeltas", "deltas", "actions"):
        assert fused_step[name].shape == torch_step[name].shape, name
        np.testing.assert_allclose(fused_step[name].cpu().numpy(), torch_step[name].cpu().numpy(), rtol=1e-5, atol=1e-5, err_msg=name)

    # two runs are bit-identical
    acc2 = torch.zeros_like(acc)
    again = run(acc2)
    for a, b in zip((loss, hstep, scalars, deltas, decoded), again):
        assert a.tobytes() == b.tobytes()
    assert acc.cpu().numpy().tobytes() == acc2.cpu().numpy().tobytes()


@pytest.mark.parametrize("B,T,N", ((3, 6, 64), (64, 25, 256)))
def test_val_loss_accumulates_an_epoch(B, T, N):
    """The accumulator after three batches is the sum of the three batches' own sums, to 1e-12 relative."""
    M, env, tf, module = scene(N)
    total = torch.zeros(3 + T, dtype=torch.float64, device="cuda")
    singles = []
    for k in range(3):
        states, _, out, _, _ = _rollout_inputs(module, B, T, N, seed=50 + k)
        own = torch.zeros_like(total)
        with torch.no_grad():
            assert module._fused_validation_loss(out, states, accum=own, outputs=False) is not None
            assert module._fused_validation_loss(out, states, accum=total, outputs=False) is not None
        singles.append(own.cpu().numpy())
    got, want = total.cpu().numpy(), singles[0] + singles[1] + singles[2]
    assert got[3] == 0.0 and np.all(got[[0, 1, 2, 4]] > 0)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


def test_val_loss_is_not_taken_for_an_unrecognised_inverse():
    """A ``Normalize`` in the observation connector (the offline-evaluation fixture) keeps the torch ops."""
    M, env, tf, _ = scene(64)
    norm = M.T.Normalize(aggregate=True, batched=True)
    norm.mean, norm.var, norm.count = torch.full((1, 1, 1), 0.1), torch.full((1, 1, 1), 2.0), 10
    other = M.T.SampleTransform([M.T.BatchTransform(norm)], [tf.forcing])
    tf2 = type(tf)(**{**vars(tf), "replay_to_world": other})
    module = sc.training_module(M, env, tf2, "cuda")
    states, actions, out, _, _ = _rollout_inputs(module, 3, 6, 64, seed=1)
    assert module._fused_validation_loss(out, states) is None
    with torch.no_grad():
        res = module.validation_step((states, actions), 0)
    assert res["hsteploss"].shape == (6,) and torch.isfinite(res["loss"])


# ----------------------------------------------------------------------------------------------------------------------
# the phase: kernel tier against the hand-written loop
# ----------------------------------------------------------------------------------------------------------------------
def _phase_setup(M, env, tf):
    """(kernel-side datamodule over a device replay, reference-side host datamodule, packed host replay)."""
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    from pdecontrol.surrogates.common.datamodule import PDEDataModule
    episodes = sc.scripted_episodes(env.N)
    host, sink = M.Replay(), DeviceExperienceReplay(device="cuda")
    for part in sc.split_replay(M, episodes):
        host.extend(part)
    for part in sc.split_replay(M, episodes):
        sink.extend(part)
    keys = list(host.episodes)
    assert list(sink.episodes) == keys and len(keys) == 6
    common = dict(train=keys[:4], val=keys[4:], bootstrapping=True, stransf=tf.replay_to_world, tau=5, batch_size=8)
    kernel_dm = PDEDataModule(data=sink.data, curriculum=sc.curriculum(), device_data="cuda", **common)
    ref_dm = PDEDataModule(data=host.data, curriculum=sc.curriculum(), **common)
    return kernel_dm, ref_dm, sc.packed(host), sink


def _same_history(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g["epoch"], g["global_step"]) == (w["epoch"], w["global_step"])
        for name in ("Val. Loss", "Val. Scaled Loss", "Val. Delta Loss"):
            assert abs(g[name] - w[name]) <= LOSS_RTOL * abs(w[name]), (name, g[name], w[name])
        np.testing.assert_allclose(g["hsteploss"], w["hsteploss"], rtol=HSTEP_RTOL)
        assert g["hsteploss"][0] == 0.0


def _robust(history):
    """Every early-stopping decision has a margin of 100 tolerances: consecutive epochs' "Val. Loss" differ by that."""
    values = [h["Val. Loss"] for h in history]
    for a, b in zip(values, values[1:]):
        assert abs(a - b) >= 100 * LOSS_RTOL * max(abs(a), abs(b)), f"scenario unsuitable: epochs at {a} and {b}"


def test_kernel_tier_against_the_hand_written_loop(monkeypatch):
    from pdecontrol.mbrl import surrogate_phase as sp
    from pdecontrol.mbrl.recognition import world_connector
    from pdecontrol.surrogates.common import dataset as ds
    monkeypatch.setenv("PDECONTROL_PIPELINED", "1")
    M, env, tf, _ = scene(64)
    kernel_dm, ref_dm, packed, sink = _phase_setup(M, env, tf)
    maps = world_connector(tf.replay_to_world, env.N, 4)
    kernel, ref = sc.training_module(M, env, tf, "cuda", seed=5), sc.training_module(M, env, tf, "cuda", seed=5)
    monkeypatch.setattr(ref, "_fused_validation_loss", lambda *a, **k: None)     # the reference validates on the torch ops
    args = dict(max_steps=7, min_steps=2, patience=1)

    # spies: no index_select on a slab, no pack of the replay, during the kernel-tier call
    slabs = {t.data_ptr() for t in sink.tensors}
    seen = []
    real_select, real_init = torch.Tensor.index_select, ds.DeviceSubSeqStore.__init__
    def select_spy(self, *a, **k):
        if self.data_ptr() in slabs:
            seen.append("index_select on a slab")
        return real_select(self, *a, **k)
    def init_spy(self, *a, **k):
        seen.append("DeviceSubSeqStore.__init__")
        return real_init(self, *a, **k)

    def both(kernel_fit, ref_fit, **kw):
        np.random.seed(17)
        torch.manual_seed(17)
        with monkeypatch.context() as m:
            m.setattr(torch.Tensor, "index_select", select_spy)
            m.setattr(ds.DeviceSubSeqStore, "__init__", init_spy)
            got = sp.update_surrogate(kernel, kernel_dm, kernel_fit, **kw)
        assert kernel_fit.tier == "kernel", kernel_fit.tier_reason
        assert not seen, seen
        after = (np.random.get_state()[1].tobytes(), np.random.get_state()[2], torch.get_rng_state().numpy().tobytes())
        np.random.seed(17)
        torch.manual_seed(17)
        want = sc.reference_fit(ref, ref_dm, ref_fit, packed, maps, **kw)
        assert after == (np.random.get_state()[1].tobytes(), np.random.get_state()[2], torch.get_rng_state().numpy().tobytes())
        torch.cuda.synchronize()
        print("kernel", [(h["epoch"], h["global_step"], h["Val. Loss"]) for h in kernel_fit.history])
        print("loop  ", [(h["epoch"], h["global_step"], h["Val. Loss"]) for h in ref_fit.history])
        _robust(ref_fit.history)
        assert (kernel_fit.current_epoch, kernel_fit.global_step, kernel_fit.wait_count) == \
               (ref_fit.current_epoch, ref_fit.global_step, ref_fit.wait_count)
        _same_history(kernel_fit.history, ref_fit.history)
        assert abs(got - want) <= LOSS_RTOL * abs(want) and abs(kernel_fit.best_score - ref_fit.best_score) <= LOSS_RTOL * abs(want)
        (kp, ka), (rp, ra) = sc.optimizer_state(kernel), sc.optimizer_state(ref)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(kp, rp)), "parameters differ"
        assert all(a.tobytes() == b.tobytes() for a, b in zip(ka, ra)), "Adam state differs"

    kernel_fit, ref_fit = sp.FitState(), sp.FitState()
    both(kernel_fit, ref_fit, **args)
    first_epochs = kernel_fit.current_epoch
    assert kernel_fit.global_step >= 2 and first_epochs >= 2                    # the curriculum changed T between epochs
    shapes = {k[0][:2] for k in kernel.__dict__["_graphed_steps"]}
    assert any(b < 8 for b, _ in shapes) and len({t for _, t in shapes}) == 2   # ragged last batches, two window lengths

    # the delta statistics are re-fitted between iterations (update_delta_transform): the captured steps are re-captured
    steps_before = dict(kernel.__dict__["_graphed_steps"])
    for m in (kernel, ref):
        norm = m.undscaling.transform
        norm.reset()
        norm.update(torch.linspace(-0.6, 0.9, 64).reshape(64, 1, 1))
    both(kernel_fit, ref_fit, max_steps=3, min_steps=0, patience=1, max_epochs=1)
    assert kernel_fit.current_epoch == first_epochs + 1
    assert any(kernel.__dict__["_graphed_steps"][k] is not v for k, v in steps_before.items()), "nothing was re-captured"


def test_an_unrecognised_connector_runs_on_the_loop_tier(caplog):
    import logging
    from pdecontrol.mbrl import surrogate_phase as sp
    from pdecontrol.surrogates import ops
    from pdecontrol.surrogates.common.datamodule import PDEDataModule
    M, env, tf, _ = scene(64)
    norm = M.T.Normalize(aggregate=True, batched=True)
    norm.mean, norm.var, norm.count = torch.full((1, 1, 1), 0.1), torch.full((1, 1, 1), 2.0), 10
    other = M.T.SampleTransform([M.T.BatchTransform(norm)], [tf.forcing, tf.pdescaling])
    tf2 = type(tf)(**{**vars(tf), "replay_to_world": other})
    module = sc.training_module(M, env, tf2, "cuda", seed=2)
    host = sc.host_replay(M, sc.scripted_episodes(env.N))
    keys = list(host.episodes)
    dm = PDEDataModule(data=host.data, train=keys[:4], val=keys[4:], bootstrapping=True, stransf=other, tau=5, batch_size=16,
                       device_data="cuda")
    fit = sp.FitState()
    ops._NOTIFIED.discard("a Normalize")
    np.random.seed(3)
    with caplog.at_level(logging.INFO, logger="pdecontrol.surrogates"):
        value = sp.update_surrogate(module, dm, fit, max_steps=2, min_steps=0, patience=1)
        value2 = sp.update_surrogate(module, dm, fit, max_steps=1, min_steps=0, patience=1)
    assert sum("loop tier" in r.getMessage() for r in caplog.records) == 1
    assert (fit.tier, fit.tier_reason, fit.global_step) == ("loop", "a Normalize", 3)
    assert isinstance(value, float) and isinstance(value2, float) and np.isfinite(value) and np.isfinite(value2)
    assert [h["Val. Loss"] for h in fit.history] == [value, value2]
