"""The device-resident real replay on an MI355X: ``ks_record_device`` against its numpy twin, the kernel
tier of ``collect`` through a sink against the kernel tier without one, and one controller slice
``collect -> extend -> world.setup -> imagine -> update_policy`` over the slabs against the same slice over host replays.
Every comparison is bit for bit: the record copies and rounds as numpy does, and both routes run the same kernels on the
same data."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _collect_scenario as sc  # noqa: E402
import _policy_phase_scenario as pp_sc  # noqa: E402
import _real_replay_scenario as rr  # noqa: E402
import _rollout_scenario as ro  # noqa: E402
import _sac_models as sm  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DEVICE_REWARD = {"batched_reward_func": lambda env: env.batched_reward_func}


# ----------------------------------------------------------------------------------------------------------------------
# ks_record_device
# ----------------------------------------------------------------------------------------------------------------------
def _shifted(array, shift):
    """``array`` on the device; ``shift``: its base 4 bytes past a 16-byte boundary."""
    flat = torch.from_numpy(np.ascontiguousarray(array)).reshape(-1)
    if not shift or flat.element_size() != 4:
        return flat.to(DEV).view(array.shape)
    room = torch.empty(flat.numel() + 1, dtype=flat.dtype, device=DEV)
    out = room[1:]
    out.copy_(flat)
    assert out.data_ptr() % 16 == 4
    return out.view(array.shape)


@pytest.mark.parametrize("N", [64, 98, 100, 256])
def test_ks_record_device_equals_the_numpy_twin(N):
    """Every row bit for bit and the untouched rows still the fill pattern, over E = 1, 5, 257 (one wave, a partial
    workgroup, several workgroups with a partial last one), A = 1, 4, 16, T = 1, 5, the four ``dst`` forms, one and 250
    sub-steps, with every base 16-byte aligned (float4 where the widths allow it) and with the trajectory and the
    observation and action slabs 4 bytes off (the scalar path)."""
    import kspde
    rs = np.random.RandomState(N)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    for E in (1, 5, 257):
        stepper = kspde.KSStepper(E, N, L=22.0 * N / 64, device=0)
        stepper.set_stream(stream)
        for A in (1, 4, 16):
            for T in (1, 5):
                for n_substeps, shift in ((1, False), (250, True), (250, False), (1, True)):
                    seg = rr.segment(rs, T, E, N, A, n_substeps)
                    for form in rr.DST_FORMS if (n_substeps, shift) != (1, True) else ("permuted",):
                        dst, rows = rr.dst_form(form, rs, T, E)
                        want = rr.filled_slabs(rows, N, A)
                        rr.record_twin(want, seg, n_substeps, dst)
                        got = [_shifted(a, shift and i < 3) for i, a in enumerate(rr.filled_slabs(rows, N, A))]
                        traj, actions = _shifted(seg[0], shift), _shifted(seg[1], False)
                        ssq, steps, d_dst = (torch.from_numpy(a).to(DEV) for a in (seg[2], seg[3], dst))
                        record = kspde.ks_record(*(t.data_ptr() for t in got), rows)
                        stepper.record_device(traj.data_ptr(), actions.data_ptr(), A, ssq.data_ptr(), steps.data_ptr(), T,
                                              n_substeps, d_dst.data_ptr(), dst, record)
                        rr.same_slabs([t.cpu().numpy() for t in got], want, (N, E, A, T, n_substeps, shift, form))
        stepper.close()


# ----------------------------------------------------------------------------------------------------------------------
# the kernel tier through the sink
# ----------------------------------------------------------------------------------------------------------------------
def _run(with_sink, E, N, stride, tmax=1.0, calls=3, capacity=None):
    """Three consecutive sampling phases (``ts >= 3 E``), each committed: per phase (what the phase returned, as a host
    replay; the state record; the plan; the replay's metadata after the commit), and the replay."""
    from pdecontrol.mbrl import collection_phase as cp
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay, StagedRollout
    from pdecontrol.mbrl.replay import ExperienceReplay
    s = sc.build(E=E, N=N, device=0, agent_device="cuda:0", agent_stride=stride, tmax=tmax)
    sc.seed()
    sc.prime(s.worker, 11)
    callback = sc.Callback()
    s.worker.callbacks.append(callback)
    replay = DeviceExperienceReplay(capacity, device=DEV) if with_sink else ExperienceReplay(capacity)
    stop, out = (lambda ts, ep: ts >= 3 * E), []
    for _ in range(calls):
        ks = s.worker.stack.ostore.env
        plan = cp.plan_phase(ks.timestep, ks.max_episode_steps, E, stop)
        got = cp.collect(s.worker, s.agent, stop, **({"sink": replay} if with_sink else {}))
        assert isinstance(got, StagedRollout if with_sink else ExperienceReplay)
        if with_sink:
            assert got.state == "open" and replay.ntimesteps + got.ntimesteps <= replay.rows
        phase = got if not with_sink else got.to_host()
        phase.tier, phase.tier_reason, phase.host_steps = got.tier, got.tier_reason, got.host_steps
        replay.extend(got)
        torch.cuda.synchronize()
        meta = dict(episodes=replay.episodes, vindex=dict(replay.vindex), ntimesteps=replay.ntimesteps, stopped=replay.stopped)
        out.append((phase, sc.state_record(s.worker), plan, meta))
    assert len(callback.seen) == calls
    return out, replay


def _compare(host_route, sink_route):
    (host_out, host), (sink_out, sink) = host_route, sink_route
    for (a, sa, plan, ma), (b, sb, _, mb) in zip(host_out, sink_out):
        rr.same_staged(b, a)
        sc.assert_same_state(sa, sb)
        assert ma == mb, (ma, mb)
        assert b.tier == "kernel" and b.tier_reason is None and b.host_steps == len(plan.truncations)
        assert plan.K * len(plan.timestep) == b.ntimesteps
    rr.same_metadata(sink, host)
    rr.pack_contract(sink, host)


@pytest.mark.parametrize("E,N,stride", [(5, 64, 1), (3, 256, 4)])
def test_kernel_tier_through_the_sink_equals_the_kernel_tier(E, N, stride):
    """``max_episode_steps = 4`` with the counters staggered: truncation steps between segments, episodes that continue
    across phases, under a capacity that evicts at the third commit."""
    host, sink = _run(False, E, N, stride, capacity=7 * E), _run(True, E, N, stride, capacity=7 * E)
    _compare(host, sink)
    assert sum(len(plan.truncations) for _, _, plan, _ in sink[0]) >= 3, "the sampling phases crossed no truncation"
    assert host[1].ntimesteps < 9 * E, "the capacity is meant to force eviction"
    assert any(len(ep.extents) > 1 for ep in sink[1]._eps.values()), "no episode spans several extents"


def test_kernel_tier_through_the_sink_with_multi_step_segments():
    """``max_episode_steps = 12``: segments of several steps, and a byte budget that cuts them to one step each."""
    from pdecontrol.mbrl import collection_phase as cp
    E, N = 5, 64
    host = _run(False, E, N, 1, tmax=3.0)
    for budget in (None, 2 * E * N * 4 + 4 * E * 20):
        saved = cp.SEGMENT_BYTES
        if budget is not None:
            cp.SEGMENT_BYTES = budget
            assert cp.segment_steps(E, N, 4) == 1
        try:
            sink = _run(True, E, N, 1, tmax=3.0)
        finally:
            cp.SEGMENT_BYTES = saved
        _compare(host, sink)
        assert [p.host_steps for p, _, _, _ in sink[0]] == [0, 0, 1]


def test_a_phase_that_raises_discards_its_staged_rows(monkeypatch):
    """The write-back of the second one-step segment raises (as an overflowing step makes it raise): nothing stays
    reserved."""
    from pdecontrol.mbrl import collection_phase as cp
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    E = 5
    s = sc.build(E=E, N=64, device=0, agent_device="cuda:0", tmax=3.0)
    monkeypatch.setattr(cp, "SEGMENT_BYTES", 2 * E * 64 * 4 + 4 * E * 20)
    sc.seed()
    sc.prime(s.worker, 11)
    sink = DeviceExperienceReplay(device=DEV)
    sink.extend(cp.collect(s.worker, s.agent, lambda ts, ep: ts >= E, sink=sink))
    assert cp.segment_steps(E, 64, 4) == 1
    live, calls, real = sink.ntimesteps, [], cp._restore

    def restore(*args):
        calls.append(1)
        if len(calls) == 2:
            raise FloatingPointError("overflow")
        return real(*args)

    monkeypatch.setattr(cp, "_restore", restore)
    with pytest.raises(FloatingPointError):
        cp.collect(s.worker, s.agent, lambda ts, ep: ts >= 6 * E, sink=sink)
    assert len(calls) == 2 and sink._staged == 0 and sink.ntimesteps == live == E
    assert sink._free.total == sink.rows - live


# ----------------------------------------------------------------------------------------------------------------------
# one controller slice
# ----------------------------------------------------------------------------------------------------------------------
def _slice(with_sink, packs):
    from pdecontrol.mbrl import collection_phase as cp, imagination_phase as ip, policy_phase as pp
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    from pdecontrol.mbrl.replay import ExperienceReplay
    from pdecontrol.surrogates.common.dataset import StartingStateDataset, SubSeqDataset
    E = 5
    c = sc.build(E=E, N=64, device=0, agent_device="cuda:0", tmax=3.0)      # max_episode_steps = 12: multi-step segments
    w = ro.build(ro.repo_namespace(), DEV, world_kwargs=DEVICE_REWARD)
    agent = c.agent
    to_agent_world, to_agent = pp_sc.controller_connectors(4, width=64)
    make = (lambda cap: DeviceExperienceReplay(cap, device=DEV)) if with_sink else ExperienceReplay
    replay, world_replay = make(60), make(40)
    sc.seed()
    sc.prime(c.worker, 11)
    tiers = []
    for _ in range(2):
        rollout = cp.collect(c.worker, agent, lambda ts, ep: ts >= 8 * E, **({"sink": replay} if with_sink else {}))
        tiers.append(rollout.tier)
        replay.extend(rollout)
        before = len(packs)
        starting = StartingStateDataset(data=replay.data, length=ro.TAU, stride=1, bootstrapping=False,
                                        stransf=w.transforms.replay_to_world)
        w.world.setup(starting)
        assert w.world._dev_starting is not None, "the world does not run its device path"
        if with_sink:
            assert w.world._dev_starting.store is replay.window_store()
        timings = {}
        imagined = ip.imagine(agent, w.stack, ro.NUM_ROLLOUTS, timings=timings, **({"sink": world_replay} if with_sink else {}))
        tiers.append(timings["tier"])
        world_replay.extend(imagined)
        if with_sink:
            sets = [world_replay.dataset(to_agent_world), replay.dataset(to_agent)]
        else:
            sets = [SubSeqDataset(data=r.data, length=1, stride=1, bootstrapping=False, stransf=t)
                    for r, t in ((world_replay, to_agent_world), (replay, to_agent))]
        timings = {}
        assert pp.update_policy(agent, sets, 32, 4, timings=timings) == 4
        tiers.append(timings["tier"])
        if with_sink:
            assert len(packs) == before, "the sink route packed a replay"
        else:
            assert len(packs) >= before + 3, "the host route packs the real replay for the world and both replays for the policy"
    torch.cuda.synchronize(DEV)
    dev = w.world._dev
    end = dict(agent=sm.full_state(agent), torch_cpu=torch.get_rng_state(), torch_dev=torch.cuda.get_rng_state(DEV),
               numpy=np.random.get_state(), timesteps=w.world.timesteps.copy(), simulated=int(w.world.simulated),
               state=dev.state.cpu().clone(), hidden=[h.cpu().clone() for hid in dev.hidden for h in hid],
               worker=sc.state_record(c.worker))
    return replay, world_replay, tiers, end


def test_controller_slice_over_the_slabs_equals_the_slice_over_host_replays(monkeypatch):
    from pdecontrol.surrogates.common import dataset as ds
    packs, real = [], ds.DeviceSubSeqStore.__init__
    monkeypatch.setattr(ds.DeviceSubSeqStore, "__init__", lambda self, *a, **k: (packs.append(1), real(self, *a, **k))[1])
    host, host_world, host_tiers, a = _slice(False, packs)
    sink, sink_world, sink_tiers, b = _slice(True, packs)
    assert host_tiers == sink_tiers == ["kernel"] * 6, (host_tiers, sink_tiers)
    monkeypatch.undo()
    rr.same_metadata(sink, host)
    rr.pack_contract(sink, host)
    rr.same_metadata(sink_world, host_world)
    rr.pack_contract(sink_world, host_world)
    assert set(a["agent"]) == set(b["agent"])
    for k in a["agent"]:
        assert torch.equal(a["agent"][k], b["agent"][k]), k
    assert torch.equal(a["torch_cpu"], b["torch_cpu"]) and torch.equal(a["torch_dev"], b["torch_dev"])
    assert a["numpy"][0] == b["numpy"][0] and np.array_equal(a["numpy"][1], b["numpy"][1]) and a["numpy"][2:] == b["numpy"][2:]
    assert np.array_equal(a["timesteps"], b["timesteps"]) and a["simulated"] == b["simulated"]
    assert torch.equal(a["state"], b["state"]) and all(torch.equal(x, y) for x, y in zip(a["hidden"], b["hidden"]))
    sc.assert_same_state(a["worker"], b["worker"])
