"""The device-resident replay on an MI355X (pdecontrol/mbrl/device_replay.py, csrc/replay.hip): ``rp_append`` alone against
its numpy twin, ``rp_episode_returns`` against Python's ``sum``, and the chain ``imagine(sink=) -> extend -> update_policy``
over the view against ``imagine -> host extend -> update_policy`` over ``SubSeqDataset``s on the same GPU.  Every comparison
is bit for bit: the append copies, the returns are the same chain of fp32 additions, and both routes run the same kernels
on the same data."""
import numpy as np
import pytest
import torch

import _device_replay_scenario as sc
import _policy_phase_scenario as pp_sc
import _rollout_scenario as ro
import _sac_models as sm

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DEVICE_REWARD = {"batched_reward_func": lambda env: env.batched_reward_func}
T_CAP = 5
FLOAT_FILL, BYTE_FILL = 0x5A5AC3C3, 0xA5          # the slab before the append: a pattern no copied value has


def _filled_slab(rows, N, A):
    ints = lambda *shape: torch.full(shape, FLOAT_FILL, dtype=torch.int32, device=DEV)
    byte = lambda: torch.full((rows,), BYTE_FILL, dtype=torch.uint8, device=DEV)
    return (ints(rows, 1, N).view(torch.float32), ints(rows, 1, A).view(torch.float32), ints(rows, 1, N).view(torch.float32),
            ints(rows).view(torch.float32), byte().view(torch.bool), byte().view(torch.bool), ints(rows))


def _bits(t):
    t = t.cpu()
    return t.view(torch.uint8 if t.dtype == torch.bool else torch.int32).numpy().reshape(t.shape[0], -1)


def _dst_cases(rs, T, B, rows):
    n = T * B
    split = np.concatenate((np.arange(1, 1 + n // 2), np.arange(rows - (n - n // 2), rows)))
    holes = rs.permutation(rows)[:n]
    holes[rs.rand(n) < 0.3] = -1
    holes[0] = -1
    return {"contiguous": np.arange(3, 3 + n), "permuted": rs.permutation(rows)[:n], "split": split, "negative": holes}


@pytest.mark.parametrize("N", [64, 98, 100, 256])
def test_rp_append_equals_its_numpy_twin(N):
    """N = 98 takes the scalar path for the observations, A = 1 for the actions, the others float4; B = 1, 5 and 257 are one
    wave, a partial workgroup and many workgroups with a partial last one; T = 1 and 5 of a block laid out for 5.  Rows that
    ``dst`` does not name keep the bit pattern they were filled with."""
    import hipbind
    from pdecontrol.mbrl import replay_hip
    replay_hip.load()
    for A in (1, 4, 16):
        for B in (1, 5, 257):
            rs = np.random.RandomState(N + A + B)
            sizes = ((T_CAP + 1) * B * N, T_CAP * B * A, T_CAP * B, T_CAP * B)
            block = torch.from_numpy(rs.randn(sum(sizes)).astype(np.float32))
            steps_view = block[sum(sizes[:3]):].view(torch.int32)
            steps_view.copy_(torch.from_numpy(rs.randint(1, 400, sizes[3]).astype(np.int32)))
            traj, actions, rewards, steps = (v.numpy() for v in torch.split(block, sizes))
            traj, actions = traj.reshape(T_CAP + 1, B, N), actions.reshape(T_CAP, B, A)
            rewards, steps = rewards.reshape(T_CAP, B), steps.view(np.int32).reshape(T_CAP, B)
            block_dev = block.to(DEV)
            for T in (1, T_CAP):
                rows = 2 * T * B + 9
                for kind, dst in _dst_cases(rs, T, B, rows).items():
                    dst = np.ascontiguousarray(dst.reshape(T, B).astype(np.int64))
                    slab = _filled_slab(rows, N, A)
                    dst_dev = torch.from_numpy(dst).to(DEV)
                    replay_hip.append(hipbind.stream(), block_dev.data_ptr(), T, T_CAP, B, N, A, dst_dev.data_ptr(), dst,
                                      replay_hip.slab(slab))
                    torch.cuda.synchronize(DEV)
                    want = [_bits(t).copy() for t in _filled_slab(rows, N, A)]
                    t_idx, b_idx = np.nonzero(dst >= 0)
                    r = dst[t_idx, b_idx]
                    as_bits = lambda v, width: np.ascontiguousarray(v).view(np.int32).reshape(len(r), width)
                    want[0][r] = as_bits(traj[t_idx, b_idx], N)
                    want[1][r] = as_bits(actions[t_idx, b_idx], A)
                    want[2][r] = as_bits(traj[t_idx + 1, b_idx], N)
                    want[3][r] = as_bits(rewards[t_idx, b_idx], 1)
                    want[4][r] = 0
                    want[5][r] = (t_idx == T - 1).astype(np.uint8)[:, None]
                    want[6][r] = steps[t_idx, b_idx][:, None]
                    for name, got, ref in zip(sc.FIELDS, slab, want):
                        assert np.array_equal(_bits(got), ref), (name, N, A, B, T, kind)


def test_rp_episode_returns_equals_pythons_sum():
    """Episodes of 1, 5, 63, 64 and 65 steps on permuted rows, and through ``statistics`` on a replay where one is split."""
    import hipbind
    from pdecontrol.mbrl import replay_hip
    replay_hip.load()
    rs = np.random.RandomState(0)
    lengths = [1, 5, 63, 64, 65]
    rewards = (-rs.uniform(0.01, 0.99, 300)).astype(np.float32)
    rows = rs.permutation(300)[:sum(lengths)].astype(np.int64)
    offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    out = torch.full((len(lengths) + 1,), 7.0, dtype=torch.float32, device=DEV)
    keep = [torch.from_numpy(v).to(DEV) for v in (rewards, rows, offsets)]
    replay_hip.episode_returns(hipbind.stream(), keep[0], keep[1], keep[2], out[:len(lengths)])
    torch.cuda.synchronize(DEV)
    want = np.asarray([sum(rewards[rows[a:b]]) for a, b in zip(offsets[:-1], offsets[1:])], dtype=np.float32)
    assert out.cpu().numpy()[:-1].tobytes() == want.tobytes() and float(out[-1]) == 7.0
    host, sink = sc.stats_pair(DEV)
    sc.same_replay(sink.to_host(), host, "the uploaded replay")
    for w, g in zip(host.statistics(), sink.statistics()):
        assert type(w) is type(g) is np.float32 and w.tobytes() == g.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------------------------------
HORIZONS, CAPACITY, B_UPD, U_UPD = (3, 2, 3), 40, 32, 4


def _route(with_sink):
    """Three controller iterations ``resize -> imagine -> extend -> update_policy`` from the scenario's seeds."""
    from pdecontrol.mbrl import imagination_phase as ip, policy_phase as pp
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    from pdecontrol.mbrl.replay import ExperienceReplay
    from pdecontrol.surrogates.common.dataset import SubSeqDataset
    s = ro.build(ro.repo_namespace(), DEV, world_kwargs=DEVICE_REWARD)
    to_agent_world, to_agent = pp_sc.controller_connectors(4, width=64)
    real = SubSeqDataset(data=s.replay.data, length=1, stride=1, bootstrapping=False, stransf=to_agent)
    world_replay = DeviceExperienceReplay(CAPACITY, device=DEV) if with_sink else ExperienceReplay(CAPACITY)
    ro.seed()
    tiers, snapshots = [], []
    for horizon in HORIZONS:
        world_replay.resize(CAPACITY)
        s.world.horizon = horizon
        s.world.setup(s.starting)
        timings = {}
        rollout = ip.imagine(s.agent, s.stack, ro.NUM_ROLLOUTS, timings=timings, **({"sink": world_replay} if with_sink else {}))
        tiers.append(timings["tier"])
        assert rollout.ntimesteps == 2 * ro.NUM_ENVS * horizon
        world_replay.extend(rollout)
        if with_sink:
            imagined = world_replay.dataset(to_agent_world)
        else:
            imagined = SubSeqDataset(data=world_replay.data, length=1, stride=1, bootstrapping=False, stransf=to_agent_world)
        timings = {}
        assert pp.update_policy(s.agent, [imagined, real], B_UPD, U_UPD, timings=timings) == U_UPD
        tiers.append(timings["tier"])
        snapshots.append(world_replay.to_host() if with_sink else None)
    torch.cuda.synchronize(DEV)
    dev = s.world._dev
    end = dict(agent=sm.full_state(s.agent), torch_cpu=torch.get_rng_state(), torch_dev=torch.cuda.get_rng_state(DEV),
               numpy=np.random.get_state(), timesteps=s.world.timesteps.copy(), simulated=int(s.world.simulated),
               state=dev.state.cpu().clone(), hidden=[h.cpu().clone() for hid in dev.hidden for h in hid])
    return s, world_replay, tiers, end


def test_chain_through_the_sink_equals_the_chain_through_the_host():
    from pdecontrol.mbrl import policy_phase as pp
    from pdecontrol.surrogates.common.dataset import DeviceSubSeqStore, SubSeqDataset
    from pdegym.common.transforms import BatchTransform, FuncTransform, SampleTransform
    _, host, host_tiers, a = _route(False)
    s, sink, sink_tiers, b = _route(True)
    assert host_tiers == sink_tiers == ["kernel"] * 6, (host_tiers, sink_tiers)
    assert host.ntimesteps <= CAPACITY < 24 + 16 + 24, "the capacity is meant to force eviction"
    sc.same_replay(sink.to_host(), host, "world_replay after three iterations")
    assert set(a["agent"]) == set(b["agent"])
    for k in a["agent"]:
        assert torch.equal(a["agent"][k], b["agent"][k]), k
    assert torch.equal(a["torch_cpu"], b["torch_cpu"]) and torch.equal(a["torch_dev"], b["torch_dev"])
    assert a["numpy"][0] == b["numpy"][0] and np.array_equal(a["numpy"][1], b["numpy"][1]) and a["numpy"][2:] == b["numpy"][2:]
    assert np.array_equal(a["timesteps"], b["timesteps"]) and a["simulated"] == b["simulated"]
    assert torch.equal(a["state"], b["state"]) and all(torch.equal(x, y) for x, y in zip(a["hidden"], b["hidden"]))

    # an unrecognised connector on the view: the torch-on-device tier, with the host loader's batches
    halve = SampleTransform(otransf=[BatchTransform(FuncTransform(lambda v: v * 0.5))])
    real = SubSeqDataset(data=s.replay.data, length=1, stride=1, bootstrapping=False)
    view = sink.dataset(halve)
    reference = [SubSeqDataset(data=host.data, length=1, stride=1, bootstrapping=False, stransf=halve), real]
    idx = np.random.RandomState(1).randint(0, len(view) + len(real), size=3 * 16)
    plan = pp.PolicyBatchPlan([view, real], 16, 3, indices=idx)
    stores = [view.slab_store(DEV), DeviceSubSeqStore(real.fields, DEV)]
    for u, got in enumerate(pp.device_batches(plan, stores)):
        pp_sc.same_batch(got, pp_sc.collate_items(reference, idx[u * 16:(u + 1) * 16]), f"update {u}")
    timings = {}
    assert pp.update_policy(s.agent, [view, real], 16, 2, timings=timings) == 2
    assert timings["tier"] == "torch-on-device"
