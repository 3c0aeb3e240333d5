"""Shared pieces of the device-resident replay tests (tests/test_device_replay_host.py, tests/test_device_replay_gpu.py):
seeded rollout rounds in the layout of the imagined-rollout phase's round block, the numpy twin of ``rp_append``, the two
routes (host ``ExperienceReplay`` / ``DeviceExperienceReplay``) fed with the same rounds, and the comparison of replays."""
import numpy as np
import torch

FIELDS = ("obs", "actions", "nxtobs", "rewards", "terminated", "truncated", "steps")
# the issue's scenario: capacity 40, five phases of 3 envs x 3 rounds with these horizons, each preceded by resize(40)
CAPACITY, ENVS, ROUNDS, HORIZONS = 40, 3, 3, (2, 2, 3, 3, 3)
ORDERS = ([0, 2, 4, 1, 3, 5, 6, 7, 8], [0, 2, 4, 1, 3, 5, 6, 7, 8] + list(range(9, 18)), list(range(12, 27)),
          list(range(23, 36)), list(range(32, 45)))
NTIMESTEPS = (18, 36, 39, 39, 39)


def make_rounds(rs, B, lengths, N=8, A=4):
    """One phase: per round (traj [T + 1, B, N], actions [T, B, A], rewards [T, B], steps int32 [T, B])."""
    return [(rs.randn(T + 1, B, N).astype(np.float32), rs.uniform(-1, 1, (T, B, A)).astype(np.float32),
             (-rs.uniform(0.01, 0.99, (T, B))).astype(np.float32), rs.randint(1, 400, (T, B)).astype(np.int32))
            for T in lengths]


def append_twin(tensors, dst, round_):
    """What ``rp_append`` writes, on numpy arrays or CPU tensors: transition (t, b) goes to row dst[t, b] unless negative."""
    traj, actions, rewards, steps = round_
    T, B = dst.shape
    as_t = lambda v: torch.as_tensor(np.asarray(v))
    for t in range(T):
        for b in range(B):
            r = int(dst[t, b])
            if r < 0:
                continue
            tensors[0][r, 0] = as_t(traj[t, b])
            tensors[1][r, 0] = as_t(actions[t, b])
            tensors[2][r, 0] = as_t(traj[t + 1, b])
            tensors[3][r] = float(rewards[t, b])
            tensors[4][r] = False
            tensors[5][r] = t == T - 1
            tensors[6][r] = int(steps[t, b])


def stage(sink, rounds, B):
    """The rounds staged in ``sink`` as ``imagine(..., sink=)`` stages them, written by the twin (``device="cpu"``)."""
    N, A = rounds[0][0].shape[2], rounds[0][1].shape[2]
    staged = sink.stage(B, N, A)
    for round_ in rounds:
        dst = staged.reserve(round_[1].shape[0])
        assert dst.shape == round_[1].shape[:2] and dst.dtype == np.int64 and dst.flags.c_contiguous
        assert len(set(dst.reshape(-1).tolist())) == dst.size and 0 <= dst.min() and dst.max() < sink.rows
        append_twin(sink.tensors, dst, round_)
    return staged


def host_rollout(rounds, B):
    """The host ``ExperienceReplay`` the imagined-rollout phase builds from the same rounds."""
    from pdecontrol.mbrl.imagination_phase import _build_replay
    return _build_replay(rounds, B)[0]


def same_replay(got, want, what=""):
    """Keys in insertion order, every deque item's value, shape and dtype, ``vindex``, ``capacity`` and the counters."""
    assert got.episodes == want.episodes, (what, got.episodes, want.episodes)
    assert dict(got.vindex) == dict(want.vindex), (what, dict(got.vindex), dict(want.vindex))
    assert got.capacity == want.capacity, (what, got.capacity, want.capacity)
    assert got.stopped == want.stopped and got.ntimesteps == want.ntimesteps, what
    for name in FIELDS:
        a, b = getattr(got, name), getattr(want, name)
        assert list(a.keys()) == list(b.keys()), (what, name)
        for key in b:
            assert len(a[key]) == len(b[key]), (what, name, key)
            for x, y in zip(a[key], b[key]):
                x, y = np.asarray(x), np.asarray(y)
                assert x.dtype == y.dtype and x.shape == y.shape, (what, name, key, x.dtype, y.dtype, x.shape, y.shape)
                assert x.tobytes() == y.tobytes(), (what, name, key)


def stats_pair(device="cpu"):
    """Host replay and sink holding stopped episodes of 1, 5, 63, 64 and 65 steps; the one of 5 is split over a hole."""
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    from pdecontrol.mbrl.replay import ExperienceReplay
    host, sink = ExperienceReplay(), DeviceExperienceReplay(device=device, rows=230)
    rs = np.random.RandomState(7)
    for lengths, shrink in (([2, 3, 2], 5), ([1, 5, 63, 64, 65], None)):
        rounds = make_rounds(rs, 1, lengths)
        host.extend(host_rollout(rounds, 1))
        if device == "cpu":
            sink.extend(stage(sink, rounds, 1))
        else:
            sink.extend(host_rollout(rounds, 1))
        if shrink:
            for r in (host, sink):
                r.resize(shrink)
                r.resize(np.inf)
    assert sorted(ep.length for ep in sink._eps.values()) == [1, 2, 3, 5, 63, 64, 65]
    assert [ep.extents for ep in sink._eps.values() if ep.length == 5] == [[(1, 1), (7, 4)]]
    return host, sink
