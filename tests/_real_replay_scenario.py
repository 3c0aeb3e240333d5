"""Shared pieces of the real-replay tests (tests/test_real_replay_host.py, tests/test_real_replay_gpu.py): the numpy
twin of ``ks_record_device`` with its inputs (``dst`` forms, reward sums that hit the roundings), the comparison of a
``DeviceExperienceReplay`` with the host ``ExperienceReplay`` after the same calls (metadata and the pack contract), and
the two routes of a collection phase."""
import numpy as np
import torch

FIELDS = ("obs", "actions", "nxtobs", "rewards", "terminated", "truncated", "steps")
FILL_F, FILL_B, FILL_I = -7.5, 7, -3                  # untouched rows keep these
DST_FORMS = ("contiguous", "permuted", "extents", "negative")


# ----------------------------------------------------------------------------------------------------------------------
# ks_record_device
# ----------------------------------------------------------------------------------------------------------------------
def halfway_sums(N, n_substeps):
    """fp64 sums whose reward ``(-1.0) * (1 / N) * ssq / n_substeps`` lies exactly halfway between two fp32 numbers (found
    by trying the neighbours of the real-valued solution; N = 64 with one sub-step always has them: the scale is a power
    of two)."""
    c, out = (-1.0) * (1 / N), []
    for f in (np.float32(-0.3), np.float32(-1.0), np.float32(-123.456), np.float32(-3e-5), np.float32(-1.5e-40)):
        g = np.nextafter(f, np.float32(-np.inf))
        mid = (np.float64(f) + np.float64(g)) / 2
        assert np.float32(f) != np.float32(g) and mid != np.float64(f) and mid != np.float64(g)
        s = mid * n_substeps / c
        for _ in range(8):
            s = np.nextafter(s, -np.inf)
        for _ in range(17):
            if (c * s) / n_substeps == mid:
                out.append(s)
                break
            s = np.nextafter(s, np.inf)
    return out


def reward_sums(rs, T, E, N, n_substeps):
    """[T, E] fp64: 0, a subnormal, 1e300, inf, NaN, a sum whose fp32 reward is subnormal, the halfway sums, then draws."""
    special = [0.0, 5e-324, 1e300, np.inf, np.nan, 6.4e-39 * n_substeps] + halfway_sums(N, n_substeps)
    flat = rs.uniform(0.0, 50.0 * N * n_substeps, T * E)
    k = min(len(special), flat.size)
    flat[:k] = special[:k]
    return rs.permutation(flat).reshape(T, E) if flat.size > k else flat.reshape(T, E)


def segment(rs, T, E, N, A, n_substeps):
    """What ``collect`` leaves behind for a segment: traj [T + 1, E, N], actions [T, E, A], ssq [T, E], steps int32 [T, E]."""
    return (rs.standard_normal((T + 1, E, N)).astype(np.float32), rs.uniform(-1, 1, (T, E, A)).astype(np.float32),
            reward_sums(rs, T, E, N, n_substeps), rs.randint(1, 400, (T, E)).astype(np.int32))


def dst_form(form, rs, T, E):
    """(int64 ``dst`` [T, E], rows of the slabs)."""
    n = T * E
    rows = n + 11
    if form == "contiguous":                                  # an env's T rows consecutive, as ``collect`` carves them
        dst = (3 + np.arange(n)).reshape(E, T).T
    elif form == "permuted":
        dst = rs.permutation(rows)[:n].reshape(T, E)
    elif form == "extents":                                   # two runs with a hole between them
        first = n // 2
        dst = np.concatenate((np.arange(first), 9 + first + np.arange(n - first))).reshape(E, T).T
    else:
        dst = rs.permutation(rows)[:n].reshape(T, E)
        dst.reshape(-1)[rs.permutation(n)[:max(1, n // 3)]] = -1 - rs.randint(0, 5)
    return np.ascontiguousarray(dst, dtype=np.int64), rows


def filled_slabs(rows, N, A):
    """Seven numpy slabs holding the fill pattern."""
    return [np.full((rows, 1, N), FILL_F, np.float32), np.full((rows, 1, A), FILL_F, np.float32),
            np.full((rows, 1, N), FILL_F, np.float32), np.full(rows, FILL_F, np.float32),
            np.full(rows, FILL_B, np.uint8), np.full(rows, FILL_B, np.uint8), np.full(rows, FILL_I, np.int32)]


def record_twin(slabs, seg, n_substeps, dst):
    """What ``ks_record_device`` writes, in numpy: the reward is ``KSBatchedVecEnv._finish_step``'s expression cast to fp32."""
    traj, actions, ssq, steps = seg
    N = traj.shape[2]
    with np.errstate(all="ignore"):
        rewards = np.asarray((-1.0) * (1 / N) * ssq / n_substeps, dtype=np.float32)
    keep = dst >= 0
    rows = dst[keep]
    slabs[0][rows, 0], slabs[1][rows, 0], slabs[2][rows, 0] = traj[:-1][keep], actions[keep], traj[1:][keep]
    slabs[3][rows], slabs[4][rows], slabs[5][rows], slabs[6][rows] = rewards[keep], 0, 0, steps[keep]


def same_slabs(got, want, what):
    for name, g, w in zip(FIELDS, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name)           # bytes: NaN rewards compare too


# ----------------------------------------------------------------------------------------------------------------------
# the replay against the host replay
# ----------------------------------------------------------------------------------------------------------------------
def same_metadata(sink, host, what=""):
    assert sink.episodes == host.episodes, (what, sink.episodes, host.episodes)
    assert dict(sink.vindex) == dict(host.vindex), (what, dict(sink.vindex), dict(host.vindex))
    assert sink.ntimesteps == host.ntimesteps and sink.stopped == host.stopped, what
    assert sink.capacity == host.capacity, what
    assert [len(c) for c in sink.data.obs.values()] == [len(d) for d in host.obs.values()], what


def pack_contract(sink, host, what=""):
    """``DeviceSubSeqStore(host.data, device).tensors`` equals the slabs read through the window store, bit for bit."""
    from pdecontrol.surrogates.common.dataset import DeviceSubSeqStore
    with np.errstate(over="ignore"):                            # (a test's 1e300 reward is inf in fp32 on both routes)
        want = DeviceSubSeqStore(host.data, sink.device)
    store = sink.window_store()
    assert store.total == want.total and store.starts == want.starts, what
    got = store.gather(torch.arange(store.total, device=sink.device))
    for name, g, w in zip(FIELDS, got, want.tensors):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert g.cpu().numpy().tobytes() == w.cpu().numpy().tobytes(), (what, name)
    assert np.array_equal(store.steps_host, want.tensors[6].cpu().numpy()), what


def same_staged(staged, replay, what=""):
    """A phase's ``StagedRollout`` answers what the phase's host replay answers (before it is committed).  ``staged`` may
    also be the ``to_host()`` of one, taken while it was open, carrying its ``tier``, ``tier_reason`` and ``host_steps``."""
    assert staged.episodes == replay.episodes and dict(staged.vindex) == dict(replay.vindex), what
    assert staged.ntimesteps == replay.ntimesteps, what
    assert (staged.tier, staged.tier_reason, staged.host_steps) == (replay.tier, replay.tier_reason, replay.host_steps), what
    host = staged.to_host() if hasattr(staged, "to_host") else staged
    for name, dt in zip(FIELDS, (np.float32, np.float32, np.float32, np.float32, np.bool_, np.bool_, np.int32)):
        a, b = getattr(host, name), getattr(replay, name)
        assert list(a.keys()) == list(b.keys()), (what, name)
        for key in b:
            with np.errstate(over="ignore"):
                x, y = np.asarray(a[key], dtype=dt), np.asarray(b[key], dtype=dt)
            assert x.tobytes() == y.tobytes(), (what, name, key)
