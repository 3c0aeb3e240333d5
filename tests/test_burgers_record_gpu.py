"""``bg_record`` (include/burgers_hip.h) on an MI355X against a numpy restatement: a segment's transitions written into
the seven slabs of a device-resident replay through a permuted destination map with negative entries, into slabs larger
than ``T E``.  Rows named are equal in every field, bit for bit; rows not named keep their fill.

The reward is the loop's: ``BurgersBatchedVecEnv.step_torch`` returns ``ssq * c`` with ``c = -(1.0 / N) / max(n, 1)``
formed on the host, one fp64 product, which the replay's dtype table casts to fp32.  The KS form ``(c' * ssq) / n`` rounds
the exact quotient instead of a product with a rounded ``c``; ``differing_sums`` finds, on the CPU, sums at which the two
end in different fp32 values (next to an fp32 rounding boundary), so that the wrong expression fails here.  With three
sub-steps ``c`` carries a rounding error of a third of an ulp and such sums are a few fp64 neighbours from every boundary
(with 50 the error of ``c`` is too small for a short search to find any: that case runs on drawn sums only)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _real_replay_scenario as rr  # noqa: E402
from test_burgers_gpu import DEV, _stream, hip  # noqa: E402,F401

pytestmark = pytest.mark.gpu


def burgers_reward(ssq, N, n):
    """``step_torch``'s expression, cast as the replay casts it."""
    with np.errstate(all="ignore"):
        return np.asarray(ssq * (-(1.0 / N) / max(n, 1)), dtype=np.float32)


def ks_reward(ssq, N, n):
    with np.errstate(all="ignore"):
        return np.asarray((-1.0) * (1 / N) * ssq / max(n, 1), dtype=np.float32)


def differing_sums(N, n):
    """fp64 sums next to an fp32 rounding boundary of the reward at which the two expressions differ in fp32."""
    c, out = -(1.0 / N) / max(n, 1), []
    for f in (-0.3, -1.0, -123.456, -3e-5, -0.0117, -7.25, -2.5e-3, -41.0):
        f = np.float32(f)
        mid = (np.float64(f) + np.float64(np.nextafter(f, np.float32(-np.inf)))) / 2
        s = np.float64(mid / c)
        for _ in range(64):
            s = np.nextafter(s, -np.inf)
        for _ in range(129):
            if burgers_reward(s, N, n) != ks_reward(s, N, n):
                out.append(float(s))
                break
            s = np.nextafter(s, np.inf)
    return out


def _segment(rs, T, E, N, A, n, special):
    """traj [T + 1, E, N], actions [T, E, A], ssq [T, E] (the special sums first, then draws), steps int32 [T, E]."""
    ssq = rs.uniform(0.0, 50.0 * N * max(n, 1), T * E)
    k = min(len(special), ssq.size)
    ssq[:k] = special[:k]
    return (rs.standard_normal((T + 1, E, N)).astype(np.float32), rs.uniform(-1, 1, (T, E, A)).astype(np.float32),
            ssq.reshape(T, E), rs.randint(1, 400, (T, E)).astype(np.int32))


def _dst(rs, T, E):
    """A permutation of the slab's rows with a third of the entries negative (none where ``T E < 3``); ``T E + 11`` rows."""
    n = T * E
    rows = n + 11
    dst = rs.permutation(rows)[:n].astype(np.int64)
    dst[rs.permutation(n)[:n // 3]] = -1 - rs.randint(0, 5)
    return np.ascontiguousarray(dst.reshape(T, E)), rows


def _twin(slabs, seg, N, n, dst):
    traj, actions, ssq, steps = seg
    keep = dst >= 0
    rows = dst[keep]
    slabs[0][rows, 0], slabs[1][rows, 0], slabs[2][rows, 0] = traj[:-1][keep], actions[keep], traj[1:][keep]
    slabs[3][rows], slabs[4][rows], slabs[5][rows], slabs[6][rows] = burgers_reward(ssq, N, n)[keep], 0, 0, steps[keep]


def _record(hip, seg, n, dst, rows):
    traj, actions, ssq, steps = seg
    T, E, A = actions.shape
    N = traj.shape[2]
    dev = [torch.from_numpy(x).to(DEV) for x in (traj, actions, ssq, steps, dst)]
    slabs = [torch.from_numpy(x).to(DEV) for x in rr.filled_slabs(rows, N, A)]
    record = hip.Slabs(*(x.data_ptr() for x in slabs), rows)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    hip.check(hip.load().bg_record(_stream(), vp(dev[0]), vp(dev[1]), E, N, A, vp(dev[2]), vp(dev[3]), T, n, vp(dev[4]),
                                   dst.ctypes.data_as(ctypes.c_void_p), ctypes.byref(record)))
    torch.cuda.synchronize(DEV)
    for before, after in zip((traj, actions, ssq, steps, dst), dev):
        assert after.cpu().numpy().tobytes() == before.tobytes(), "bg_record wrote one of its inputs"
    return [x.cpu().numpy() for x in slabs]


def _check(hip, T, E, N, A, n, special):
    rs = np.random.RandomState(1000 * T + 100 * E + N + A + n)
    seg = _segment(rs, T, E, N, A, n, special)
    dst, rows = _dst(rs, T, E)
    want = rr.filled_slabs(rows, N, A)
    _twin(want, seg, N, n, dst)
    rr.same_slabs(_record(hip, seg, n, dst, rows), want, (T, E, N, A, n))
    named = np.zeros(rows, dtype=bool)
    named[dst[dst >= 0]] = True
    assert named.sum() == (dst >= 0).sum() and (want[3][~named] == rr.FILL_F).all() and (want[6][~named] == rr.FILL_I).all()


def test_the_two_reward_expressions_differ_on_the_special_sums():
    """On the CPU: the sums the record cases start with separate the Burgers reward from the KS form."""
    for N in (64, 256):
        sums = np.asarray(differing_sums(N, 3))
        assert sums.size >= 3, (N, sums)
        assert (burgers_reward(sums, N, 3) != ks_reward(sums, N, 3)).all()
        assert (np.abs(burgers_reward(sums, N, 3).view(np.int32) - ks_reward(sums, N, 3).view(np.int32)) == 1).all()


@pytest.mark.parametrize("A", [1, 4])
@pytest.mark.parametrize("N", [64, 256])
@pytest.mark.parametrize("E", [1, 5])
@pytest.mark.parametrize("T", [1, 3])
def test_bg_record_equals_the_numpy_restatement(hip, T, E, N, A):
    special = differing_sums(N, 3)
    assert special and burgers_reward(np.float64(special[0]), N, 3) != ks_reward(np.float64(special[0]), N, 3)
    _check(hip, T, E, N, A, 3, special)


@pytest.mark.parametrize("n", [0, 1, 50])
def test_bg_record_over_sub_step_counts(hip, n):
    """``max(n, 1)``: no sub-step divides by one; 50 is the env's default."""
    _check(hip, 3, 5, 64, 4, n, [0.0, 5e-324, 1e300, np.inf, np.nan])
