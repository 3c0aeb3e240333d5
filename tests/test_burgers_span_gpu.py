"""``bg_step_span`` (include/burgers_hip.h) on an MI355X: T env steps in one launch against T successive ``bg_step``
launches, byte for byte in every output (``u``, ``traj[1 .. T]``, ``ssq``, ``status``), and against the fp32 twin
oracle/burgers_oracle.c chained T times (``traj`` bit for bit, ``ssq`` at ``_burgers_cases.ssq_rtol``).

Inputs are the white-noise fields of tests/_burgers_cases.py at its ``params(N)``; the four Gaussian actuators for
``n_act = 4``, a white-noise ``F`` for ``n_act = 1``.  Every buffer carries the sentinels of tests/test_burgers_gpu.py: one
NaN row past ``u``, one NaN / -7 cell past ``ssq`` and ``status``, and around the trajectory slot 0 and slot T + 1, all NaN,
which must come back untouched."""
import numpy as np
import pytest
import torch

import _burgers_cases as bc
from hipbind import ptr
from oracle import burgers_oracle as bo
from test_burgers_gpu import DEV, NAN_BITS, STATUS_SENTINEL, _dev, _padded, _stream, _untouched, hip  # noqa: F401

pytestmark = pytest.mark.gpu


def _inputs(N, E, T, n_act, seed=3):
    """(u0 [E, N], actions [T, E, n_act], F [n_act, N]) of a case."""
    u0 = bc.noise(seed + N + E, E, N)
    acts = np.stack([bc.actions(seed + N + 17 * t, E, n_act) for t in range(T)])
    return u0, acts, bc.forcing(N, n_act, random_F=n_act != 4)


def _buffers(u0, T):
    """Padded outputs of a T-step segment: u [E + 1, N], traj [T + 2, E, N] all NaN, ssq [T E + 1], status [T E + 1]."""
    E, N = u0.shape
    return (_padded(u0), torch.full((T + 2, E, N), float("nan"), dtype=torch.float32, device=DEV),
            _padded((T * E,), dtype=torch.float64), _padded((T * E,), fill=STATUS_SENTINEL, dtype=torch.int32))


def _finish(u, traj, q, st, T, what):
    """Synchronise, check every sentinel, return the outputs as numpy arrays (the sentinels included: ``*_raw``)."""
    torch.cuda.synchronize(DEV)
    E = u.shape[0] - 1
    _untouched(u, f"{what}: u")
    if q is not None:
        _untouched(q, f"{what}: ssq")
    if st is not None:
        _untouched(st, f"{what}: status")
    t = traj.cpu().numpy()
    assert (t[0].view(np.uint32) == NAN_BITS).all(), f"{what}: trajectory slot 0 was written"
    assert (t[T + 1].view(np.uint32) == NAN_BITS).all(), f"{what}: trajectory slot T + 1 was written"
    return {"u": u[:-1].cpu().numpy(), "traj": t[1:T + 1], "ssq": None if q is None else q[:-1].cpu().numpy().reshape(T, E),
            "status": None if st is None else st[:-1].cpu().numpy().reshape(T, E)}


def span(hip, u0, acts, F, dx, dt, nu, n, ssq=True, status=True):
    """One ``bg_step_span`` launch on padded buffers."""
    T, E, A = acts.shape
    u, traj, q, st = _buffers(u0, T)
    q, st = q if ssq else None, st if status else None
    a, f = _dev(acts), _dev(F)
    hip.check(hip.load().bg_step_span(_stream(), ptr(u), ptr(a), ptr(f), A, E, u0.shape[1], T, dx, dt, nu, n, ptr(traj), ptr(q),
                                      ptr(st)))
    return _finish(u, traj, q, st, T, f"span N{u0.shape[1]}-E{E}-T{T}-act{A}-n{n}")


def launches(hip, u0, acts, F, dx, dt, nu, n):
    """T successive ``bg_step`` launches on buffers of the same layout: ``bg_step(actions + t E A, obs = traj[t + 1])``."""
    T, E, A = acts.shape
    u, traj, q, st = _buffers(u0, T)
    a, f = _dev(acts), _dev(F)
    for t in range(T):
        hip.check(hip.load().bg_step(_stream(), ptr(u), ptr(a[t]), ptr(f), A, E, u0.shape[1], dx, dt, nu, n, ptr(traj[t + 1]),
                                     ptr(q[t * E:]), ptr(st[t * E:])))
    return _finish(u, traj, q, st, T, f"launches N{u0.shape[1]}-E{E}-T{T}-act{A}-n{n}")


def _same_bytes(got, want, what, keys=("u", "traj", "ssq", "status")):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert got[k].tobytes() == want[k].tobytes(), f"{what}: {k} differs from the T launches"


def _check(hip, N, E, T, n_act, n):
    dx, dt, nu = bc.params(N)
    u0, acts, F = _inputs(N, E, T, n_act)
    what = f"N{N}-E{E}-T{T}-act{n_act}-n{n}"
    got = span(hip, u0, acts, F, dx, dt, nu, n)
    _same_bytes(got, launches(hip, u0, acts, F, dx, dt, nu, n), what)
    bc.assert_bits(got["u"], got["traj"][T - 1], f"{what}: u against the last slot")
    state = u0
    for t in range(T):
        state, twin_ssq = bo.twin_step(state, acts[t], F, dx, dt, nu, n)
        bc.assert_bits(got["traj"][t], state, f"{what}: slot {t + 1} against the twin")
        np.testing.assert_allclose(got["ssq"][t], twin_ssq, rtol=bc.ssq_rtol(N), atol=0, err_msg=f"{what}: ssq[{t}]")
    assert not got["status"].any(), (what, got["status"])


@pytest.mark.parametrize("E", [1, 4, 5])           # one wave, one full workgroup, one past it
@pytest.mark.parametrize("N", [64, 128, 256])      # P = 1 scalar, P = 2 packed scalar, P = 4 pair-native
def test_span_equals_successive_launches_and_the_twin(hip, N, E):
    for T in (1, 2, 3):
        for n in (1, 2):
            for n_act in (1, 4):
                _check(hip, N, E, T, n_act, n)


@pytest.mark.parametrize("N", [512, 1024])         # P = 8 (the BASELINE width) and P = 16
def test_span_at_the_wide_layouts(hip, N):
    _check(hip, N, 5, 2, 4, 2)


def test_zero_substeps_copy_the_state_into_every_slot(hip):
    N, E, T = 128, 5, 3
    dx, dt, nu = bc.params(N)
    u0, acts, F = _inputs(N, E, T, 4)
    got = span(hip, u0, acts, F, dx, dt, nu, 0)
    _same_bytes(got, launches(hip, u0, acts, F, dx, dt, nu, 0), "0 sub-steps")
    bc.assert_bits(got["u"], u0, "u after 0 sub-steps")
    for t in range(T):
        bc.assert_bits(got["traj"][t], u0, f"slot {t + 1} after 0 sub-steps")
    assert (got["ssq"] == 0).all() and (got["status"] == 0).all()


@pytest.mark.parametrize("N", [64, 256])
def test_status_is_per_env_and_per_step(hip, N):
    """env 2 holds one inf: its status is set at every step from the first on, nobody else's, and the other envs' bytes
    are those of the clean run."""
    E, T = 5, 3
    dx, dt, nu = bc.params(N)
    u0, acts, F = _inputs(N, E, T, 4)
    clean = span(hip, u0, acts, F, dx, dt, nu, 2)
    bad = u0.copy()
    bad[2, 7] = np.inf
    got = span(hip, bad, acts, F, dx, dt, nu, 2)
    _same_bytes(got, launches(hip, bad, acts, F, dx, dt, nu, 2), f"N{N} with an inf")
    assert got["status"].tolist() == [[0, 0, 1, 0, 0]] * T and not clean["status"].any()
    keep = [0, 1, 3, 4]
    for k, rows in (("u", got["u"][keep]), ("traj", got["traj"][:, keep]), ("ssq", got["ssq"][:, keep])):
        want = clean[k][keep] if k == "u" else clean[k][:, keep]
        assert rows.tobytes() == want.tobytes(), (N, k)


def test_null_outputs_leave_the_others_unchanged(hip):
    N, E, T = 256, 5, 2
    dx, dt, nu = bc.params(N)
    u0, acts, F = _inputs(N, E, T, 4)
    full = span(hip, u0, acts, F, dx, dt, nu, 2)
    for off in ({"ssq"}, {"status"}, {"ssq", "status"}):
        r = span(hip, u0, acts, F, dx, dt, nu, 2, **{k: False for k in off})
        assert all(r[k] is None for k in off)
        _same_bytes(r, full, sorted(off), keys=[k for k in ("u", "traj", "ssq", "status") if k not in off])
