"""Inputs, references and bounds shared by tests/test_burgers.py (the C twin's CPU anchors) and tests/test_burgers_gpu.py
(libburgers_hip.so against the twin).

Fields are WHITE NOISE, not the env's smooth initial condition: on a smooth field a wrong or shifted stencil tap moves the
result only at order dx; on white noise a swapped +-2 halo tap moves one sub-step by about 9e-5 at N = 64, against an
fp32-vs-fp64 noise of about 3e-8.  L = 2 pi, nu = 0.02, dt = 5e-4 (1e-4 at N = 1024): finite for 50 sub-steps at all five
widths with |u| <= 1.1."""
import functools

import numpy as np

from oracle import burgers_oracle as bo

WIDTHS = (64, 128, 256, 512, 1024)
L = 2 * np.pi
NU = 0.02
EPS = float(np.finfo(np.float32).eps)
FLOOR_ULPS = 8           # the bar of tests/test_burgers.py::_close, in ulp of the field scale
ORDER_FACTOR = 4         # "another order of the same fp32 operations" (tests/test_sac_gpu.py)


def params(N):
    """(dx, dt, nu) as the fp32 values every side of a comparison is given."""
    return np.float32(L / N), np.float32(5e-4 if N < 1024 else 1e-4), np.float32(NU)


def noise(seed, E, N):
    return np.random.RandomState(seed).uniform(-1, 1, (E, N)).astype(np.float32)


def four_actuators(N, sigma=0.15, Xi=(0.0, 0.25, 0.5, 0.75)):
    """Four Gaussian bumps [4, N] fp32 (the shape of the env's forcing, computed here so that the test owns its F)."""
    x = np.linspace(0.0, L - L / N, N)
    xi = L * np.asarray(Xi)[:, None]
    return (np.exp(-((x[None, :] - xi) ** 2) / (2 * sigma ** 2)) / np.sqrt(2 * np.pi * sigma)).astype(np.float32)


def forcing(N, n_act, random_F=False, seed=11):
    """Forcing matrix [n_act, N] of a case: the four Gaussian actuators, or white noise (any n_act)."""
    if n_act == 4 and not random_F:
        return four_actuators(N)
    assert random_F
    return np.random.RandomState(seed + n_act).uniform(-1, 1, (n_act, N)).astype(np.float32)


def actions(seed, E, n_act):
    return np.random.RandomState(1000 + seed).uniform(-1, 1, (E, n_act)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(N, E, n_act, n_substeps, random_F=False, seed=5):
    """One stepping case, computed once and shared (treat every array as read-only):
    u0, act (None for n_act == 0), F, the twin's (u, ssq), the fp64 numpy reference and the measured deviation of the
    fp32 numpy oracle from it, and the bound the issue derives from them: max(4 x that deviation, 8 ulp of the scale)."""
    dx, dt, nu = params(N)
    u0 = noise(seed + N + E, E, N)
    act = actions(seed + N, E, n_act) if n_act else None
    F = forcing(N, n_act, random_F) if n_act else None
    phi64 = act.astype(np.float64) @ F.astype(np.float64) if n_act else None
    phi32 = act @ F if n_act else None
    ref64, ssq64 = bo.step(u0, phi64, float(dx), float(dt), float(nu), n_substeps, dtype=np.float64)
    np32, _ = bo.step(u0, phi32, dx, dt, nu, n_substeps, dtype=np.float32)
    twin_u, twin_ssq = bo.twin_step(u0, act, F, dx, dt, nu, n_substeps)
    scale = float(np.abs(ref64).max())
    numpy_dev = float(np.abs(np32.astype(np.float64) - ref64).max())
    bound = max(ORDER_FACTOR * numpy_dev, FLOOR_ULPS * EPS * scale)
    out = dict(N=N, E=E, n_act=n_act, n_substeps=n_substeps, dx=dx, dt=dt, nu=nu, u0=u0, act=act, F=F, twin_u=twin_u,
               twin_ssq=twin_ssq, ref64=ref64, ssq64=ssq64, scale=scale, numpy_dev=numpy_dev, bound=bound)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def fp64_distance(got, c):
    """max |got - fp64 reference| of a case, and the same in ulp of the field scale."""
    err = float(np.abs(np.asarray(got, dtype=np.float64) - c["ref64"]).max())
    return err, err / (EPS * c["scale"])


def ssq_rtol(N):
    """ssq_sum against the twin's fp64 sum: each lane sums its P = N / 64 squares by an fp32 fmaf chain of positive terms
    (P roundings, each at most 2^-24 of the running sum, which never exceeds the lane's total); everything after that is
    fp64.  The bound is 2 (P + 1) of those."""
    return 2 * (N // 64 + 1) * 2.0 ** -24


def flip(a):
    """flip(u)[i] = u[(-i) mod N] along the last axis."""
    return np.roll(np.flip(a, axis=-1), 1, axis=-1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bits(got, want, msg=""):
    """Bit equality of two fp32 arrays, with the worst offender in the message."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (msg, got.dtype, got.shape, want.shape)
    bad = bits(got) != bits(want)
    if bad.any():
        idx = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{msg}: {int(bad.sum())} of {bad.size} values differ in bits; first at {idx}: "
                             f"{got[idx]!r} != {want[idx]!r} (max |diff| {np.nanmax(np.abs(got.astype(np.float64) - want)):.3e})")
