"""Inputs, references and bounds shared by tests/test_burgers_objective_host.py and tests/test_burgers_objective_gpu.py
(the objective entries of libburgers_hip.so, include/burgers/objective.h).

Fields are the env's SMOOTH initial condition (a four-mode Fourier series of amplitude O(1)), not the white noise of
tests/_burgers_cases.py: on white noise nu * sum G^2 grows like N^2 and buries sum u * phi, on a smooth field both terms
of the dissipation sum stand well above their bounds.  Grid, dt and nu are _burgers_cases.params'."""
import ctypes

import numpy as np

import _burgers_cases as bc
from _rollout_scenario import fma_chain          # the phi chain: one rounded product, one fmaf per further actuator
from oracle import burgers_oracle as bo

U24, U53 = 2.0 ** -24, 2.0 ** -53


def smooth(seed, E, N, modes=4):
    """[E, N] fp32: sum_k a_k / k * sin(k x + p_k), a_k uniform in (-1, 1): ``BurgersBatchedVecEnv._initial``."""
    rs = np.random.RandomState(seed)
    x = np.linspace(0.0, bc.L - bc.L / N, N)
    k = np.arange(1, modes + 1)
    amp = rs.uniform(-1.0, 1.0, (E, modes)) / k
    ph = rs.uniform(0.0, 2 * np.pi, (E, modes))
    return (amp[:, :, None] * np.sin(k[None, :, None] * x[None, None, :] + ph[:, :, None])).sum(1).astype(np.float32)


def inputs(N, E, n_act, seed=31):
    """(u0 [E, N], actions [E, n_act] or None, F [n_act, N] or None): the four Gaussian actuators at n_act = 4, white-noise
    forcing matrices at the other widths.  The seed is the first from 5 on at which |sum u phi| >= 0.01 nu sum G^2 holds in
    every case of both test files (at the earlier ones some row's sum u phi nearly cancels): a property of the fp64
    reference's two terms, read off the reference alone."""
    u0 = smooth(seed + N + E, E, N)
    if not n_act:
        return u0, None, None
    return u0, bc.actions(seed + N, E, n_act), bc.forcing(N, n_act, random_F=n_act != 4)


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_step(lib, u0, act, F, N, n_substeps, objective, nu=None):
    """``bg_step_objective_host`` on a copy of u0: (u, obs, sum fp64 [E], status int32 [E])."""
    dx, dt, nu0 = bc.params(N)
    nu = nu0 if nu is None else np.float32(nu)
    u = np.array(u0, dtype=np.float32, order="C", copy=True)
    E = u.shape[0]
    obs, ssq, status = np.full_like(u, np.nan), np.full(E, np.nan), np.full(E, -1, dtype=np.int32)
    rc = lib.bg_step_objective_host(ptr(u), ptr(act), ptr(F), 0 if act is None else act.shape[1], E, N, dx, dt, nu,
                                    int(n_substeps), ptr(obs), ptr(ssq), ptr(status), objective)
    assert rc == 0, lib.bg_objective_last_error()
    return u, obs, ssq, status


def dissipation_reference(u0, act, F, N, n_substeps, nu=None):
    """(S fp64 [E], bound [E], nu sum G^2 [E], sum u phi [E], sum |u phi| [E]) of the dissipation sum over the C twin's own
    fp32 pre-update states: G = (u[+1] - u[-1]) * (double)half_inv_dx_f, phi the fp32 chain, nu_d = (double)(float)nu, all
    sums in fp64 (numpy's pairwise sum: its error is far inside the bound's last term).  The bound, summed over the
    sub-steps: 2^-24 [(P + 5) nu sum G^2 + (P + 1) sum |u phi|] + 64 * 2^-53 (nu sum G^2 + sum |u phi|) -- two fp32
    roundings in g (each enters G^2 twice), a P-term fmaf chain per lane, the cast, and the fp64 tree."""
    dx, dt, nu0 = bc.params(N)
    nu = nu0 if nu is None else np.float32(nu)
    E, P = u0.shape[0], N // 64
    hid = np.float64(np.float32(0.5) / dx)
    zeros = np.zeros(E)
    if n_substeps == 0:
        return zeros, zeros, zeros, zeros, zeros
    _, _, states = bo.twin_step(u0, act, F, dx, dt, nu, n_substeps, states=True)     # [E, n, N] fp32
    u = states.astype(np.float64)
    G = (np.roll(u, -1, axis=2) - np.roll(u, 1, axis=2)) * hid
    phi = np.zeros((E, N)) if act is None else fma_chain(act, F).astype(np.float64)
    d = np.float64(nu) * (G * G).sum(axis=(1, 2))
    up = u * phi[:, None, :]
    p, pabs = up.sum(axis=(1, 2)), np.abs(up).sum(axis=(1, 2))
    bound = U24 * ((P + 5) * d + (P + 1) * pabs) + 64 * U53 * (d + pabs)
    return d + p, bound, d, p, pabs


def row_reward_numpy(u, phi, dx, nu):
    """The row reward of include/burgers/objective.h in numpy, every row summed in index order: fp64 [M]."""
    u = np.asarray(u, dtype=np.float32).astype(np.float64)
    p = np.asarray(phi, dtype=np.float32).astype(np.float64)
    M, N = u.shape
    ux = (np.roll(u, -1, axis=1) - np.roll(u, 1, axis=1)) / (2.0 * dx)
    sd, sp = np.zeros(M), np.zeros(M)
    for i in range(N):
        sd = sd + ux[:, i] * ux[:, i]
        sp = sp + u[:, i] * p[:, i]
    return (-1.0) * (np.float64(np.float32(nu)) * (sd / N) + sp / N)


def row_reward_terms(u, phi, dx, nu):
    """(nu <ux^2>, <|u phi|>) fp64 [M]: the scales the tolerances of the row rewards are written in."""
    u = np.asarray(u, dtype=np.float32).astype(np.float64)
    p = np.asarray(phi, dtype=np.float32).astype(np.float64)
    ux = (np.roll(u, -1, axis=1) - np.roll(u, 1, axis=1)) / (2.0 * dx)
    return np.float64(np.float32(nu)) * (ux * ux).mean(axis=1), np.abs(u * p).mean(axis=1)
