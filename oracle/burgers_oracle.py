"""CPU restatement of the reference's ONLY Burgers artefact.  TEST INFRASTRUCTURE ONLY.

The reference ships no Burgers environment (``pdegym/__init__.py:2`` imports a ``pdegym.burgers`` that does not exist)
and no FNO; what it does define is the discretisation, in ``BurgersPhyPDELoss``
(pdecontrol/surrogates/phyloss/phyloss.py:36-86):

    residual(u) = nu * laplace(u) - u * grad(u)                         (:62-81)
      grad    : cross-correlation with [-1/2, 0, 1/2] / dx,             circular   (:39,46-52)
      laplace : cross-correlation with [-1/12, 4/3, -5/2, 4/3, -1/12] / dx^2, circular   (:40,54-60)
    phyevolve(u) = u + dt * residual(u + dt/2 * residual(u))            (:83-86; "improved Euler" = explicit midpoint)

Parity pin: ``residual`` / ``phyevolve`` below are checked against tensors produced by the reference's own class
(oracle/gen_golden.py::burgers_fixtures -> tests/golden/burgers_golden.npz) in tests/test_burgers.py.  Everything
the Burgers ENVIRONMENT adds around this step (forcing, reward, episode logic) has no reference and is
"parity unpinned"; it follows the Kuramoto-Sivashinsky env's conventions.

The second half of this module loads oracle/burgers_oracle.c, the fp32 twin of csrc/burgers.hip: the same operations in
the same order (one rounded fp32 operation or one fmaf each), as flat loops.  The HIP kernels are compared with it bit for
bit (tests/test_burgers_gpu.py); the twin itself is anchored on the CPU against the golden fixtures, against the numpy
functions above run in fp64, and against the two exact symmetries of its arithmetic (tests/test_burgers.py).
"""
import ctypes
import os
import subprocess

import numpy as np

GRAD = (-0.5, 0.0, 0.5)                                  # u_{i-1}, u_i, u_{i+1}
LAPLACE = (-1 / 12, 4 / 3, -5 / 2, 4 / 3, -1 / 12)       # u_{i-2} .. u_{i+2}


def grad(u, dx, dtype=np.float32):
    """2nd-order central first derivative of periodic rows [..., N] (taps in ascending index order)."""
    u = np.asarray(u, dtype=dtype)
    return sum(dtype(c) * np.roll(u, -(k - 1), axis=-1) for k, c in enumerate(GRAD) if c != 0.0) / dtype(dx)


def laplace(u, dx, dtype=np.float32):
    """4th-order central second derivative of periodic rows [..., N]."""
    u = np.asarray(u, dtype=dtype)
    return sum(dtype(c) * np.roll(u, -(k - 2), axis=-1) for k, c in enumerate(LAPLACE)) / dtype(dx ** 2)


def residual(u, dx, nu, phi=None, dtype=np.float32):
    """nu * u_xx - u * u_x (+ phi) for rows of a periodic field [..., N]; computed in ``dtype`` like the reference's
    fp32 torch convolutions."""
    u = np.asarray(u, dtype=dtype)
    r = dtype(nu) * laplace(u, dx, dtype) - u * grad(u, dx, dtype)
    return r if phi is None else r + np.asarray(phi, dtype=dtype)


def evolve(u, dx, dt, nu, phi=None, dtype=np.float32):
    """One explicit-midpoint step (the reference's ``phyevolve``)."""
    u = np.asarray(u, dtype=dtype)
    utilde = u + dtype(0.5) * dtype(dt) * residual(u, dx, nu, phi, dtype)
    return u + dtype(dt) * residual(utilde, dx, nu, phi, dtype)


def step(u, phi, dx, dt, nu, n_substeps, dtype=np.float32):
    """n_substeps midpoint steps with a constant forcing field; returns (u_new, sum over sub-steps of sum_i u_i^2 taken
    BEFORE each update, like the KS env's left-Riemann reward, in fp64)."""
    u = np.array(u, dtype=dtype, copy=True)
    ssq = np.zeros(u.shape[:-1], dtype=np.float64)
    for _ in range(int(n_substeps)):
        ssq += np.sum(u.astype(np.float64) ** 2, axis=-1)
        u = evolve(u, dx, dt, nu, phi, dtype)
    return u, ssq


# --------------------------------------------------------------------------------------------------------------------- #
# fp32 C twin (oracle/burgers_oracle.c): ``twin_*`` reproduce libburgers_hip.so's arithmetic bit for bit
# --------------------------------------------------------------------------------------------------------------------- #
_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "_build", "libburgers_oracle.so")
_lib = None

_dp = ctypes.POINTER(ctypes.c_double)
_fp = ctypes.POINTER(ctypes.c_float)
_cf, _ci = ctypes.c_float, ctypes.c_int


def build(force=False):
    """Compile oracle/burgers_oracle.c with gcc (oracle/Makefile)."""
    if force or not os.path.exists(_LIB_PATH) or (
            os.path.getmtime(_LIB_PATH) < os.path.getmtime(os.path.join(_HERE, "burgers_oracle.c"))):
        subprocess.check_call(["make", "-C", _HERE, "-s"])
    return _LIB_PATH


def lib():
    global _lib
    if _lib is None:
        build()     # also when burgers_oracle.c is newer than the library: never load a stale twin
        L = ctypes.CDLL(_LIB_PATH)
        L.bgo_residual.argtypes = [_fp, _fp, _ci, _ci, _cf, _cf, _fp]
        L.bgo_step.argtypes = [_fp, _fp, _fp, _ci, _ci, _ci, _cf, _cf, _cf, ctypes.c_long, _dp]
        L.bgo_step_states.argtypes = L.bgo_step.argtypes + [_fp]
        for f in (L.bgo_residual, L.bgo_step, L.bgo_step_states):
            f.restype = ctypes.c_int
        _lib = L
    return _lib


def _f(a):
    return None if a is None else a.ctypes.data_as(_fp)


def _rows(a):
    return None if a is None else np.ascontiguousarray(np.atleast_2d(a), dtype=np.float32)


def twin_residual(u, dx, nu, phi=None):
    """u [M, N] fp32 (any N >= 5), phi [M, N] fp32 or None -> residual [M, N] fp32."""
    u, phi = _rows(u), _rows(phi)
    assert phi is None or phi.shape == u.shape
    out = np.empty_like(u)
    rc = lib().bgo_residual(_f(u), _f(phi), u.shape[0], u.shape[1], dx, nu, _f(out))
    assert rc == 0, rc
    return out


def twin_step(u, actions, F, dx, dt, nu, n_substeps, states=False):
    """Advance a copy of u [E, N] fp32 by n_substeps sub-steps.  actions [E, n_act] with F [n_act, N], or actions None
    for no forcing.  Returns (u_new fp32, ssq [E] fp64) and, with ``states``, the state before each sub-step
    [E, n_substeps, N] fp32 as a third value."""
    u = np.array(np.atleast_2d(u), dtype=np.float32, order="C", copy=True)
    E, N = u.shape
    n_act = 0
    if actions is not None:
        actions, F = _rows(actions), _rows(F)
        n_act = F.shape[0]
        assert actions.shape == (E, n_act) and F.shape == (n_act, N)
    else:
        F = None
    ssq = np.zeros(E, dtype=np.float64)
    before = np.empty((E, int(n_substeps), N), dtype=np.float32) if states else None
    rc = lib().bgo_step_states(_f(u), _f(actions), _f(F), n_act, E, N, dx, dt, nu, int(n_substeps),
                               ssq.ctypes.data_as(_dp), _f(before))
    assert rc == 0, rc
    return (u, ssq, before) if states else (u, ssq)


def twin_phyloss(a, dx, dt, nu, substeps):
    """The physics-informed loss forward on a [B, T, N] fp32 through the twin: (loss, diff, states) with
    diff[:, t] = a[:, t] - Phi(a[:, t-1]), diff[:, 0] = a[:, 0] - a[:, T-1] (fp32 subtractions), loss = diff * diff in fp32,
    states [B, T-1, substeps-1, N] = the state before sub-steps 1 .. substeps-1 of every row t <= T-2."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    B, T, N = a.shape
    target = np.empty_like(a)
    target[:, 0] = a[:, T - 1]
    states = np.empty((B, T - 1, substeps - 1, N), dtype=np.float32)
    if T > 1:
        new, _, before = twin_step(a[:, :-1].reshape(-1, N), None, None, dx, dt, nu, substeps, states=True)
        target[:, 1:] = new.reshape(B, T - 1, N)
        states[...] = before.reshape(B, T - 1, substeps, N)[:, :, 1:]
    diff = a - target
    return diff * diff, diff, states
