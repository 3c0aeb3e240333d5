"""Shared pieces of the KS stepper geometry tests (test_ks_geometry_host.py, test_ks_geometry_gpu.py): the table of
instantiated layouts, the inputs, the oracle references and the recorder of what was observed.

Reference: oracle.ks_oracle (the C restatement test_oracle_ks.py ties to the reference's recorded vectors); for the
dissipation accumulator the oracle's rhs along the oracle's trajectory (_trajectory_sums of test_dissipation_host.py).

Tolerances are the project's contract (test_ks_gpu_parity.py, test_dissipation_gpu.py):
  exact mode  state and fp32 obs bit-equal, l2 accumulator rtol 1e-13, dissipation accumulator rtol 1e-12
  fast mode   state L_inf <= 1e-12 after one sub-step and <= 1e-11 after 20 (and after 5, the LDS range test); three
              sub-steps get 3e-12, the per-sub-step bound added up; accumulators rtol 1e-10; state and fp32 obs bit-equal
              to the CPU twin's (device = -1): every fast-mode form runs the same IEEE fp64 operations per accumulator in
              the same order (csrc/ks_internal.h fast_point, rhs_tile_fast, rhs_hybrid_fast), only the reward sums are
              reduced in another order
  both        state and obs bit-identical under the two objectives, status all 0
"""
import functools
import json
import math
import os
import sys

import numpy as np

from oracle import ks_oracle as ko

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import GRAD_LOG  # noqa: E402
from test_dissipation_host import _trajectory_sums  # noqa: E402

# beside the suite's other records of what was observed (conftest.check_grads)
OBSERVED = os.path.join(os.path.dirname(GRAD_LOG), "ks_geometry_observed.jsonl")

DT = 1e-3
L_PER_POINT = 0.34375                       # L = 22 at N = 64, as every KS_CONFIGS entry
KS_ERR_UNSUPPORTED = -4
SENTINEL, OBS_SENTINEL, STATUS_SENTINEL = -12345.678, -777.0, 0x5A5A

# ---- the layout table: what csrc/ks_kernels.hip instantiates -------------------------------------------------------
POINTS_PER_LANE = (1, 2, 3, 4, 6, 8, 12, 16)
LANES = {"row16_dpp": 16, "row16_bperm": 16, "half32_bperm": 32, "wave64_dpp": 64, "wave64_bperm": 64}
HYBRID = ("wave64_hybrid", "wave64_hybrid1")                        # N = 64 only: one point per lane, no dissipation form
FUSED = tuple(LANES)
LDS_N = (9, 2048)                           # the LDS kernel's range, both ends included
VARIANTS = FUSED + ("lds",) + HYBRID

#: every (variant, points per lane) pair with a fused instantiation: 5 families x 8 P = 40, and the two hybrids at P = 1
LAYOUT_TABLE = frozenset([(v, p) for v in FUSED for p in POINTS_PER_LANE] + [(v, 1) for v in HYBRID])

#: section 1's sizes: together they reach every pair of LAYOUT_TABLE
MATRIX_N = (16, 32, 48, 64, 96, 128, 192, 256, 384, 512, 768, 1024)
BLOCKS = (0, 64, 128, 256)


def lanes_of(variant):
    """Lanes per env of a variant (0 for the LDS kernel, which has no per-lane layout)."""
    if variant in HYBRID:
        return 64
    return LANES.get(variant, 0)


def supported(variant, N):
    """Does ``variant`` have an instantiated kernel for grid size N?  (ks::layout_supported restated.)"""
    if variant in HYBRID:
        return N == 64
    G = lanes_of(variant)
    if not G:
        return LDS_N[0] <= N <= LDS_N[1]
    return N % G == 0 and (N // G) in POINTS_PER_LANE


def expected_layout(variant, N, E, block):
    """What KSStepper.layout() must report for E envs (E small: the default block is one wave, or the LDS kernel's pick
    by N)."""
    G = lanes_of(variant)
    if not G:
        b = block or (64 if N <= 64 else (128 if N <= 128 else 256))
        return {"variant": variant, "lanes_per_env": 0, "points_per_lane": 0, "block": b, "grid": E}
    b = block or 64
    waves = -(-E // (64 // G))
    return {"variant": variant, "lanes_per_env": G, "points_per_lane": N // G, "block": b, "grid": -(-waves // (b // 64))}


# ---- inputs and references -----------------------------------------------------------------------------------------
def length_of(N):
    return L_PER_POINT * N


@functools.lru_cache(maxsize=None)
def inputs(N, E):
    """(u0 [E, N] f64, phi [E, N] f32, actions [E, 4] f32), drawn in this order from RandomState(N)."""
    rs = np.random.RandomState(N)
    u0 = rs.uniform(-0.4, 0.4, (E, N))
    phi = rs.uniform(-0.5, 0.5, (E, N)).astype(np.float32)
    actions = rs.uniform(-1, 1, (E, 4)).astype(np.float32)
    for a in (u0, phi, actions):
        a.setflags(write=False)
    return u0, phi, actions


def reference(u0, phi, N, ns):
    """{n: (state, l2 accumulator, dissipation accumulator)} from the oracle, for the sub-step counts ``ns``."""
    dx = length_of(N) / N
    diss = _trajectory_sums(u0, phi, dx, tuple(ns))
    out = {}
    for n in ns:
        u, _, ssq, st = ko.step(u0, phi, dx, DT, n)
        assert not st.any() and np.isfinite(u).all(), (N, n)
        out[n] = (u, ssq, diss[n] * N)
    return out


@functools.lru_cache(maxsize=None)
def case(N, E, ns):
    """The usual draw at (N, E) and its oracle references, computed once and shared (read-only)."""
    u0, phi, _ = inputs(N, E)
    ref = reference(u0, phi, N, ns)
    for n in ns:
        for a in ref[n]:
            a.setflags(write=False)
    return u0, phi, ref


FAST_STATE_TOL = {1: 1e-12, 3: 3e-12, 5: 1e-11, 20: 1e-11}
ACC_RTOL = {("exact", "l2control"): 1e-13, ("exact", "dissipation"): 1e-12,
            ("fast", "l2control"): 1e-10, ("fast", "dissipation"): 1e-10}


@functools.lru_cache(maxsize=None)
def _twin(E, N, dt):
    """The CPU twin (device = -1) at this geometry: what every layout's fast-mode state is bit-equal to."""
    import kspde
    return kspde.KSStepper(E, N, length_of(N), dt, device=-1, mode="fast")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _rel(got, ref):
    """max |got - ref| / |ref| (absolute where the reference is exactly 0)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    den = np.where(ref == 0.0, 1.0, np.abs(ref))
    return float((np.abs(got - ref) / den).max())


def check_steps(s, u0, phi, ref, mode, objectives=("l2control", "dissipation"), label=""):
    """Runs ``s`` (already on the variant and block under test) from u0 under ``phi`` for every n of ``ref`` and every
    objective, and asserts the contract of the module docstring.  Returns the observed maxima
    {"state": L_inf, "l2control": rel, "dissipation": rel}."""
    s.set_mode(mode)
    seen = {"state": 0.0}
    for n, (u_ref, l2_ref, diss_ref) in ref.items():
        first = None
        for obj in objectives:
            msg = f"{label} {mode} {obj} n={n}"
            s.set_objective(obj)
            s.set_state(u0)
            obs, acc, st = s.step(phi, n)
            u = s.get_state()
            assert not st.any(), msg
            np.testing.assert_array_equal(obs, u.astype(np.float32), err_msg=msg)
            if mode == "exact":
                np.testing.assert_array_equal(u, u_ref, err_msg=msg)
            else:
                err = float(np.abs(u - u_ref).max())
                seen["state"] = max(seen["state"], err)
                assert err <= FAST_STATE_TOL[n], (msg, err)
                twin = _twin(len(u0), u0.shape[1], DT)
                twin.set_objective(obj)
                twin.set_state(u0)
                obs_t, _, _ = twin.step(phi, n)
                np.testing.assert_array_equal(_bits(u), _bits(twin.get_state()), err_msg=msg + " state bits vs the twin")
                np.testing.assert_array_equal(_bits(obs), _bits(obs_t), err_msg=msg + " obs bits vs the twin")
            acc_ref = l2_ref if obj == "l2control" else diss_ref
            seen[obj] = max(seen.get(obj, 0.0), _rel(acc, acc_ref))
            np.testing.assert_allclose(acc, acc_ref, rtol=ACC_RTOL[mode, obj], atol=0, err_msg=msg)
            if first is None:
                first = (u, obs)
            else:   # the objective changes only the accumulator
                np.testing.assert_array_equal(u, first[0], err_msg=msg)
                np.testing.assert_array_equal(obs, first[1], err_msg=msg)
    return seen


def record(**rec):
    """Print what was observed and append it to OBSERVED (ks_geometry_observed.jsonl)."""
    print("ks geometry", json.dumps(rec))
    try:
        os.makedirs(os.path.dirname(OBSERVED), exist_ok=True)
        with open(OBSERVED, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


# ---- entries per layout: actions @ F in the kernel, subset stepping -------------------------------------------------
ENTRY_SUBSTEPS = 10


def subset_envs(N):
    return 37 if N <= 256 else 11


def subset_ids(E):
    return np.array([E - 1, 0, 5, 3, 9], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def actions_case(N, E):
    """(u0, actions, F, phi = actions @ F as the oracle's fp32 fma chain, the oracle's state after ENTRY_SUBSTEPS)."""
    u0, _, actions = inputs(N, E)
    F = ko.forcing_matrix(length_of(N), N)
    phi = ko.phi_from_actions(actions, F)
    ref = ko.step(u0, phi, length_of(N) / N, DT, ENTRY_SUBSTEPS)[0]
    for a in (F, phi, ref):
        a.setflags(write=False)
    return u0, actions, F, phi, ref


@functools.lru_cache(maxsize=None)
def subset_case(N):
    """(u0 [E, N], ids, the oracle's rows and l2 accumulator after ENTRY_SUBSTEPS with phi = 0)."""
    E = subset_envs(N)
    u0, _, _ = inputs(N, E)
    ids = subset_ids(E)
    rows, _, ssq, st = ko.step(u0[ids], np.zeros((len(ids), N), np.float32), length_of(N) / N, DT, ENTRY_SUBSTEPS)
    assert not st.any()
    for a in (ids, rows, ssq):
        a.setflags(write=False)
    return u0, ids, rows, ssq


def check_actions_path(s, N, E, label=""):
    """In-kernel phi = actions @ F (F indexed by the lane's points) against the phi path and the oracle, exact mode."""
    u0, actions, F, phi, ref = actions_case(N, E)
    s.set_mode("exact")
    s.set_objective("l2control")
    s.set_forcing(F)
    s.set_state(u0)
    _, ssq_a, st = s.step_actions(actions, ENTRY_SUBSTEPS)
    ua = s.get_state()
    assert not st.any(), label
    s.set_state(u0)
    _, ssq_p, _ = s.step(phi, ENTRY_SUBSTEPS)
    np.testing.assert_array_equal(ua, s.get_state(), err_msg=label)
    np.testing.assert_array_equal(ssq_a, ssq_p, err_msg=label)
    np.testing.assert_array_equal(ua, ref, err_msg=label)
    # fast mode: the in-kernel phi feeds the same operations as the twin's, state and fp32 obs bit for bit
    twin = _twin(E, N, DT)
    twin.set_objective("l2control")
    twin.set_forcing(F)
    twin.set_state(u0)
    obs_t, _, _ = twin.step_actions(actions, ENTRY_SUBSTEPS)
    s.set_mode("fast")
    s.set_state(u0)
    obs_f, _, st = s.step_actions(actions, ENTRY_SUBSTEPS)
    assert not st.any(), label
    np.testing.assert_array_equal(_bits(s.get_state()), _bits(twin.get_state()), err_msg=label + " fast state bits vs the twin")
    np.testing.assert_array_equal(_bits(obs_f), _bits(obs_t), err_msg=label + " fast obs bits vs the twin")


def check_step_rows(s, N, label=""):
    """step_rows on [E-1, 0, 5, 3, 9]: the listed rows follow the oracle, the others stay, outputs in list order."""
    u0, ids, rows, ssq_ref = subset_case(N)
    s.set_mode("exact")
    s.set_objective("l2control")
    s.set_state(u0)
    obs, ssq, st = s.step_rows(ids, ENTRY_SUBSTEPS)
    u = s.get_state()
    np.testing.assert_array_equal(u[ids], rows, err_msg=label)
    rest = np.ones(len(u0), bool)
    rest[ids] = False
    np.testing.assert_array_equal(u[rest], u0[rest], err_msg=label)
    np.testing.assert_array_equal(obs, rows.astype(np.float32), err_msg=label)
    np.testing.assert_allclose(ssq, ssq_ref, rtol=1e-13, atol=0, err_msg=label)
    assert not st.any(), label


def check_step_device_subset(s, N, to_device, to_host, label=""):
    """The same subset through step_device: outputs indexed by env id, the untouched entries keep their sentinel.
    ``to_device(array)`` -> (holder, pointer), ``to_host(holder)`` -> array (torch on the GPU, numpy on the CPU twin)."""
    u0, ids, rows, ssq_ref = subset_case(N)
    E = len(u0)
    s.set_mode("exact")
    s.set_objective("l2control")
    s.set_state(u0)
    d_ids, p_ids = to_device(ids)
    d_obs, p_obs = to_device(np.full((E, N), OBS_SENTINEL, np.float32))
    d_ssq, p_ssq = to_device(np.full(E, SENTINEL, np.float64))
    d_st, p_st = to_device(np.full(E, STATUS_SENTINEL, np.int32))
    s.step_device(d_env_ids=p_ids, n_rows=len(ids), n_substeps=ENTRY_SUBSTEPS, d_obs=p_obs, d_ssq=p_ssq, d_status=p_st)
    s.sync()
    obs, ssq, st = to_host(d_obs), to_host(d_ssq), to_host(d_st)
    u = s.get_state()
    rest = np.ones(E, bool)
    rest[ids] = False
    np.testing.assert_array_equal(u[ids], rows, err_msg=label)
    np.testing.assert_array_equal(u[rest], u0[rest], err_msg=label)
    np.testing.assert_array_equal(obs[ids], rows.astype(np.float32), err_msg=label)
    np.testing.assert_allclose(ssq[ids], ssq_ref, rtol=1e-13, atol=0, err_msg=label)
    assert not st[ids].any(), label
    assert (obs[rest] == np.float32(OBS_SENTINEL)).all(), f"{label}: obs of an unlisted env was written"
    assert (ssq[rest] == SENTINEL).all(), f"{label}: ssq of an unlisted env was written"
    assert (st[rest] == STATUS_SENTINEL).all(), f"{label}: status of an unlisted env was written"


def host_buffers():
    """(to_device, to_host) for the CPU twin: "device" pointers are host pointers."""
    def to_device(a):
        a = np.array(a, copy=True)
        return a, a.ctypes.data
    return to_device, lambda a: a


# ---- zeros under the upwind switch ---------------------------------------------------------------------------------
ZERO_N = (64, 48)
ZERO_ROWS = (2, 3)       # the rows that are zero everywhere


@functools.lru_cache(maxsize=None)
def zero_case(N, zero_rows_forced, ns=(1, 3)):
    """Six rows with zeros of both signs where the upwind switch reads them (u == 0 selects the backward stencil), the
    rest the usual draw.  Rows 2 / 3 are +0.0 / -0.0 everywhere; with ``zero_rows_forced`` False their phi is 0 as well
    and they must stay exactly zero."""
    u0, phi, _ = inputs(N, 6)
    u0, phi = u0.copy(), phi.copy()
    u0[0, ::5] = 0.0
    u0[1, ::3] = -0.0
    u0[2, :] = 0.0
    u0[3, :] = -0.0
    u0[4, [0, N - 1]] = 0.0
    u0[5, [0, N - 1]] = -0.0
    if not zero_rows_forced:
        phi[list(ZERO_ROWS)] = 0.0
    ref = reference(u0, phi, N, ns)
    if not zero_rows_forced:
        for n in ns:
            assert not ref[n][0][list(ZERO_ROWS)].any()
    for a in (u0, phi) + tuple(x for n in ns for x in ref[n]):
        a.setflags(write=False)
    return u0, phi, ref


def check_zero_rows_stay_zero(s, u0, phi, mode, label=""):
    """With phi = 0 the all-zero rows stay exactly zero, in either mode."""
    s.set_mode(mode)
    for n in (1, 3):
        s.set_state(u0)
        obs, _, st = s.step(phi, n)
        u = s.get_state()
        rows = list(ZERO_ROWS)
        assert not st.any()
        assert not u[rows].any() and not obs[rows].any(), f"{label} {mode} n={n}: a zero state moved"


# ---- per-row reward ------------------------------------------------------------------------------------------------
REWARD_N = (9, 50, 64, 65, 100, 333, 512, 513, 1000, 2048)
REWARD_ROWS = (1, 5, 37)


@functools.lru_cache(maxsize=None)
def reward_case(N, n_rows):
    """obs / phi fp32 uniform(-1, 1) and, for (objective, phi given), the fsum reference with its bound.

    Bound (absolute): (N + 16) * 2^-53 * sum|terms| / N.  The kernel forms every per-point term exactly as the oracle's
    rhs does, so only the order of the N fp64 additions differs: any order errs by at most (N - 1) u sum|t|; the extra
    16 covers the three divisions by N (or the rounded 1 / N) and the final additions."""
    rs = np.random.RandomState(N)
    obs = rs.uniform(-1, 1, (n_rows, N)).astype(np.float32)
    phi = rs.uniform(-1, 1, (n_rows, N)).astype(np.float32)
    u = obs.astype(np.float64)
    dx = length_of(N) / N
    _, ux, uxx, _ = ko.rhs(u, phi, dx)
    out = {}
    for with_phi in (True, False):
        up = u * phi.astype(np.float64) if with_phi else np.zeros_like(u)
        terms = np.concatenate([uxx * uxx, ux * ux, up], axis=1)
        out["dissipation", with_phi] = terms
        out["l2control", with_phi] = u * u
    refs = {}
    for key, terms in out.items():
        ref = np.array([-math.fsum(row) / N for row in terms])
        bound = np.array([(N + 16) * 2.0 ** -53 * math.fsum(np.abs(row)) / N for row in terms])
        refs[key] = (ref, bound)
    for a in (obs, phi):
        a.setflags(write=False)
    return obs, phi, refs
