"""libburgers_hip.so at its C ABI against the fp32 twin oracle/burgers_oracle.c, on an MI355X.

The library is built with -ffp-contract=off and every device operation is one rounded fp32 operation or one explicit fmaf,
so the twin (flat loops, anchored on the CPU in tests/test_burgers.py) must be met BIT FOR BIT: by ``bg_step`` at all five
widths (P = 1 scalar, P = 2 packed scalar, P >= 4 pair-native), by ``bg_phyloss_forward`` (scalar ``midpoint_step``), by
``bg_residual`` (its own wrap logic).  Inputs are white noise (tests/_burgers_cases.py): a swapped halo tap moves one
sub-step by ~9e-5 there, three thousand times the fp32 noise.  Beside the twin, every stepping case is held to the numpy
oracle run in fp64, within 4 x the fp32 numpy oracle's deviation measured for that case (floor 8 ulp of the field scale),
so that a mistake shared by twin and kernel would still show; the observed distances are appended to
burgers_parity_observed.jsonl next to conftest's gradient parity log.  The reference-free tests (translation, mirror,
split launches, repeated launches) need neither.

``ssq_sum`` is compared with the twin's fp64 sum at rtol = 2 (P + 1) 2^-24 (``_burgers_cases.ssq_rtol``).

Every launch here runs on buffers with one padding row past E (NaN, status -7) that must come back untouched.  Tail waves
of the last workgroup redo the last env: what the sentinel guards is that clamp of ``env`` to ``n_envs - 1`` and the row
indexing (``off``, the ``lane == 0`` stores).  It does not guard ``active``: with ``env`` clamped, a store that lost its
``active`` test would rewrite row E - 1 with identical values and never reach row E."""
import json
import os

import numpy as np
import pytest
import torch

import _burgers_cases as bc
from conftest import GRAD_LOG
from hipbind import ptr
from oracle import burgers_oracle as bo

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
OBSERVED = os.path.join(os.path.dirname(GRAD_LOG), "burgers_parity_observed.jsonl")
NAN_BITS = np.uint32(0x7FC00000)
STATUS_SENTINEL = -7


def _record(**rec):
    print("burgers parity", json.dumps(rec))
    try:
        os.makedirs(os.path.dirname(OBSERVED), exist_ok=True)
        with open(OBSERVED, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


@pytest.fixture(scope="module")
def hip():
    from pdegym.burgers import _hip
    _hip.load()
    return _hip


def _stream():
    import ctypes
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(0))


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)    # a copy: shared cases are read-only


def _padded(rows, fill=float("nan"), dtype=torch.float32):
    """A device buffer of ``rows.shape[0] + 1`` rows: the rows (or ``fill`` where rows is a shape), then the sentinel."""
    shape = rows if isinstance(rows, tuple) else rows.shape
    t = torch.full((shape[0] + 1,) + tuple(shape[1:]), fill, dtype=dtype, device=DEV)
    if not isinstance(rows, tuple):
        t[:-1] = _dev(rows)
    return t


def _untouched(t, what):
    last = t[-1].cpu().numpy()
    if last.dtype == np.float32:
        assert (np.atleast_1d(last).view(np.uint32) == NAN_BITS).all(), f"{what}: the padding row was written"
    elif last.dtype == np.float64:
        assert np.isnan(last).all(), f"{what}: the padding row was written"
    else:
        assert (last == STATUS_SENTINEL).all(), f"{what}: the padding row was written"


def step(hip, u0, act, F, dx, dt, nu, n, obs=True, ssq=True, status=True):
    """One bg_step launch on padded buffers; returns the E rows of every output asked for (others None)."""
    E, N = u0.shape
    u = _padded(u0)
    o = _padded((E, N)) if obs else None
    q = _padded((E,), dtype=torch.float64) if ssq else None
    st = _padded((E,), fill=STATUS_SENTINEL, dtype=torch.int32) if status else None
    a, f = _dev(act), _dev(F)
    hip.check(hip.load().bg_step(_stream(), ptr(u), ptr(a), ptr(f), 0 if act is None else act.shape[1], E, N, dx, dt, nu, n,
                                 ptr(o), ptr(q), ptr(st)))
    torch.cuda.synchronize(DEV)
    for t, what in ((u, "u"), (o, "obs"), (q, "ssq_sum"), (st, "status")):
        if t is not None:
            _untouched(t, f"{what} (E = {E}, N = {N})")
    return {k: None if t is None else t[:-1].cpu().numpy() for k, t in (("u", u), ("obs", o), ("ssq", q), ("status", st))}


def step_case(hip, c, **kw):
    return step(hip, c["u0"], c["act"], c["F"], c["dx"], c["dt"], c["nu"], c["n_substeps"], **kw)


def _check_case(hip, c, label):
    """bit for bit against the twin (u, obs), status 0, ssq at the derived rtol, and the fp64 bound measured for the case"""
    r = step_case(hip, c)
    err, ulps = bc.fp64_distance(r["u"], c)
    unit = bc.EPS * c["scale"]
    _record(case=label, N=c["N"], E=c["E"], n_act=c["n_act"], n_substeps=c["n_substeps"],
            numpy_fp32_vs_fp64_ulp=c["numpy_dev"] / unit, kernel_vs_fp64_ulp=ulps, twin_vs_fp64_ulp=bc.fp64_distance(c["twin_u"], c)[1],
            bound_ulp=c["bound"] / unit, kernel_equals_twin=bool(np.array_equal(bc.bits(r["u"]), bc.bits(c["twin_u"]))),
            ssq_rel=float(np.abs(r["ssq"] / c["twin_ssq"] - 1).max()) if c["n_substeps"] else 0.0, ssq_rtol=bc.ssq_rtol(c["N"]))
    bc.assert_bits(r["u"], c["twin_u"], f"{label}: u against the twin")
    bc.assert_bits(r["obs"], c["twin_u"], f"{label}: obs against the twin")
    assert not r["status"].any(), (label, r["status"])
    np.testing.assert_allclose(r["ssq"], c["twin_ssq"], rtol=bc.ssq_rtol(c["N"]), atol=0, err_msg=label)
    assert err <= c["bound"], f"{label}: {ulps:.2f} ulp of scale from fp64, bound {c['bound'] / unit:.2f}"


# ---------------------------------------------------------------------------------------------------------------------
# bit for bit against the twin
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_substeps", [1, 2, 50])
@pytest.mark.parametrize("N", bc.WIDTHS)
def test_step_equals_twin_with_four_actuators(hip, N, n_substeps):
    _check_case(hip, bc.case(N, 37, 4, n_substeps), f"N{N}-E37-act4-n{n_substeps}")


@pytest.mark.parametrize("N", bc.WIDTHS)
def test_step_equals_twin_without_actions(hip, N):
    _check_case(hip, bc.case(N, 5, 0, 3), f"N{N}-E5-noactions-n3")


@pytest.mark.parametrize("E", [1, 4, 5, 37])      # one wave, one full workgroup, one past it, several and a partial last
@pytest.mark.parametrize("N", [64, 128, 256])     # P = 1 scalar, P = 2 packed scalar, P = 4 pair-native
def test_step_equals_twin_over_env_counts(hip, N, E):
    _check_case(hip, bc.case(N, E, 4, 2), f"N{N}-E{E}-act4-n2")


@pytest.mark.parametrize("n_act", [1, 4, 7])
@pytest.mark.parametrize("N", [64, 128, 256])
def test_step_equals_twin_over_actuator_counts(hip, N, n_act):
    _check_case(hip, bc.case(N, 5, n_act, 2, True), f"N{N}-E5-act{n_act}-randomF-n2")


# ---------------------------------------------------------------------------------------------------------------------
# reference-free exactness
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", bc.WIDTHS)
def test_translation_and_mirror_symmetry_on_the_gpu(hip, N):
    """Rolling u and the columns of F rolls the result; (u, F, act) -> (-flip u, flip F, -act) gives -flip(result).  Both are
    exact in the arithmetic, and move every point to another lane, register and pair half.  ssq is held to the derived
    rtol only: rolling changes which squares a lane sums in fp32."""
    c = bc.case(N, 5, 4, 3)
    base = step_case(hip, c)
    for shift in (1, N // 64, N // 2 + 1):
        r = step(hip, np.roll(c["u0"], shift, axis=1), c["act"], np.roll(c["F"], shift, axis=1), c["dx"], c["dt"], c["nu"], 3)
        bc.assert_bits(r["u"], np.roll(base["u"], shift, axis=1), f"N = {N}, roll by {shift}")
        np.testing.assert_allclose(r["ssq"], base["ssq"], rtol=bc.ssq_rtol(N), atol=0)
        assert not r["status"].any()
    r = step(hip, -bc.flip(c["u0"]), -c["act"], bc.flip(c["F"]), c["dx"], c["dt"], c["nu"], 3)
    bc.assert_bits(r["u"], -bc.flip(base["u"]), f"N = {N}, mirror")
    np.testing.assert_allclose(r["ssq"], base["ssq"], rtol=bc.ssq_rtol(N), atol=0)


@pytest.mark.parametrize("N", bc.WIDTHS)
def test_split_and_repeated_launches(hip, N):
    """a then b sub-steps = a + b in one launch (u bit for bit; the fp64 ssq adds come in another order: rtol 1e-12), and
    the same launch twice gives the same bytes."""
    c = bc.case(N, 5, 4, 3)
    args = (c["act"], c["F"], c["dx"], c["dt"], c["nu"])
    whole = step(hip, c["u0"], *args, 5)
    first = step(hip, c["u0"], *args, 2)
    second = step(hip, first["u"], *args, 3)
    bc.assert_bits(second["u"], whole["u"], f"N = {N}: 2 + 3 sub-steps against 5")
    np.testing.assert_allclose(first["ssq"] + second["ssq"], whole["ssq"], rtol=1e-12, atol=0)
    again = step(hip, c["u0"], *args, 5)
    for k in ("u", "obs", "ssq", "status"):
        assert again[k].tobytes() == whole[k].tobytes(), (N, k)


# ---------------------------------------------------------------------------------------------------------------------
# outputs and edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 128, 256])
def test_null_outputs_leave_the_others_unchanged(hip, N):
    c = bc.case(N, 5, 4, 2)
    full = step_case(hip, c)
    bc.assert_bits(full["obs"], full["u"], "obs against u")
    for off in ({"obs"}, {"ssq"}, {"status"}, {"obs", "ssq", "status"}):
        r = step_case(hip, c, **{k: False for k in off})
        for k in ("u", "obs", "ssq", "status"):
            if k in off:
                assert r[k] is None
            else:
                assert r[k].tobytes() == full[k].tobytes(), (N, sorted(off), k)


@pytest.mark.parametrize("N", bc.WIDTHS)
def test_zero_substeps(hip, N):
    c = bc.case(N, 5, 4, 3)
    r = step(hip, c["u0"], c["act"], c["F"], c["dx"], c["dt"], c["nu"], 0)
    bc.assert_bits(r["u"], c["u0"], "u after 0 sub-steps")
    bc.assert_bits(r["obs"], c["u0"], "obs after 0 sub-steps")
    assert (r["ssq"] == 0).all() and (r["status"] == 0).all()


@pytest.mark.parametrize("N", [64, 256])
def test_status_is_per_env(hip, N):
    """env 2 holds one inf, env 4 one NaN: only they are flagged, and the four finite envs do not notice."""
    c = bc.case(N, 6, 4, 2)
    clean = step_case(hip, c)
    u0 = c["u0"].copy()
    u0[2, 7] = np.inf
    u0[4, N - 3] = np.nan
    r = step(hip, u0, c["act"], c["F"], c["dx"], c["dt"], c["nu"], 2)
    assert r["status"].tolist() == [0, 0, 1, 0, 1, 0]
    assert clean["status"].tolist() == [0] * 6
    keep = [0, 1, 3, 5]
    bc.assert_bits(r["u"][keep], clean["u"][keep], "finite envs next to non-finite ones")
    bc.assert_bits(r["obs"][keep], clean["obs"][keep], "finite envs next to non-finite ones (obs)")
    assert r["ssq"][keep].tobytes() == clean["ssq"][keep].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# the loss forward (scalar midpoint_step) against the stepper (packed / pair-native) and against the twin
# ---------------------------------------------------------------------------------------------------------------------
def phyloss_forward(hip, a, dx, dt, nu, substeps):
    """bg_phyloss_forward on padded outputs: loss and diff carry one row past B * T, states one float past its need."""
    B, T, N = a.shape
    need = B * (T - 1) * (substeps - 1) * N
    loss, diff = _padded((B * T, N)), _padded((B * T, N))
    states = torch.full((need + 1,), float("nan"), dtype=torch.float32, device=DEV)
    a_dev = _dev(a)
    hip.check(hip.load().bg_phyloss_forward(_stream(), ptr(a_dev), B, T, N, dx, dt, nu, substeps, ptr(loss), ptr(diff),
                                            ptr(states), need))
    torch.cuda.synchronize(DEV)
    _untouched(loss, "loss")
    _untouched(diff, "diff")
    _untouched(states, "states")
    return (loss[:-1].cpu().numpy().reshape(B, T, N), diff[:-1].cpu().numpy().reshape(B, T, N),
            states[:-1].cpu().numpy().reshape(B, T - 1, substeps - 1, N))


@pytest.mark.parametrize("substeps", [1, 3])
@pytest.mark.parametrize("N", bc.WIDTHS)
def test_loss_forward_steps_like_the_stepper(hip, N, substeps):
    """augmented = [u; 0]: diff[:, 1] = 0 - Phi(u) is exactly -Phi(u) and diff[:, 0] = u - 0 is exactly u.  -diff[:, 1] must
    be the state bg_step leaves without actions: scalar ``midpoint_step<P>`` against the packed / pair-native stepper, no
    tolerance.  (White noise does not produce an exact zero, where 0 - (+0) and -(+0) would differ in sign.)"""
    dx, dt, nu = bc.params(N)
    u = bc.noise(77 + N, 5, N)
    a = np.stack([u, np.zeros_like(u)], axis=1)
    _, diff, _ = phyloss_forward(hip, a, dx, dt, nu, substeps)
    stepped = step(hip, u, None, None, dx, dt, nu, substeps)
    assert not stepped["status"].any() and (stepped["u"] != 0).all()
    bc.assert_bits(diff[:, 0], u, "diff[:, 0] against u")
    bc.assert_bits(-diff[:, 1], stepped["u"], f"N = {N}, {substeps} sub-steps: loss forward against bg_step")


@pytest.mark.parametrize("substeps", [1, 2, 4])
@pytest.mark.parametrize("N", [64, 256, 1024])
@pytest.mark.parametrize("B,T", [(1, 2), (3, 5), (5, 3)], ids=["B1-T2", "B3-T5", "B5-T3"])
def test_loss_forward_equals_twin(hip, B, T, N, substeps):
    dx, dt, nu = bc.params(N)
    a = (0.5 * bc.noise(B + 10 * T + N, B * T, N)).reshape(B, T, N)
    want_loss, want_diff, want_states = bo.twin_phyloss(a, dx, dt, nu, substeps)
    loss, diff, states = phyloss_forward(hip, a, dx, dt, nu, substeps)
    bc.assert_bits(diff, want_diff, "diff")
    bc.assert_bits(loss, want_loss, "loss")
    bc.assert_bits(states, want_states, "states [B, T-1, substeps-1, N]")


@pytest.mark.parametrize("n_rows", [1, 3])
@pytest.mark.parametrize("with_phi", [False, True], ids=["nophi", "phi"])
@pytest.mark.parametrize("N", [5, 7, 100, 512])
def test_residual_hook_equals_twin(hip, N, with_phi, n_rows):
    dx, nu = np.float32(bc.L / N), np.float32(bc.NU)
    u = bc.noise(N + n_rows, n_rows, N)
    phi = bc.noise(N + n_rows + 50, n_rows, N) if with_phi else None
    out = _padded((n_rows, N))
    u_dev, phi_dev = _dev(u), _dev(phi)
    hip.check(hip.load().bg_residual(_stream(), ptr(u_dev), ptr(phi_dev), n_rows, N, dx, nu, ptr(out)))
    torch.cuda.synchronize(DEV)
    _untouched(out, "residual")
    bc.assert_bits(out[:-1].cpu().numpy(), bo.twin_residual(u, dx, nu, phi), f"bg_residual, N = {N}")


# ---------------------------------------------------------------------------------------------------------------------
def test_single_env_is_row_zero_of_the_batch():
    """BurgersEnv (the batch-of-one view) against row 0 of a BurgersBatchedVecEnv seeded the same: reset and two steps."""
    from pdegym.burgers.burgers import BurgersBatchedVecEnv, BurgersEnv
    cfg = dict(N=256, nu=0.02, dt=5e-4)
    one, many = BurgersEnv(**cfg), BurgersBatchedVecEnv(3, **cfg)
    obs1, obsm = one.reset(seed=9), many.reset(seed=9)
    bc.assert_bits(obs1, obsm[0], "reset")
    act = bc.actions(4, 3, 4).reshape(3, 1, 4)
    for k in range(2):
        o1, r1, term1, trunc1, info1 = one.step(act[0])
        om, rm, termm, truncm, infom = many.step(act)
        bc.assert_bits(o1, om[0], f"step {k}")
        assert r1 == rm[0] and term1 == bool(termm[0]) and trunc1 == bool(truncm[0]) and info1["step"] == infom["step"][0] == k + 1
