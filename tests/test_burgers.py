"""f4: viscous-Burgers path.  The reference has no Burgers env; its discretisation is BurgersPhyPDELoss
(pdecontrol/surrogates/phyloss/phyloss.py:36-86).  tests/golden/burgers_golden.npz holds residual() / phyevolve() of
THAT class (oracle/gen_golden.py::burgers_fixtures): the oracle and the HIP kernel are pinned to it at fp32 rounding
(torch's convolution sums its taps in an order we do not restate: a few ulp of the field scale).  Everything the env adds
around the step is "parity unpinned" and checked through properties (order of accuracy, energy decay, determinism).

What pins the kernel's ARITHMETIC is oracle/burgers_oracle.c, an fp32 twin written from the header's order of operations
as flat loops (libburgers_hip.so is built with -ffp-contract=off: every device operation is one rounded fp32 operation or
one explicit fmaf, so the twin can be, and is, compared bit for bit: tests/test_burgers_gpu.py, and
test_kernel_against_oracle_with_forcing_and_reward below through the env).  This file anchors the twin on the CPU:
against the golden fixtures at the bars above; against the numpy oracle run in fp64 on white-noise fields, within 4 x the
deviation of the fp32 numpy oracle measured in the test (never below 8 ulp of the field scale); and against the two exact
symmetries of its arithmetic (translation, and the mirror u -> -flip(u)), bit for bit.  The host refusals of bg_step and
bg_phyloss_forward are checked here too: they return before any device call."""
import ctypes
import os
import sys

import numpy as np
import pytest

import _burgers_cases as bc
from oracle import burgers_oracle as bo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "burgers_golden.npz")
TAGS = ("n512", "n128")


def _close(a, b, ulps=8):
    scale = np.abs(b).max()
    np.testing.assert_allclose(a, b, rtol=0, atol=ulps * np.finfo(np.float32).eps * scale)


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_against_reference_class(tag):
    g = np.load(GOLDEN)
    dx, dt, nu, _ = g[f"{tag}_params"]
    u = g[f"{tag}_u"]
    _close(bo.residual(u, dx, nu), g[f"{tag}_residual"])
    _close(bo.evolve(u, dx, dt, nu), g[f"{tag}_evolve"])
    c = u.copy()
    for _ in range(10):
        c = bo.evolve(c, dx, dt, nu)
    _close(c, g[f"{tag}_evolve10"])


@pytest.mark.parametrize("tag", TAGS)
def test_twin_against_reference_class(tag):
    g = np.load(GOLDEN)
    dx, dt, nu, _ = g[f"{tag}_params"].astype(np.float32)
    u = g[f"{tag}_u"]
    _close(bo.twin_residual(u, dx, nu), g[f"{tag}_residual"])
    _close(bo.twin_step(u, None, None, dx, dt, nu, 1)[0], g[f"{tag}_evolve"])
    _close(bo.twin_step(u, None, None, dx, dt, nu, 10)[0], g[f"{tag}_evolve10"])


@pytest.mark.parametrize("n_act,n_substeps,E", [(4, 1, 37), (4, 2, 37), (4, 50, 37), (0, 3, 5)])
@pytest.mark.parametrize("N", bc.WIDTHS)
def test_twin_against_fp64_on_white_noise(N, n_act, n_substeps, E):
    """The twin is another order of the fp32 numpy oracle's operations (with FMAs): within 4 x the numpy oracle's own
    measured deviation from fp64, floor 8 ulp of the field scale.  Its ssq is the fp64 sum of the fp32 state's squares."""
    c = bc.case(N, E, n_act, n_substeps)
    assert np.isfinite(c["ref64"]).all() and c["scale"] <= 1.1
    err, ulps = bc.fp64_distance(c["twin_u"], c)
    print(f"N={N} n_act={n_act} n={n_substeps}: numpy fp32 {c['numpy_dev'] / (bc.EPS * c['scale']):.2f} ulp, twin {ulps:.2f} ulp, "
          f"bound {c['bound'] / (bc.EPS * c['scale']):.2f} ulp of scale")
    assert err <= c["bound"]
    np.testing.assert_allclose(c["twin_ssq"], c["ssq64"], rtol=1e-6)


def test_twin_states_variant_and_residual_with_phi():
    """The state before sub-step s is what s sub-steps leave; residual with phi is the same chain started from phi."""
    c = bc.case(64, 5, 0, 3)
    u, ssq, before = bo.twin_step(c["u0"], None, None, c["dx"], c["dt"], c["nu"], 3, states=True)
    bc.assert_bits(u, c["twin_u"], "states variant, final state")
    assert np.array_equal(ssq, c["twin_ssq"])
    for s in range(3):
        bc.assert_bits(before[:, s], bo.twin_step(c["u0"], None, None, c["dx"], c["dt"], c["nu"], s)[0], f"state before sub-step {s}")
    for N in (5, 7, 100):
        u, phi = bc.noise(N, 3, N), bc.noise(N + 1, 3, N)
        dx, nu = np.float32(bc.L / N), np.float32(bc.NU)
        for p in (None, phi):
            np.testing.assert_allclose(bo.twin_residual(u, dx, nu, p), bo.residual(u, float(dx), float(nu), p, dtype=np.float64),
                                       rtol=0, atol=8 * bc.EPS * np.abs(bo.residual(u, float(dx), float(nu), p, dtype=np.float64)).max())


@pytest.mark.parametrize("N", bc.WIDTHS)
def test_twin_symmetries_bit_for_bit(N):
    """Rolling u and the columns of F rolls the result; u -> -flip(u), F -> flip(F), act -> -act gives -flip(result):
    both are exact in the twin's arithmetic (a + b is commutative, fmaf(-a, -b, c) = fmaf(a, b, c), negation is exact).
    ssq sums the same N exact fp64 squares in another order: two sequential fp64 sums of N positive terms differ by at
    most 2 (N - 1) 2^-53 of the sum, held here as rtol = N 2^-52."""
    c = bc.case(N, 5, 4, 3)
    dx, dt, nu = c["dx"], c["dt"], c["nu"]
    for shift in (1, N // 64, N // 2 + 1):
        u, ssq = bo.twin_step(np.roll(c["u0"], shift, axis=1), c["act"], np.roll(c["F"], shift, axis=1), dx, dt, nu, 3)
        bc.assert_bits(u, np.roll(c["twin_u"], shift, axis=1), f"roll by {shift}")
        np.testing.assert_allclose(ssq, c["twin_ssq"], rtol=N * 2.0 ** -52)
        r = bo.twin_residual(np.roll(c["u0"], shift, axis=1), dx, nu)
        bc.assert_bits(r, np.roll(bo.twin_residual(c["u0"], dx, nu), shift, axis=1), f"residual, roll by {shift}")
    u, ssq = bo.twin_step(-bc.flip(c["u0"]), -c["act"], bc.flip(c["F"]), dx, dt, nu, 3)
    bc.assert_bits(u, -bc.flip(c["twin_u"]), "mirror")
    np.testing.assert_allclose(ssq, c["twin_ssq"], rtol=N * 2.0 ** -52)


def test_stencil_orders_of_accuracy():
    """grad is 2nd order, laplace 4th order on sin(3x) (fp64 so that truncation, not rounding, is what is measured)."""
    eg, el = [], []
    for N in (32, 64, 128):
        L = 2 * np.pi
        x = np.linspace(0, L, N, endpoint=False)
        u = np.sin(3 * x)
        eg.append(np.abs(bo.grad(u, L / N, np.float64) - 3 * np.cos(3 * x)).max())
        el.append(np.abs(bo.laplace(u, L / N, np.float64) + 9 * np.sin(3 * x)).max())
    assert all(3.7 < a / b < 4.3 for a, b in zip(eg, eg[1:]))          # halving dx: error / 4
    assert all(14.0 < a / b < 18.0 for a, b in zip(el, el[1:]))        # halving dx: error / 16


def test_c_abi_exports_and_python_binding():
    """load() types every row of the binding's table (a missing export raises); that the table is the header's:
    tests/test_capi_symbols.py.  bg_step refuses bad arguments on the host."""
    import ctypes
    from pdegym.burgers import _hip
    lib = _hip.load()
    assert lib.bg_step(None, None, None, None, 0, 0, 0, ctypes.c_float(1), ctypes.c_float(1), ctypes.c_float(1), 0, None, None, None) < 0
    assert b"bad argument" in lib.bg_last_error()


def _host_buffer(n=4096):
    """A host array whose address stands for a device pointer: every refusal below returns before any device call."""
    a = np.zeros(n, dtype=np.float32)
    return a, ctypes.c_void_p(a.ctypes.data)


def test_bg_step_host_refusals_name_the_cause():
    from pdegym.burgers import _hip
    lib = _hip.load()
    keep, p = _host_buffer()
    ok = dict(u=p, actions=None, F=None, n_act=0, E=1, N=64, dx=0.1, dt=1e-3, nu=0.01, n=1)

    def call(**kw):
        a = {**ok, **kw}
        rc = lib.bg_step(None, a["u"], a["actions"], a["F"], a["n_act"], a["E"], a["N"], a["dx"], a["dt"], a["nu"], a["n"],
                         None, None, None)
        return rc, lib.bg_last_error().decode()

    for kw, cause in [(dict(N=100), "N = 100 is not a multiple of 64"),
                      (dict(N=192), "N = 192: supported sizes are 64, 128, 256, 512, 1024"),
                      (dict(dt=0.0), "dt must be positive"),
                      (dict(nu=-0.01), "nu non-negative"),
                      (dict(n=-1), "n_substeps = -1 is negative"),
                      (dict(actions=p, F=None, n_act=4), "actions need the forcing matrix F"),
                      (dict(actions=p, F=p, n_act=0), "n_act > 0")]:
        rc, text = call(**kw)
        assert rc < 0 and text.startswith("bg_step:") and cause in text, (kw, rc, text)
    assert keep.sum() == 0


def test_bg_phyloss_forward_host_refusals_name_the_cause():
    from pdegym.burgers import _hip
    lib = _hip.load()
    keep, p = _host_buffer()

    def call(B=2, T=3, N=64, S=2, loss=p, diff=p, states=p, states_len=1 << 20):
        rc = lib.bg_phyloss_forward(None, p, B, T, N, 0.1, 1e-3, 0.01, S, loss, diff, states, states_len)
        return rc, lib.bg_last_error().decode()

    for kw, cause in [(dict(diff=None), "a state store without diff"),
                      (dict(states=None, states_len=0), "substeps > 1 with diff needs the state store"),
                      (dict(states_len=2 * 2 * 1 * 64 - 1), "holds 255 floats, B (T-1) (substeps-1) N = 256 are needed")]:
        rc, text = call(**kw)
        assert rc < 0 and text.startswith("bg_phyloss_forward:") and cause in text, (kw, rc, text)
    assert keep.sum() == 0


def test_env_registration_without_gpu():
    import pdegym  # noqa: F401
    from pdegym._gym import gym
    env = gym.make("BurgersEnv-v0", new_step_api=True)
    assert env.unwrapped.N == 512 and env.unwrapped.max_episode_steps == 200
    assert env.observation_space.shape == (1, 512) and env.action_space.shape == (1, 4)


# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vec():
    from pdegym.burgers import make_vec
    return make_vec


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_kernel_against_reference_class(vec, tag):
    import torch
    g = np.load(GOLDEN)
    dx, dt, nu, L = g[f"{tag}_params"]
    u = g[f"{tag}_u"]
    env = vec(len(u), config=dict(L=float(L), N=u.shape[1], dt=float(dt), nu=float(nu)))
    _close(env.residual(u).cpu().numpy(), g[f"{tag}_residual"])
    env.u.copy_(torch.from_numpy(u))
    env.step_torch(None, n_substeps=1)
    _close(env.u.cpu().numpy(), g[f"{tag}_evolve"])
    env.u.copy_(torch.from_numpy(u))
    env.step_torch(None, n_substeps=10)
    _close(env.u.cpu().numpy(), g[f"{tag}_evolve10"], ulps=16)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [64, 128, 256, 512, 1024])
def test_kernel_against_oracle_with_forcing_and_reward(vec, N):
    import torch
    E = 37                                    # not a multiple of the 4 envs per workgroup
    env = vec(E, config=dict(N=N, nu=0.02, dt=5e-4 if N < 1024 else 1e-4))
    env.reset(seed=3)
    u0 = env.u.cpu().numpy().copy()
    act = np.random.RandomState(1).uniform(-1, 1, (E, 4)).astype(np.float32)
    # the twin gets the env's own F and the fp32 roundings of its Python-float dx, dt, nu: the binding's conversion is pinned too
    ref, ssq = bo.twin_step(u0, act, env.forcing.forcing.numpy(), np.float32(env.dx), np.float32(env.dt), np.float32(env.nu), 50)
    u, rew = env.step_torch(torch.from_numpy(act).to(env.device))
    bc.assert_bits(u.cpu().numpy(), ref, f"env step at N = {N} against the twin")
    np.testing.assert_allclose(rew.cpu().numpy(), ssq * (-(1.0 / N) / 50), rtol=bc.ssq_rtol(N), atol=0)
    assert int(env._status.sum()) == 0


@pytest.mark.gpu
def test_env_contract_energy_decay_autoreset_and_overflow(vec):
    env = vec(5, config=dict(N=512, Tmax=0.15))            # 3 steps per episode
    obs = env.reset(seed=7)
    again = vec(5, config=dict(N=512, Tmax=0.15)).reset(seed=7)
    np.testing.assert_array_equal(obs, again)               # seeded resets are reproducible
    assert obs.shape == (5, 1, 512) and obs.dtype == np.float32
    energy = [(obs.astype(np.float64) ** 2).sum(axis=(1, 2))]
    for k in range(3):
        obs, rew, term, trunc, infos = env.step(np.zeros((5, 1, 4), np.float32))
        if k < 2:
            energy.append((obs.astype(np.float64) ** 2).sum(axis=(1, 2)))
            assert not trunc.any() and (rew <= 0).all() and rew.dtype == np.float64
    assert all((b <= a * (1 + 1e-6)).all() for a, b in zip(energy, energy[1:]))   # unforced viscous flow loses energy
    assert trunc.all() and infos["_final_observation"].all() and list(infos["step"]) == [3] * 5
    assert all(f.shape == (1, 512) for f in infos["final_observation"]) and (env.timestep == 0).all()
    wild = vec(2, config=dict(N=512, dt=0.5))               # far beyond the explicit stability limit
    wild.reset(seed=0)
    with pytest.raises(FloatingPointError):
        for _ in range(5):
            wild.step(np.ones((2, 1, 4), np.float32))
