"""The dissipation objective (objective="", reference pdegym/kuramoto/kuramoto.py:67-73) on the CPU twin (device = -1):
reward -(mean(u_xx^2) + mean(u_x^2) + mean(u*phi)) at the pre-update state of every sub-step, u_x the upwind derivative
of u^2 that rhs returns.  Pinned to the reference's own rhs outputs in the fixture ({tag}_ux / {tag}_uxx) and to the
oracle's rhs evaluated along the oracle's trajectory -- never to the new code itself.

Measured on the twin before these tolerances were set: exact mode <= 2.1e-15 relative everywhere, fast mode <= 2.0e-15
on one state and <= 2.9e-14 after 250 sub-steps (n256), so the fast-mode trajectory tolerance 1e-10 (the l2control fast
test's figure) has a margin of more than 3000x.
"""
import numpy as np
import pytest

from conftest import KS_CONFIGS
from oracle import ks_oracle as ko

DT = 1e-3


@pytest.fixture(scope="module")
def kspde():
    import kspde
    kspde.load()
    return kspde


def _terms(u, phi, dx):
    """mean(u_xx^2) + mean(u_x^2) + mean(u*phi) per row, from the oracle's rhs (the reference's operation order)."""
    _, ux, uxx, _ = ko.rhs(u, phi, dx)
    return (uxx * uxx).mean(1) + (ux * ux).mean(1) + (u * phi.astype(np.float64)).mean(1)


def _trajectory_sums(u0, phi, dx, ns):
    """{n: sum over the first n sub-steps of _terms}, the state advanced one oracle sub-step at a time."""
    tot, u, out = np.zeros(len(u0)), np.array(u0, dtype=np.float64), {}
    for k in range(1, max(ns) + 1):
        tot += _terms(u, phi, dx)
        u = ko.step(u, phi, dx, DT, 1)[0]
        if k in ns:
            out[k] = tot.copy()
    return out


@pytest.mark.parametrize("mode,rtol", [("exact", 1e-13), ("fast", 1e-12)])
@pytest.mark.parametrize("tag", list(KS_CONFIGS))
def test_per_state_pin(kspde, ks_golden, tag, mode, rtol):
    L, N = KS_CONFIGS[tag]
    u, phi = ks_golden[f"{tag}_rhs_u"], ks_golden[f"{tag}_rhs_phi"]
    expected = -((ks_golden[f"{tag}_uxx"] ** 2).mean(1) + (ks_golden[f"{tag}_ux"] ** 2).mean(1)
                 + (u * phi.astype(np.float64)).mean(1))
    s = kspde.KSStepper(len(u), N, L, DT, device=-1, mode=mode)
    s.set_objective("dissipation")
    s.set_state(u)
    _, acc, st = s.step(phi, 1)
    np.testing.assert_allclose(-acc / N, expected, rtol=rtol)
    assert not st.any()


@pytest.mark.parametrize("mode,rtol", [("exact", 1e-12), ("fast", 1e-10)])
@pytest.mark.parametrize("tag", list(KS_CONFIGS))
def test_trajectory_pin(kspde, ks_golden, tag, mode, rtol):
    L, N = KS_CONFIGS[tag]
    u0, phi = ks_golden[f"{tag}_traj_u0"], ks_golden[f"{tag}_phi"]
    ns = (1, 2, 10, 250)
    sums = _trajectory_sums(u0, phi, L / N, ns)
    s = kspde.KSStepper(len(u0), N, L, DT, device=-1, mode=mode)
    s.set_objective("dissipation")
    for n in ns:
        s.set_state(u0)
        _, acc, _ = s.step(phi, n)
        np.testing.assert_allclose(-(acc / N) / n, -sums[n] / n, rtol=rtol, err_msg=f"n={n}")


@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_objective_changes_only_the_accumulator(kspde, ks_golden, mode):
    for tag in ("n64", "n48"):
        L, N = KS_CONFIGS[tag]
        u0, phi = ks_golden[f"{tag}_traj_u0"], ks_golden[f"{tag}_phi"]
        s = kspde.KSStepper(len(u0), N, L, DT, device=-1, mode=mode)
        out = {}
        for obj in ("l2control", "dissipation"):
            s.set_objective(obj)
            s.set_state(u0)
            obs, acc, _ = s.step(phi, 10)
            out[obj] = (s.get_state(), obs, acc)
        np.testing.assert_array_equal(out["l2control"][0], out["dissipation"][0])
        np.testing.assert_array_equal(out["l2control"][1], out["dissipation"][1])
        assert not np.allclose(out["l2control"][2], out["dissipation"][2])


def test_rows_and_device_entries_follow_the_objective(kspde, ks_golden):
    L, N = KS_CONFIGS["n64"]
    u0 = ks_golden["n64_traj_u0"]
    zero = np.zeros_like(u0, dtype=np.float32)
    ids = np.array([5, 0, 3], dtype=np.int32)
    sums = _trajectory_sums(u0[ids], zero[ids], L / N, (7,))
    s = kspde.KSStepper(len(u0), N, L, DT, device=-1, mode="exact")
    s.set_objective("dissipation")
    s.set_state(u0)
    _, acc, _ = s.step_rows(ids, 7)
    np.testing.assert_allclose(acc, sums[7] * N, rtol=1e-12)
    # split form, then the "device" entry (host pointers on the twin)
    s.set_state(u0)
    s.step_begin(None, ids, 7)
    _, acc2, _ = s.step_end()
    np.testing.assert_array_equal(acc2, acc)
    s.set_state(u0)
    acc3 = np.zeros(len(u0))
    s.step_device(d_phi=zero.ctypes.data, n_substeps=7, d_ssq=acc3.ctypes.data)
    np.testing.assert_array_equal(acc3[ids], acc)


def test_reward_rows_matches_reward_func(kspde, ks_golden):
    from pdegym.kuramoto import KuramotoSivashinskyEnv
    L, N = KS_CONFIGS["n64"]
    env = KuramotoSivashinskyEnv(objective="", device="cpu")
    obs = ks_golden["n64_rhs_u"].astype(np.float32)
    phi = ks_golden["n64_rhs_phi"]
    s = kspde.KSStepper(1, N, L, DT, device=-1)
    out = np.zeros(len(obs))
    s.reward_rows_device("dissipation", obs.ctypes.data, phi.ctypes.data, len(obs), out.ctypes.data)
    ref = np.array([float(env.reward_func(o, p)) for o, p in zip(obs, phi)])
    np.testing.assert_allclose(out, ref, rtol=1e-13)
    s.reward_rows_device("l2control", obs.ctypes.data, 0, len(obs), out.ctypes.data)
    np.testing.assert_allclose(out, -(obs.astype(np.float64) ** 2).sum(1) / N, rtol=1e-13)
    with pytest.raises(ValueError):
        s.reward_rows_device("power", obs.ctypes.data, phi.ctypes.data, len(obs), out.ctypes.data)


def test_single_env_step_reward(kspde, ks_golden):
    from pdegym.kuramoto import KuramotoSivashinskyEnv
    cfg_steps = 10
    env = KuramotoSivashinskyEnv(objective="", device="cpu", cfg_steps=cfg_steps, step_mode="exact")
    u0 = ks_golden["n64_traj_u0"][:1]
    action = np.array([[0.3, -0.7, 0.1, 0.9]], dtype=np.float32)
    phi = ko.phi_from_actions(action, env.forcing.forcing.numpy())
    sums = _trajectory_sums(u0, phi, env.dx, (cfg_steps,))
    env.u = u0[0]
    obs, reward, term, trunc, info = env.step(action)
    np.testing.assert_allclose(reward, -sums[cfg_steps][0] / cfg_steps, rtol=1e-12)
    np.testing.assert_array_equal(env.u, ko.step(u0, phi, env.dx, DT, cfg_steps)[0][0])
    assert env.stepper.objective == "dissipation"
    # the burn-in runs the l2control kernels; the next step switches back
    env.reset(seed=1)
    assert env.stepper.objective == "l2control"
    env.step(action)
    assert env.stepper.objective == "dissipation"


def test_batched_env_equals_single_envs_with_autoreset(kspde):
    from pdegym.kuramoto import KuramotoSivashinskyEnv
    from pdegym.kuramoto.batched import KSBatchedVecEnv
    E = 3
    cfg = {"objective": "", "Tmax": 0.03, "cfg_steps": 10}   # 3 steps per episode
    vec = KSBatchedVecEnv(E, config=cfg, device=-1, burn_in=False)
    obs = vec.reset(seed=7)
    singles = []
    for i in range(E):
        s = KuramotoSivashinskyEnv(device="cpu", **cfg)
        s.u = vec.stepper.get_state()[i]
        singles.append(s)
    rs = np.random.RandomState(0)
    for t in range(1, 6):
        actions = rs.uniform(-1, 1, (E, 1, 4)).astype(np.float32)
        o, r, term, trunc, infos = vec.step(actions)
        ref = [s.step(a) for s, a in zip(singles, actions)]
        np.testing.assert_allclose(r, [x[1] for x in ref], rtol=1e-13)
        np.testing.assert_array_equal(trunc, [x[3] for x in ref])
        if trunc.any():
            assert t == 3
            finals = np.stack(list(infos["final_observation"]))
            np.testing.assert_array_equal(finals[:, 0], np.stack([x[0][0] for x in ref]).astype(np.float32))
            fresh = vec.stepper.get_state()
            for i, s in enumerate(singles):    # the singles continue from the vector env's fresh ICs
                s.u = fresh[i]
                s.timestep = 0
        else:
            np.testing.assert_array_equal(o[:, 0], np.stack([x[0][0] for x in ref]).astype(np.float32))
    vec.close()


def test_batched_reward_func_numpy_equals_reward_func(kspde, ks_golden):
    from pdegym.kuramoto import KuramotoSivashinskyEnv
    import torch
    env = KuramotoSivashinskyEnv(objective="", device="cpu")
    obs = ks_golden["n64_rhs_u"].astype(np.float32)[:, None, :]
    phi = ks_golden["n64_rhs_phi"][:, None, :]
    got = env.batched_reward_func(obs, phi)
    assert got.dtype == np.float32 and got.shape == (len(obs),)
    ref = np.array([float(env.reward_func(o, p)) for o, p in zip(obs, phi)])
    np.testing.assert_allclose(got, ref.astype(np.float32), rtol=1e-6)
    got64 = env.batched_reward_func(obs.astype(np.float64), phi)
    np.testing.assert_allclose(got64, ref, rtol=1e-13)
    # actions in place of the field (what the world model hands its reward function)
    actions = np.random.RandomState(2).uniform(-1, 1, (4, 1, 4)).astype(np.float32)
    got_a = env.batched_reward_func(obs[:4].astype(np.float64), actions)
    ref_a = np.array([float(env.reward_func(o, a)) for o, a in zip(obs[:4], actions)])
    np.testing.assert_allclose(got_a, ref_a, rtol=1e-13)
    # torch (host) input: torch output of the input's dtype
    got_t = env.batched_reward_func(torch.from_numpy(obs), torch.from_numpy(phi))
    assert isinstance(got_t, torch.Tensor) and got_t.dtype == torch.float32
    np.testing.assert_allclose(got_t.numpy(), ref.astype(np.float32), rtol=1e-6)


def test_invalid_objective_rejected(kspde):
    s = kspde.KSStepper(2, 64, device=-1)
    with pytest.raises(ValueError):
        s.set_objective("power")
    lib = kspde.load()
    assert lib.ks_set_objective(s._h, 2) == -1
    assert lib.ks_set_objective(s._h, -1) == -1
    assert s.objective == "l2control"
