"""The dissipation objective on the MI355X: the fused layouts that the four KS_CONFIGS sizes reach (17 of the 40
instantiated ones: row16 at P = 3, 4, 8, 16, half32 at P = 2, 4, 8, wave64 at P = 1, 2, 4) and the LDS kernel against the
reference's rhs outputs in the fixture and the oracle's trajectory (the pins of test_dissipation_host.py), GPU exact against
the CPU twin, the env layers, and the world model's per-row reward kernel.  All 40 layouts, every block size and the
reward kernel's other lane-group widths run against the oracle in test_ks_geometry_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import KS_CONFIGS
from oracle import ks_oracle as ko

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dissipation_host import DT, _trajectory_sums  # noqa: E402
from _ks_geometry import supported as _supported  # noqa: E402  (the table of instantiated layouts)

pytestmark = pytest.mark.gpu

FUSED = ["row16_dpp", "row16_bperm", "wave64_dpp", "wave64_bperm", "half32_bperm", "lds"]
HYBRID = ["wave64_hybrid", "wave64_hybrid1"]
KS_ERR_UNSUPPORTED = -4


@pytest.fixture(scope="module")
def kspde():
    import kspde
    kspde.load()
    return kspde


@pytest.mark.parametrize("variant", FUSED)
@pytest.mark.parametrize("tag", list(KS_CONFIGS))
def test_per_state_trajectory_and_state_pins(kspde, ks_golden, tag, variant):
    L, N = KS_CONFIGS[tag]
    if not _supported(variant, N):
        pytest.skip("layout not instantiated for this N")
    u, phi = ks_golden[f"{tag}_rhs_u"], ks_golden[f"{tag}_rhs_phi"]
    expected = -((ks_golden[f"{tag}_uxx"] ** 2).mean(1) + (ks_golden[f"{tag}_ux"] ** 2).mean(1)
                 + (u * phi.astype(np.float64)).mean(1))
    u0, phi0 = ks_golden[f"{tag}_traj_u0"], ks_golden[f"{tag}_phi"]
    ns = (1, 2, 10, 250)
    sums = _trajectory_sums(u0, phi0, L / N, ns)
    for mode, r_state, r_traj in (("exact", 1e-13, 1e-12), ("fast", 1e-12, 1e-10)):
        s = kspde.KSStepper(len(u), N, L, DT, mode=mode, variant=variant)
        assert s.layout()["variant"] == variant
        s.set_objective("dissipation")
        s.set_state(u)
        _, acc, st = s.step(phi, 1)
        np.testing.assert_allclose(-acc / N, expected, rtol=r_state, err_msg=mode)
        t = kspde.KSStepper(len(u0), N, L, DT, mode=mode, variant=variant)
        for n in ns:
            states = {}
            for obj in ("l2control", "dissipation"):
                t.set_objective(obj)
                t.set_state(u0)
                obs, acc, st = t.step(phi0, n)
                states[obj] = (t.get_state(), obs)
                assert not st.any()
            np.testing.assert_allclose(-(acc / N) / n, -sums[n] / n, rtol=r_traj, err_msg=f"{mode} n={n}")
            # the objective changes only the accumulator
            np.testing.assert_array_equal(states["l2control"][0], states["dissipation"][0])
            np.testing.assert_array_equal(states["l2control"][1], states["dissipation"][1])
            if mode == "exact":
                np.testing.assert_array_equal(states["dissipation"][0], ks_golden[f"{tag}_traj_u{n}"])


@pytest.mark.parametrize("variant", HYBRID)
def test_hybrid_layouts_refuse_dissipation(kspde, ks_golden, variant):
    L, N = KS_CONFIGS["n64"]
    s = kspde.KSStepper(8, N, L, DT, variant=variant)
    s.set_objective("dissipation")
    s.set_state(ks_golden["n64_traj_u0"])
    with pytest.raises(kspde.KSError) as e:
        s.step(ks_golden["n64_phi"], 1)
    assert f"error {KS_ERR_UNSUPPORTED}" in str(e.value)
    # no reward buffer: the l2control kernels run (what a burn-in does)
    s.step_device(n_substeps=3)
    s.sync()


@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_ragged_batch_against_cpu_twin(kspde, mode):
    L, N = KS_CONFIGS["n64"]
    rs = np.random.RandomState(3)
    u0 = rs.uniform(-0.4, 0.4, (37, N))
    phi = rs.uniform(-0.5, 0.5, (37, N)).astype(np.float32)
    cpu = kspde.KSStepper(37, N, L, DT, device=-1, mode=mode)
    cpu.set_objective("dissipation")
    cpu.set_state(u0)
    _, acc_cpu, _ = cpu.step(phi, 25)
    u_cpu = cpu.get_state()
    for variant in FUSED:
        s = kspde.KSStepper(37, N, L, DT, mode=mode, variant=variant)
        s.set_objective("dissipation")
        s.set_state(u0)
        _, acc, _ = s.step(phi, 25)
        if mode == "exact":
            np.testing.assert_array_equal(s.get_state(), u_cpu, err_msg=variant)
            np.testing.assert_allclose(acc, acc_cpu, rtol=1e-13, err_msg=variant)
        else:
            np.testing.assert_allclose(acc, acc_cpu, rtol=1e-12, err_msg=variant)


def test_rows_and_device_entries(kspde, ks_golden):
    L, N = KS_CONFIGS["n64"]
    u0 = ks_golden["n64_traj_u0"]
    ids = np.array([5, 0, 3], dtype=np.int32)
    zero = np.zeros((len(ids), N), np.float32)
    sums = _trajectory_sums(u0[ids], zero, L / N, (7,))
    s = kspde.KSStepper(len(u0), N, L, DT, mode="exact")
    s.set_objective("dissipation")
    s.set_state(u0)
    _, acc, _ = s.step_rows(ids, 7)
    np.testing.assert_allclose(acc, sums[7] * N, rtol=1e-12)
    u_rows = s.get_state()
    s.set_state(u0)
    s.step_begin(None, ids, 7)
    _, acc2, _ = s.step_end()
    np.testing.assert_array_equal(acc2, acc)
    # device-resident entry, subset by device env ids, phi = 0
    dev = torch.device("cuda", 0)
    s.set_state(u0)
    d_ids = torch.from_numpy(ids).to(dev)
    d_ssq = torch.zeros(len(u0), dtype=torch.float64, device=dev)
    s.step_device(d_env_ids=d_ids.data_ptr(), n_rows=len(ids), n_substeps=7, d_ssq=d_ssq.data_ptr())
    s.sync()
    np.testing.assert_array_equal(d_ssq.cpu().numpy()[ids], acc)
    np.testing.assert_array_equal(s.get_state(), u_rows)


def test_sharded_env_equals_batched_env(kspde):
    from pdegym.kuramoto.batched import KSBatchedVecEnv
    from pdegym.kuramoto.sharded import KSShardedVecEnv
    E = 6
    cfg = {"objective": "", "Tmax": 0.03, "cfg_steps": 10}
    kw = dict(burn_in=False, step_mode="exact", reset_mode="exact")
    vec = KSBatchedVecEnv(E, config=dict(cfg), device=0, **kw)
    sh = KSShardedVecEnv(E, config=dict(cfg), devices=[0, 0], **kw)
    np.testing.assert_array_equal(vec.reset(seed=11), sh.reset(seed=11))
    rs = np.random.RandomState(1)
    for _ in range(4):                         # crosses the autoreset after step 3
        a = rs.uniform(-1, 1, (E, 1, 4)).astype(np.float32)
        o1, r1, _, t1, _ = vec.step(a)
        o2, r2, _, t2, _ = sh.step(a)
        np.testing.assert_array_equal(o1, o2)
        np.testing.assert_array_equal(r1, r2)
        np.testing.assert_array_equal(t1, t2)
    vec.close()
    sh.close()


def test_batched_step_torch_matches_host_step(kspde):
    from pdegym.kuramoto.batched import KSBatchedVecEnv
    E = 5
    cfg = {"objective": "", "cfg_steps": 10}
    host = KSBatchedVecEnv(E, config=dict(cfg), device=0, burn_in=False, step_mode="exact", reset_mode="exact")
    dev = KSBatchedVecEnv(E, config=dict(cfg), device=0, burn_in=False, step_mode="exact", reset_mode="exact")
    host.reset(seed=4)
    dev.reset(seed=4)
    a = np.random.RandomState(2).uniform(-1, 1, (E, 1, 4)).astype(np.float32)
    _, r_host, _, _, _ = host.step(a)
    _, r_dev, _, _ = dev.step_torch(torch.from_numpy(a).cuda())
    torch.cuda.synchronize()
    # same accumulator; the two paths scale it by -(1/N)/cfg_steps in different orders (<= 1 ulp apart)
    np.testing.assert_allclose(r_dev.cpu().numpy(), r_host, rtol=1e-15)
    host.close()
    dev.close()


def test_reward_rows_device_matches_dissipation(kspde, ks_golden):
    from pdegym.kuramoto import KuramotoSivashinskyEnv
    for tag in ("n64", "n256", "n48"):
        L, N = KS_CONFIGS[tag]
        env = KuramotoSivashinskyEnv(objective="", L=L, N=N, device=0)
        obs = ks_golden[f"{tag}_rhs_u"].astype(np.float32)
        phi = ks_golden[f"{tag}_rhs_phi"]
        ref = np.array([float(env._dissipation(o, p)) for o, p in zip(obs, phi)])
        d_obs, d_phi = torch.from_numpy(obs).cuda(), torch.from_numpy(phi).cuda()
        s = kspde.KSStepper(1, N, L, DT)
        out = torch.empty(len(obs), dtype=torch.float64, device="cuda")
        s.reward_rows_device("dissipation", d_obs.data_ptr(), d_phi.data_ptr(), len(obs), out.data_ptr())
        s.sync()
        np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-13, err_msg=tag)
        # through the env: fp64 in -> fp64 out, fp32 in -> fp32 out
        got = env.batched_reward_func(d_obs.double(), d_phi)
        assert got.is_cuda and got.dtype == torch.float64
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-13, err_msg=tag)
        got32 = env.batched_reward_func(d_obs[:, None, :], d_phi[:, None, :])
        assert got32.dtype == torch.float32
        np.testing.assert_allclose(got32.cpu().numpy(), ref.astype(np.float32), rtol=1e-6)
        env.close()


def test_world_env_device_resident_dissipation_reward(kspde):
    import _world_scenario as sc
    from test_world_env import namespace
    from pdegym.kuramoto import KuramotoSivashinskyEnv
    M = namespace()
    M.Env = lambda: KuramotoSivashinskyEnv(objective="", device=0)
    seen = []

    to_np = lambda v: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)

    def recording(env):
        def f(obs, act):
            got = env.batched_reward_func(obs, act)
            seen.append((to_np(obs), to_np(act), to_np(got), env))
            return got
        return f

    sc.run(M, device=torch.device("cuda", 0), world_kwargs={"batched_reward_func": recording})
    world = sc.run.last_world
    assert world._dev is not None, "device-resident path did not engage"
    assert len(seen) == 5
    for obs, act, got, env in seen:
        assert got.dtype == np.float32
        host = np.asarray([env.reward_func(o, a) for o, a in zip(obs, act)], dtype=np.float32)
        np.testing.assert_allclose(got, host, rtol=1e-6)
