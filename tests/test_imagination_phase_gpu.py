"""The imagined-rollout phase on the GPU: the two kernels of csrc/rollout.hip alone against the host wrappers, the kernel
tier of ``imagine`` against the per-step loop of ``Worker.rollout`` on the same GPU, and against the arrays recorded from
the reference (tests/golden/rollout_golden.npz)."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rollout_scenario as sc  # noqa: E402
from _rollout_scenario import fma_chain, host_matmul_is_fma_chain  # noqa: E402
from conftest import GOLDEN  # noqa: E402
from test_capi_symbols import LIBDIR, declared_functions  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1, 5, 257)                     # one wave, a partial workgroup, more than one workgroup with a partial last one
DEVICE_REWARD = {"batched_reward_func": lambda env: env.batched_reward_func}


def test_rollout_library_exports_what_its_header_declares():
    """(that the binding's table holds exactly these names and the library exports them: tests/test_capi_symbols.py,
    which skips without the library where this test fails)"""
    assert declared_functions("rollout_hip.h", "ro") == ["ro_act_chain", "ro_last_error", "ro_settle", "ro_supported"]
    assert os.path.exists(os.path.join(LIBDIR, "librollout_hip.so")), "librollout_hip.so not built (run __graft_entry__.build())"


def test_rollout_geometry_refusals_are_numbered():
    from pdecontrol.mbrl import rollout_hip as ro
    lib = ro.load()
    good = dict(B=4, T=3, N=64, A=4, L=64, act_start=0, act_stride=1, obs_start=0, obs_stride=1, members=2)
    assert ro.supported(ro.Geometry(**good)) is None
    for code, change in ((-2, dict(B=0)), (-3, dict(T=0)), (-4, dict(N=8)), (-4, dict(N=1028)), (-5, dict(A=17)),
                         (-6, dict(L=0)), (-7, dict(act_stride=0)), (-7, dict(act_start=64)), (-8, dict(obs_stride=0)),
                         (-8, dict(obs_start=64)), (-9, dict(members=9)), (-9, dict(members=0))):
        g = ro.Geometry(**{**good, **change})
        assert lib.ro_supported(ctypes.byref(g)) == code, change
        assert ro.last_error().startswith("rollout:")
    assert lib.ro_supported(None) == -1
    for N in (16, 100, 1024):
        assert ro.supported(ro.Geometry(**{**good, "N": N})) is None


def _act_case(N, A, stride, with_in, with_out):
    """Transforms of one action chain: ascaling (inverse of a frozen [lo, hi] -> [-1, 1] scaling), forcing over A
    actuators, a frozen per-column scaling of the forcing, the sensor."""
    from pdegym.common import transforms as T
    L = 22.0 * N / 64
    x = np.linspace(0.0, L - L / N, N, dtype=np.float32)
    forcing = T.GaussianForcing(x, np.linspace(0.0, 1.0, A, endpoint=False), 0.4, L, N)
    rs = np.random.RandomState(N + A)
    lo = rs.uniform(-2.0, -1.0, (1, 1, A)).astype(np.float32)
    hi = rs.uniform(1.0, 2.0, (1, 1, A)).astype(np.float32)
    chain = []
    if with_in:
        chain.append(T.ScaleTransform(bounds=(lo, hi), aggregate=False, frozen=True, batched=True).Inverse)
    chain.append(T.BatchTransform(forcing))
    if with_out:
        flo = rs.uniform(-3.0, -1.0, (1, N)).astype(np.float32)
        fhi = rs.uniform(1.0, 3.0, (1, N)).astype(np.float32)
        chain.append(T.BatchTransform(T.ScaleTransform(bounds=(flo, fhi), scale=(-1, 1), frozen=True)))
    chain.append(T.BatchTransform(T.SensorTransform(stride=stride)))
    return chain, forcing


@pytest.mark.gpu
@pytest.mark.parametrize("N,A,stride", [(64, 4, 1), (100, 1, 1), (256, 16, 4), (98, 4, 1)])
def test_ro_act_chain_equals_the_host_wrappers(N, A, stride):
    """World action rows and the raw-action record, bit for bit, with and without each affine map.  The kernel's forcing
    product is compared with the fma chain on every host, and with the host wrappers' matmul where that forms the same
    chain (an Intel MKL; tests/conftest.py::require_fma_sgemm says why other hosts round it differently); a host where it
    does not is reported with a TOLERANT MODE warning.  N = 98 (no multiple of 4) and stride 4 take the scalar path."""
    from pdecontrol.mbrl import rollout_hip as ro
    from pdecontrol.mbrl.recognition import field_map
    from pdegym.common import transforms as T
    dev = torch.device("cuda", 0)
    ro.load()
    tolerant = []
    for with_in in (False, True):
        for with_out in (False, True):
            chain, forcing = _act_case(N, A, stride, with_in, with_out)
            split = next(i for i, t in enumerate(chain) if getattr(t, "transform", None) is forcing)
            act_in, act_out = field_map(T.Operation(chain[:split]), A), field_map(T.Operation(chain[split + 1:]), N)
            F = forcing.forcing.numpy()
            for B in BATCHES:
                actions = np.random.RandomState(B).uniform(-1, 1, (B, 1, A)).astype(np.float32)
                host = actions
                for t in chain:
                    host = t(host)
                twin = act_out.apply_numpy(fma_chain(act_in.apply_numpy(actions), F))
                if host_matmul_is_fma_chain(F, act_in.apply_numpy(actions)):
                    np.testing.assert_array_equal(twin, host)
                else:
                    tolerant.append((with_in, with_out, B))
                T_slots, t_now = 3, 1
                g = ro.Geometry(B, T_slots, N, A, N, act_out.start, act_out.stride, 0, 1, 1)
                W = act_out.width
                d = lambda a: None if a is None else torch.as_tensor(a).to(dev).contiguous()
                record = torch.full((T_slots, B, A), 7.0, device=dev)
                out = torch.full((B, W), 7.0, device=dev)
                step = torch.tensor([5, t_now], dtype=torch.int32, device=dev)
                keep = (d(actions.reshape(B, A)), d(act_in.coef), d(F), d(act_out.coef))
                ro.act_chain(ro.stream(), g, ro.act_args(keep[0], record, keep[1], keep[2], keep[3], out, step))
                torch.cuda.synchronize()
                tag = (with_in, with_out, B)
                np.testing.assert_array_equal(out.cpu().numpy(), twin.reshape(B, W), err_msg=str(tag))
                assert host.shape == (B, 1, W)
                np.testing.assert_array_equal(record[t_now].cpu().numpy(), actions.reshape(B, A), err_msg=str(tag))
                assert bool((record[[0, 2]] == 7.0).all()), "a slot of another step was written"
                assert step.tolist() == [t_now, t_now]
    if tolerant:
        warnings.warn(f"TOLERANT MODE: this host's CPU matmul is not the fma chain for {len(tolerant)} of 12 cases "
                      f"{tolerant}; there the kernel was compared with the fma-chain twin only, not with the host wrappers")


@pytest.mark.gpu
@pytest.mark.parametrize("N,obs_stride", [(64, 1), (100, 1), (256, 4), (64, 4), (98, 1), (98, 3)])
def test_ro_settle_picks_records_and_rewards(N, obs_stride):
    """N = 98 is no multiple of 4 and takes the scalar path, the others the float4 path.
    Three members: state, trajectory slot, agent observations and steps exact, the counter advanced, and the reward
    within 2^-23 relative of the fp64 host value of (-1.0) * (1.0 / N) * sum(w^2) (one fp32 rounding of the result plus
    the reordering of an fp64 sum of at most 1024 non-negative terms, which is below 2^-43)."""
    from pdecontrol.mbrl import rollout_hip as ro
    from pdecontrol.mbrl.recognition import field_map
    from pdegym.common import transforms as T
    dev = torch.device("cuda", 0)
    ro.load()
    scale = T.ScaleTransform(bounds=(np.full((1, 1, 1), -3.0, np.float32), np.full((1, 1, 1), 3.0, np.float32)),
                             batched=True, aggregate=True, frozen=True)
    for reward_map in (field_map(scale.Inverse, N), field_map(None, N)):
        sensor = field_map(T.SensorTransform(obs_stride), N)
        for B in BATCHES:
            rs = np.random.RandomState(N + B)
            members = rs.uniform(-1, 1, (3, B, N)).astype(np.float32)
            T_slots, t_now = 4, 2
            chosen = rs.randint(0, 3, (T_slots, B)).astype(np.int32)
            steps0 = rs.randint(0, 300, B).astype(np.int32)
            g = ro.Geometry(B, T_slots, N, 4, N, 0, 1, sensor.start, sensor.stride, 3)
            d = lambda a: None if a is None else torch.as_tensor(a).to(dev).contiguous()
            mem = [d(m) for m in members]
            state, traj = torch.full((B, N), 7.0, device=dev), torch.full((T_slots + 1, B, N), 7.0, device=dev)
            pol = torch.full((B, sensor.width), 7.0, device=dev)
            steps = torch.full((T_slots, B), -1, dtype=torch.int32, device=dev)
            rewards = torch.full((T_slots, B), 7.0, device=dev)
            step = torch.tensor([t_now, 9], dtype=torch.int32, device=dev)
            keep = (d(chosen), d(steps0), d(reward_map.coef))
            ro.settle(ro.stream(), g, ro.settle_args(mem, keep[0], state, traj, pol, keep[1], steps, rewards, keep[2],
                                                           step))
            torch.cuda.synchronize()
            want = members[chosen[t_now], np.arange(B)]
            np.testing.assert_array_equal(state.cpu().numpy(), want)
            np.testing.assert_array_equal(traj[t_now + 1].cpu().numpy(), want)
            assert bool((traj[:t_now + 1] == 7.0).all()) and bool((traj[t_now + 2:] == 7.0).all())
            np.testing.assert_array_equal(pol.cpu().numpy(), sensor.apply_numpy(want))
            np.testing.assert_array_equal(steps[t_now].cpu().numpy(), steps0 + t_now + 1)
            assert bool((steps[[0, 1, 3]] == -1).all()) and bool((rewards[[0, 1, 3]] == 7.0).all())
            assert step.tolist() == [t_now, t_now + 1]
            w = reward_map.apply_numpy(want).astype(np.float64)
            ref = (-1.0) * (1.0 / N) * (w * w).sum(axis=1)
            got = rewards[t_now].cpu().numpy().astype(np.float64)
            err = np.abs(got - ref) / np.abs(ref)
            print(f"ro_settle N={N} B={B} coef={reward_map.coef is not None}: max reward error {err.max():.3e} (bound {2.0 ** -23:.3e})")
            assert err.max() <= 2.0 ** -23


# ----------------------------------------------------------------------------------------------------------------------
# the phase
# ----------------------------------------------------------------------------------------------------------------------
def _generator_states():
    return (np.random.get_state(), torch.get_rng_state().clone(), torch.cuda.get_rng_state(0).clone())


def _assert_same_generators(a, b):
    assert a[0][0] == b[0][0] and np.array_equal(a[0][1], b[0][1]) and a[0][2:] == b[0][2:], "numpy's global generator"
    assert torch.equal(a[1], b[1]), "torch's CPU generator"
    assert torch.equal(a[2], b[2]), "torch's device generator"


def _world_state(world):
    dev = world._dev
    return (world.timesteps.copy(), int(world.simulated), dev.state.clone(), [tuple(h.clone() for h in hid) for hid in dev.hidden])


def _run_both(num_rollouts=sc.NUM_ROLLOUTS, deterministic=False, **kwargs):
    """(loop scene, loop replay, loop end, phase scene, phase replay, phase end) from equal generator states."""
    from pdecontrol.mbrl import imagination_phase as ip
    dev = torch.device("cuda", 0)
    out = []
    for phase in (False, True):
        s = sc.build(sc.repo_namespace(), dev, world_kwargs=DEVICE_REWARD, **kwargs)
        s.world.setup(s.starting)
        sc.seed()
        if phase:
            timings = {}
            replay = ip.imagine(s.agent, s.stack, num_rollouts, deterministic, timings=timings)
            assert timings["tier"] == "kernel", timings
        else:
            replay = sc.repo_namespace().Worker(s.stack).rollout(s.agent, sc.stop(num_rollouts), deterministic)
            assert s.world._dev is not None, "the loop's world is not device-resident"
        torch.cuda.synchronize()
        out += [s, replay, (_generator_states(), _world_state(s.world))]
    return out


def _host_forcing_is_the_fma_chain(scene):
    """Whether the loop's forcing product, torch's CPU matmul, is the fma chain of ``ro_act_chain`` on this host
    (tests/conftest.py::require_fma_sgemm: MKL on CPUs of other vendors than Intel rounds some products differently)."""
    F = scene.env.forcing.forcing.numpy()
    rs = np.random.RandomState(3)        # batches of the loop's own shape: the sgemm path may depend on it
    return all(host_matmul_is_fma_chain(F, rs.uniform(-1, 1, (scene.world.num_envs, 1, F.shape[0])).astype(np.float32))
               for _ in range(64))


def _same(a, b, exact, what):
    """Bit for bit; on a host whose forcing matmul rounds differently from the fma chain the float fields can only agree
    to the device path's tolerance against the reference (tests/test_world_env.py: 1e-4 relative, 1e-5 absolute)."""
    a, b = np.asarray(a), np.asarray(b)
    if exact or a.dtype.kind != "f":
        np.testing.assert_array_equal(a, b, err_msg=what)
    else:
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5, err_msg=what)


def _compare_replays(loop, phase, N, exact):
    """obs, actions, nxtobs, steps and the flags bit for bit; rewards within (N + 4) * 2^-24 relative: the loop squares an
    fp32 vector_norm (a sum of N squares in fp32, a square root and a square, each within 2^-24) and scales it, the phase
    rounds an fp64 sum once."""
    assert loop.episodes == phase.episodes and dict(loop.vindex) == dict(phase.vindex)
    assert (loop.ntimesteps, loop.nstopped) == (phase.ntimesteps, phase.nstopped)
    worst = 0.0
    for key in loop.episodes:
        for name in sc.FIELDS:
            a, b = list(getattr(loop, name)[key]), list(getattr(phase, name)[key])
            assert len(a) == len(b), (key, name)
            for x, y in zip(a, b):
                assert type(x) is type(y) and np.asarray(x).dtype == np.asarray(y).dtype and np.shape(x) == np.shape(y), (key, name)
            if name == "rewards":
                a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
                worst = max(worst, float((np.abs(a - b) / np.abs(a)).max()))
            else:
                _same(a, b, exact, f"episode {key} {name}")
    bound = (N + 4) * 2.0 ** -24 if exact else 1e-4
    if not exact:
        warnings.warn(f"TOLERANT MODE: this host's CPU matmul is not the fma chain of ro_act_chain, so the loop's forcing "
                      f"differs in its last bits; float fields were compared to 1e-4 relative and the rewards to {bound:.1e}, "
                      f"not bit for bit")
    print(f"phase against loop, N={N}, host forcing {'is' if exact else 'IS NOT'} the fma chain: max relative reward "
          f"difference {worst:.3e} (bound {bound:.3e})")
    assert worst <= bound


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["scenario", "limit", "b5_n256_stride4"])
def test_phase_equals_the_loop_on_the_same_gpu(case):
    from pdecontrol.mbrl import imagination_phase as ip
    from pdecontrol.surrogates.common.dataset import DeviceSubSeqStore
    kwargs = {"scenario": {}, "limit": {"limit": True},
              "b5_n256_stride4": dict(num_envs=5, agent_stride=4, env_kwargs=dict(L=88.0, N=256))}[case]
    N = 256 if "env_kwargs" in kwargs else 64
    ls, loop, lend, ps, phase, pend = _run_both(**kwargs)
    exact = _host_forcing_is_the_fma_chain(ls)          # the loop's forcing is the host's matmul
    assert loop.nepisodes == 2 * ls.world.num_envs
    assert loop.ntimesteps == (2 if case == "limit" else 6) * ls.world.num_envs
    _compare_replays(loop, phase, N, exact)
    _assert_same_generators(lend[0], pend[0])
    (lt, lsim, lstate, lhid), (pt, psim, pstate, phid) = lend[1], pend[1]
    np.testing.assert_array_equal(lt, pt)
    assert lsim == psim == 0
    _same(lstate.cpu(), pstate.cpu(), exact, "world state")
    for x, y in zip(lhid, phid):
        for a, b in zip(x, y):
            _same(a.cpu(), b.cpu(), exact, "hidden state")
    # the packed device copy is what packing the returned replay gives
    store = DeviceSubSeqStore(phase.data, torch.device("cuda", 0))
    roll = phase.device_rollout
    assert roll.starts == store.starts and roll.total == store.total
    for got, want in zip(roll.tensors, store.tensors):
        assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)
    if case != "scenario":
        return
    # a second phase reuses the graph; re-scaling a member as update_delta_transform does recaptures it
    cap = ps.world._imagination
    ip.imagine(ps.agent, ps.stack, sc.NUM_ROLLOUTS)
    assert ps.world._imagination is cap
    from _latent_models import normalize_pair
    _, dscaling = normalize_pair(mean=0.0, var=0.25)
    ps.ensemble.modules[0].surrogate.dscaling = dscaling
    assert not ps.world._dev.valid()
    again = ip.imagine(ps.agent, ps.stack, sc.NUM_ROLLOUTS)
    assert ps.world._imagination is not cap and ps.world._imagination.dev is ps.world._dev
    # ... and the recaptured graph computes what the loop computes with the re-scaled member
    ls.ensemble.modules[0].surrogate.dscaling = dscaling
    for s in (ls, ps):
        s.world.setup(s.starting)
    sc.seed()
    loop2 = sc.repo_namespace().Worker(ls.stack).rollout(ls.agent, sc.stop())
    sc.seed()
    phase2 = ip.imagine(ps.agent, ps.stack, sc.NUM_ROLLOUTS)
    _compare_replays(loop2, phase2, N, exact)
    assert again.ntimesteps == phase2.ntimesteps


@pytest.mark.gpu
def test_phase_equals_the_loop_with_the_deterministic_flag():
    """``select_action`` accepts ``deterministic`` and ignores it, as the reference's does: the loop samples and draws its
    noise, so the phase must too.  Replay and generator states against the loop with the flag set, and the same graph
    serves both values of the flag."""
    from pdecontrol.mbrl import imagination_phase as ip
    ls, loop, lend, ps, phase, pend = _run_both(deterministic=True)
    exact = _host_forcing_is_the_fma_chain(ls)
    _compare_replays(loop, phase, 64, exact)
    _assert_same_generators(lend[0], pend[0])
    np.testing.assert_array_equal(lend[1][0], pend[1][0])
    _same(lend[1][2].cpu(), pend[1][2].cpu(), exact, "world state")
    # the flag changes nothing: the sampled actions are those of a run without it
    _, _, _, ps2, plain, pend2 = _run_both(deterministic=False)
    _compare_replays(plain, phase, 64, True)
    _assert_same_generators(pend[0], pend2[0])
    cap = ps.world._imagination
    ip.imagine(ps.agent, ps.stack, sc.NUM_ROLLOUTS, deterministic=False)
    assert ps.world._imagination is cap


@pytest.mark.gpu
def test_phase_against_the_reference_arrays():
    """Against tests/golden/rollout_golden.npz (the reference's Worker, wrappers, world and SAC on the CPU), with the
    tolerance of the device world path (tests/test_world_env.py): 1e-4 relative, 1e-5 absolute."""
    from pdecontrol.mbrl import imagination_phase as ip
    from pdecontrol.sac import policies
    g = np.load(os.path.join(GOLDEN, "rollout_golden.npz"))
    # the policy's noise comes from the device generator here and from torch's CPU generator there: record the CPU draws
    # of the same scenario (they depend on the generator alone; this repository's CPU loop makes the reference's draws,
    # test_imagination_phase_host.py) and hand them to the phase
    draws, original = [], policies.draw_noise

    def recording(like):
        draws.append(original(like).clone())
        return draws[-1].clone()

    policies.draw_noise = recording
    try:
        host = sc.run(sc.repo_namespace())
    finally:
        policies.draw_noise = original
    assert sorted(host) == sorted(g.files)
    per_pass = {"free": draws[:6], "limit": draws[6:]}
    assert len(draws) == 8 and all(d.shape == (sc.NUM_ENVS, 1, 4) for d in draws)
    passes = iter(sc.PASSES)

    def rollout(s):
        timings = {}
        replay = ip.imagine(s.agent, s.stack, sc.NUM_ROLLOUTS, timings=timings, noise=per_pass[next(passes)])
        assert timings["tier"] == "kernel"
        return replay

    rec = sc.run(sc.repo_namespace(), torch.device("cuda", 0), rollout=rollout, world_kwargs=DEVICE_REWARD)
    assert sorted(rec) == sorted(g.files)
    for k in g.files:
        a, b = np.asarray(rec[k]), g[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.dtype.kind == "f":
            np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5, err_msg=k)
        else:
            np.testing.assert_array_equal(a, b, err_msg=k)
