"""The imagined-rollout phase on the host: ``Worker`` against arrays recorded from the reference's own Worker, wrappers,
world and SAC (tools/gen_rollout_golden.py -> tests/golden/rollout_golden.npz), ``imagine`` on the CPU against
``Worker.rollout``, stack recognition, the round length, and a numpy twin of the two kernels of csrc/rollout.hip against
the host wrapper chain."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rollout_scenario as sc  # noqa: E402
from conftest import GOLDEN, KS_CONFIGS, require_fma_sgemm  # noqa: E402
from _rollout_scenario import fma32, fma_chain  # noqa: E402

DEVICE_REWARD = {"batched_reward_func": lambda env: env.batched_reward_func}


@pytest.fixture(scope="module")
def M():
    return sc.repo_namespace()


# ----------------------------------------------------------------------------------------------------------------------
# the worker
# ----------------------------------------------------------------------------------------------------------------------
def test_worker_rollout_equals_the_reference(M):
    """Every field of every episode, the episode keys, ntimesteps and nstopped of both passes, bit for bit."""
    require_fma_sgemm("n64")          # the fixture holds the forcing products of an fma sgemm
    g = np.load(os.path.join(GOLDEN, "rollout_golden.npz"))
    rec = sc.run(M)
    assert sorted(rec) == sorted(g.files)
    assert int(g["free_ntimesteps"]) == 24 and int(g["free_nstopped"]) == 8          # two rounds of three steps, four envs
    assert int(g["limit_ntimesteps"]) == 8 and int(g["limit_nstopped"]) == 8         # the env limit cuts after one step
    for k in g.files:
        a = np.asarray(rec[k])
        assert a.dtype == g[k].dtype and a.shape == g[k].shape, k
        np.testing.assert_array_equal(a, g[k], err_msg=k)


def test_worker_continues_and_resets(M):
    """A second rollout continues from the kept observation without resetting the stack; ``reset()`` makes it reset."""
    s = sc.build(M)
    s.world.setup(s.starting)
    sc.seed()
    worker, resets = M.Worker(s.stack), []
    original = s.world.reset
    s.world.reset = lambda **kw: (resets.append(1), original(**kw))[1]
    seen = []

    class Callback:
        def on_rollout_end(self, replay):
            seen.append(replay)

    worker.callbacks.append(Callback())
    first = worker.rollout(s.agent, lambda ts, eps: ts >= 4)           # one step of four envs: no truncation yet
    assert first.ntimesteps == 4 and first.nstopped == 0 and seen == [first]
    before = len(resets)
    second = worker.rollout(s.agent, lambda ts, eps: ts >= 4)
    assert len(resets) == before, "a running worker reset its stack"
    np.testing.assert_array_equal(np.asarray(second.obs[0][0]), np.asarray(first.nxtobs[0][0]))
    assert int(second.steps[0][0]) == int(first.steps[0][0]) + 1
    worker.reset()
    assert worker._last_obs is None and worker._last_stored_obs is None
    third = worker.rollout(s.agent, lambda ts, eps: ts >= 4)
    assert len(resets) == before + 1 and third.ntimesteps == 4


def _states():
    return np.random.get_state(), torch.get_rng_state().clone()


def _same_replay(a, b):
    assert a.episodes == b.episodes and dict(a.vindex) == dict(b.vindex)
    assert (a.ntimesteps, a.nstopped, a.capacity) == (b.ntimesteps, b.nstopped, b.capacity)
    for key in a.episodes:
        for name in sc.FIELDS:
            x, y = list(getattr(a, name)[key]), list(getattr(b, name)[key])
            assert len(x) == len(y)
            for u, v in zip(x, y):
                assert type(u) is type(v) and np.asarray(u).dtype == np.asarray(v).dtype
                np.testing.assert_array_equal(np.asarray(u), np.asarray(v), err_msg=f"{key} {name}")


@pytest.mark.parametrize("limit,deterministic", [(False, False), (True, False), (False, True)])
def test_imagine_on_the_cpu_is_the_worker(M, limit, deterministic):
    from pdecontrol.mbrl import imagination_phase as ip
    out = []
    for phase in (False, True):
        s = sc.build(M, limit=limit, world_kwargs=DEVICE_REWARD)
        s.world.setup(s.starting)
        sc.seed()
        if phase:
            timings = {}
            replay = ip.imagine(s.agent, s.stack, sc.NUM_ROLLOUTS, deterministic, timings=timings)
            assert timings["tier"] == "loop" and replay.device_rollout is None
        else:
            replay = M.Worker(s.stack).rollout(s.agent, sc.stop(), deterministic)
        out.append((replay, _states(), s.world.timesteps.copy(), s.world.simulated))
    (a, (na, ta), tsa, sa), (b, (nb, tb), tsb, sb) = out
    _same_replay(a, b)
    assert na[0] == nb[0] and np.array_equal(na[1], nb[1]) and na[2:] == nb[2:]
    assert torch.equal(ta, tb)
    np.testing.assert_array_equal(tsa, tsb)
    assert sa == sb == 0


@pytest.mark.parametrize("lengths", [(3, 1), (1, 1, 2), (2,)])
def test_build_replay_is_what_add_builds(M, lengths):
    """The kernel tier's one-pass replay construction against ``Sample.split`` + ``ExperienceReplay.add``: structure,
    item types and ``vindex``."""
    from pdecontrol.mbrl import imagination_phase as ip
    B, N, A, rs = 3, 16, 4, np.random.RandomState(0)
    rounds, loop = [], M.Replay()
    for T in lengths:
        traj = rs.randn(T + 1, B, N).astype(np.float32)
        actions, rewards = rs.randn(T, B, A).astype(np.float32), rs.randn(T, B).astype(np.float32)
        steps = rs.randint(0, 50, (T, B)).astype(np.int32)
        rounds.append((traj, actions, rewards, steps))
        for t in range(T):
            cut = np.full(B, t == T - 1)
            loop.add(M.Sample(traj[t][:, None], actions[t][:, None], traj[t + 1][:, None], rewards[t], np.zeros(B, dtype=np.bool_),
                              cut, steps[t]).split(axis=0))
    replay, keys = ip._build_replay(rounds, B)
    _same_replay(loop, replay)
    assert sorted(k for r in keys for k in r) == sorted(loop.episodes)


# ----------------------------------------------------------------------------------------------------------------------
# recognition
# ----------------------------------------------------------------------------------------------------------------------
def test_the_controllers_stack_is_recognised(M):
    from pdecontrol.mbrl import imagination_phase as ip
    for stride, env_kwargs in ((1, None), (4, dict(L=88.0, N=256))):
        s = sc.build(M, agent_stride=stride, env_kwargs=env_kwargs, world_kwargs=DEVICE_REWARD)
        geo = ip.recognize_stack(s.stack)
        N = s.env.N
        assert geo.world is s.world and tuple(geo.forcing.shape) == (4, N)
        assert (geo.act_in.start, geo.act_in.stride, geo.act_in.width) == (0, 1, 4) and geo.act_in.coef.shape == (4, 4)
        assert (geo.act_out.start, geo.act_out.stride, geo.act_out.width) == (0, 1, N) and geo.act_out.coef.shape == (4, N)
        assert (geo.agent_obs.start, geo.agent_obs.stride, geo.agent_obs.width) == (stride // 2, stride, N // stride)
        assert geo.agent_obs.coef is None
        assert (geo.reward.start, geo.reward.stride, geo.reward.width) == (0, 1, N)
        np.testing.assert_array_equal(geo.reward.coef[:, 0].numpy(), np.asarray([-1.0, 2.0, 6.0, -3.0], dtype=np.float32))


def test_unrecognised_stacks_name_their_reason(M):
    from pdecontrol.mbrl import imagination_phase as ip
    from pdecontrol.mbrl.recognition import Unrecognized
    T = M.T
    s = sc.build(M, world_kwargs=DEVICE_REWARD)
    tf, world = s.transforms, s.world
    good = sc.controller_action_transforms(tf)
    ip.recognize_stack(sc.make_stack(M, world, [tf.agent_sensor], good))
    extra = T.BatchTransform(T.ScaleTransform(bounds=(np.float32(-2.0), np.float32(2.0)), frozen=True))
    norm = T.Normalize(aggregate=True, batched=True)
    norm.mean, norm.var, norm.count = torch.zeros(1, 1, 1), torch.ones(1, 1, 1), 10
    cases = [
        ("two scalings in a row", [tf.agent_sensor], good[:1] + [(extra, True)] + good[1:]),
        ("a Normalize", [tf.agent_sensor], good[:2] + [(T.BatchTransform(norm), True)] + good[2:]),
        ("without a GaussianForcing", [tf.agent_sensor], [good[0], good[1], good[3]]),
        ("a scaling on the agent's observations", [tf.oscaling, tf.agent_sensor], good),
    ]
    for reason, obs_transforms, action_transforms in cases:
        with pytest.raises(Unrecognized, match=reason):
            ip.recognize_stack(sc.make_stack(M, world, obs_transforms, action_transforms))
    diss = sc.build(M, env_kwargs=dict(objective=""), world_kwargs=DEVICE_REWARD)
    with pytest.raises(Unrecognized, match="the dissipation objective"):
        ip.recognize_stack(diss.stack)
    plain = sc.build(M, world_kwargs={"batched_reward_func": lambda env: (lambda obs, phi=None: -np.square(obs).mean(axis=(1, 2)))})
    with pytest.raises(Unrecognized, match="batched reward of a KuramotoSivashinskyEnv"):
        ip.recognize_stack(plain.stack)
    with pytest.raises(Unrecognized, match="batched reward of a KuramotoSivashinskyEnv"):
        ip.recognize_stack(sc.build(M).stack)                      # the per-sample host reward of the reference
    # a stack whose outermost wrapper is not the action store
    bare = M.PDEEnvStack(envs=s.stack.envs.env, ostore=s.stack.ostore, astore=s.stack.astore)
    with pytest.raises(Unrecognized, match="in place of the action store"):
        ip.recognize_stack(bare)


def test_cpu_agents_and_the_opt_out_take_the_loop(M):
    """No GPU here: the tier choice for a CPU agent, and that stored noise is refused outside the kernel tier."""
    from pdecontrol.mbrl import imagination_phase as ip
    s = sc.build(M, world_kwargs=DEVICE_REWARD)
    assert ip._kernel_tier(s.agent, s.stack) == (None, None)
    s.world.setup(s.starting)
    with pytest.raises(ValueError, match="kernel tier"):
        ip.imagine(s.agent, s.stack, 2, noise=[torch.zeros(4, 1, 4)])


# ----------------------------------------------------------------------------------------------------------------------
# round length
# ----------------------------------------------------------------------------------------------------------------------
def _brute_force_round(timesteps0, horizon, limit):
    """``WorldVecEnv.step_async`` / ``step_wait`` counters, stepped until the joint truncation."""
    timesteps, simulated = np.asarray(timesteps0).copy(), 0
    while True:
        simulated += 1
        timesteps += 1
        env_limit = np.broadcast_to(timesteps >= limit, timesteps.shape)
        rll_limit = np.broadcast_to(simulated >= horizon, timesteps.shape)
        if np.any(np.broadcast_to(np.all(env_limit | rll_limit), timesteps.shape)):
            return simulated


@pytest.mark.parametrize("horizon", [1, 3])
def test_round_length_is_the_step_wait_rule(horizon):
    from pdecontrol.mbrl.imagination_phase import round_length
    limit = 400
    cases = {"none": [5, 17, 120, 396], "some": [399, 5, 398, 17], "all": [399, 399, 399, 399], "all staggered": [398, 399, 399, 398],
             "past": [400, 405, 399, 399], "one env": [399]}
    for name, start in cases.items():
        start = np.asarray(start, dtype=np.int32)
        want = _brute_force_round(start, horizon, limit)
        assert round_length(start, horizon, limit) == want, (name, horizon)
        assert 1 <= want <= horizon
    assert round_length(np.asarray([399, 399]), 3, limit) == 1 and round_length(np.asarray([398, 399]), 3, limit) == 2
    assert round_length(np.asarray([1, 399]), 3, limit) == 3


# ----------------------------------------------------------------------------------------------------------------------
# numpy twin of the kernels
# ----------------------------------------------------------------------------------------------------------------------
def test_fma32_is_one_rounding():
    """The twin's fp32 fma against exact rational arithmetic, ties included."""
    from fractions import Fraction
    rs = np.random.RandomState(1)
    a, b, c = (rs.uniform(-2, 2, 2000).astype(np.float32) for _ in range(3))
    # products that land exactly between two fp32 values once c is added
    a[:4] = np.float32(1 + 2.0 ** -12)
    b[:4] = np.float32(1 + 2.0 ** -12)
    c[:4] = np.asarray([2.0 ** -24, -2.0 ** -24, 2.0 ** -25, 1.0], dtype=np.float32)
    got = fma32(a, b, c)
    for x, y, z, r in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo, hi = np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))
        err = abs(Fraction(float(r)) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact)
        if err == abs(Fraction(float(lo)) - exact) or err == abs(Fraction(float(hi)) - exact):
            assert (np.asarray(r).view(np.int32) & 1) == 0, "a tie must go to the even neighbour"


@pytest.mark.parametrize("tag", ["n64", "n256"])
def test_numpy_twin_of_the_kernels_equals_the_host_chain(M, tag):
    """``ro_act_chain``'s arithmetic (``FieldMap.apply_numpy`` around the fma chain) against the wrappers' transforms on the
    host, bit for bit, at B = 1, 5, 257; ``ro_settle``'s sensor against the agent sensor, and its reward against the
    host's batched reward within (N + 4) * 2^-24 relative (the host squares an fp32 vector_norm)."""
    from pdecontrol.mbrl import imagination_phase as ip
    require_fma_sgemm(tag)
    L, N = KS_CONFIGS[tag]
    stride = 1 if N == 64 else 4
    s = sc.build(M, agent_stride=stride, env_kwargs=dict(L=L, N=N), world_kwargs=DEVICE_REWARD, members=1)
    geo = ip.recognize_stack(s.stack)
    tf = s.transforms
    F = geo.forcing.numpy()
    for B in (1, 5, 257):
        rs = np.random.RandomState(B)
        actions = rs.uniform(-1, 1, (B, 1, 4)).astype(np.float32)
        host = actions
        for t in (tf.ascaling, tf.forcing, tf.pdescaling, tf.world_sensor):      # outermost wrapper first
            host = t(host)
        twin = geo.act_out.apply_numpy(fma_chain(geo.act_in.apply_numpy(actions), F))
        assert twin.dtype == host.dtype == np.float32 and twin.shape == host.shape == (B, 1, N)
        np.testing.assert_array_equal(twin, host)
        as_tensor = tf.world_sensor(tf.pdescaling(tf.forcing(tf.ascaling(torch.from_numpy(actions)))))
        np.testing.assert_array_equal(twin, as_tensor.numpy())
        state = rs.uniform(-1, 1, (B, 1, N)).astype(np.float32)
        np.testing.assert_array_equal(geo.agent_obs.apply_numpy(state), tf.agent_sensor(state))
        w = geo.reward.apply_numpy(state).astype(np.float64).reshape(B, N)
        reward = ((-1.0) * (1.0 / N) * (w * w).sum(axis=1)).astype(np.float32)
        loop = np.asarray(s.world.batched_reward_func(s.world.stransf.otransf(state), None), dtype=np.float32).reshape(B)
        assert np.abs(reward.astype(np.float64) - loop).max() <= (N + 4) * 2.0 ** -24 * np.abs(loop).max()
