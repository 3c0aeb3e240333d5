"""The real-env collection phase on the host: header, binding and exports of libcollect_hip.so and its numbered
refusals, ``recognize_real_stack`` on the controller's two stacks over the stepper's CPU twin, ``plan_phase`` against a
brute-force replay of the loop's integers, the replay builder against ``Sample.split`` + ``ExperienceReplay.add``, and the
loop tier of ``collect`` against ``Worker.rollout``."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _collect_scenario as sc  # noqa: E402
from test_capi_symbols import LIBDIR, declared_functions  # noqa: E402

from pdecontrol.mbrl import collect_hip as co  # noqa: E402
from pdecontrol.mbrl import collection_phase as cp  # noqa: E402
from pdecontrol.mbrl.recognition import Unrecognized  # noqa: E402
from pdecontrol.mbrl.replay import ExperienceReplay  # noqa: E402
from pdecontrol.mbrl.types import Sample  # noqa: E402


# ----------------------------------------------------------------------------------------------------------------------
# header and binding
# ----------------------------------------------------------------------------------------------------------------------
def test_collect_library_exports_what_its_header_declares():
    """(that the binding's table holds exactly these names and the library exports them: tests/test_capi_symbols.py,
    which skips without the library where this test fails)"""
    assert declared_functions("collect_hip.h", "co") == ["co_act", "co_last_error", "co_observe", "co_supported",
                                                         "co_workspace_floats"]
    assert os.path.exists(os.path.join(LIBDIR, "libcollect_hip.so")), "libcollect_hip.so not built (run __graft_entry__.build())"


def test_collect_geometry_refusals_are_numbered():
    lib = co.load()
    good = dict(E=5, T=3, N=64, A=4, obs_start=0, obs_stride=1)
    assert co.supported(co.Geometry(**good)) is None
    seen = {}
    for code, change in ((-2, dict(E=0)), (-3, dict(T=0)), (-4, dict(N=8)), (-4, dict(N=1028)), (-5, dict(A=17)),
                         (-6, dict(obs_stride=0)), (-6, dict(obs_start=64))):
        g = co.Geometry(**{**good, **change})
        assert lib.co_supported(ctypes.byref(g)) == code, change
        assert co.last_error().startswith("collect:")
        seen.setdefault(code, co.last_error())
        assert lib.co_workspace_floats(ctypes.byref(g)) == code
    assert len(set(seen.values())) == len(seen)                       # one text per reason
    assert lib.co_supported(None) == -1 and "NULL" in co.last_error()
    for N in (16, 100, 1024):
        assert co.supported(co.Geometry(**{**good, "N": N})) is None
    assert co.workspace_floats(co.Geometry(**good)) == 4               # two workgroups of four rows, (min, max) each
    assert co.workspace_floats(co.Geometry(**{**good, "E": 4096})) == 2048
    with pytest.raises(co.CollectHipError, match="state width"):
        co.workspace_floats(co.Geometry(**{**good, "N": 8}))


def test_launch_arguments_are_validated_before_any_hip_call():
    """No GPU here: every refusal below returns before the first HIP call."""
    lib = co.load()
    g = co.Geometry(E=5, T=3, N=64, A=4, obs_start=0, obs_stride=1)
    assert lib.co_act(None, ctypes.byref(g), ctypes.byref(co.ActArgs()), 0) == -10
    assert lib.co_observe(None, ctypes.byref(g), ctypes.byref(co.ObserveArgs()), 0) == -10
    fake = ctypes.c_void_p(64)                                         # never dereferenced on the host
    act = co.ActArgs(fake, None, fake, fake, 0)
    for t in (-1, 3):
        assert lib.co_act(None, ctypes.byref(g), ctypes.byref(act), t) == -11
        assert lib.co_observe(None, ctypes.byref(g), ctypes.byref(co.ObserveArgs(fake, fake, None, -1.0, 1.0, 0, None)), t) == -11
    assert lib.co_observe(None, ctypes.byref(g), ctypes.byref(co.ObserveArgs(fake, fake, fake, -1.0, 1.0, 1, None)), 0) == -12
    assert "workspace" in co.last_error()


# ----------------------------------------------------------------------------------------------------------------------
# recognition
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    return sc.build(E=3)


@pytest.mark.parametrize("N,stride", [(64, 1), (256, 4)])
def test_the_controllers_stacks_are_recognised(N, stride):
    s = sc.build(E=3, N=N, agent_stride=stride)
    for stack, env, update in ((s.stack, s.env, 1), (s.eval_stack, s.eval_env, 0)):
        geo = cp.recognize_real_stack(stack)
        assert geo.env is env and geo.scaling is s.transforms.oscaling and geo.update == update
        assert geo.record_raw is False                                 # the store sits below the scaling: env-side actions
        assert (geo.action.start, geo.action.stride, geo.action.width) == (0, 1, 4)
        np.testing.assert_array_equal(geo.action.coef[:, 0].numpy(), np.asarray([-1.0, 2.0, 2.0, -1.0], dtype=np.float32))
        assert (geo.agent_obs.start, geo.agent_obs.stride, geo.agent_obs.width) == (stride // 2, stride, N // stride)
        assert geo.agent_obs.coef is None
    on_top = sc.make_stack(s.env, s.transforms, frozen=False, store_on_top=True)
    assert cp.recognize_real_stack(on_top).record_raw is True


def test_unrecognised_real_stacks_name_their_reason(scene):
    from pdegym.common import transforms as T
    env, tf = scene.env, scene.transforms
    running = lambda **kw: T.ScaleTransform(**{**dict(batched=True, aggregate=True, frozen=False), **kw})
    sensor2 = T.BatchTransform(T.SensorTransform(stride=2))
    moving = T.ScaleTransform(bounds=(np.float32(-2.0), np.float32(2.0)), aggregate=True, batched=True, frozen=False).Inverse
    norm = T.Normalize(aggregate=True, batched=True)
    norm.mean, norm.var, norm.count = torch.zeros(1, 1, 1), torch.ones(1, 1, 1), 10

    def action_wrapper(transform, frozen):
        """The controller's stack with another transform in its action wrapper (set after construction: the wrapper's
        constructor inverts its transform to derive the action space, which a sensor or a forcing over four columns
        does not allow)."""
        stack = sc.make_stack(env, tf, frozen=False)
        stack.envs.transform, stack.envs.frozen = transform, frozen
        return stack

    obs = lambda *entries: sc.make_stack(env, tf, frozen=False, obs_transforms=list(entries))
    cases = {
        "an observation store of 2 steps": sc.make_stack(env, tf, frozen=False, obs_steps=2),
        "an action store of 2 steps": sc.make_stack(env, tf, frozen=False, act_steps=2),
        "per-column running bounds": obs((running(aggregate=False), False), (tf.agent_sensor, False)),
        "a sensor under the running scaling": obs((sensor2, False), (running(), False)),
        "two observation scalings": obs((running(), False), (running(frozen=True), True)),
        "a running scaling inside a composite transform": obs((T.Operation([running()]), False)),
        "a Normalize": obs((norm, True)),
        "an action transform that updates its statistics": action_wrapper(moving, False),
        "a forcing in the action stack": action_wrapper(T.BatchTransform(env.forcing), True),
        "a sensor on the agent's actions": action_wrapper(sensor2, True),
    }
    assert len(cases) == 10
    for reason, stack in cases.items():
        with pytest.raises(Unrecognized) as e:
            cp.recognize_real_stack(stack)
        assert reason in str(e.value), (reason, str(e.value))
    good = sc.make_stack(env, tf, frozen=False)
    with pytest.raises(Unrecognized, match="in place of the action store"):
        cp.recognize_real_stack(good._replace(envs=good.ostore))
    with pytest.raises(Unrecognized, match="not the stack's astore"):
        cp.recognize_real_stack(good._replace(astore=None))
    with pytest.raises(Unrecognized, match="in place of the observation store"):
        cp.recognize_real_stack(good._replace(ostore=None))

    class Other(type(env)):
        pass

    odd = sc.make_stack(env, tf, frozen=False)
    odd.ostore.env.__class__ = Other
    try:
        with pytest.raises(Unrecognized, match="a Other in place of the KSBatchedVecEnv"):
            cp.recognize_real_stack(odd)
    finally:
        odd.ostore.env.__class__ = Other.__bases__[0]


# ----------------------------------------------------------------------------------------------------------------------
# the plan
# ----------------------------------------------------------------------------------------------------------------------
def _brute_force(timestep0, limit, E, stop):
    """The loop's integers through the real ``ExperienceReplay``: counters as ``KSBatchedVecEnv._finish_step`` keeps
    them, ``stop`` called on the replay's own ``ntimesteps`` / ``nstopped``."""
    replay, ts = ExperienceReplay(), np.asarray(timestep0, dtype=np.int64).copy()
    calls, cuts, steps, k = [], [], [], 0

    def asked(a, b):
        calls.append((a, b))
        return stop(a, b)

    while not asked(replay.ntimesteps, replay.nstopped):
        ts += 1
        truncated = ts >= limit
        steps.append(ts.copy())
        if truncated.any():
            cuts.append(k)
            ts[truncated] = 0
        z = np.zeros(E, dtype=np.float32)
        replay.add(Sample(z, z, z, z, np.zeros(E, dtype=bool), truncated, steps[-1]).split(axis=0))
        k += 1
    return k, cuts, np.asarray(steps, dtype=np.int64).reshape(k, E), calls, ts


def test_plan_phase_is_the_loops_integers():
    rs = np.random.RandomState(0)
    for trial in range(200):
        E = (1, 3, 8)[trial % 3]
        limit = (1, 4)[(trial // 3) % 2]
        ts0 = rs.randint(0, limit, E)
        episodes = 1 + trial % 5
        # the controller's three stop forms (mbrl.py:249-251): warm-up and sampling count steps, evaluation episodes
        stops = {"warmup": lambda ts, _: ts >= 5 * E + 2, "sampling": lambda ts, _: ts >= 3 * E,
                 "eval": lambda _, ep: ep >= episodes}
        for name in ("warmup", "sampling", "eval"):
            want = _brute_force(ts0, limit, E, stops[name])
            calls = []

            def stop(a, b):
                calls.append((a, b))
                return stops[name](a, b)

            plan = cp.plan_phase(ts0, limit, E, stop)
            assert plan.K == want[0] and plan.truncations == want[1], (trial, name)
            np.testing.assert_array_equal(plan.steps, want[2])
            assert plan.steps.dtype == np.int64 and plan.steps.shape == (plan.K, E)
            assert calls == want[3], (trial, name)
            np.testing.assert_array_equal(plan.timestep, want[4])
    # a stop that already holds asks once and plans nothing
    plan = cp.plan_phase(np.zeros(3, dtype=np.int64), 4, 3, lambda ts, ep: True)
    assert plan.K == 0 and plan.truncations == [] and plan.steps.shape == (0, 3)


def test_segments_cut_at_truncations_and_at_the_budget():
    plan = cp.plan_phase(np.asarray([0, 2]), 4, 2, lambda ts, ep: ts >= 2 * 9)
    assert plan.truncations == [1, 3, 5, 7]
    assert cp.segments(plan, 100) == [("kernel", 0, 1), ("host", 1, 1), ("kernel", 2, 1), ("host", 3, 1), ("kernel", 4, 1),
                                      ("host", 5, 1), ("kernel", 6, 1), ("host", 7, 1), ("kernel", 8, 1)]
    plan = cp.plan_phase(np.asarray([0]), 8, 1, lambda ts, ep: ts >= 10)
    assert cp.segments(plan, 3) == [("kernel", 0, 3), ("kernel", 3, 3), ("kernel", 6, 1), ("host", 7, 1), ("kernel", 8, 2)]
    # 4096 x 256: a step is 4 MB of observations; the default budget holds 61 steps beside slot 0
    assert cp.segment_steps(4096, 256, 4) == (cp.SEGMENT_BYTES - 4 * 4096 * 256) // (4096 * (1024 + 16 + 12)) == 61
    assert cp.segment_steps(4096, 256, 4, budget=1) == 1


# ----------------------------------------------------------------------------------------------------------------------
# the replay builder
# ----------------------------------------------------------------------------------------------------------------------
def test_build_replay_is_what_add_builds():
    """A segment of 3 steps, a host step with a partial truncation, a segment of 2 steps -- against ``Sample.split`` +
    ``ExperienceReplay.add`` fed step by step: every field of every episode, keys in order, item types, ``vindex``."""
    E, N, A, rs = 3, 16, 4, np.random.RandomState(0)

    def block(T):
        return (rs.randn(T + 1, E, N).astype(np.float32), rs.randn(T, E, A).astype(np.float32), rs.randn(T, E),
                rs.randint(0, 50, (T, E)).astype(np.int64))

    first, last = block(3), block(2)
    cut = np.asarray([False, True, False])
    host = Sample(rs.randn(E, 1, N).astype(np.float32), rs.randn(E, 1, A).astype(np.float32), rs.randn(E, 1, N).astype(np.float32),
                  rs.randn(E), np.zeros(E, dtype=bool), cut, rs.randint(0, 50, E).astype(np.int64))
    loop = ExperienceReplay()
    for piece in (first, host, last):
        if isinstance(piece, Sample):
            loop.add(Sample(*piece).split(axis=0))
            continue
        traj, actions, rewards, steps = piece
        for t in range(actions.shape[0]):
            none = np.zeros(E, dtype=bool)
            loop.add(Sample(traj[t][:, None], actions[t][:, None], traj[t + 1][:, None], rewards[t], none, none.copy(),
                            steps[t]).split(axis=0))
    built = cp.build_replay([first, host, last], E)
    sc.assert_same_replay(loop, built)
    assert built.episodes == [0, 1, 2, 3] and dict(built.vindex) == {0: 0, 1: 3, 2: 2}
    assert [len(built.obs[k]) for k in built.episodes] == [6, 4, 6, 2] and built.nstopped == 1
    # a first step that truncates interleaves the keys, as ``add`` hands them out
    all_cut = Sample(*(list(host)[:5] + [np.ones(E, dtype=bool), host.steps]))
    loop = ExperienceReplay()
    loop.add(Sample(*all_cut).split(axis=0))
    loop.add(Sample(*host).split(axis=0))
    sc.assert_same_replay(loop, cp.build_replay([all_cut, host], E))
    empty = cp.build_replay([], E)
    assert empty.ntimesteps == 0 and dict(empty.vindex) == {}


# ----------------------------------------------------------------------------------------------------------------------
# the loop tier
# ----------------------------------------------------------------------------------------------------------------------
def _two_calls(route):
    s = sc.build(E=3)
    sc.seed()
    callback = sc.Callback()
    s.worker.callbacks.append(callback)
    sc.prime(s.worker, 11)
    stop, out = (lambda ts, ep: ts >= 3 * 3), []
    for _ in range(2):
        replay = s.worker.rollout(s.agent, stop) if route == "loop" else cp.collect(s.worker, s.agent, stop)
        out.append((replay, sc.state_record(s.worker)))
    assert callback.seen == [r for r, _ in out]
    return out


def test_collect_with_a_cpu_agent_is_the_worker():
    """Bit for bit over two consecutive calls on the CPU-twin stack: the replay, the worker state, the stores, the
    bounds, the generators; ``tier == "loop"`` with its reason."""
    for (a, sa), (b, sb) in zip(_two_calls("loop"), _two_calls("collect")):
        sc.assert_same_replay(a, b)
        sc.assert_same_state(sa, sb)
        assert b.tier == "loop" and "on the CPU" in b.tier_reason and b.host_steps == 3
        assert tuple(sb["vmin"].shape) == (1, 1, 1) and sb["vmin"].dtype == torch.float32
    assert b.nstopped > 0                                  # max_episode_steps = 4: the second call crossed truncations


def test_other_agents_take_the_loop():
    s = sc.build(E=3)

    class RandomAgent:
        def select_action(self, obs, deterministic=False):
            return np.zeros((obs.shape[0], 1, 4), dtype=np.float32)

    geo, fused, reason = cp._kernel_tier(s.worker, RandomAgent())
    assert geo is None and fused is None and "RandomAgent" in reason
    sc.prime(s.worker, 3, stagger=False)
    replay = cp.collect(s.worker, RandomAgent(), lambda ts, ep: ts >= 3)
    assert replay.tier == "loop" and replay.ntimesteps == 3 and "RandomAgent" in replay.tier_reason
    assert cp._kernel_tier(s.worker, s.agent) == (None, None, "a SAC agent on the CPU")
