"""The collection phase over a ``BurgersBatchedVecEnv`` on an MI355X: ``collect`` on the kernel tiers (a fused ``SAC``
per step around ``bg_step``; ``RandomAgent`` and ``ActionRepeatAgent`` on ``co_act_span -> bg_step_span ->
co_observe_span``; with a sink, one ``bg_record`` per segment) against the per-step loop of ``Worker.rollout`` on the same
GPU from the same seeds, bit for bit in everything the loop returns and mutates; and the launches a scripted segment
makes.  The stacks are the controller's two (tests/_collect_scenario.py) over a Burgers env with two sub-steps per step and
``Tmax`` chosen so that an episode has 4 steps (nearly every phase crosses a truncation) or 12 (multi-step segments)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _collect_scenario as sc  # noqa: E402
import _real_replay_scenario as rr  # noqa: E402
import _sac_models as sm  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CFG_STEPS = 2
TMAX = {4: 0.0079, 12: 0.0239}            # Tmax / (dt * cfg_steps) with dt = 1e-3, rounded up: episodes of 4 and of 12 steps


def make_env(E, N, episode):
    from pdegym.burgers.burgers import BurgersBatchedVecEnv
    env = BurgersBatchedVecEnv(E, N=N, cfg_steps=CFG_STEPS, Tmax=TMAX[episode], device=0)
    assert env.max_episode_steps == episode
    return env


def build(E, N, stride, episode):
    from pdecontrol.mbrl.worker import Worker
    env, eval_env = make_env(E, N, episode), make_env(E, N, episode)
    tf = sc.transforms(env, stride)
    stack, eval_stack = sc.make_stack(env, tf, frozen=False), sc.make_stack(eval_env, tf, frozen=True)
    agent = sm.build(hidden=256, obs_dim=len(range(stride // 2, N, stride)), act_dim=4, seed=7, device="cuda:0")
    return types.SimpleNamespace(env=env, eval_env=eval_env, stack=stack, eval_stack=eval_stack, agent=agent,
                                 worker=Worker(stack), eval_worker=Worker(eval_stack))


def state_record(worker):
    """Everything ``Worker.rollout`` mutates besides the replay it returns, over a Burgers env."""
    stack = worker.stack
    env = stack.ostore.env
    scaling = next(w.transform for w in sc._wrappers(stack.envs) if hasattr(w, "transform") and hasattr(w.transform, "vmin"))
    rngs = [r.get_state() for r in env._rngs]
    return {"last_obs": worker._last_obs.copy(), "last_stored_obs": worker._last_stored_obs.copy(),
            "ostore_obs": stack.ostore.obs.copy(), "ostore_mask": stack.ostore.mask.copy(),
            "ostore_finals": stack.ostore.finals.copy(), "astore_actions": stack.astore.actions.copy(),
            "astore_mask": stack.astore.mask.copy(), "vmin": scaling.vmin.clone(), "vmax": scaling.vmax.clone(),
            "timestep": env.timestep.copy(), "u": env.u.cpu().numpy(), "rng_keys": np.stack([r[1] for r in rngs]),
            "rng_pos": np.asarray([r[2:] for r in rngs], dtype=np.float64), "numpy": np.random.get_state(),
            "torch_cpu": torch.get_rng_state().clone(), "torch_cuda": torch.cuda.get_rng_state(0).clone()}


def _space_state(space):
    rng = getattr(space, "_rng", None)
    if rng is None:
        rng = space.np_random
    return rng.bit_generator.state


def _agent(kind, s, stack, E):
    from pdecontrol.mbrl import utils
    if kind == "sac":
        return s.agent, None
    space = stack.envs.action_space
    space.seed(7)
    if kind == "random":
        return utils.RandomAgent(space), space
    table = np.random.RandomState(17).uniform(-1, 1, (E, 16, 1, 4)).astype(np.float32)
    return utils.ActionRepeatAgent(table), space


def _run(route, kind, E, N, stride, episode, with_sink, steps=7, calls=3):
    """``calls`` phases in a row on the collection stack, then one on the evaluation stack (the same scaling, frozen).
    ``route``: "loop" is ``Worker.rollout`` into a host replay, "collect" the phase under test."""
    from pdecontrol.mbrl import collection_phase as cp
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    from pdecontrol.mbrl.replay import ExperienceReplay
    s = build(E, N, stride, episode)
    sc.seed()
    sc.prime(s.worker, 11)
    agent, space = _agent(kind, s, s.stack, E)
    stop = lambda ts, ep: ts >= steps
    sink = DeviceExperienceReplay(device=DEV) if with_sink and route == "collect" else None
    total = ExperienceReplay() if sink is None else sink
    out = []
    for worker, n in ((s.worker, calls), (s.eval_worker, 1)):
        if worker is s.eval_worker:                                    # (without a sink: nothing is committed)
            sc.prime(worker, 5)
            agent, space = _agent(kind, s, s.eval_stack, E)
            sink = None
        for _ in range(n):
            env = worker.stack.ostore.env
            plan = cp.plan_phase(env.timestep, env.max_episode_steps, E, stop)
            if route == "loop":
                got = worker.rollout(agent, stop)
            else:
                got = cp.collect(worker, agent, stop, **({} if sink is None else {"sink": sink}))
            phase = got.to_host() if hasattr(got, "to_host") else got
            if route == "collect":
                phase.tier, phase.tier_reason, phase.host_steps = got.tier, got.tier_reason, got.host_steps
            if worker is s.worker:
                total.extend(got)
            torch.cuda.synchronize()
            record = state_record(worker)
            extra = (None if space is None else _space_state(space), getattr(agent, "nstep", None))
            out.append((phase, record, plan, extra))
    return out, total


def _same_rows(a, b, what):
    """The fields of two host replays as the slabs hold them (fp32 rewards, int32 steps), byte for byte."""
    assert a.episodes == b.episodes and dict(a.vindex) == dict(b.vindex) and a.ntimesteps == b.ntimesteps, what
    for name, dt in zip(rr.FIELDS, (np.float32, np.float32, np.float32, np.float32, np.bool_, np.bool_, np.int32)):
        x, y = getattr(a, name), getattr(b, name)
        assert list(x.keys()) == list(y.keys()), (what, name)
        for key in y:
            assert np.asarray(x[key], dtype=dt).tobytes() == np.asarray(y[key], dtype=dt).tobytes(), (what, name, key)


def _compare(loop, kernel, with_sink):
    (loop_out, loop_total), (out, total) = loop, kernel
    assert len(loop_out) == len(out)
    for i, ((a, sa, _, xa), (b, sb, plan, xb)) in enumerate(zip(loop_out, out)):
        assert b.tier == "kernel" and b.tier_reason is None, (b.tier, b.tier_reason)
        assert b.host_steps == len(plan.truncations) and plan.K * len(plan.timestep) == b.ntimesteps
        if with_sink:
            _same_rows(b, a, i)
        else:
            sc.assert_same_replay(a, b)
        assert xa == xb, "the action space's generator and the agent's step counter"
        sc.assert_same_state(sa, sb)
    if with_sink:
        rr.same_metadata(total, loop_total)
        rr.pack_contract(total, loop_total)


CASES = [(5, 64, 1, 4), (3, 256, 4, 4), (5, 64, 1, 12)]


@pytest.mark.parametrize("kind", ["random", "repeat", "sac"])
@pytest.mark.parametrize("with_sink", [False, True], ids=["replay", "sink"])
@pytest.mark.parametrize("E,N,stride,episode", CASES)
def test_the_kernel_tiers_equal_the_loop(E, N, stride, episode, with_sink, kind):
    """Three phases in a row (``ts >= 7``) and one on the frozen evaluation stack, counters staggered: every field of
    every episode, keys and vindex (through a sink: the staged rows, the metadata and the pack contract), the worker's
    observations, the stores, the bounds, ``env.timestep``, ``env.u``, the envs' generators, numpy's, torch's and the
    action space's generators and ``agent.nstep``, bit for bit."""
    loop = _run("loop", kind, E, N, stride, episode, False)
    kernel = _run("collect", kind, E, N, stride, episode, with_sink)
    _compare(loop, kernel, with_sink)
    crossed = sum(len(plan.truncations) for _, _, plan, _ in kernel[0][:3])
    if episode == 4:
        assert crossed >= 3, "the phases crossed no truncation"
    else:
        assert all(len(plan.truncations) < plan.K for _, _, plan, _ in kernel[0])


def test_long_segments_across_a_truncation():
    """Episodes of 12 steps with ``ts >= 7 E``: segments of up to seven steps in one ``bg_step_span``, a truncation step
    between two."""
    E = 5
    loop = _run("loop", "random", E, 64, 1, 12, False, steps=7 * E)
    kernel = _run("collect", "random", E, 64, 1, 12, True, steps=7 * E)
    _compare(loop, kernel, True)
    assert sum(len(plan.truncations) for _, _, plan, _ in kernel[0][:3]) >= 1


def test_a_scripted_segment_is_three_span_calls(monkeypatch):
    from pdecontrol.mbrl import collect_hip as co
    from pdecontrol.mbrl import collection_phase as cp
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    E, Tn = 5, 3
    s = build(E, 64, 1, 12)
    sc.seed()
    sc.prime(s.worker, 11, stagger=False)
    agent, _ = _agent("random", s, s.stack, E)
    counts = {}

    def counted(name, fn):
        def call(*args, **kwargs):
            counts[name] = counts.get(name, 0) + 1
            return fn(*args, **kwargs)
        return call

    for name in ("act", "observe", "act_span", "observe_span"):
        monkeypatch.setattr(co, name, counted(name, getattr(co, name)))
    stepper = s.env.stepper
    for name in ("step_device", "step_span", "record_device"):
        monkeypatch.setattr(stepper, name, counted(name, getattr(stepper, name)))
    got = cp.collect(s.worker, agent, lambda ts, ep: ts >= Tn * E)
    torch.cuda.synchronize()
    assert got.tier == "kernel" and got.host_steps == 0 and got.ntimesteps == Tn * E
    assert counts == {"act_span": 1, "step_span": 1, "observe_span": 1}, counts
    counts.clear()
    got = cp.collect(s.worker, agent, lambda ts, ep: ts >= Tn * E, sink=DeviceExperienceReplay(device=DEV))
    torch.cuda.synchronize()
    assert got.tier == "kernel" and got.host_steps == 0
    assert counts == {"act_span": 1, "step_span": 1, "observe_span": 1, "record_device": 1}, counts


def test_a_sac_segment_is_t_times_act_step_observe(monkeypatch):
    """One segment of three steps of the SAC tier: three ``co_act``, three ``bg_step`` and three ``co_observe`` calls and no
    span call; through a sink, one ``bg_record`` call more."""
    from pdecontrol.mbrl import collect_hip as co
    from pdecontrol.mbrl import collection_phase as cp
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    E, Tn = 5, 3
    s = build(E, 64, 1, 12)
    sc.seed()
    sc.prime(s.worker, 11, stagger=False)
    counts = {}

    def counted(name, fn):
        def call(*args, **kwargs):
            counts[name] = counts.get(name, 0) + 1
            return fn(*args, **kwargs)
        return call

    for name in ("act", "observe", "act_span", "observe_span"):
        monkeypatch.setattr(co, name, counted(name, getattr(co, name)))
    stepper = s.env.stepper
    for name in ("step_device", "step_span", "record_device"):
        monkeypatch.setattr(stepper, name, counted(name, getattr(stepper, name)))
    got = cp.collect(s.worker, s.agent, lambda ts, ep: ts >= Tn * E)
    torch.cuda.synchronize()
    assert got.tier == "kernel" and got.host_steps == 0 and got.ntimesteps == Tn * E
    assert counts == {"act": Tn, "step_device": Tn, "observe": Tn}, counts
    counts.clear()
    got = cp.collect(s.worker, s.agent, lambda ts, ep: ts >= Tn * E, sink=DeviceExperienceReplay(device=DEV))
    torch.cuda.synchronize()
    assert got.tier == "kernel" and got.host_steps == 0
    assert counts == {"act": Tn, "step_device": Tn, "observe": Tn, "record_device": 1}, counts
