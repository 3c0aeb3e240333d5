"""The real-env collection phase on the GPU: ``co_act`` against the host action wrapper and ``co_observe`` against a
numpy twin (``ScaleTransform.update`` + ``_affine`` + ``SensorTransform``) bit for bit, and the kernel tier of ``collect``
against the per-step loop of ``Worker.rollout`` on the same GPU from the same seeds."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _collect_scenario as sc  # noqa: E402

pytestmark = pytest.mark.gpu

ENVS = (1, 5, 257)                        # one wave, a partial workgroup, several workgroups with a partial last one
FILL = -7.5


def _dev():
    return torch.device("cuda", 0)


# ----------------------------------------------------------------------------------------------------------------------
# co_act
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 4, 16])
def test_co_act_equals_the_host_wrapper(A):
    """The stepper's action rows and the action-store record, bit for bit: with and without the affine map, env-side and
    raw record; only slot ``t`` of ``actions`` is written."""
    from pdecontrol.mbrl import collect_hip as co
    from pdecontrol.mbrl.recognition import field_map
    from pdegym.common import transforms as T
    dev, stream = _dev(), None
    rs = np.random.RandomState(A)
    lo = rs.uniform(-2.0, -1.0, (1, 1, A)).astype(np.float32)
    hi = rs.uniform(1.0, 2.0, (1, 1, A)).astype(np.float32)
    scaling = T.ScaleTransform(bounds=(lo, hi), aggregate=False, frozen=True, batched=True).Inverse
    coef = field_map(scaling, A).coef.to(dev)
    co.load()
    stream = co.stream()
    for E in ENVS:
        raw = rs.uniform(-1, 1, (E, 1, A)).astype(np.float32)
        action = torch.from_numpy(raw).to(dev).reshape(E, A).contiguous()
        for with_map in (True, False):
            want_env = scaling(raw) if with_map else raw
            for record_raw in (False, True):
                Tn, t = 3, 1
                geometry = co.Geometry(E, Tn, 64, A, 0, 1)
                env_action = torch.full((E, A), FILL, dtype=torch.float32, device=dev)
                actions = torch.full((Tn, E, A), FILL, dtype=torch.float32, device=dev)
                co.act(stream, geometry, co.act_args(action, coef if with_map else None, env_action, actions, record_raw), t)
                torch.cuda.synchronize()
                np.testing.assert_array_equal(env_action.cpu().numpy().view(np.int32), want_env.reshape(E, A).view(np.int32))
                got = actions.cpu().numpy()
                want = (raw if record_raw else want_env).reshape(E, A)
                np.testing.assert_array_equal(got[t].view(np.int32), want.view(np.int32))
                assert np.all(got[0] == FILL) and np.all(got[2] == FILL), "a slot other than t was written"


# ----------------------------------------------------------------------------------------------------------------------
# co_observe
# ----------------------------------------------------------------------------------------------------------------------
def _block(rs, E, N, placement):
    """Normal fp32 draws with unique, non-zero extrema placed where ``placement`` says."""
    x = rs.standard_normal((E, N)).astype(np.float32)
    lo, hi = np.float32(x.min() - 1.0), np.float32(x.max() + 1.0)
    flat = {"min_first": ((0, 0), None), "max_last": (None, (E - 1, N - 1)), "last_group": ((E - 1, 1), (E - 1, N - 2)),
            "inside": (None, None)}[placement]
    if flat[0] is not None:
        x[flat[0]] = lo
    if flat[1] is not None:
        x[flat[1]] = hi
    assert (x == x.min()).sum() == 1 and (x == x.max()).sum() == 1 and x.min() != 0 and x.max() != 0
    return x


def _twin(scale, obs, update, stride):
    """What the wrappers compute on the host: ``ScaleTransform.update`` (aggregate, batched), ``_affine``, the sensor."""
    from pdegym.common import transforms as T
    if scale is None:
        return T.SensorTransform(stride)(obs)
    if update:
        scale.update(obs)
    return T.SensorTransform(stride)(scale(obs))


@pytest.mark.parametrize("E,N", [(E, N) for N in (64, 98, 100, 256) for E in ENVS] + [(1025, 64)])
def test_co_observe_equals_the_numpy_twin(E, N):
    """``policy_obs`` bit for bit, the bounds by value, ``traj`` untouched: four extrema placements over two steps in a
    row (both ping-pong cells carry a value), unset bounds at the first step, a frozen scaling, and no scaling at all,
    for the sensors (0, 1) and (2, 4).  E = 1025 at N = 64 gives 257 partials: more than a wave has lanes."""
    from pdecontrol.mbrl import collect_hip as co
    from pdegym.common import transforms as T
    dev = _dev()
    co.load()
    stream = co.stream()
    rs = np.random.RandomState(E * 1000 + N)
    Tn = 2
    for stride in (1, 4):
        start = stride // 2
        O = len(range(start, N, stride))
        geometry = co.Geometry(E, Tn, N, 4, start, stride)
        workspace = torch.full((co.workspace_floats(geometry),), float("nan"), dtype=torch.float32, device=dev)
        cases = [(p, "running", 1) for p in ("min_first", "max_last", "last_group", "inside")]
        cases += [("min_first", "unset", 1), ("last_group", "frozen", 0), ("max_last", "none", 0)]
        for placement, kind, update in cases:
            blocks = [_block(rs, E, N, placement), _block(rs, E, N, "last_group" if placement == "inside" else placement)]
            host = np.stack([np.full((E, N), FILL, dtype=np.float32)] + blocks)
            traj = torch.from_numpy(host).to(dev)
            before = traj.clone()
            scale, bounds = None, None
            if kind != "none":
                scale = T.ScaleTransform(batched=True, aggregate=True, frozen=False)
                if kind != "unset":
                    first = blocks[0]
                    inside = placement == "inside"
                    scale.vmin = torch.full((1, 1, 1), float(first.min()) - 1.0 if inside else -0.5)
                    scale.vmax = torch.full((1, 1, 1), float(first.max()) + 1.0 if inside else 0.5)
                v0, v1 = float(scale.vmin), float(scale.vmax)
                # cell 0 is read by step 0; a frozen scaling has both cells set; the other cell of a running one is junk
                junk = (v0, v1) if kind == "frozen" else (123.0, -123.0)
                bounds = torch.tensor([v0, v1, *junk], dtype=torch.float32, device=dev)
            pobs = torch.full((E, O), FILL, dtype=torch.float32, device=dev)
            args = co.observe_args(traj, pobs, bounds, -1.0, 1.0, update, workspace)
            for t in range(Tn):
                co.observe(stream, geometry, args, t)
                torch.cuda.synchronize()
                want = _twin(scale, blocks[t][:, None, :], update, stride).reshape(E, O)
                label = (stride, placement, kind, t)
                np.testing.assert_array_equal(pobs.cpu().numpy().view(np.int32), want.view(np.int32), err_msg=str(label))
                if scale is not None:
                    cells = bounds.cpu().numpy().reshape(2, 2)
                    if update:
                        got = cells[(t + 1) & 1]
                        assert got[0] == float(scale.vmin) and got[1] == float(scale.vmax), label
                        if placement == "inside" and t == 0:
                            assert (got[0], got[1]) == (np.float32(v0), np.float32(v1)), "bounds inside: unchanged"
                    else:
                        assert cells.tolist() == [[np.float32(v0), np.float32(v1)]] * 2, "a frozen scaling wrote its bounds"
            assert torch.equal(traj, before), "co_observe wrote the trajectory"


# ----------------------------------------------------------------------------------------------------------------------
# the phase
# ----------------------------------------------------------------------------------------------------------------------
def _sampling(E):
    return lambda ts, ep: ts >= 3 * E


def _run(route, E, N, stride, obs_steps=1, tmax=1.0, calls=3, eval_episodes=2, stagger=True):
    """Three consecutive sampling phases on the collection worker, then one evaluation phase on the evaluation worker:
    [(replay, state record)] per call."""
    from pdecontrol.mbrl import collection_phase as cp
    s = sc.build(E=E, N=N, device=0, agent_device="cuda:0", agent_stride=stride, obs_steps=obs_steps, tmax=tmax)
    sc.seed()
    sc.prime(s.worker, 11, stagger=stagger)
    callback = sc.Callback()
    s.worker.callbacks.append(callback)
    out = []
    phases = [(s.worker, _sampling(E), calls)]
    if eval_episodes:
        phases.append((s.eval_worker, lambda ts, ep: ep >= eval_episodes, 1))
    for worker, stop, n in phases:
        if worker is s.eval_worker:
            sc.prime(worker, 5)
        for _ in range(n):
            ks = worker.stack.ostore.env
            plan = cp.plan_phase(ks.timestep, ks.max_episode_steps, E, stop)      # host integers only
            replay = worker.rollout(s.agent, stop) if route == "loop" else cp.collect(worker, s.agent, stop)
            torch.cuda.synchronize()
            out.append((replay, sc.state_record(worker), plan))
    assert callback.seen == [r for r, _, _ in out[:calls]]
    return out, s


def _compare(loop, kernel, tier, reason=None):
    for (a, sa, _), (b, sb, plan) in zip(loop, kernel):
        sc.assert_same_replay(a, b)
        sc.assert_same_state(sa, sb)
        assert tuple(sb["vmin"].shape) == (1, 1, 1) and sb["vmin"].dtype == torch.float32
        assert b.tier == tier, (b.tier, b.tier_reason)
        assert plan.K * len(plan.timestep) == b.ntimesteps
        if tier == "kernel":
            assert b.host_steps == len(plan.truncations) and b.tier_reason is None
        else:
            assert reason in b.tier_reason and b.host_steps == plan.K


@pytest.mark.parametrize("E,N,stride", [(5, 64, 1), (3, 256, 4)])
def test_kernel_tier_equals_the_loop(E, N, stride):
    """Three consecutive sampling phases (``ts >= 3 E``) crossing several truncation steps, then the evaluation stack
    with ``ep >= 2``, with ``env.timestep`` staggered to [0, 1, 2, 3, 0]: every field of every episode, keys and vindex,
    the worker's observations, the stores, the bounds, ``env.timestep``, the stepper's state, the MT streams and numpy's
    and torch's generators, bit for bit."""
    loop, _ = _run("loop", E, N, stride)
    kernel, _ = _run("collect", E, N, stride)
    _compare(loop, kernel, "kernel")
    assert sum(r.nstopped for r, _, _ in kernel[:3]) >= 3, "the sampling phases crossed no truncation"


def test_kernel_tier_runs_multi_step_segments():
    """``max_episode_steps = 12``: segments of several steps (both ping-pong cells of the running bounds carry a value
    inside a segment), an evaluation phase whose frozen scaling runs inside segments, and a byte budget that cuts a run of
    steps into segments of one."""
    from pdecontrol.mbrl import collection_phase as cp
    E, N = 5, 64
    loop, _ = _run("loop", E, N, 1, tmax=3.0, eval_episodes=3)
    for budget in (None, 2 * E * N * 4 + 4 * E * 20):
        saved = cp.SEGMENT_BYTES
        if budget is not None:
            cp.SEGMENT_BYTES = budget
            assert cp.segment_steps(E, N, 4) == 1
        try:
            kernel, _ = _run("collect", E, N, 1, tmax=3.0, eval_episodes=3)
        finally:
            cp.SEGMENT_BYTES = saved
        _compare(loop, kernel, "kernel")
        assert [r.host_steps for r, _, _ in kernel[:3]] == [0, 0, 1]      # counters 0 1 2 3 0 + 9 steps: env 3 ends at step 9


def test_a_two_step_observation_store_runs_the_loop():
    """One sampling phase from counters 0, so that no env truncates: at a truncation ``Worker.rollout`` itself cannot index
    the finals of a two-step store (on any device), and this test is about the tier choice."""
    kwargs = dict(obs_steps=2, calls=1, eval_episodes=0, stagger=False)
    loop, _ = _run("loop", 5, 64, 1, **kwargs)
    kernel, _ = _run("collect", 5, 64, 1, **kwargs)
    assert len(kernel) == 1 and kernel[0][0].ntimesteps == 15
    _compare(loop, kernel, "loop", "an observation store of 2 steps")


# ----------------------------------------------------------------------------------------------------------------------
# launches
# ----------------------------------------------------------------------------------------------------------------------
def test_a_sac_segment_is_t_times_act_step_observe(monkeypatch):
    """One segment of three steps: three ``co_act``, three ``ks_step_device`` and three ``co_observe`` calls and no span
    call; through a sink, one ``ks_record_device`` call more."""
    from pdecontrol.mbrl import collect_hip as co
    from pdecontrol.mbrl import collection_phase as cp
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    E, Tn = 5, 3
    s = sc.build(E=E, N=64, device=0, agent_device="cuda:0", tmax=3.0)
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
        if hasattr(stepper, name):
            monkeypatch.setattr(stepper, name, counted(name, getattr(stepper, name)))
    got = cp.collect(s.worker, s.agent, lambda ts, ep: ts >= Tn * E)
    torch.cuda.synchronize()
    assert got.tier == "kernel" and got.host_steps == 0 and got.ntimesteps == Tn * E
    assert counts == {"act": Tn, "step_device": Tn, "observe": Tn}, counts
    counts.clear()
    got = cp.collect(s.worker, s.agent, lambda ts, ep: ts >= Tn * E, sink=DeviceExperienceReplay(device=torch.device("cuda", 0)))
    torch.cuda.synchronize()
    assert got.tier == "kernel" and got.host_steps == 0
    assert counts == {"act": Tn, "step_device": Tn, "observe": Tn, "record_device": 1}, counts
