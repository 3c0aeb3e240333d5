"""The whole-segment collection kernels on the GPU (include/collect/span.h): ``co_act_span`` against the host action
wrapper and ``co_observe_span`` against ``T`` successive ``ScaleTransform.update`` + ``_affine`` + ``SensorTransform`` on
the host, bit for bit; the scripted tier of ``collect`` (``RandomAgent``, ``ActionRepeatAgent``) against the per-step loop
of ``Worker.rollout`` on the same GPU from the same seeds; and the launches a scripted segment makes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _collect_scenario as sc  # noqa: E402
import _real_replay_scenario as rr  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ENVS = (1, 5, 257)                        # one wave, a partial workgroup, several workgroups with a partial last one
FILL = -7.5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ----------------------------------------------------------------------------------------------------------------------
# co_act_span
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 4, 16])
def test_co_act_span_equals_the_host_wrapper(A):
    """Every row of the stepper's actions and of the action-store record, bit for bit: with and without the affine map,
    env-side and raw record; the guard rows before and behind the ``T * E * A`` outputs keep their fill."""
    from pdecontrol.mbrl import collect_hip as co
    from pdecontrol.mbrl.recognition import field_map
    from pdegym.common import transforms as T
    rs = np.random.RandomState(A)
    lo = rs.uniform(-2.0, -1.0, (1, 1, A)).astype(np.float32)
    hi = rs.uniform(1.0, 2.0, (1, 1, A)).astype(np.float32)
    scaling = T.ScaleTransform(bounds=(lo, hi), aggregate=False, frozen=True, batched=True).Inverse
    coef = field_map(scaling, A).coef.to(DEV)
    co.load()
    stream = co.stream()
    for E in ENVS:
        for Tn in (1, 3):
            raw = rs.uniform(-1, 1, (Tn, E, 1, A)).astype(np.float32)
            table = torch.from_numpy(raw).to(DEV).reshape(Tn, E, A).contiguous()
            before = table.clone()
            mapped = np.stack([scaling(raw[t]) for t in range(Tn)]).reshape(Tn, E, A)
            for with_map in (True, False):
                want_env = mapped if with_map else raw.reshape(Tn, E, A)
                for record_raw in (False, True):
                    geometry = co.Geometry(E, Tn, 64, A, 0, 1)
                    env_room = torch.full((Tn + 2, E, A), FILL, dtype=torch.float32, device=DEV)
                    act_room = torch.full((Tn + 2, E, A), FILL, dtype=torch.float32, device=DEV)
                    co.act_span(stream, geometry, co.act_span_args(table, coef if with_map else None, env_room[1:Tn + 1],
                                                                   act_room[1:Tn + 1], record_raw))
                    torch.cuda.synchronize()
                    label = (A, E, Tn, with_map, record_raw)
                    env_got, act_got = env_room.cpu().numpy(), act_room.cpu().numpy()
                    np.testing.assert_array_equal(_bits(env_got[1:Tn + 1]), _bits(want_env), err_msg=str(label))
                    want = raw.reshape(Tn, E, A) if record_raw else want_env
                    np.testing.assert_array_equal(_bits(act_got[1:Tn + 1]), _bits(want), err_msg=str(label))
                    for room in (env_got, act_got):
                        assert np.all(room[0] == FILL) and np.all(room[Tn + 1] == FILL), ("a guard row was written", label)
            assert torch.equal(table, before), "co_act_span wrote its table"


# ----------------------------------------------------------------------------------------------------------------------
# co_observe_span
# ----------------------------------------------------------------------------------------------------------------------
def _segment(rs, Tn, E, N, where, nan_slot=None):
    """[Tn + 1, E, N] normal draws.  The unique minimum and maximum of slots 1 ... Tn sit in slot ``where``; slot 0 holds
    values beyond both, the largest and the smallest of the whole block."""
    x = rs.standard_normal((Tn + 1, E, N)).astype(np.float32)
    lo, hi = np.float32(x.min() - 1.0), np.float32(x.max() + 1.0)
    x[where, E - 1, 1] = lo
    x[where, 0, N - 2] = hi
    x[0, 0, 0], x[0, E - 1, N - 1] = hi + np.float32(100.0), lo - np.float32(100.0)
    assert (x[1:] == lo).sum() == 1 and (x[1:] == hi).sum() == 1 and x[1:].min() == lo and x[1:].max() == hi
    assert x.max() == x[0].max() > hi and x.min() == x[0].min() < lo
    if nan_slot is not None:
        x[nan_slot, E // 2, N // 2] = np.nan
    return x


def _slots(Tn):
    return sorted({1, (Tn + 1) // 2, Tn})


def _observe_cases(Tn):
    cases = [(where, "running", 1, None) for where in _slots(Tn)]
    cases += [(1, "unset", 1, None), (Tn, "unset_max", 1, None), (1, "unset_min", 1, None), (Tn, "frozen", 0, None),
              (1, "none", 0, None), (Tn, "running", 1, (Tn + 1) // 2)]
    return cases


def _check_observe_span(E, N, Tn, strides=(1, 4)):
    from pdecontrol.mbrl import collect_hip as co
    from pdegym.common import transforms as T
    co.load()
    stream = co.stream()
    rs = np.random.RandomState(E * 1000 + N + Tn)
    for stride in strides:
        start = stride // 2
        O = len(range(start, N, stride))
        geometry = co.Geometry(E, Tn, N, 4, start, stride)
        floats = co.span_workspace_floats(geometry)
        assert floats == 2 * min(-(-(Tn * E) // 4), co.SPAN_MAX_PARTS)
        room = torch.full((floats + 8,), float("nan"), dtype=torch.float32, device=DEV)
        workspace = room[4:4 + floats]                                 # 16-byte aligned, guards around it
        for where, kind, update, nan_slot in _observe_cases(Tn):
            host = _segment(rs, Tn, E, N, where, nan_slot)
            traj = torch.from_numpy(host).to(DEV)
            before = traj.clone()
            scale, bounds, cell0 = None, None, None
            if kind != "none":
                scale = T.ScaleTransform(batched=True, aggregate=True, frozen=False)
                if kind in ("running", "frozen", "unset_max"):
                    scale.vmin = torch.full((1, 1, 1), -0.5)
                if kind in ("running", "frozen", "unset_min"):
                    scale.vmax = torch.full((1, 1, 1), 0.5)
                cell0 = (float(scale.vmin), float(scale.vmax))
                bounds = torch.tensor([*cell0, 123.0, -123.0], dtype=torch.float32, device=DEV)
            pobs = torch.full((E, O), FILL, dtype=torch.float32, device=DEV)
            room.fill_(float("nan"))
            co.observe_span(stream, geometry, co.observe_args(traj, pobs, bounds, -1.0, 1.0, update, workspace))
            torch.cuda.synchronize()
            # the host: T successive updates, then the affine map and the sensor of the last block
            if scale is not None and update:
                for t in range(1, Tn + 1):
                    scale.update(host[t][:, None, :])
            last = host[Tn][:, None, :]
            want = T.SensorTransform(stride)(last if scale is None else scale(last)).reshape(E, O)
            label = (E, N, Tn, stride, where, kind, nan_slot)
            got = pobs.cpu().numpy()
            if nan_slot is None:
                np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=str(label))
            else:
                assert np.isnan(want).all() and np.isnan(got).all(), label
            if scale is not None:
                cells = bounds.cpu().numpy().reshape(2, 2)
                assert (cells[0, 0], cells[0, 1]) == (np.float32(cell0[0]), np.float32(cell0[1])), ("cell 0 was written", label)
                if update and nan_slot is None:
                    assert (cells[1, 0], cells[1, 1]) == (float(scale.vmin), float(scale.vmax)), label
                    assert (cells[1, 0], cells[1, 1]) == (host[1:].min(), host[1:].max()), label
                    assert cells[1, 1] < host[0].max() and cells[1, 0] > host[0].min(), ("slot 0 reached the bounds", label)
                elif update:
                    assert np.isnan(cells[1]).all() and bool(torch.isnan(scale.vmin)) and bool(torch.isnan(scale.vmax)), label
                else:
                    assert cells[1].tolist() == [123.0, -123.0], ("a frozen scaling wrote its bounds", label)
            guards = room.cpu().numpy()
            assert np.isnan(guards[:4]).all() and np.isnan(guards[4 + floats:]).all(), ("the workspace's guards", label)
            assert torch.equal(traj.view(torch.int32), before.view(torch.int32)), "co_observe_span wrote the trajectory"


@pytest.mark.parametrize("E,N", [(E, N) for N in (64, 98, 100, 256) for E in ENVS])
def test_co_observe_span_equals_successive_host_updates(E, N):
    """``policy_obs`` bit for bit and the bounds by value for T = 1 and 3, the sensors (0, 1) and (2, 4): the extrema of
    slots 1 ... T in slot 1, a middle slot and slot T, the largest and the smallest value of all in slot 0 (they must not
    reach the bounds), unset bounds, one unset bound either way, a NaN in a middle slot, a frozen scaling, no scaling.
    Cell 0 is unchanged, cell 1 written only with ``update = 1``, ``traj`` untouched."""
    for Tn in (1, 3):
        _check_observe_span(E, N, Tn)


def test_co_observe_span_walks_the_rows_with_a_grid_stride():
    """E = 1025, T = 5: 1282 row groups over CO_SPAN_MAX_PARTS = 1024 workgroups."""
    from pdecontrol.mbrl import collect_hip as co
    assert -(-(5 * 1025) // 4) > co.SPAN_MAX_PARTS
    _check_observe_span(1025, 64, 5)


# ----------------------------------------------------------------------------------------------------------------------
# the scripted tier against the loop
# ----------------------------------------------------------------------------------------------------------------------
def _space_state(space):
    rng = getattr(space, "_rng", None)
    if rng is None:
        rng = space.np_random
    return rng.bit_generator.state


def _agent(kind, stack, E):
    from pdecontrol.mbrl import utils
    space = stack.envs.action_space
    space.seed(7)
    if kind == "random":
        return utils.RandomAgent(space), space
    table = np.random.RandomState(17).uniform(-1, 1, (E, 16, 1, 4)).astype(np.float32)
    return utils.ActionRepeatAgent(table), space


def _run(route, kind, E, N, stride, tmax=1.0, with_sink=False, steps=7, calls=3):
    """``calls`` warm-up phases in a row on the collection stack, then one on the evaluation stack (the same scaling,
    frozen).  ``route``: "loop" is ``Worker.rollout`` into a host replay, "collect" the phase under test."""
    from pdecontrol.mbrl import collection_phase as cp
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    from pdecontrol.mbrl.replay import ExperienceReplay
    s = sc.build(E=E, N=N, device=0, agent_device="cuda:0", agent_stride=stride, tmax=tmax)
    sc.seed()
    sc.prime(s.worker, 11)
    agent, space = _agent(kind, s.stack, E)
    stop = lambda ts, ep: ts >= steps
    sink = DeviceExperienceReplay(device=DEV) if with_sink and route == "collect" else None
    total = ExperienceReplay() if sink is None else sink
    out = []
    for worker, n in ((s.worker, calls), (s.eval_worker, 1)):
        if worker is s.eval_worker:                                    # (without a sink: nothing is committed)
            sc.prime(worker, 5)
            agent, space = _agent(kind, s.eval_stack, E)
            sink = None
        for _ in range(n):
            ks = worker.stack.ostore.env
            plan = cp.plan_phase(ks.timestep, ks.max_episode_steps, E, stop)
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
            record = sc.state_record(worker)
            record["space"] = _space_state(space)
            record["nstep"] = getattr(agent, "nstep", None)
            out.append((phase, record, plan))
    return out, total


def _same_rows(a, b, what):
    """The fields of two host replays as the slabs hold them (fp32 rewards, int32 steps), byte for byte."""
    assert a.episodes == b.episodes and dict(a.vindex) == dict(b.vindex) and a.ntimesteps == b.ntimesteps, what
    for name, dt in zip(rr.FIELDS, (np.float32, np.float32, np.float32, np.float32, np.bool_, np.bool_, np.int32)):
        x, y = getattr(a, name), getattr(b, name)
        assert list(x.keys()) == list(y.keys()), (what, name)
        for key in y:
            assert np.asarray(x[key], dtype=dt).tobytes() == np.asarray(y[key], dtype=dt).tobytes(), (what, name, key)


def _compare(loop, scripted, with_sink):
    (loop_out, loop_total), (out, total) = loop, scripted
    assert len(loop_out) == len(out)
    for i, ((a, sa, _), (b, sb, plan)) in enumerate(zip(loop_out, out)):
        assert b.tier == "kernel" and b.tier_reason is None, (b.tier, b.tier_reason)
        assert b.host_steps == len(plan.truncations) and plan.K * len(plan.timestep) == b.ntimesteps
        if with_sink:
            _same_rows(b, a, i)
        else:
            sc.assert_same_replay(a, b)
        assert sa.pop("space") == sb.pop("space"), "the action space's generator"
        assert sa.pop("nstep") == sb.pop("nstep")
        sc.assert_same_state(sa, sb)
    if with_sink:
        rr.same_metadata(total, loop_total)
        rr.pack_contract(total, loop_total)


CASES = [(5, 64, 1, 1.0), (3, 256, 4, 1.0), (5, 64, 1, 3.0)]


@pytest.mark.parametrize("kind", ["random", "repeat"])
@pytest.mark.parametrize("with_sink", [False, True])
@pytest.mark.parametrize("E,N,stride,tmax", CASES)
def test_scripted_tier_equals_the_loop(E, N, stride, tmax, with_sink, kind):
    """Three warm-up phases in a row (``ts >= 7``) and one on the frozen evaluation stack, counters staggered, with
    ``max_episode_steps = 4`` (nearly every step truncates) and 12 (multi-step segments): every field of every episode,
    keys and vindex, the worker's observations, the stores, the bounds, ``env.timestep``, the stepper's state, the MT
    streams, numpy's, torch's and the action space's generators and ``agent.nstep``, bit for bit; through a sink, the
    staged rows, the metadata and the pack contract."""
    loop = _run("loop", kind, E, N, stride, tmax)
    scripted = _run("collect", kind, E, N, stride, tmax, with_sink)
    _compare(loop, scripted, with_sink)
    if tmax == 1.0:
        assert sum(len(plan.truncations) for _, _, plan in scripted[0][:3]) >= 3, "the phases crossed no truncation"
    else:
        assert all(len(plan.truncations) < plan.K for _, _, plan in scripted[0])


def test_scripted_tier_runs_long_segments_across_a_truncation():
    """``max_episode_steps = 12`` with ``ts >= 7 E``: segments of up to seven steps, a truncation step between two."""
    E = 5
    loop = _run("loop", "random", E, 64, 1, 3.0, steps=7 * E)
    scripted = _run("collect", "random", E, 64, 1, 3.0, with_sink=True, steps=7 * E)
    _compare(loop, scripted, True)
    assert sum(len(plan.truncations) for _, _, plan in scripted[0][:3]) >= 1


# ----------------------------------------------------------------------------------------------------------------------
# launches
# ----------------------------------------------------------------------------------------------------------------------
def test_a_scripted_segment_is_one_act_span_t_steps_and_one_observe_span(monkeypatch):
    from pdecontrol.mbrl import collect_hip as co
    from pdecontrol.mbrl import collection_phase as cp
    E, Tn = 5, 3
    s = sc.build(E=E, N=64, device=0, agent_device="cuda:0", tmax=3.0)
    sc.seed()
    sc.prime(s.worker, 11, stagger=False)
    agent, _ = _agent("random", s.stack, E)
    counts = {}

    def counted(name, fn):
        def call(*args, **kwargs):
            counts[name] = counts.get(name, 0) + 1
            return fn(*args, **kwargs)
        return call

    for name in ("act", "observe", "act_span", "observe_span"):
        monkeypatch.setattr(co, name, counted(name, getattr(co, name)))
    stepper = s.env.stepper
    monkeypatch.setattr(stepper, "step_device", counted("step_device", stepper.step_device))
    monkeypatch.setattr(stepper, "record_device", counted("record_device", stepper.record_device))
    got = cp.collect(s.worker, agent, lambda ts, ep: ts >= Tn * E)
    torch.cuda.synchronize()
    assert got.tier == "kernel" and got.host_steps == 0 and got.ntimesteps == Tn * E
    assert counts == {"act_span": 1, "step_device": Tn, "observe_span": 1}, counts
