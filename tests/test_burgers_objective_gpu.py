"""The dissipation objective of the Burgers env on an MI355X: ``bg_step_objective`` and ``bg_step_span_objective`` against the
host twin and against ``bg_step`` (bit for bit), ``bg_reward_rows`` against its host twin, ``ro_settle_burgers_dissipation``
against ``ro_settle`` and the fp64 twin of its reward, and the phases of the controller over a dissipation env: collection,
imagination and the toy ``learn()``.  Inputs, references and bounds: tests/_burgers_objective.py."""
import itertools
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _burgers_cases as bc  # noqa: E402
import _burgers_objective as ob  # noqa: E402
import _burgers_world_scenario as bw  # noqa: E402
from _rollout_scenario import fma_chain  # noqa: E402
from hipbind import ptr  # noqa: E402
from test_burgers_gpu import DEV, NAN_BITS, STATUS_SENTINEL, _dev, _padded, _stream, _untouched, hip, step  # noqa: E402,F401
from test_imagination_dissipation_gpu import (BATCHES, FILL, MEMBERS, T_NOW, T_SLOTS, _coef, _guarded,  # noqa: E402
                                              _guards_untouched)

pytestmark = pytest.mark.gpu

L2, DISS = 0, 1
KEYS = ("u", "obs", "ssq", "status")


# ----------------------------------------------------------------------------------------------------------------------
# the stepper
# ----------------------------------------------------------------------------------------------------------------------
def step_objective(hip, u0, act, F, N, n, objective):
    """One ``bg_step_objective`` launch on padded buffers (tests/test_burgers_gpu.py::step): the E rows of every output."""
    dx, dt, nu = bc.params(N)
    E = u0.shape[0]
    u, o = _padded(u0), _padded((E, N))
    q, st = _padded((E,), dtype=torch.float64), _padded((E,), fill=STATUS_SENTINEL, dtype=torch.int32)
    a, f = _dev(act), _dev(F)
    hip.check_objective(hip.load().bg_step_objective(_stream(), ptr(u), ptr(a), ptr(f), 0 if act is None else act.shape[1], E, N,
                                                     dx, dt, nu, n, ptr(o), ptr(q), ptr(st), objective))
    torch.cuda.synchronize(DEV)
    for t, what in ((u, "u"), (o, "obs"), (q, "ssq_sum"), (st, "status")):
        _untouched(t, f"{what} (E = {E}, N = {N}, objective {objective})")
    return {k: t[:-1].cpu().numpy() for k, t in zip(KEYS, (u, o, q, st))}


def _same_bytes(got, want, what, keys=KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert got[k].tobytes() == want[k].tobytes(), f"{what}: {k} differs"


@pytest.mark.parametrize("N", [64, 128, 256, 512, 1024])                 # every P
def test_step_objective_has_the_bits_of_the_host_twin_and_of_bg_step(hip, N):
    """Both objectives, E = 1, 3, 5 (tail waves), 0, 1, 2 and 50 sub-steps, no forcing and 1, 4, 16 actuators: u, obs,
    status and the fp64 sum bit for bit the host twin's, the padding intact, a second launch bit-equal, and objective 0
    byte for byte ``bg_step``."""
    dx, dt, nu = bc.params(N)
    lib = hip.load()
    for E, n, A in itertools.product((1, 3, 5), (0, 1, 2, 50), (0, 1, 4, 16)):
        u0, act, F = ob.inputs(N, E, A)
        for objective in (L2, DISS):
            what = f"N{N}-E{E}-n{n}-act{A}-objective{objective}"
            got = step_objective(hip, u0, act, F, N, n, objective)
            u, obs, ssq, status = ob.host_step(lib, u0, act, F, N, n, objective)
            _same_bytes(got, dict(u=u, obs=obs, ssq=ssq, status=status), f"{what} against the host twin")
            _same_bytes(step_objective(hip, u0, act, F, N, n, objective), got, f"{what}, a second launch")
            if objective == L2:
                _same_bytes(got, step(hip, u0, act, F, dx, dt, nu, n), f"{what} against bg_step")
            else:
                assert n == 0 or (got["ssq"] != 0).all(), what


@pytest.mark.parametrize("objective", [L2, DISS])
@pytest.mark.parametrize("N", [64, 256, 1024])
def test_status_rises_for_the_row_with_an_inf_alone(hip, N, objective):
    u0, act, F = ob.inputs(N, 5, 4)
    clean = step_objective(hip, u0, act, F, N, 2, objective)
    bad = u0.copy()
    bad[2, 7] = np.inf
    got = step_objective(hip, bad, act, F, N, 2, objective)
    assert got["status"].tolist() == [0, 0, 1, 0, 0] and not clean["status"].any()
    keep = [0, 1, 3, 4]
    for k in KEYS:
        assert got[k][keep].tobytes() == clean[k][keep].tobytes(), (N, objective, k)
    lib = hip.load()
    u, obs, ssq, status = ob.host_step(lib, bad, act, F, N, 2, objective)
    assert status.tolist() == [0, 0, 1, 0, 0] and got["u"][keep].tobytes() == u[keep].tobytes()


def _span_inputs(N, E, T):
    u0, _, F = ob.inputs(N, E, 4)
    return u0, np.stack([bc.actions(31 + N + 17 * t, E, 4) for t in range(T)]), F


def _span_buffers(u0, T):
    E, N = u0.shape
    return (_padded(u0), torch.full((T + 2, E, N), float("nan"), dtype=torch.float32, device=DEV),
            _padded((T * E,), dtype=torch.float64), _padded((T * E,), fill=STATUS_SENTINEL, dtype=torch.int32))


def _span_finish(u, traj, q, st, T, what):
    torch.cuda.synchronize(DEV)
    E = u.shape[0] - 1
    for t, name in ((u, "u"), (q, "ssq"), (st, "status")):
        _untouched(t, f"{what}: {name}")
    t = traj.cpu().numpy()
    assert (t[0].view(np.uint32) == NAN_BITS).all() and (t[T + 1].view(np.uint32) == NAN_BITS).all(), f"{what}: a slot outside 1 .. T"
    return {"u": u[:-1].cpu().numpy(), "traj": t[1:T + 1], "ssq": q[:-1].cpu().numpy().reshape(T, E),
            "status": st[:-1].cpu().numpy().reshape(T, E)}


@pytest.mark.parametrize("objective", [L2, DISS])
@pytest.mark.parametrize("N,E", [(64, 5), (256, 3), (1024, 2)])
def test_span_objective_is_t_step_launches_and_replays_in_a_graph(hip, N, E, objective):
    """T = 1, 3: u, traj[1 .. T], ssq and status byte for byte those of T ``bg_step_objective`` launches; the same launch
    captured in a hipGraph and replayed gives the same bytes again."""
    from pdecontrol.surrogates.graph_step import capture_graph
    from pdecontrol.surrogates.hipops import pooled_streams
    dx, dt, nu = bc.params(N)
    lib, n = hip.load(), 2
    for T in (1, 3):
        what = f"N{N}-E{E}-T{T}-objective{objective}"
        u0, acts, F = _span_inputs(N, E, T)
        a, f = _dev(acts), _dev(F)

        def launch_span(u, traj, q, st):
            hip.check_objective(lib.bg_step_span_objective(_stream(), ptr(u), ptr(a), ptr(f), 4, E, N, T, dx, dt, nu, n, ptr(traj),
                                                           ptr(q), ptr(st), objective))

        bufs = _span_buffers(u0, T)
        launch_span(*bufs)
        got = _span_finish(*bufs, T, f"span {what}")
        u, traj, q, st = _span_buffers(u0, T)
        for t in range(T):
            hip.check_objective(lib.bg_step_objective(_stream(), ptr(u), ptr(a[t]), ptr(f), 4, E, N, dx, dt, nu, n, ptr(traj[t + 1]),
                                                      ptr(q[t * E:]), ptr(st[t * E:]), objective))
        want = _span_finish(u, traj, q, st, T, f"launches {what}")
        _same_bytes(got, want, what, keys=("u", "traj", "ssq", "status"))
        assert not got["status"].any() and (got["ssq"] != 0).all()
        # the graph: warm-up and capture on a side stream, then the inputs again and one replay
        bufs = _span_buffers(u0, T)
        (side,) = pooled_streams(DEV, 1, "capture")
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            launch_span(*bufs)
        graph = torch.cuda.CUDAGraph()
        capture_graph(graph, lambda: launch_span(*bufs), side)
        torch.cuda.current_stream(DEV).wait_stream(side)
        fresh = _span_buffers(u0, T)
        for dst, src in zip(bufs, fresh):
            dst.copy_(src)
        graph.replay()
        _same_bytes(_span_finish(*bufs, T, f"graph {what}"), got, f"{what}, replayed in a graph", keys=("u", "traj", "ssq", "status"))


# ----------------------------------------------------------------------------------------------------------------------
# the row reward
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [5, 16, 64, 98, 512, 1024])
def test_reward_rows_against_the_host_twin(hip, N):
    """The host twin sums a row in index order, the kernel per lane (points gl, gl + G, ...) and then across the group: the
    group's tree is NOT reproduced on the host, so the two are held to 2^-52 N of the sum of the absolute terms,
    2^-52 N (nu <ux^2> + <|u phi|>) in the reward's units (each of the N - 1 fp64 additions of either order is within
    2^-53 of a partial sum that the sum of absolute terms bounds).  M = 1, 5 and 37 rows: one group, a partial block, more
    than one block; a field, actions through the forcing chain, and no forcing; the padding intact; two runs equal."""
    lib = hip.load()
    rs = np.random.RandomState(N)
    dx, nu = 2 * np.pi / N, 0.01
    worst = 0.0
    for M in (1, 5, 37):
        u = ob.smooth(3 + N, M, N) + 0.05 * rs.uniform(-1, 1, (M, N)).astype(np.float32)
        phi = rs.uniform(-1, 1, (M, N)).astype(np.float32)
        act, F = rs.uniform(-1, 1, (M, 4)).astype(np.float32), rs.uniform(-1, 1, (4, N)).astype(np.float32)
        for field, actions in ((phi, None), (None, act), (None, None)):
            runs = []
            for _ in range(2):
                out = _padded((M,), dtype=torch.float64)
                keep = [_dev(u), _dev(field), _dev(actions), _dev(F if actions is not None else None)]
                hip.check_objective(lib.bg_reward_rows(_stream(), *(ptr(t) for t in keep), M, N, 4, dx, nu, ptr(out)))
                torch.cuda.synchronize(DEV)
                _untouched(out, f"reward N{N} M{M}")
                runs.append(out[:-1].cpu().numpy())
            assert runs[0].tobytes() == runs[1].tobytes(), "two runs differ"
            host = np.full(M, np.nan)
            rc = lib.bg_reward_rows_host(ob.ptr(u), ob.ptr(field), ob.ptr(actions), ob.ptr(F) if actions is not None else None, M, N, 4,
                                         dx, nu, ob.ptr(host))
            assert rc == 0
            used = field if field is not None else (fma_chain(act, F) if actions is not None else np.zeros_like(u))
            d, pabs = ob.row_reward_terms(u, used, dx, nu)
            bound = 2.0 ** -52 * N * (d + pabs)
            err = np.abs(runs[0] - host)
            worst = max(worst, float((err / bound).max()))
            assert np.isfinite(runs[0]).all() and (err <= bound).all(), (N, M, err / bound)
    print(f"bg_reward_rows against its host twin at N={N}: worst difference {worst:.3f} of the bound")


# ----------------------------------------------------------------------------------------------------------------------
# the settle kernel
# ----------------------------------------------------------------------------------------------------------------------
NU_SETTLE = 0.05


def _settle_case(N, A, B, with_reward_coef, with_in_coef, spike_row):
    """The inputs of tests/test_imagination_dissipation_gpu.py::_kernel_case on the Burgers grid (dx = 2 pi / N) and the fp64
    twin of the Burgers reward: smooth rows lifted by 1.5 so that u keeps its sign, and at ``spike_row`` a row that is zero
    but for spikes at columns 0 and N - 1, which a wrong periodic wrap moves out of the stencil that must see them."""
    from pdecontrol.mbrl.recognition import FieldMap
    rs = np.random.RandomState(1000 * N + 10 * A + B + (5 if with_reward_coef else 0) + (3 if with_in_coef else 0))
    dx = 2.0 * np.pi / N
    x = np.linspace(0, 2 * np.pi, N, endpoint=False)
    phase = rs.uniform(0, 6, (MEMBERS, B, 1))
    u = (1.5 + 0.25 * (np.sin(x + phase) + 0.5 * np.cos(2 * x - 0.7 * phase))).astype(np.float32)
    reward = _coef(rs, N, -1.0, 2.0, 6.0, -3.0) if with_reward_coef else FieldMap(0, 1, N, None)
    if spike_row is not None:
        u[:, spike_row] = 0.0
        u[:, spike_row, 0], u[:, spike_row, N - 1] = 2.0, -1.5
    if with_reward_coef:
        a, ba, dc, c = (reward.coef[i].numpy() for i in range(4))
        members = ((u - c) / dc * ba + a).astype(np.float32)
    else:
        members = u
    act_in = _coef(rs, A, -1.0, 2.0, 1.5, -0.75) if with_in_coef else FieldMap(0, 1, A, None)
    centres = (np.arange(A) + 0.25) / A * 2 * np.pi
    dist = np.abs(x[None, :] - centres[:, None])
    F = np.exp(-0.5 * (np.minimum(dist, 2 * np.pi - dist) / 0.4) ** 2).astype(np.float32)
    actions = rs.uniform(-1, 1, (T_SLOTS, B, A)).astype(np.float32)
    chosen = rs.randint(0, MEMBERS, (T_SLOTS, B)).astype(np.int32)
    steps0 = rs.randint(0, 300, B).astype(np.int32)
    want = members[chosen[T_NOW], np.arange(B)]
    ref, scale = _reward_twin(want, actions[T_NOW], reward, act_in, F, dx, NU_SETTLE)
    return types.SimpleNamespace(members=members, actions=actions, chosen=chosen, steps0=steps0, F=F, reward=reward,
                                 act_in=act_in, dx=dx, want=want, ref=ref, scale=scale)


def _reward_twin(rows, raw_actions, reward, act_in, F, dx, nu):
    """(fp64 reward [n], mean_i(|u_i| sum_k |a_k| F_ki) [n]): the row reward of include/burgers/objective.h on the rescaled
    rows under the fp32 forcing chain of the scaled actions."""
    w = reward.apply_numpy(np.asarray(rows, dtype=np.float32))
    a = act_in.apply_numpy(np.asarray(raw_actions, dtype=np.float32))
    phi = fma_chain(a, F)
    scale = (np.abs(w.astype(np.float64)) * (np.abs(a).astype(np.float64) @ np.abs(F).astype(np.float64))).mean(axis=1)
    return ob.row_reward_numpy(w, phi, dx, nu), scale


def _settle(ro, c, N, A, B, sensor, dissipation):
    dev = torch.device("cuda", 0)
    d = lambda a: None if a is None else torch.as_tensor(a).to(dev).contiguous()
    g = ro.Geometry(B, T_SLOTS, N, A, N, 0, 1, sensor.start, sensor.stride, MEMBERS)
    mem = [d(m) for m in c.members]
    bufs = dict(state=_guarded((B, N), torch.float32, FILL, dev), traj=_guarded((T_SLOTS + 1, B, N), torch.float32, FILL, dev),
                pol=_guarded((B, sensor.width), torch.float32, FILL, dev), steps=_guarded((T_SLOTS, B), torch.int32, -1, dev),
                rewards=_guarded((T_SLOTS, B), torch.float32, FILL, dev), step=_guarded((2,), torch.int32, -5, dev))
    bufs["step"][1].copy_(torch.tensor((T_NOW, 9), dtype=torch.int32))
    keep = (d(c.chosen), d(c.steps0), d(c.reward.coef), d(c.actions), d(c.act_in.coef), d(c.F))
    args = ro.settle_args(mem, keep[0], bufs["state"][1], bufs["traj"][1], bufs["pol"][1], keep[1], bufs["steps"][1],
                          bufs["rewards"][1], keep[2], bufs["step"][1])
    if dissipation:
        ro.settle_burgers_dissipation(ro.stream(), g, args, ro.burgers_dissipation_args(keep[3], keep[4], keep[5], c.dx, NU_SETTLE))
    else:
        ro.settle(ro.stream(), g, args)
    torch.cuda.synchronize()
    fills = dict(state=FILL, traj=FILL, pol=FILL, steps=-1, rewards=FILL, step=-5)
    for name, (full, _) in bufs.items():
        assert _guards_untouched(full, fills[name]), f"{name}: written outside the output"
    return {name: view.cpu().numpy() for name, (_, view) in bufs.items()}


@pytest.mark.parametrize("A", [1, 4, 16])
@pytest.mark.parametrize("N", [16, 64, 98, 256, 1024])
def test_ro_settle_burgers_dissipation_settles_as_ro_settle_and_rewards_as_the_twin(N, A):
    """tests/test_imagination_dissipation_gpu.py's test of ``ro_settle_dissipation``, for this kernel: N = 16 leaves lanes
    idle, 98 takes the scalar path, the others the float4 path; three members with a chosen array, with and without each
    affine map, step 2 of 4.  Everything but the reward is ``ro_settle``'s, bit for bit; the reward lies within
        2^-23 |r| + (A + 1) 2^-24 mean_i(|u_i| sum_k |a_k| F_ki)
    of the fp64 twin; two runs are equal."""
    from pdecontrol.mbrl import rollout_hip as ro
    from pdecontrol.mbrl.recognition import field_map
    from pdegym.common import transforms as T
    ro.load()
    sensor = field_map(T.SensorTransform(3 if N == 98 else (4 if N == 256 else 1)), N)
    worst = 0.0
    for with_reward_coef, with_in_coef, B in itertools.product((False, True), (False, True), BATCHES):
        for spike_row in ([B - 1] if B > 1 else [None, 0]):
            tag = (N, A, B, with_reward_coef, with_in_coef, spike_row)
            c = _settle_case(N, A, B, with_reward_coef, with_in_coef, spike_row)
            plain = _settle(ro, c, N, A, B, sensor, dissipation=False)
            got = _settle(ro, c, N, A, B, sensor, dissipation=True)
            again = _settle(ro, c, N, A, B, sensor, dissipation=True)
            for name in ("state", "traj", "pol", "steps", "step"):
                np.testing.assert_array_equal(got[name].view(np.int32), plain[name].view(np.int32), err_msg=f"{tag} {name}")
            np.testing.assert_array_equal(got["state"], c.want, err_msg=str(tag))
            np.testing.assert_array_equal(got["traj"][T_NOW + 1], c.want, err_msg=str(tag))
            others = [t for t in range(T_SLOTS) if t != T_NOW]
            assert (got["steps"][others] == -1).all() and (got["rewards"][others] == FILL).all(), tag
            assert got["step"].tolist() == [T_NOW, T_NOW + 1]
            for name in got:
                np.testing.assert_array_equal(got[name].view(np.int32), again[name].view(np.int32),
                                              err_msg=f"{tag} {name}: two runs differ")
            r = got["rewards"][T_NOW].astype(np.float64)
            assert np.isfinite(r).all() and np.isfinite(c.ref).all(), tag
            assert not np.array_equal(got["rewards"][T_NOW], plain["rewards"][T_NOW]), tag
            err = np.abs(r - c.ref)
            bound = 2.0 ** -23 * np.abs(c.ref) + (A + 1) * 2.0 ** -24 * c.scale
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), f"{tag}: {float((err / bound).max()):.3f} of the bound"
    print(f"ro_settle_burgers_dissipation N={N} A={A}: worst reward error {worst:.3f} of the bound")


# ----------------------------------------------------------------------------------------------------------------------
# the phases
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "sac"])
def test_collection_over_a_dissipation_env_equals_the_loop(monkeypatch, kind):
    """``collect`` (N = 64, 4 envs, 5 sub-steps per step) against ``Worker.rollout`` from the same seeds, with the harness of
    tests/test_burgers_collect_gpu.py: bit for bit in everything the loop returns and mutates, rewards included (both go
    through the objective entries, and a span's bytes are its step launches')."""
    import test_burgers_collect_gpu as cg
    from pdegym.burgers.burgers import BurgersBatchedVecEnv

    def make_env(E, N, episode):
        env = BurgersBatchedVecEnv(E, N=N, cfg_steps=5, Tmax=0.0199, device=0, objective="dissipation")
        assert env.max_episode_steps == episode == 4 and env.scenario["objective"] == "dissipation"
        return env

    monkeypatch.setattr(cg, "make_env", make_env)
    loop = cg._run("loop", kind, 4, 64, 1, 4, False)
    kernel = cg._run("collect", kind, 4, 64, 1, 4, False)
    cg._compare(loop, kernel, False)
    rewards = np.concatenate([np.asarray(list(v), dtype=np.float32) for v in kernel[1].rewards.values()])
    assert np.isfinite(rewards).all() and (rewards != 0).all()
    # the same phases over an l2control env collect other rewards
    monkeypatch.setattr(cg, "make_env", lambda E, N, episode: BurgersBatchedVecEnv(E, N=N, cfg_steps=5, Tmax=0.0199, device=0))
    plain = cg._run("collect", kind, 4, 64, 1, 4, False)
    plain_rewards = np.concatenate([np.asarray(list(v), dtype=np.float32) for v in plain[1].rewards.values()])
    assert plain_rewards.shape == rewards.shape and not np.array_equal(plain_rewards, rewards)


def test_imagination_over_a_dissipation_world(monkeypatch):
    """``imagine`` over a 2-member ``BurgersFNO`` world (4 envs, horizon 3) whose reward owner is a dissipation env: the
    kernel tier, whose captured step ends in ``ro_settle_burgers_dissipation``, against the loop tier bit for bit but the
    rewards; the rewards within the settle test's bound of the twin on the kernel tier's own rows."""
    from pdecontrol.mbrl import imagination_phase as ip
    from pdecontrol.mbrl import rollout_hip as ro
    from pdegym.burgers.burgers import BurgersBatchedVecEnv
    from test_imagination_phase_gpu import _host_forcing_is_the_fma_chain, _same
    M = bw.repo_namespace()
    dev = torch.device("cuda", 0)
    calls = []
    settle = ro.settle_burgers_dissipation
    monkeypatch.setattr(ro, "settle_burgers_dissipation", lambda *a: (calls.append(1), settle(*a))[1])
    out = {}
    for route in ("loop", "kernel"):
        env = BurgersBatchedVecEnv(4, device=0, objective="dissipation", **bw.CFG)
        s = bw.build(M, dev, env=env, num_envs=4, horizon=3, members=2)
        s.world.setup(s.starting)
        bw.seed()
        if route == "loop":
            replay = M.Worker(s.stack).rollout(s.agent, bw.stop(8))
            assert s.world._dev is not None and not calls
        else:
            timings = {}
            replay = ip.imagine(s.agent, s.stack, 8, timings=timings)
            assert timings["tier"] == "kernel" and s.world._imagination.select and calls
            assert (s.world._imagination.objective, s.world._imagination.owner) == ("dissipation", "burgers")
        torch.cuda.synchronize()
        out[route] = (s, replay)
    (ls, loop), (ks, kernel) = out["loop"], out["kernel"]
    exact = _host_forcing_is_the_fma_chain(ls)
    assert loop.episodes == kernel.episodes and loop.ntimesteps == kernel.ntimesteps == 2 * 3 * 4
    geo = ip.recognize_stack(ks.stack, objectives=("l2control", "dissipation"))
    A, N = (int(v) for v in geo.forcing.shape)
    rows, actions, rewards, loop_rewards = [], [], [], []
    for key in loop.episodes:
        for name in bw.FIELDS:
            a, b = list(getattr(loop, name)[key]), list(getattr(kernel, name)[key])
            assert len(a) == len(b), (key, name)
            if name != "rewards":
                _same(a, b, exact, f"episode {key} {name}")
        rows += [np.asarray(v).reshape(N) for v in kernel.nxtobs[key]]
        actions += [np.asarray(v).reshape(A) for v in kernel.actions[key]]
        rewards += [np.asarray(v) for v in kernel.rewards[key]]
        loop_rewards += [np.asarray(v) for v in loop.rewards[key]]
    rewards = np.asarray(rewards)
    assert rewards.dtype == np.float32 and np.isfinite(rewards).all() and (rewards != 0).all()
    ref, scale = _reward_twin(np.stack(rows), np.stack(actions), geo.reward, geo.act_in, geo.forcing.numpy(), geo.dx, geo.nu)
    err = np.abs(rewards.astype(np.float64) - ref)
    bound = 2.0 ** -23 * np.abs(ref) + (A + 1) * 2.0 ** -24 * scale
    print(f"imagined dissipation rewards against the twin: worst error {float((err / bound).max()):.3f} of the bound; against the "
          f"loop tier: {float(np.abs(rewards - np.asarray(loop_rewards)).max()):.3e} absolute")
    assert (err <= bound).all()


def test_the_controller_learns_under_dissipation(monkeypatch, tmp_path):
    """The toy ``learn()`` of tests/test_burgers_controller_gpu.py with ``env_config={"objective": "dissipation"}``: every
    phase but ``evaluate_surrogate`` on its kernel tier, and the logged returns finite and other than the l2control run's."""
    import test_burgers_controller_gpu as cg
    returns = {}
    for objective in ("dissipation", "l2control"):
        monkeypatch.setattr(cg, "ENV_CONFIG", dict(cg.ENV_CONFIG, objective=objective))
        c, snapshots = cg._run(tmp_path / objective, "kernel")
        assert c.stack.ostore.env.scenario["objective"] == objective and c.iteration == 2 and len(snapshots) == 3
        tiers = {}
        for name, _, tier in c.tiers:
            tiers.setdefault(name, set()).add(tier)
        assert tiers.pop("evaluate_surrogate") == {"loop"}
        assert tiers == {name: {"kernel"} for name in ("warmup", "evaluate", "collect", "update_delta_transform",
                                                       "update_surrogate", "imagine", "update_policy")}, c.tiers
        assert all(t.tier == "kernel" for t in c.trainers), [t.tier_reason for t in c.trainers]
        logged = [(k, float(v)) for row in c.log.history for k, v in sorted(row.items()) if k.startswith("Avg.") and "Return" in k]
        assert logged and all(np.isfinite(v) for _, v in logged), logged
        returns[objective] = logged
    assert [k for k, _ in returns["dissipation"]] == [k for k, _ in returns["l2control"]]
    assert all(a != b for (_, a), (_, b) in zip(returns["dissipation"], returns["l2control"])), returns
