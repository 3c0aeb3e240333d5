"""The dissipation objective of the imagined-rollout phase on the GPU: ``ro_settle_dissipation`` alone against
``ro_settle`` (everything but the reward, bit for bit) and against the fp64 twin of its reward
(tests/_rollout_dissipation.py), the kernel tier of ``imagine`` against the per-step loop of ``Worker.rollout`` on the same
GPU, and the phase with a device sink."""
import json
import os
import sys
import types
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rollout_scenario as sc  # noqa: E402
from _rollout_dissipation import dissipation_terms  # noqa: E402
from _rollout_scenario import host_matmul_is_fma_chain  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_REWARD = {"batched_reward_func": lambda env: env.batched_reward_func}
BATCHES = (1, 5, 257)                     # one wave, a partial workgroup, more than one workgroup with a partial last one
T_SLOTS, T_NOW, MEMBERS, GUARD, FILL = 4, 2, 3, 64, 7.0
WAVELENGTHS, RIPPLE = 64.0, 0.25          # the smooth rows' period in x over 2 pi, and their amplitude: see _kernel_case


# ----------------------------------------------------------------------------------------------------------------------
# the kernel alone
# ----------------------------------------------------------------------------------------------------------------------
def _coef(rs, width, a, ba, dc, c):
    """[4, width] = (a, b - a, d - c, c), each column its own values around the given ones."""
    from pdecontrol.mbrl.recognition import FieldMap
    jitter = lambda v: (v + rs.uniform(-0.1, 0.1, width)).astype(np.float32)
    return FieldMap(0, 1, width, torch.from_numpy(np.stack([jitter(a), jitter(ba), jitter(dc), jitter(c)])))


def _kernel_case(N, A, B, with_reward_coef, with_in_coef, spike_row):
    """Inputs of one launch and their twin, all on the host.

    Rows: the scenario's ``sin + cos`` fields over one period, scaled by RIPPLE and lifted by 1.5 so that u keeps its
    sign, and at ``spike_row`` a row that is zero but for spikes at columns 0 and N - 1 (after the rescaling: the
    world-scale row is the pre-image), which a wrong periodic wrap moves out of the stencils that must see them, and whose
    reward is nearly all derivative terms.  dx = 2 pi WAVELENGTHS / N: the derivative terms of the smooth rows then are a
    few 1e-4 of mean(u * phi) for an action of size 1, so that |mean(u * phi)| >= 1 % of |r| holds for every smooth row
    (asserted by the caller; the actions are uniform in [-1, 1] and may cancel) while an error of the stencil of 1e-3
    relative still exceeds the reward's tolerance on the smooth rows."""
    from pdecontrol.mbrl.recognition import FieldMap
    from _oracle_stepper import OracleStepper
    from pdegym.kuramoto import KuramotoSivashinskyEnv
    rs = np.random.RandomState(1000 * N + 10 * A + B + (5 if with_reward_coef else 0) + (3 if with_in_coef else 0))
    dx = 2.0 * np.pi * WAVELENGTHS / N
    x = np.linspace(0, 2 * np.pi, N, endpoint=False)
    phase = rs.uniform(0, 6, (MEMBERS, B, 1))
    u = (1.5 + RIPPLE * (np.sin(x + phase) + 0.5 * np.cos(2 * x - 0.7 * phase))).astype(np.float32)
    reward = _coef(rs, N, -1.0, 2.0, 6.0, -3.0) if with_reward_coef else FieldMap(0, 1, N, None)
    if spike_row is not None:
        u[:, spike_row] = 0.0
        u[:, spike_row, 0], u[:, spike_row, N - 1] = 2.0, -1.5
    if with_reward_coef:                      # the world-scale pre-image: v = (u - c) / dc * ba + a, close enough to invert
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
    env = KuramotoSivashinskyEnv(L=dx * N, N=N, _stepper_cls=OracleStepper)
    assert env.dx == dx or abs(env.dx - dx) <= 2.0 ** -52 * dx
    geo = types.SimpleNamespace(reward=reward, act_in=act_in, forcing=F)
    want = members[chosen[T_NOW], np.arange(B)]
    ref, scale = dissipation_terms(want, actions[T_NOW], geo, env)
    # mean(u * phi) alone: the reward of the same rows without their derivative terms is what a dx -> infinity leaves
    w = reward.apply_numpy(want).astype(np.float64)
    from _rollout_scenario import fma_chain
    uphi = (w * fma_chain(act_in.apply_numpy(actions[T_NOW]), F).astype(np.float64)).sum(axis=1) / N
    return types.SimpleNamespace(members=members, actions=actions, chosen=chosen, steps0=steps0, F=F, reward=reward,
                                 act_in=act_in, dx=float(env.dx), want=want, ref=ref, scale=scale, uphi=uphi)


def _guarded(shape, dtype, fill, dev):
    """(buffer, view): ``view`` of ``shape`` lies GUARD elements inside a buffer filled with ``fill`` (16-byte aligned)."""
    n = int(np.prod(shape))
    full = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return full, full[GUARD:GUARD + n].view(shape)


def _guards_untouched(full, fill):
    return bool((full[:GUARD] == fill).all()) and bool((full[-GUARD:] == fill).all())


def _launch(ro, c, N, A, B, sensor, dissipation, step_cells=(T_NOW, 9), chosen=None):
    """One settle launch into fresh guarded outputs; returns them on the host."""
    dev = torch.device("cuda", 0)
    d = lambda a: None if a is None else torch.as_tensor(a).to(dev).contiguous()
    g = ro.Geometry(B, T_SLOTS, N, A, N, 0, 1, sensor.start, sensor.stride, MEMBERS)
    mem = [d(m) for m in c.members]
    bufs = dict(state=_guarded((B, N), torch.float32, FILL, dev), traj=_guarded((T_SLOTS + 1, B, N), torch.float32, FILL, dev),
                pol=_guarded((B, sensor.width), torch.float32, FILL, dev), steps=_guarded((T_SLOTS, B), torch.int32, -1, dev),
                rewards=_guarded((T_SLOTS, B), torch.float32, FILL, dev), step=_guarded((2,), torch.int32, -5, dev))
    bufs["step"][1].copy_(torch.tensor(step_cells, dtype=torch.int32))
    keep = (d(c.chosen if chosen is None else chosen), d(c.steps0), d(c.reward.coef), d(c.actions), d(c.act_in.coef), d(c.F))
    args = ro.settle_args(mem, keep[0], bufs["state"][1], bufs["traj"][1], bufs["pol"][1], keep[1], bufs["steps"][1],
                          bufs["rewards"][1], keep[2], bufs["step"][1])
    if dissipation:
        ro.settle_dissipation(ro.stream(), g, args, ro.dissipation_args(keep[3], keep[4], keep[5], c.dx))
    else:
        ro.settle(ro.stream(), g, args)
    torch.cuda.synchronize()
    fills = dict(state=FILL, traj=FILL, pol=FILL, steps=-1, rewards=FILL, step=-5)
    for name, (full, _) in bufs.items():
        assert _guards_untouched(full, fills[name]), f"{name}: written outside the output"
    return {name: view.cpu().numpy() for name, (_, view) in bufs.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 4, 16])
@pytest.mark.parametrize("N", [16, 64, 98, 100, 256, 1024])
def test_ro_settle_dissipation_settles_as_ro_settle_and_rewards_as_the_twin(N, A):
    """N = 16 leaves lanes idle, 98 is no multiple of 4 and takes the scalar path, the others the float4 path; three
    members with a chosen array, with and without each affine map, step 2 of 4.  State, trajectory, policy observations,
    steps and the step cells are those of ``ro_settle`` on the same inputs, bit for bit; the reward lies within
        2^-23 |r| + (A + 1) 2^-24 mean_i(|u_i| sum_k |a_k| F_ki)
    of the fp64 twin evaluated with the fp32 phi of the fma chain (one fp32 rounding plus the reordering of fp64 sums of
    at most 1024 terms; only the first term should be needed, and the worst case is printed in its units)."""
    from pdecontrol.mbrl import rollout_hip as ro
    from pdecontrol.mbrl.recognition import field_map
    from pdegym.common import transforms as T
    ro.load()
    sensor = field_map(T.SensorTransform(3 if N == 98 else (4 if N == 256 else 1)), N)
    worst, worst_first = 0.0, 0.0
    for with_reward_coef in (False, True):
        for with_in_coef in (False, True):
            for B in BATCHES:
                for spike_row in ([B - 1] if B > 1 else [None, 0]):
                    tag = (N, A, B, with_reward_coef, with_in_coef, spike_row)
                    c = _kernel_case(N, A, B, with_reward_coef, with_in_coef, spike_row)
                    smooth = np.arange(B) != (-1 if spike_row is None else spike_row)
                    assert (np.abs(c.uphi[smooth]) >= 0.01 * np.abs(c.ref[smooth])).all(), \
                        f"{tag}: a smooth row whose mean(u * phi) hides behind its derivative terms"
                    plain = _launch(ro, c, N, A, B, sensor, dissipation=False)
                    got = _launch(ro, c, N, A, B, sensor, dissipation=True)
                    again = _launch(ro, c, N, A, B, sensor, dissipation=True)
                    for name in ("state", "traj", "pol", "steps", "step"):
                        np.testing.assert_array_equal(got[name].view(np.int32), plain[name].view(np.int32), err_msg=f"{tag} {name}")
                    np.testing.assert_array_equal(got["state"], c.want, err_msg=str(tag))
                    np.testing.assert_array_equal(got["traj"][T_NOW + 1], c.want, err_msg=str(tag))
                    others = [t for t in range(T_SLOTS) if t != T_NOW]
                    assert (got["traj"][:T_NOW + 1] == FILL).all() and (got["traj"][T_NOW + 2:] == FILL).all(), tag
                    assert (got["steps"][others] == -1).all() and (got["rewards"][others] == FILL).all(), tag
                    np.testing.assert_array_equal(got["steps"][T_NOW], c.steps0 + T_NOW + 1)
                    assert got["step"].tolist() == [T_NOW, T_NOW + 1]
                    for name in got:
                        np.testing.assert_array_equal(got[name].view(np.int32), again[name].view(np.int32),
                                                      err_msg=f"{tag} {name}: two runs differ")
                    r = got["rewards"][T_NOW].astype(np.float64)
                    assert np.isfinite(r).all() and np.isfinite(c.ref).all(), tag
                    err = np.abs(r - c.ref)
                    first = 2.0 ** -23 * np.abs(c.ref)
                    bound = first + (A + 1) * 2.0 ** -24 * c.scale
                    worst, worst_first = max(worst, float((err / bound).max())), max(worst_first, float((err / first).max()))
                    assert (err <= bound).all(), f"{tag}: {float((err / bound).max()):.3f} of the bound"
    print(f"ro_settle_dissipation N={N} A={A}: worst reward error {worst:.3f} of the bound, {worst_first:.3f} of 2^-23 |r|")


@pytest.mark.gpu
@pytest.mark.parametrize("N", [64, 98])
def test_ro_settle_dissipation_outside_the_trajectory_and_outside_the_ensemble(N):
    """A step outside [0, T) writes nothing but the next step cell; a member index outside the ensemble gives the NaN row
    and a NaN reward for that env alone, exactly as ``ro_settle``."""
    from pdecontrol.mbrl import rollout_hip as ro
    from pdecontrol.mbrl.recognition import field_map
    from pdegym.common import transforms as T
    ro.load()
    A, B = 4, 5
    sensor = field_map(T.SensorTransform(1), N)
    c = _kernel_case(N, A, B, True, True, None)
    for t in (-1, T_SLOTS, T_SLOTS + 3):
        got = _launch(ro, c, N, A, B, sensor, dissipation=True, step_cells=(t, 9))
        for name in ("state", "traj", "pol", "rewards"):
            assert (got[name] == FILL).all(), (t, name)
        assert (got["steps"] == -1).all() and got["step"].tolist() == [t, t + 1]
    chosen = c.chosen.copy()
    chosen[T_NOW, 1], chosen[T_NOW, 3] = MEMBERS, -1
    got = _launch(ro, c, N, A, B, sensor, dissipation=True, chosen=chosen)
    plain = _launch(ro, c, N, A, B, sensor, dissipation=False, chosen=chosen)
    for name in ("state", "traj", "pol", "steps", "step"):
        np.testing.assert_array_equal(got[name].view(np.int32), plain[name].view(np.int32), err_msg=name)
    poisoned = np.asarray([False, True, False, True, False])
    assert np.isnan(got["state"][poisoned]).all() and np.isnan(got["traj"][T_NOW + 1][poisoned]).all()
    assert np.isnan(got["rewards"][T_NOW][poisoned]).all()
    np.testing.assert_array_equal(got["state"][~poisoned], c.want[~poisoned])
    r = got["rewards"][T_NOW][~poisoned].astype(np.float64)
    ref, scale = c.ref[~poisoned], c.scale[~poisoned]
    assert (np.abs(r - ref) <= 2.0 ** -23 * np.abs(ref) + (A + 1) * 2.0 ** -24 * scale).all()


# ----------------------------------------------------------------------------------------------------------------------
# the phase
# ----------------------------------------------------------------------------------------------------------------------
SIZES = {"n64": {}, "n256": dict(L=88.0, N=256)}
A_SCENARIO = 4
# C of the reward bound of the phase against the loop, in units of 2^-24 mean_i(|u_i| sum_k |a_k| F_ki): four times the
# worst excess measured on an MI355X at both sizes (profiles/imagination_dissipation_observed.json), rounded up to a
# power of two and not below 2 (A + 1)
OBSERVED = os.path.join(ROOT, "profiles", "imagination_dissipation_observed.json")


def _phase_bound_factor():
    worst = max(float(v) for v in json.load(open(OBSERVED))["worst_excess_in_units_of_the_second_term"].values())
    power = 1.0
    while power < 4.0 * worst:
        power *= 2.0
    return max(power, 2.0 * (A_SCENARIO + 1))


def _generator_states():
    return (np.random.get_state(), torch.get_rng_state().clone(), torch.cuda.get_rng_state(0).clone())


def _world_state(world):
    dev = world._dev
    return (world.timesteps.copy(), int(world.simulated), dev.state.clone(), [tuple(h.clone() for h in hid) for hid in dev.hidden])


def _run(tag, limit, phase, sink=None):
    """(scene, what the call returns, (generator states, world state)) of the loop or the phase from equal seeds."""
    from pdecontrol.mbrl import imagination_phase as ip
    M = sc.repo_namespace()
    s = sc.build(M, torch.device("cuda", 0), limit=limit, env_kwargs=dict(objective="", **SIZES[tag]), world_kwargs=DEVICE_REWARD)
    s.world.setup(s.starting)
    sc.seed()
    if phase:
        timings = {}
        out = ip.imagine(s.agent, s.stack, sc.NUM_ROLLOUTS, timings=timings, **({} if sink is None else {"sink": sink}))
        assert timings["tier"] == "kernel", timings
        assert s.world._imagination.objective == "dissipation"
    else:
        out = M.Worker(s.stack).rollout(s.agent, sc.stop())
        assert s.world._dev is not None, "the loop's world is not device-resident"
    torch.cuda.synchronize()
    return s, out, (_generator_states(), _world_state(s.world))


def _same(a, b, exact, what):
    """Bit for bit; on a host whose forcing matmul rounds differently from the fma chain the float fields can only agree
    to the device path's tolerance (1e-4 relative, 1e-5 absolute)."""
    a, b = np.asarray(a), np.asarray(b)
    if exact or a.dtype.kind != "f":
        np.testing.assert_array_equal(a, b, err_msg=what)
    else:
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5, err_msg=what)


def _flat(replay, name, width=None):
    out = [np.asarray(v) for key in replay.episodes for v in getattr(replay, name)[key]]
    return np.stack(out) if width is None else np.stack(out).reshape(len(out), width)


def phase_against_loop(tag, limit):
    """Runs both tiers and compares everything but the rewards; returns what the reward comparison needs:
    (|loop - phase|, |r| of the loop, the scale of the second term from the loop's own replay, exact)."""
    from pdecontrol.mbrl import imagination_phase as ip
    ls, loop, lend = _run(tag, limit, phase=False)
    ps, phase, pend = _run(tag, limit, phase=True)
    F = ls.env.forcing.forcing.numpy()
    rs = np.random.RandomState(3)
    exact = all(host_matmul_is_fma_chain(F, rs.uniform(-1, 1, (ls.world.num_envs, 1, F.shape[0])).astype(np.float32))
                for _ in range(64))
    assert loop.episodes == phase.episodes and dict(loop.vindex) == dict(phase.vindex)
    assert (loop.ntimesteps, loop.nstopped) == (phase.ntimesteps, phase.nstopped)
    assert loop.ntimesteps == (2 if limit else 6) * ls.world.num_envs
    for key in loop.episodes:
        for name in sc.FIELDS:
            a, b = list(getattr(loop, name)[key]), list(getattr(phase, name)[key])
            assert len(a) == len(b), (key, name)
            for x, y in zip(a, b):
                assert type(x) is type(y) and np.asarray(x).dtype == np.asarray(y).dtype and np.shape(x) == np.shape(y), (key, name)
            if name != "rewards":
                _same(a, b, exact, f"episode {key} {name}")
    (lg, (lt, lsim, lstate, lhid)), (pg, (pt, psim, pstate, phid)) = lend, pend
    assert lg[0][0] == pg[0][0] and np.array_equal(lg[0][1], pg[0][1]) and lg[0][2:] == pg[0][2:], "numpy's global generator"
    assert torch.equal(lg[1], pg[1]), "torch's CPU generator"
    assert torch.equal(lg[2], pg[2]), "torch's device generator"
    np.testing.assert_array_equal(lt, pt)
    assert lsim == psim == 0
    _same(lstate.cpu(), pstate.cpu(), exact, "world state")
    for x, y in zip(lhid, phid):
        for a, b in zip(x, y):
            _same(a.cpu(), b.cpu(), exact, "hidden state")
    geo = ip.recognize_stack(ls.stack, objectives=("l2control", "dissipation"))
    A, N = F.shape
    out = []
    for replay in (loop, phase):
        r64, scale = dissipation_terms(_flat(replay, "nxtobs", N), _flat(replay, "actions", A), geo, ls.env)
        out.append((_flat(replay, "rewards").astype(np.float64), r64, scale))
    return out, exact


@pytest.mark.gpu
@pytest.mark.parametrize("limit", [False, True], ids=["free", "limit"])
@pytest.mark.parametrize("tag", sorted(SIZES))
def test_phase_equals_the_loop_under_dissipation(tag, limit):
    """4 envs, horizon 3, 6 rollouts, both passes.  obs, actions, nxtobs, steps and the flags bit for bit (on a host whose
    matmul is the fma chain), generators and the world's end state as the loop leaves them, and every reward within
        2^-22 |r| + C 2^-24 mean_i(|u_i| sum_k |a_k| F_ki)
    of the loop's, u and the actions taken from the loop's own replay: one fp32 rounding per side, and C for the loop's
    phi, which goes through the inverse forcing, the inverse scaling and the device matmul (``_phase_bound_factor``).
    On a host whose matmul is not the fma chain the trajectories differ in their last bits, so each tier's rewards are
    compared with the twin of its own replay instead, within the host test's bound."""
    (loop, phase), exact = phase_against_loop(tag, limit)
    C = _phase_bound_factor()
    (lr, l64, lscale), (pr, p64, pscale) = loop, phase
    if exact:
        err = np.abs(lr - pr)
        first, second = 2.0 ** -22 * np.abs(lr), 2.0 ** -24 * lscale
        excess = float((np.maximum(err - first, 0.0) / second).max())
        print(f"phase against loop under dissipation, {tag}, limit={limit}: worst error {float((err / (first + C * second)).max()):.3f} "
              f"of the bound, worst excess over 2^-22 |r| {excess:.3f} units of the second term (C = {C:g})")
        assert (err <= first + C * second).all()
    else:
        warnings.warn("TOLERANT MODE: this host's CPU matmul is not the fma chain of ro_act_chain, so the loop's forcing "
                      "differs in its last bits; each tier's rewards were compared with the twin of its own replay")
        for got, r64, scale in (loop, phase):
            assert (np.abs(got - r64) <= 2.0 ** -23 * np.abs(r64) + 2 * (A_SCENARIO + 1) * 2.0 ** -24 * scale).all()
    # the phase's rewards are the kernel's: one fp32 rounding of the twin of its own replay
    assert (np.abs(pr - p64) <= 2.0 ** -23 * np.abs(p64) + (A_SCENARIO + 1) * 2.0 ** -24 * pscale).all()


@pytest.mark.gpu
def test_phase_with_a_sink_under_dissipation():
    """After ``extend`` the slabs hold the no-sink run's replay bit for bit, rewards included, and the world and the
    generators end where the no-sink run leaves them."""
    import _device_replay_scenario as dr_sc
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    from pdecontrol.mbrl.replay import ExperienceReplay
    _, host, hend = _run("n64", False, phase=True)
    sink = DeviceExperienceReplay(64, device=torch.device("cuda", 0))
    _, staged, send = _run("n64", False, phase=True, sink=sink)
    assert staged.ntimesteps == host.ntimesteps == 6 * sc.NUM_ENVS
    sink.extend(staged)
    world_replay = ExperienceReplay(64)              # the host route: the same rollout extended into a host replay
    world_replay.extend(host)
    dr_sc.same_replay(sink.to_host(), world_replay, "the sink after the dissipation phase")
    rewards = _flat(host, "rewards")
    assert rewards.dtype == np.float32 and np.isfinite(rewards).all() and (rewards != 0).all()
    assert torch.equal(hend[0][1], send[0][1]) and torch.equal(hend[0][2], send[0][2])
    np.testing.assert_array_equal(hend[1][0], send[1][0])
    assert torch.equal(hend[1][2], send[1][2])
