"""The imagined-rollout phase over the Burgers / FNO world on the GPU (scenario: tests/_burgers_world_scenario.py): the
world is device-resident for an ensemble of FNO members, the kernel tier equals the per-step loop of ``Worker.rollout``,
the member-select step (``fno_forward_select``) equals the generic member loop bit for bit, a re-scaled member recaptures
the graph, and a sink receives the loop's replay.  Every run is made once per process and shared by the tests that read it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _burgers_world_scenario as bw  # noqa: E402
import _rollout_scenario as sc  # noqa: E402
from test_imagination_phase_gpu import (_assert_same_generators, _compare_replays, _generator_states,  # noqa: E402
                                        _host_forcing_is_the_fma_chain, _same, _world_state)

_runs = {}


def _run(route, sink=None, fresh=False):
    """(scene, what the call returns, (generator states, world state)) of ``route`` from equal seeds: "loop"
    (``Worker.rollout``), "select" (the kernel tier as it is by default) or "generic" (``PDECONTROL_FNO_SELECT=0``)."""
    from pdecontrol.mbrl import imagination_phase as ip
    key = (route, sink is not None)
    if not fresh and key in _runs:
        return _runs[key]
    M = bw.repo_namespace()
    s = bw.build(M, torch.device("cuda", 0))
    s.world.setup(s.starting)
    bw.seed()
    saved = os.environ.pop("PDECONTROL_FNO_SELECT", None)
    try:
        if route == "loop":
            out = M.Worker(s.stack).rollout(s.agent, bw.stop(bw.NUM_ROLLOUTS))
            assert s.world._dev is not None, "the loop's world is not device-resident"
        else:
            if route == "generic":
                os.environ["PDECONTROL_FNO_SELECT"] = "0"
            timings = {}
            out = ip.imagine(s.agent, s.stack, bw.NUM_ROLLOUTS, timings=timings, **({} if sink is None else {"sink": sink}))
            assert timings["tier"] == "kernel", timings
            cap = s.world._imagination
            assert cap.select is (route == "select") and cap.geometry.members == bw.MEMBERS
    finally:
        os.environ.pop("PDECONTROL_FNO_SELECT", None)
        if saved is not None:
            os.environ["PDECONTROL_FNO_SELECT"] = saved
    torch.cuda.synchronize()
    result = (s, out, (_generator_states(), _world_state(s.world)))
    if not fresh:
        _runs[key] = result
    return result


@pytest.mark.gpu
def test_an_fno_ensemble_keeps_the_world_on_the_device():
    M = bw.repo_namespace()
    dev = torch.device("cuda", 0)
    s = bw.build(M, dev)
    assert s.world._use_device_path()
    s.world.setup(s.starting)
    s.world.reset()
    assert s.world._dev is not None and s.world._dev_starting is not None
    assert s.world._dev.hidden == [(), (), ()] and tuple(s.world._dev.state.shape) == (bw.NUM_ENVS, 1, 1, bw.N)
    # a step through the gym interface is the device-resident one
    obs, rewards, _, _, _ = s.world.step(np.zeros((bw.NUM_ENVS, 1, bw.N), dtype=np.float32))
    assert obs.shape == (bw.NUM_ENVS, 1, bw.N) and np.isfinite(obs).all() and (rewards < 0).all()
    tstep = s.env.cfg_steps * s.env.dt
    # one FNO of another width: the whole-network kernels do not cover it
    narrow = bw.build(M, dev, env=s.env, modules=[bw.fno_module(M, tstep, 0, dev, width=16)])
    assert not narrow.world._use_device_path()
    # an FNO member beside a ConvLSTM member: no single kernel family
    K = sc.repo_namespace()
    torch.manual_seed(1)
    f = K.factory_n_cls()                                      # the any-N ConvLSTM layout
    lstm = K.TrainingModule(surrogate=f.surrogate(delta=tstep, dscaling=None, tau=bw.TAU, **f.model(N=bw.N)),
                            loss=torch.nn.MSELoss(reduction="none"), tstep=tstep, delta=tstep, tau=bw.TAU, tbtt=10).to(dev)
    mixed = bw.build(M, dev, env=s.env, modules=[bw.fno_module(M, tstep, 0, dev), lstm])
    assert not mixed.world._use_device_path()
    alone = bw.build(M, dev, env=s.env, modules=[lstm])
    assert alone.world._use_device_path()                      # the ConvLSTM family keeps its path


def _end_states_equal(lend, pend, exact):
    _assert_same_generators(lend[0], pend[0])
    (lt, lsim, lstate, lhid), (pt, psim, pstate, phid) = lend[1], pend[1]
    np.testing.assert_array_equal(lt, pt)
    assert lsim == psim == 0
    _same(lstate.cpu(), pstate.cpu(), exact, "world state")
    assert lhid == phid == [(), (), ()]


@pytest.mark.gpu
def test_phase_equals_the_loop():
    """5 envs, horizon 3, 2 rounds.  obs, actions, nxtobs, steps and the flags bit for bit, the rewards within
    (N + 4) * 2^-24 relative (``_compare_replays`` of tests/test_imagination_phase_gpu.py: Burgers' batched reward is the
    same fp32 ``vector_norm`` squared), generators and the world's end state as the loop leaves them."""
    ls, loop, lend = _run("loop")
    ps, phase, pend = _run("select")
    exact = _host_forcing_is_the_fma_chain(ls)
    assert loop.nepisodes == 2 * bw.NUM_ENVS and loop.ntimesteps == 2 * bw.HORIZON * bw.NUM_ENVS
    _compare_replays(loop, phase, bw.N, exact)
    _end_states_equal(lend, pend, exact)
    # the three members differ and the draws reach all of them: a step that ignored `chosen` could not pass
    assert len({int(c) for c in ps.world._imagination.chosen.cpu().numpy().reshape(-1)}) == bw.MEMBERS


@pytest.mark.gpu
def test_the_select_step_equals_the_generic_member_loop():
    """Same ``ro_settle``, same row bytes: the two replays are equal bit for bit, rewards included."""
    gs, generic, gend = _run("generic")
    ss, select, send = _run("select")
    assert generic.episodes == select.episodes and generic.ntimesteps == select.ntimesteps
    for key in generic.episodes:
        for name in bw.FIELDS:
            a, b = np.asarray(list(getattr(generic, name)[key])), np.asarray(list(getattr(select, name)[key]))
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (key, name)
    _end_states_equal(gend, send, True)
    for got, want in zip(select.device_rollout.tensors, generic.device_rollout.tensors):
        assert torch.equal(got, want)


@pytest.mark.gpu
def test_a_rescaled_member_recaptures_the_step():
    from _latent_models import normalize_pair
    from pdecontrol.mbrl import imagination_phase as ip
    M = bw.repo_namespace()
    ls, _, _ = _run("loop", fresh=True)
    ps, _, _ = _run("select", fresh=True)
    exact = _host_forcing_is_the_fma_chain(ls)
    cap = ps.world._imagination
    ip.imagine(ps.agent, ps.stack, bw.NUM_ROLLOUTS)
    assert ps.world._imagination is cap, "a second phase reuses the captured graph"
    _, dscaling = normalize_pair(mean=0.0, var=0.25)
    ps.ensemble.modules[0].surrogate.dscaling = dscaling
    assert not ps.world._dev.valid()
    again = ip.imagine(ps.agent, ps.stack, bw.NUM_ROLLOUTS)
    assert ps.world._imagination is not cap and ps.world._imagination.dev is ps.world._dev and ps.world._imagination.select
    ls.ensemble.modules[0].surrogate.dscaling = dscaling
    for s in (ls, ps):
        s.world.setup(s.starting)
    bw.seed()
    loop2 = M.Worker(ls.stack).rollout(ls.agent, bw.stop(bw.NUM_ROLLOUTS))
    bw.seed()
    phase2 = ip.imagine(ps.agent, ps.stack, bw.NUM_ROLLOUTS)
    _compare_replays(loop2, phase2, bw.N, exact)
    assert again.ntimesteps == phase2.ntimesteps


@pytest.mark.gpu
def test_phase_with_a_sink_holds_the_loops_replay():
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    from pdecontrol.mbrl.replay import ExperienceReplay
    ls, loop, lend = _run("loop")
    exact = _host_forcing_is_the_fma_chain(ls)
    sink = DeviceExperienceReplay(64, device=torch.device("cuda", 0))
    _, staged, send = _run("select", sink=sink)
    assert staged.ntimesteps == loop.ntimesteps == 2 * bw.HORIZON * bw.NUM_ENVS
    sink.extend(staged)
    packed = ExperienceReplay(64)                    # the host route: the loop's rollout extended into a host replay
    packed.extend(loop)
    got = sink.to_host()
    assert got.episodes == packed.episodes and got.ntimesteps == packed.ntimesteps and dict(got.vindex) == dict(packed.vindex)
    bound = (bw.N + 4) * 2.0 ** -24 if exact else 1e-4
    for key in packed.episodes:
        for name in bw.FIELDS:
            a, b = np.asarray(list(getattr(packed, name)[key])), np.asarray(list(getattr(got, name)[key]))
            assert a.dtype == b.dtype and a.shape == b.shape, (key, name)
            if name == "rewards":
                worst = float((np.abs(a.astype(np.float64) - b) / np.abs(a.astype(np.float64))).max())
                assert worst <= bound, (key, worst, bound)
            else:
                _same(a, b, exact, f"episode {key} {name}")
    _end_states_equal(lend, send, exact)
