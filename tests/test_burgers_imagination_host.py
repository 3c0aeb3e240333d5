"""The imagined-rollout phase over a Burgers reward owner, without a GPU: ``recognize_stack`` accepts a world whose batched
reward is a ``BurgersBatchedVecEnv``'s (objective l2control, dx = L / N), refuses another width and another objective
each with its own text, recognises the KS stack as before, and on a CPU ``imagine`` over the Burgers / FNO stack runs the
loop tier and returns the ``Worker.rollout`` replay bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _burgers_world_scenario as bw  # noqa: E402
import _rollout_scenario as sc  # noqa: E402

from pdecontrol.mbrl import imagination_phase as ip  # noqa: E402
from pdecontrol.mbrl.recognition import Unrecognized  # noqa: E402


@pytest.fixture(scope="module")
def M():
    return bw.repo_namespace()


def test_a_burgers_reward_owner_is_recognised(M):
    from pdegym.burgers.burgers import BurgersBatchedVecEnv
    s = bw.build(M)
    owner = s.world.batched_reward_func.__self__
    assert owner is s.env and type(owner) is BurgersBatchedVecEnv
    for objectives in (("l2control",), ("l2control", "dissipation")):
        geo = ip.recognize_stack(s.stack, objectives=objectives)
        assert geo.world is s.world and geo.objective == "l2control" and geo.dx == s.env.L / s.env.N
        assert tuple(geo.forcing.shape) == (4, bw.N) and geo.act_out.width == bw.N
        assert (geo.agent_obs.start, geo.agent_obs.stride, geo.agent_obs.width) == (2, 4, bw.N // 4)
        assert (geo.reward.start, geo.reward.stride, geo.reward.width) == (0, 1, bw.N)
    with pytest.raises(Unrecognized, match="the l2control objective"):
        ip.recognize_stack(s.stack, objectives=("dissipation",))
    # what BurgersEnv.batched_reward_func forwards to is the vec env's bound method
    from pdegym.burgers.burgers import BurgersEnv
    single = BurgersEnv.__new__(BurgersEnv)
    single._vec = s.env
    assert single.batched_reward_func.__self__ is s.env


def test_a_burgers_owner_of_another_width_or_objective_is_refused(M):
    s = bw.build(M)
    wide = bw.bare_env(N=2 * bw.N)
    s.world.batched_reward_func = wide.batched_reward_func
    with pytest.raises(Unrecognized, match=f"a reward over {2 * bw.N} grid points for observations of {bw.N}") as width_refusal:
        ip.recognize_stack(s.stack)
    scenario = {**bw.bare_env().scenario, "objective": "tracking"}
    other = bw.bare_env(scenario=scenario)
    assert other.scenario["objective"] == "tracking"
    s.world.batched_reward_func = other.batched_reward_func
    with pytest.raises(Unrecognized, match="BurgersBatchedVecEnv whose scenario names the tracking objective") as objective_refusal:
        ip.recognize_stack(s.stack, objectives=("l2control", "dissipation", "tracking"))
    assert str(width_refusal.value) != str(objective_refusal.value)
    # the refusal for any other owner keeps its wording
    s.world.batched_reward_func = lambda obs, act=None: -np.square(obs).mean(axis=(1, 2))
    with pytest.raises(Unrecognized, match="^a world without the batched reward of a KuramotoSivashinskyEnv$"):
        ip.recognize_stack(s.stack)


def test_the_ks_stack_is_recognised_as_before():
    K = sc.repo_namespace()
    s = sc.build(K, world_kwargs={"batched_reward_func": lambda env: env.batched_reward_func})
    geo = ip.recognize_stack(s.stack)
    assert geo.world is s.world and geo.objective == "l2control" and geo.dx == s.env.L / s.env.N == 22.0 / 64
    assert tuple(geo.forcing.shape) == (4, 64) and torch.equal(geo.forcing, s.env.forcing.forcing)
    assert (geo.act_out.start, geo.act_out.stride, geo.act_out.width) == (0, 1, 64)
    assert (geo.agent_obs.start, geo.agent_obs.stride, geo.agent_obs.width, geo.agent_obs.coef) == (0, 1, 64, None)
    assert (geo.reward.start, geo.reward.stride, geo.reward.width) == (0, 1, 64) and geo.reward.coef is not None
    assert geo.act_in.coef is not None and geo.act_out.coef is not None
    d = sc.build(K, env_kwargs=dict(objective=""), world_kwargs={"batched_reward_func": lambda env: env.batched_reward_func})
    with pytest.raises(Unrecognized, match="^the dissipation objective$"):
        ip.recognize_stack(d.stack)
    assert ip.recognize_stack(d.stack, objectives=("l2control", "dissipation")).objective == "dissipation"


def test_imagine_on_the_cpu_is_the_loop(M):
    """A CPU agent keeps the loop tier; the replay is ``Worker.rollout``'s, field by field and bit for bit, and the
    generators end where the loop leaves them."""
    out = []
    for phase in (False, True):
        s = bw.build(M)
        s.world.setup(s.starting)
        bw.seed()
        if phase:
            timings = {}
            replay = ip.imagine(s.agent, s.stack, bw.NUM_ROLLOUTS, timings=timings)
            assert timings["tier"] == "loop" and replay.device_rollout is None
        else:
            replay = M.Worker(s.stack).rollout(s.agent, bw.stop(bw.NUM_ROLLOUTS))
        out.append((replay, np.random.get_state(), torch.get_rng_state().clone()))
    (loop, lnp, ltorch), (phase, pnp, ptorch) = out
    assert not s.world._use_device_path()
    assert loop.episodes == phase.episodes and loop.nepisodes == 2 * bw.NUM_ENVS
    assert loop.ntimesteps == phase.ntimesteps == 2 * bw.HORIZON * bw.NUM_ENVS
    for key in loop.episodes:
        for name in bw.FIELDS:
            a, b = np.asarray(list(getattr(loop, name)[key])), np.asarray(list(getattr(phase, name)[key]))
            assert a.dtype == b.dtype
            np.testing.assert_array_equal(a, b, err_msg=f"episode {key} {name}")
        assert np.isfinite(np.asarray(list(loop.rewards[key]))).all() and (np.asarray(list(loop.rewards[key])) < 0).all()
    assert lnp[0] == pnp[0] and np.array_equal(lnp[1], pnp[1]) and lnp[2:] == pnp[2:]
    assert torch.equal(ltorch, ptorch)
