"""``PDEModelBasedController`` on the host (pdecontrol/mbrl/mbrl.py), over the stepper's CPU twin: the reference's import
paths and derived quantities, the sequence of phase calls ``learn()`` makes, a toy run end to end with its row counts
and its reproducibility, and the train / validation split against sklearn's."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _controller_scenario as cs  # noqa: E402


# ----------------------------------------------------------------------------------------------------------------------
# 1. imports and arithmetic
# ----------------------------------------------------------------------------------------------------------------------
def test_the_reference_import_paths_resolve():
    from pdecontrol.mbrl import utils
    from pdecontrol.mbrl.mbrl import PDEModelBasedController
    from pdecontrol.mbrl.utils import ActionRepeatAgent, RandomAgent, tonumpy, totorch  # noqa: F401
    assert utils.RandomAgent is RandomAgent
    for name in ("samples_per_iteration", "num_pol_updates_per_iteration", "sur_train_freq"):
        assert name in PDEModelBasedController.__init__.__code__.co_names, name
    for name in ("imaginary_buffer_capacity", "num_world_rollouts", "num_steps_sampled"):
        assert isinstance(getattr(PDEModelBasedController, name), property), name
    for name in ("setup_transforms", "setup_surrogate", "setup_wrapped_envs", "setup_world_envs", "setup_stopping_conditions",
                 "learn", "update_policy", "update_surrogate", "update_delta_transform", "evaluate_policy",
                 "evaluate_surrogate", "log_world_stats", "end_iteration", "summarize"):
        assert callable(getattr(PDEModelBasedController, name)), name
    assert PDEModelBasedController.HEADERS[:5] == ["Iterations", "Time", "Num. Sur. Upd.", "Num. Pol. Upd.", "Num. Steps Sampled"]
    assert len(PDEModelBasedController.HEADERS) == 14


def _two_stage():
    # iteration 0 -> 2, later iterations -> 5 (searchsorted(steps, iteration, "left"))
    return json.dumps(dict(scheduler="StepScheduler", steptype="iteration", steps=[0], values=[2, 5]))


def test_derived_quantities_equal_the_hand_computed_values(tmp_path):
    args = cs.toy_args(cpus=3, rollout_length=2, policy_train_steps_per_sample=1.5, surrogate_train_freq=12,
                       model_rollouts_per_sample=2, model_buffer_store_iterations=3, model_buffer_max_capacity=50,
                       rollout_length_schedule=_two_stage())
    c = cs.build(tmp_path / "a", args=args)
    assert c.samples_per_iteration == 6                       # 3 * 2
    assert c.num_pol_updates_per_iteration == 9               # int(1.5 * 6)
    assert c.sur_train_freq == 2                              # int(12 / 6)
    assert c.num_world_rollouts == 12                         # 2 * 6
    assert c.world.horizon == 2 and c.eval_world.horizon == 2
    assert c.imaginary_buffer_capacity == 50                  # min(3 * 2 * 6 * 2 = 72, 50): at the cap
    assert c.world_replay.capacity == 50
    args.model_buffer_max_capacity = 100
    assert c.imaginary_buffer_capacity == 72                  # below the cap
    c.world.horizon = int(c.schedule(iteration=1))
    assert c.world.horizon == 5 and c.imaginary_buffer_capacity == 100    # min(180, 100)
    assert c.num_steps_sampled == 0
    c.iteration = 7
    assert c.num_steps_sampled == 42
    assert c.warmup(11, 0) is False and c.warmup(12, 0) is True
    assert c.sampling(5, 99) is False and c.sampling(6, 0) is True
    assert c.eval_stop(10 ** 6, 2) is False and c.eval_stop(0, 3) is True
    assert c.world_stop(10 ** 6, 11) is False and c.world_stop(0, 12) is True
    assert c.world_eval_stop(10 ** 6, 0) is False and c.world_eval_stop(0, 1) is True

    # the reference's defaults at five envs
    args = cs.toy_args(cpus=5, rollout_length=1, policy_train_steps_per_sample=5, surrogate_train_freq=500,
                       model_rollouts_per_sample=100, model_buffer_store_iterations=30, model_buffer_max_capacity=1000000)
    c = cs.build(tmp_path / "b", args=args)
    assert (c.samples_per_iteration, c.num_pol_updates_per_iteration, c.sur_train_freq, c.num_world_rollouts) == (5, 25, 100, 500)
    assert c.imaginary_buffer_capacity == 30000               # 30 * 100 * 5 * 2
    c.iteration = 3
    assert c.num_steps_sampled == 15
    assert c.replay.device.type == "cpu" and c.world_replay.device.type == "cpu"


# ----------------------------------------------------------------------------------------------------------------------
# 2. the sequence of phase calls
# ----------------------------------------------------------------------------------------------------------------------
class _StubReplay:
    def __init__(self, name, events):
        self.name, self.events = name, events
        self.ntimesteps, self.stopped, self.episodes, self.data = 0, [], [0, 1, 2, 3], ("data", name)

    def extend(self, rollout):
        self.events.append(("extend", self.name, rollout.label))
        self.ntimesteps += rollout.ntimesteps

    def resize(self, size):
        self.events.append(("resize", self.name, size))

    def statistics(self):
        self.events.append(("statistics", self.name))
        return np.float32(-1.0), np.float32(0.5)

    def dataset(self, stransf=None):
        return ("view", self.name, stransf)


def test_learn_makes_the_phase_calls_of_the_reference_in_order(tmp_path, monkeypatch):
    from pdecontrol.mbrl import mbrl, utils
    spi = 3
    args = cs.toy_args(total_timesteps=12 + 4 * spi, surrogate_train_freq=2 * spi, agent_eval_freq=2, status_report_freq=3,
                       rollout_length_schedule=_two_stage())
    config = cs.toy_config()
    config.training["initial"]["patience"], config.training["iterations"]["patience"] = 11, 22
    config.trainer["initial"].update(max_steps=100, min_steps=10)
    config.trainer["iterations"].update(max_steps=40, min_steps=4)
    c = cs.build(tmp_path, args=args, config=config)
    assert c.sur_train_freq == 2 and c.samples_per_iteration == spi
    events = []
    c.replay, c.world_replay = _StubReplay("replay", events), _StubReplay("world_replay", events)

    def stop_name(stop):
        return next(n for n in ("warmup", "sampling", "eval_stop") if getattr(c, n) is stop)

    def rollout(label, n):
        return types.SimpleNamespace(label=label, tier="stub", ntimesteps=n, statistics=lambda: (np.float32(-2.0), np.float32(0.1)),
                                     dataset=lambda: (np.zeros((n, 1, 64)), np.zeros((n, 1, 4)), None, np.zeros(n)))

    def collect(worker, agent, stop, deterministic=False, sink=None):
        who = "worker" if worker is c.worker else "eval_worker" if worker is c.eval_worker else "?"
        what = "agent" if agent is c.agent else type(agent).__name__
        if type(agent) is utils.RandomAgent:
            assert agent.action_space is c.envs.action_space
        events.append(("collect", who, what, stop_name(stop), deterministic, getattr(sink, "name", None),
                       c.stack.world_wrapper._enabled))
        return rollout("real", 12 if stop is c.warmup else spi)

    def delta(replay, otransf, undscaling, delta):
        assert otransf is c.replay_to_world.otransf and undscaling is c.undscaling
        events.append(("delta", replay.name, round(float(delta), 6)))
        return types.SimpleNamespace(tier="stub")

    def split(items, test_size):
        events.append(("split", tuple(items), test_size))
        return [0, 1, 2], [3]

    def surrogate(module, datamodule, fit, *, max_steps, min_steps, patience):
        assert datamodule.data == ("data", "replay") and (datamodule.train, datamodule.val) == ([0, 1, 2], [3])
        assert datamodule.tau == cs.TAU and datamodule.stransf is c.replay_to_world and datamodule.bootstrapping is True
        assert datamodule.curriculum is c.curriculum and datamodule.iteration == c.iteration
        fit.tier = "stub"
        events.append(("surrogate", c.modules.index(module), c.trainers.index(fit), max_steps, min_steps, patience))
        return 0.25 + c.modules.index(module)

    def starting(data, length, stride, bootstrapping, stransf):
        assert stransf is c.replay_to_world
        events.append(("starting", data, length, stride, bootstrapping))
        return "starting"

    def imagine(agent, stack, num_rollouts, timings=None, sink=None):
        assert agent is c.agent and stack is c.world_stack
        timings["tier"] = "stub"
        events.append(("imagine", num_rollouts, getattr(sink, "name", None), c.world.horizon))
        return rollout("imagined", num_rollouts * c.world.horizon)

    def policy(agent, datasets, batch_size, num_updates, timings=None):
        assert agent is c.agent
        assert datasets == [("view", "world_replay", c.world_replay_to_agent), ("view", "replay", c.replay_to_agent)]
        events.append(("policy", batch_size, num_updates))
        return num_updates

    for name, fn in (("collect", collect), ("update_delta_transform", delta), ("split_episodes", split),
                     ("update_surrogate", surrogate), ("imagine", imagine), ("update_policy", policy),
                     ("StartingStateDataset", starting)):
        monkeypatch.setattr(mbrl, name, fn)
    monkeypatch.setattr(c.world, "setup", lambda s: events.append(("world.setup", s)))
    monkeypatch.setattr(c.ensemble, "update_elites", lambda scores: events.append(("elites", tuple(scores))))
    monkeypatch.setattr(c, "summarize", lambda: events.append(("summarize", c.iteration)))
    c.learn()

    tstep = round(c.env.cfg_steps * c.env.dt, 6)
    evaluate = [("collect", "eval_worker", "agent", "eval_stop", True, None, True)]
    want = [("collect", "worker", "RandomAgent", "warmup", False, "replay", False), ("extend", "replay", "real")] + evaluate
    for it in range(4):
        horizon = 2 if it == 0 else 5
        want += [("collect", "worker", "agent", "sampling", False, "replay", True), ("extend", "replay", "real")]
        if it % 2 == 0:
            steps = (100, 10, 11) if it == 0 else (40, 4, 22)
            want += [("delta", "replay", tstep)]
            for m in range(2):
                want += [("split", (0, 1, 2, 3), 0.34), ("surrogate", m, m) + steps]
            want += [("elites", (0.25, 1.25))]
        want += [("starting", ("data", "replay"), cs.TAU, 1, False), ("world.setup", "starting"),
                 ("resize", "world_replay", min(3 * 2 * spi * horizon, 1000000)),
                 ("imagine", 2 * spi, "world_replay", horizon), ("extend", "world_replay", "imagined"),
                 ("policy", 8, spi)]
        if it % 2 == 0:
            want += evaluate + [("statistics", "world_replay")]
        if (it + 1) % 3 == 0:
            want += [("summarize", it + 1)]
    assert events == want, "\n".join(f"{a}   |   {b}" for a, b in zip(events, want) if a != b)
    assert c.iteration == 4 and c.num_pol_updates == 4 * spi and c.num_ensemble_updates == 2

    # the log: the reference's keys, row by row (evaluate_policy and end_iteration commit)
    history = c.log.history
    assert len(history) == 1 + 2 + 4
    assert set(history[0]) == {"Start", "Avg. Eval. Ep. Return", "Std. Eval. Ep. Return"}
    ends = [row for row in history if "Iterations" in row]
    assert [row["Iterations"] for row in ends] == [0, 1, 2, 3]
    for it, row in enumerate(ends):
        assert {"Iterations", "Num. Steps Sampled", "Horizon", "World Buffer Cap.", "World Buffer Filled", "World Buffer Samples",
                "World Rollouts", "Time"} <= set(row)
        assert row["Num. Steps Sampled"] == 12 + it * spi and row["Horizon"] == (2 if it == 0 else 5)
        assert row["World Rollouts"] == 2 * spi * it and row["World Buffer Samples"] == c.world_replay.ntimesteps or it < 3
        assert ("Avg. World Rll. Return" in row) == (it % 2 == 0)
        assert "Num. Pol. Upd." in row or "Num. Pol. Upd." in history[history.index(row) - 1]
    assert history[1]["Num. Ensemble Updates"] == 1 and history[1]["Num. Pol. Upd."] == spi
    assert c.log.summary["Num. Pol. Upd."] == 4 * spi and c.log.summary["Num. Ensemble Updates"] == 2


# ----------------------------------------------------------------------------------------------------------------------
# 3. a toy run end to end
# ----------------------------------------------------------------------------------------------------------------------
def _toy(log_dir):
    c = cs.build(log_dir)
    cs.seed_spaces(c)
    c.learn()
    return c


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    return _toy(tmp_path_factory.mktemp("toy"))


def test_the_toy_run_completes_with_the_predicted_rows(toy):
    c = toy
    assert c.iteration == 2 and c.num_ensemble_updates == 2 and c.num_pol_updates == 2 * 3
    assert c.replay.ntimesteps == 12 + 2 * 3                  # learning_starts + two iterations of cpus * rollout_length
    assert c.world_replay.ntimesteps == 2 * 6 * 2             # per iteration: 2 * 3 rollouts of horizon 2
    assert c.world_replay.capacity == 3 * 2 * 3 * 2
    scalars = [(k, v) for row in c.log.history for k, v in row.items()]
    assert len(scalars) > 20 and all(np.isfinite(float(v)) for _, v in scalars), scalars
    assert [n for n, _, _ in c.tiers[:3]] == ["warmup", "evaluate", "collect"]
    assert c.tiers[0][2] == "loop"                            # the CPU twin
    for it in (0, 1):
        path = os.path.join(c.log.dir, "evaluation", f"eval_{it}.npz")
        assert os.path.exists(path), path
        with np.load(path) as z:
            assert sorted(z.files) == ["actions", "obs", "rewards"]
            assert z["obs"].shape[0] == z["actions"].shape[0] == z["rewards"].shape[0] >= 3 * 4
    ev = c.last_surrogate_eval
    assert sorted(ev) == ["actions", "obs", "opred", "rewards", "rpred"]
    horizon = c.args.surrogate_eval_horizon
    assert ev["obs"].shape == ev["opred"].shape == (horizon, 64) and ev["actions"].shape[0] == horizon
    assert ev["rewards"].shape == ev["rpred"].shape == (horizon,)
    assert all(np.isfinite(v).all() for v in ev.values())


def test_a_second_toy_run_from_the_same_seeds_is_identical(toy, tmp_path):
    a, b = toy, _toy(tmp_path)
    for x, y in ((a.agent.policy, b.agent.policy), (a.agent.critic, b.agent.critic), (a.agent.critic_target, b.agent.critic_target)):
        for (k, u), (_, v) in zip(x.state_dict().items(), y.state_dict().items()):
            assert torch.equal(u, v), k
    for m, n in zip(a.modules, b.modules):
        for (k, u), (_, v) in zip(m.state_dict().items(), n.state_dict().items()):
            assert torch.equal(u, v), k
    for r, s in ((a.replay, b.replay), (a.world_replay, b.world_replay)):
        (rows_r, meta_r), (rows_s, meta_s) = cs.slabs(r), cs.slabs(s)
        assert meta_r == meta_s
        for u, v in zip(rows_r, rows_s):
            assert u.tobytes() == v.tobytes()
    assert torch.equal(a.oscaling.vmin, b.oscaling.vmin) and torch.equal(a.oscaling.vmax, b.oscaling.vmax)
    assert torch.equal(a.undscaling.mean, b.undscaling.mean) and torch.equal(a.undscaling.var, b.undscaling.var)
    # what each controller owns: the env streams and the action space's generator (the global generators are compared
    # at the same point of two fresh runs in the next test)
    ga, gb = cs.generators(a), cs.generators(b)
    for k in ("space", "mt_state", "mt_pos"):
        cs.same_generators({k: ga[k]}, {k: gb[k]}, k)
    strip = lambda rows: [{k: v for k, v in row.items() if k not in ("Start", "Time")} for row in rows]
    assert json.dumps(strip(a.log.history), default=float) == json.dumps(strip(b.log.history), default=float)


def test_the_global_generators_end_where_a_first_run_left_them(tmp_path):
    ends = []
    for name in ("a", "b"):
        c = _toy(tmp_path / name)
        ends.append(cs.generators(c))
    cs.same_generators(ends[0], ends[1])


# ----------------------------------------------------------------------------------------------------------------------
# 4. the split
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 7, 10, 33])
@pytest.mark.parametrize("test_size", [0.1, 0.25, 0.5])
def test_the_local_split_equals_sklearns(n, test_size):
    model_selection = pytest.importorskip("sklearn.model_selection")
    from pdecontrol.mbrl.mbrl import _split_episodes, split_episodes
    items = [3 * i + 1 for i in range(n)]
    np.random.seed(n)
    want = model_selection.train_test_split(items, test_size=test_size)
    state = np.random.get_state()
    for fn in (_split_episodes, split_episodes):
        np.random.seed(n)
        train, val = fn(items, test_size)
        assert (train, val) == (want[0], want[1]), fn.__name__
        after = np.random.get_state()
        assert after[0] == state[0] and np.array_equal(after[1], state[1]) and after[2:] == state[2:], fn.__name__
