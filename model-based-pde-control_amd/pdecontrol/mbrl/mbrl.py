"""The model-based controller (reference ``pdecontrol/mbrl/mbrl.py``): ``PDEModelBasedController.learn()`` over this
repository's phases.  Class, constructor positionals, attribute names, ``HEADERS``, properties and method names are the
reference's; every phase is one call of this tree:

    warm-up, sampling   ``replay.extend(collect(worker, agent, stop, sink=replay))``        collection_phase
    evaluate_policy     ``collect(eval_worker, policy, eval_stop, deterministic=True)``      collection_phase
    delta statistics    ``update_delta_transform(replay, otransf, undscaling, delta)``       delta_phase
    surrogate update    ``update_surrogate(module, datamodule, fit, ...)``, a ``FitState`` per member in the trainer's place
    world rollouts      ``world_replay.extend(imagine(agent, world_stack, n, sink=world_replay))``   imagination_phase
    policy update       ``update_policy(agent, [world_replay.dataset(..), replay.dataset(..)], B, n)``   policy_phase

Both replays are ``DeviceExperienceReplay``s, on the agent's device with ``args.cuda`` and on the CPU otherwise, where
every phase takes its documented host route.  There is no wandb, Lightning, gym or plotting here: what the reference logs
goes to ``log`` (a callable ``(dict, commit)``; default a ``RunLog``), the visualisation callbacks and artifacts are not
built, and ``evaluate_surrogate`` returns the arrays the reference hands to its plot.

Keyword-only extensions of the constructor, all optional:

    log          callable ``(dict, commit)``; ``summarize`` / ``end_iteration`` read its ``summary`` where the reference
                 reads ``wandb.run.summary``; evaluation episodes go to ``<log.dir>/evaluation/eval_{iteration}.npz``
    make_env     factory of the single env (spaces, forcing, reward function, scenario); default ``gym.make(env_id)``
    make_envs    factory ``n -> vector env`` of ``n`` envs; default for the KS id a ``KSBatchedVecEnv`` on the GPU with
                 ``args.cuda`` and on the stepper's CPU twin otherwise, for the Burgers id (``pdegym.burgers.ENV_ID``) a
                 ``BurgersBatchedVecEnv`` on the GPU (refused without ``args.cuda``: no CPU twin), else ``gym.vector.make``
    env_config   dict for the default factories
    phase_tiers  "kernel" (default): every phase through its phase call, which picks its tier; "loop": the loop each
                 phase replaces (``Worker.rollout`` for the collection and the world rollouts, the reference's expression
                 over all transitions for the delta statistics, the datamodule's own loaders for the surrogate, the
                 reference's sampler and loader for the policy) over the same replays, agent and surrogate kernels --
                 the route tests/test_controller_gpu.py compares the kernel tiers with
"""
import json
import math
import os
import time

import numpy as np
import torch

from pdecontrol.mbrl import utils
from pdecontrol.mbrl.collection_phase import collect
from pdecontrol.mbrl.delta_phase import update_delta_transform
from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
from pdecontrol.mbrl.imagination_phase import imagine
from pdecontrol.mbrl.policy_phase import update_policy
from pdecontrol.mbrl.surrogate_phase import FitState, update_surrogate
from pdecontrol.mbrl.worker import PDEEnvStack, Worker
from pdecontrol.mbrl.world.world import WorldVecEnv
from pdecontrol.mbrl.world.wrappers import BaseWorldVecEnvWrapper
from pdecontrol.sac.sac import SAC
from pdecontrol.surrogates.common.datamodule import PDEDataModule
from pdecontrol.surrogates.common.dataset import StartingStateDataset, SubSeqDataset
from pdecontrol.surrogates.common.schedulers import Scheduler
from pdecontrol.surrogates.phyloss import phyloss
from pdecontrol.surrogates.surrogate import PDEEnsemble
from pdecontrol.surrogates.training import PDETrainingModule
from pdecontrol.surrogates.utils import ignore_extra_keywords
from pdegym.common.transforms import BatchTransform, Normalize, SampleTransform, ScaleTransform, SensorTransform
from pdegym.common.vec_wrappers import (StoreNActionsVecWrapper, StoreNObsVecWrapper, TransformActionWrapper,
                                        TransformObsWrapper)


def split_episodes(items, test_size):
    """``sklearn.model_selection.train_test_split(items, test_size=test_size)`` -> ``(train, test)``: sklearn's where it
    is importable, else the same draw from numpy's global generator (``n_test = ceil(test_size * n)``, one
    ``np.random.permutation(n)``, the test set its first ``n_test`` items, the train set the next ``n - n_test``)."""
    try:
        from sklearn.model_selection import train_test_split
    except ImportError:
        return _split_episodes(items, test_size)
    return train_test_split(items, test_size=test_size)


def _split_episodes(items, test_size):
    items = list(items)
    n = len(items)
    n_test = int(math.ceil(test_size * n))
    n_train = n - n_test
    if n_train < 1 or n_test < 1:
        raise ValueError(f"a split of {n} episodes with test_size={test_size} leaves the train or the test set empty")
    order = np.random.permutation(n)
    return [items[i] for i in order[n_test:n_test + n_train]], [items[i] for i in order[:n_test]]


class RunLog:
    """The default ``log``: ``log(data, commit)`` collects ``data`` into the current row and into ``summary`` (the last
    value of every key); ``commit`` closes the row into ``history``.  ``dir`` is the run directory."""

    def __init__(self, dir="pdecontrol-run"):
        self.dir = str(dir)
        self.summary, self.history, self._row = {}, [], {}

    def __call__(self, data, commit=True):
        self._row.update(data)
        self.summary.update(data)
        if commit:
            self.history.append(self._row)
            self._row = {}


class PDEModelBasedController:
    HEADERS = [
        "Iterations",
        "Time",
        "Num. Sur. Upd.",
        "Num. Pol. Upd.",
        "Num. Steps Sampled",
        "Avg. Eval. Ep. Return",
        "Avg. World Ep. Return",
        "Horizon",
        "World Buffer Samples",
        "Train Loss",
        "Val. Loss",
        "Sur./K",
        "SAC/Qloss",
        "SAC/PolicyLoss",
    ]

    def __init__(self, env_id, factory, config, args, *, log=None, make_env=None, make_envs=None, env_config=None,
                 phase_tiers="kernel"):
        if phase_tiers not in ("kernel", "loop"):
            raise ValueError(f"phase_tiers is {phase_tiers!r}: 'kernel' or 'loop'")
        self.env_id, self.factory, self.config, self.args = env_id, factory, config, args
        self.phase_tiers = phase_tiers
        self.log = RunLog(getattr(args, "name", None) or "pdecontrol-run") if log is None else log
        self.device = torch.device("cuda" if getattr(args, "cuda", False) else "cpu")
        self.env_config = dict(env_config or {})
        make_env = self._default_env if make_env is None else make_env
        make_envs = self._default_envs if make_envs is None else make_envs

        self.env = make_env()
        # vector environments used for experience collection and for the evaluation
        self.envs = make_envs(self.args.cpus)
        self.eval_envs = make_envs(self.args.cpus)

        self.samples_per_iteration = self.args.cpus * self.args.rollout_length
        self.num_pol_updates_per_iteration = int(self.args.policy_train_steps_per_sample * self.samples_per_iteration)
        self.sur_train_freq = int(self.args.surrogate_train_freq / self.samples_per_iteration)
        self.iteration, self.num_ensemble_updates, self.num_pol_updates = 0, 0, 0
        self.tau = self.config.training["tau"]
        self.tiers = []                                   # (phase, iteration, tier) of every phase call, in order
        self.last_surrogate_eval = None

        # length of the model rollouts, and of the training subsequences
        if isinstance(self.args.rollout_length_schedule, str):
            self.args.rollout_length_schedule = json.loads(self.args.rollout_length_schedule)
        self.schedule = Scheduler.factory(config=self.args.rollout_length_schedule)
        self.curriculum = Scheduler.factory(config=self.config.curriculum)

        self.setup_transforms()
        self.modules = [self.setup_surrogate() for _ in range(self.args.num_dynamics_models)]
        self.ensemble = PDEEnsemble(modules=self.modules, num_elites=self.args.num_elite_models)
        self.trainers = [FitState() for _ in range(self.args.num_dynamics_models)]

        self.setup_wrapped_envs()
        self.setup_world_envs()

        # replay buffers for real and imaginary experience
        self.replay = DeviceExperienceReplay(self.args.capacity, device=self.device)
        self.world_replay = DeviceExperienceReplay(self.imaginary_buffer_capacity, device=self.device)

        self.worker = Worker(self.stack)
        self.eval_worker = Worker(self.eval_stack)

        self.agent = SAC(self.stack.envs.single_observation_space, self.stack.envs.single_action_space, config=args)

        self.setup_stopping_conditions()
        os.makedirs(os.path.join(self.log.dir, "evaluation"), exist_ok=True)

    # -- default factories -------------------------------------------------------------------------------------------
    def _stepper_config(self):
        config = dict(self.env_config)
        config.setdefault("device", 0 if self.device.type == "cuda" else -1)
        return config

    def _burgers_config(self):
        """The env config of the Burgers id.  Its stepper has no CPU twin, so the default factories refuse it without
        ``args.cuda``, by name, as ``generate_dataset`` refuses ``device="cpu"``."""
        from pdegym import burgers
        if self.device.type != "cuda":
            raise ValueError(f"{burgers.ENV_ID}: a controller without args.cuda is refused, the Burgers stepper runs on a GPU "
                             f"only (set cuda, or pass make_env / make_envs)")
        return dict(self.env_config)

    def _default_env(self):
        from pdegym import burgers
        from pdegym._gym import gym
        from pdegym.kuramoto import ENV_ID
        if self.env_id == ENV_ID:
            return gym.make(self.env_id, config=self._stepper_config())
        if self.env_id == burgers.ENV_ID:
            return burgers.make(config=self._burgers_config())
        return gym.make(self.env_id, **self.env_config)

    def _default_envs(self, n):
        from pdegym import burgers
        from pdegym._gym import gym
        from pdegym.kuramoto import ENV_ID, make_vec
        if self.env_id == ENV_ID:
            config = self._stepper_config()
            return make_vec(n, config=config, device=config.pop("device"))
        if self.env_id == burgers.ENV_ID:
            return burgers.make_vec(n, config=self._burgers_config(), device=0)
        return gym.vector.make(self.env_id, num_envs=n, **self.env_config)

    # -- set-up ----------------------------------------------------------------------------------------------------
    @property
    def _scenario(self):
        return self.env.unwrapped.scenario

    @property
    def _tstep(self):
        return self._scenario["cfg_steps"] * self._scenario["dt"]

    def setup_transforms(self):
        self.oscaling = ScaleTransform(batched=True, aggregate=True, frozen=False)

        low = self.envs.single_action_space.low[np.newaxis, ...]
        high = self.envs.single_action_space.high[np.newaxis, ...]
        self.ascaling = ScaleTransform(bounds=(low, high), aggregate=True, frozen=True, batched=True).Inverse

        # the external forcing term of an action, and its scaling
        self.forcing = BatchTransform(self.env.unwrapped.forcing)
        lo, hi = np.squeeze(self.forcing(low), axis=0), np.squeeze(self.forcing(high), axis=0)
        self.pdescaling = BatchTransform(ScaleTransform(bounds=(lo, hi), scale=(-1, 1), aggregate=True, frozen=True))

        # normalisation of the scaled state changes: the delta phase fits the bare Normalize, the surrogates and
        # their training modules share it through one batch view (the form the fused rollout recognises)
        self.undscaling = Normalize(aggregate=True, batched=True)
        self._undscaling_view = BatchTransform(self.undscaling)

        self.agent_sensor = BatchTransform(SensorTransform(stride=1))
        self.world_sensor = BatchTransform(SensorTransform(stride=1))

        # connectors: replay -> agent, replay -> world model, world replay -> agent
        self.replay_to_agent = SampleTransform(otransf=[self.oscaling, self.agent_sensor], atransf=self.ascaling.Inverse)
        self.replay_to_world = SampleTransform([self.oscaling, self.world_sensor],
                                               [self.forcing, self.pdescaling, self.world_sensor])
        self.world_replay_to_agent = SampleTransform(atransf=self.ascaling.Inverse)

    def _phase(self):
        return "initial" if self.iteration <= 0 else "iterations"

    def setup_surrogate(self):
        scenario = self._scenario
        dataloss = ignore_extra_keywords(getattr(phyloss, self.config.loss))(**scenario, reduction="none")
        model = self.factory.model(**scenario, **self.config.model)
        surrogate = self.factory.surrogate(delta=self._tstep, dscaling=self._undscaling_view.Inverse, tau=self.tau, **scenario,
                                           **self.config.surrogate, **model)
        module = PDETrainingModule(surrogate=surrogate, loss=dataloss, tau=self.tau, stransf=self.replay_to_world.Inverse,
                                   tstep=self._tstep, delta=self._tstep, undscaling=self._undscaling_view,
                                   **self.config.training[self._phase()])
        return module.to(self.device)

    def setup_stopping_conditions(self):
        self.warmup = lambda ts, _: ts >= self.args.learning_starts
        self.sampling = lambda ts, _: ts >= self.samples_per_iteration
        self.eval_stop = lambda _, ep: ep >= self.args.num_eval_episodes
        self.world_stop = lambda _, eps: eps >= self.num_world_rollouts
        self.world_eval_stop = lambda ts, eps: eps >= 1

    def _real_stack(self, envs, frozen):
        ostore = StoreNObsVecWrapper(envs, num_steps=1)
        envs = TransformObsWrapper(ostore, self.oscaling, frozen=frozen)
        envs = TransformObsWrapper(envs, self.world_sensor)
        world_wrapper = BaseWorldVecEnvWrapper(env=envs, surrogate=self.ensemble, tstep=self._tstep)
        envs = TransformObsWrapper(world_wrapper, self.agent_sensor)
        astore = StoreNActionsVecWrapper(envs, num_steps=1)
        envs = TransformActionWrapper(astore, self.ascaling, frozen=True)
        return PDEEnvStack(envs=envs, ostore=ostore, astore=astore, world_wrapper=world_wrapper)

    def setup_wrapped_envs(self):
        self.stack = self._real_stack(self.envs, frozen=False)
        self.envs = self.stack.envs
        self.eval_stack = self._real_stack(self.eval_envs, frozen=True)
        self.eval_envs = self.eval_stack.envs

    def _world(self, num_envs, horizon):
        env = self.env.unwrapped
        return WorldVecEnv(surrogate=self.ensemble, observation_space=self.env.observation_space,
                           action_space=self.env.action_space, max_episode_steps=env.max_episode_steps,
                           stransf=self.replay_to_world.Inverse, reward_func=env.reward_func, num_envs=num_envs,
                           horizon=horizon, tstep=self._tstep, batched_reward_func=getattr(env, "batched_reward_func", None))

    def _world_stack(self, world):
        ostore = StoreNObsVecWrapper(world, num_steps=1)
        envs = TransformObsWrapper(ostore, self.agent_sensor)
        envs = TransformActionWrapper(envs, self.world_sensor)
        envs = TransformActionWrapper(envs, self.pdescaling, frozen=True)
        envs = TransformActionWrapper(envs, self.forcing, frozen=True)
        envs = TransformActionWrapper(envs, self.ascaling, frozen=True)
        astore = StoreNActionsVecWrapper(envs, num_steps=1)
        return PDEEnvStack(envs=astore, ostore=ostore, astore=astore, world_wrapper=None)

    def setup_world_envs(self):
        horizon = int(self.schedule(iteration=self.iteration))
        self.world = self._world(self.args.model_rollouts_batch_size, horizon)
        self.eval_world = self._world(1, horizon)
        self.world_stack = self._world_stack(self.world)
        self.world_env = self.world_stack.envs
        self.eval_world_stack = self._world_stack(self.eval_world)
        self.eval_world_env = self.eval_world_stack.envs

    # -- phases ------------------------------------------------------------------------------------------------------
    def _collect(self, worker, agent, stop, name, deterministic=False, sink=None):
        """One real-env phase: ``collect`` (which picks its tier), or with ``phase_tiers = "loop"`` the loop itself."""
        if self.phase_tiers == "loop":
            rollout = worker.rollout(agent, stop, deterministic)
            rollout.tier = "loop"
        else:
            rollout = collect(worker, agent, stop, deterministic, **({} if sink is None else {"sink": sink}))
        self.tiers.append((name, self.iteration, rollout.tier))
        return rollout

    def _imagine(self, agent, stack, num_rollouts, name, sink=None):
        timings = {}
        if self.phase_tiers == "loop":
            rollout = Worker(stack).rollout(agent, lambda ts, eps: eps >= num_rollouts)
            timings["tier"] = "loop"
        else:
            rollout = imagine(agent, stack, num_rollouts, timings=timings, **({} if sink is None else {"sink": sink}))
        self.tiers.append((name, self.iteration, timings.get("tier")))
        return rollout

    def learn(self):
        self.log({"Start": time.time()}, commit=False)

        # initial exploration with a random policy; the world wrapper is off while it runs
        self.stack.world_wrapper.disable()
        explore = utils.RandomAgent(self.envs.action_space)
        self.replay.extend(self._collect(self.worker, explore, self.warmup, "warmup", sink=self.replay))
        self.stack.world_wrapper.enable()

        # evaluate the untrained policy
        self.evaluate_policy(self.agent)

        while self.num_steps_sampled < self.args.total_timesteps - self.args.learning_starts:
            self.replay.extend(self._collect(self.worker, self.agent, self.sampling, "collect", sink=self.replay))

            # update the surrogate models every `sur_train_freq` iterations
            if self.iteration % self.sur_train_freq == 0:
                self.update_delta_transform()
                scores = [self.update_surrogate(module, trainer) for module, trainer in zip(self.ensemble.modules, self.trainers)]
                self.ensemble.update_elites(scores)
                self.num_ensemble_updates += 1
                self.log({"Num. Ensemble Updates": self.num_ensemble_updates}, commit=False)

            # starting states of the world env. from the replay, the horizon from the schedule
            starting = StartingStateDataset(data=self.replay.data, length=self.tau, stride=1, bootstrapping=False,
                                            stransf=self.replay_to_world)
            self.world.setup(starting)
            self.world.horizon = int(self.schedule(iteration=self.iteration))
            self.world_replay.resize(self.imaginary_buffer_capacity)

            # imagined rollouts of the policy into their own buffer (a fresh worker every time)
            self.world_replay.extend(self._imagine(self.agent, self.world_stack, self.num_world_rollouts, "imagine",
                                                   sink=self.world_replay))

            self.update_policy()

            if self.iteration % self.args.agent_eval_freq == 0:
                self.evaluate_policy(self.agent)
                self.evaluate_surrogate()
                self.log_world_stats()

            self.end_iteration()

            if self.iteration % self.args.status_report_freq == 0:
                self.summarize()

    def log_world_stats(self):
        mean, std = self.world_replay.statistics()
        self.log({"Avg. World Rll. Return": mean, "Std. World. Rll. Return": std,
                  "Avg. World Step Rew.": mean / self.world.horizon}, commit=False)

    def evaluate_policy(self, policy):
        rollout = self._collect(self.eval_worker, policy, self.eval_stop, "evaluate", deterministic=True)
        mean, std = rollout.statistics()
        self.log({"Avg. Eval. Ep. Return": mean, "Std. Eval. Ep. Return": std}, commit=True)
        obs, actions, _, rewards, *_ = rollout.dataset()
        np.savez(os.path.join(self.log.dir, "evaluation", f"eval_{self.iteration}.npz"), obs=obs, actions=actions,
                 rewards=rewards)
        return rollout

    def evaluate_surrogate(self, horizon=None):
        """The surrogate against one stored episode: ``horizon`` steps (default ``args.surrogate_eval_horizon``, else the
        reference's 30) of the episode's actions replayed in the evaluation world from ``tau`` of its states.  Returns,
        and keeps as ``last_surrogate_eval``, what the reference plots: ``obs`` / ``opred`` [horizon, N], ``actions``
        [horizon, N], ``rewards`` / ``rpred`` [horizon].  None without a stopped episode, or (after the episode's draw)
        when the drawn episode is shorter than ``tau + horizon + 1`` steps, where the reference's second draw raises."""
        horizon = int(getattr(self.args, "surrogate_eval_horizon", 30) if horizon is None else horizon)
        if not self.replay.stopped:
            return None
        index = np.random.choice(self.replay.stopped)
        sample = self.replay.sample(index)
        sample = sample.apply(lambda x: x.unsqueeze(0)).tonumpy()
        length = sample.obs.shape[1]
        if length - self.tau - horizon <= 0:
            return None
        start = np.random.randint(0, length - self.tau - horizon)

        # warm-start the episode in the evaluation world with states taken from the replay
        starting = sample.apply(lambda x: x[:, start:start + self.tau])
        starting = SubSeqDataset(data=starting, length=self.tau, bootstrapping=False, stransf=self.replay_to_world)
        self.eval_world.setup(starting)
        self.eval_world.horizon = horizon

        # repeat the episode's actions
        actions = self.replay_to_agent.atransf(np.squeeze(sample.actions, axis=0))
        actions = actions[np.newaxis, start + self.tau:start + self.tau + horizon]
        rollout = self._imagine(utils.ActionRepeatAgent(actions), self.eval_world_stack, 1, "evaluate_surrogate")
        prediction = rollout.sample(0).tonumpy()

        sample = sample.apply(lambda x: x[:, start + self.tau:start + self.tau + horizon])
        sample = self.replay_to_world(sample.apply(lambda x: np.squeeze(x, axis=0)))
        self.last_surrogate_eval = dict(actions=np.squeeze(sample.actions, axis=1), obs=np.squeeze(sample.obs, axis=1),
                                        opred=np.squeeze(prediction.obs, axis=1), rewards=np.asarray(sample.rewards),
                                        rpred=np.asarray(prediction.rewards))
        return self.last_surrogate_eval

    def update_policy(self):
        batch_size, num_updates = self.args.policy_batch_size, self.num_pol_updates_per_iteration
        if self.phase_tiers == "loop":
            done, tier = self._update_policy_loop(batch_size, num_updates), "loop"
        else:
            timings = {}
            done = update_policy(self.agent, [self.world_replay.dataset(self.world_replay_to_agent),
                                              self.replay.dataset(self.replay_to_agent)], batch_size, num_updates,
                                 timings=timings)
            tier = timings.get("tier")
        self.tiers.append(("update_policy", self.iteration, tier))
        self.num_pol_updates += done
        self.log({"Num. Pol. Upd.": self.num_pol_updates}, commit=False)

    def _update_policy_loop(self, batch_size, num_updates):
        """The reference's lines: two one-step datasets, a sampler with replacement, a loader, ``agent.update``."""
        from torch.utils.data import ConcatDataset, DataLoader, RandomSampler
        from pdecontrol.surrogates.common.dataset import PDEDataLoader
        sets = [SubSeqDataset(data=r.data, length=1, stride=1, bootstrapping=False, stransf=t)
                for r, t in ((self.world_replay, self.world_replay_to_agent), (self.replay, self.replay_to_agent))]
        data = ConcatDataset(sets)
        sampler = RandomSampler(data, replacement=True, num_samples=batch_size * num_updates)
        loader = DataLoader(dataset=data, batch_size=batch_size, shuffle=False, sampler=sampler,
                            collate_fn=PDEDataLoader.sample_collate)
        done = 0
        for batch in loader:
            self.agent.update(batch)
            done += 1
        return done

    def update_surrogate(self, module, trainer):
        train, val = split_episodes(self.replay.episodes, test_size=self.args.val_split_ratio)
        phase = self._phase()
        training_config = dict(self.config.training[phase])
        trainer_config = self.config.trainer[phase]
        algorithm = trainer_config.get("gradient_clip_algorithm")
        if algorithm not in (None, "norm"):
            raise ValueError(f"trainer config: gradient_clip_algorithm is {algorithm!r}, and only 'norm' (gradient_clip_val "
                             f"as a bound on the global gradient norm) is built")
        if self.device.type == "cuda":
            training_config.setdefault("device_data", self.device)
        forced = {"tier": "loop"} if self.phase_tiers == "loop" else {}   # the datamodule's own loaders
        if trainer_config.get("gradient_clip_val") is not None:           # the trainer's own key (reference mbrl.py:357-365)
            forced["gradient_clip_val"] = trainer_config["gradient_clip_val"]
        datamodule = PDEDataModule(data=self.replay.data, train=train, val=val, tau=self.tau, stransf=self.replay_to_world,
                                   curriculum=self.curriculum, iteration=self.iteration, bootstrapping=True,
                                   **training_config)
        score = update_surrogate(module, datamodule, trainer, max_steps=trainer_config.get("max_steps", 0),
                                 min_steps=trainer_config.get("min_steps", 0), patience=training_config["patience"], **forced)
        self.tiers.append(("update_surrogate", self.iteration, trainer.tier))
        self.log({"Val. Loss": score}, commit=False)
        return score

    def update_delta_transform(self):
        if self.phase_tiers == "loop":
            from pdecontrol.mbrl.delta_phase import _fit_reference
            _fit_reference(self.replay.transitions(), self.replay_to_world.otransf, self.undscaling, self._tstep)
            update, tier = None, "loop"
        else:
            update = update_delta_transform(self.replay, self.replay_to_world.otransf, self.undscaling, self._tstep)
            tier = update.tier
        # the statistics of a replay in HBM come back as device tensors; the captured training step reads them as host
        # scalars while it is being captured, where a copy from the device is not allowed: keep them on the host
        und = self.undscaling
        if isinstance(und.mean, torch.Tensor) and und.mean.is_cuda:
            und.mean, und.var = und.mean.cpu(), und.var.cpu()
        self.tiers.append(("update_delta_transform", self.iteration, tier))
        return update

    def summarize(self):
        summary = self.log.summary
        values = [summary[key] if key in summary else "-X-" for key in self.HEADERS]
        try:
            from tabulate import tabulate
            print(tabulate([values], headers=self.HEADERS))
        except ImportError:
            print(" | ".join(f"{k}: {v}" for k, v in zip(self.HEADERS, values)))

    def end_iteration(self):
        self.log({
            "Iterations": self.iteration,
            "Num. Steps Sampled": self.num_steps_sampled + self.args.learning_starts,
            "Horizon": self.world.horizon,
            "World Buffer Cap.": self.imaginary_buffer_capacity,
            "World Buffer Filled": self.world_replay.ntimesteps / self.imaginary_buffer_capacity,
            "World Buffer Samples": self.world_replay.ntimesteps,
            "World Rollouts": self.num_world_rollouts * self.iteration,
            "Time": time.time() - self.log.summary["Start"],
        }, True)
        self.iteration += 1

    @property
    def imaginary_buffer_capacity(self):
        capacity = (self.args.model_buffer_store_iterations * self.args.model_rollouts_per_sample
                    * self.samples_per_iteration * self.world.horizon)
        return min(capacity, self.args.model_buffer_max_capacity)

    @property
    def num_world_rollouts(self):
        return int(self.args.model_rollouts_per_sample * self.samples_per_iteration)

    @property
    def num_steps_sampled(self):
        return self.iteration * self.samples_per_iteration


__all__ = ["PDEModelBasedController", "RunLog", "split_episodes"]
