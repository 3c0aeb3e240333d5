"""Experience collection (mirror of the reference's ``pdecontrol/mbrl/worker.py:13-93``).

``PDEEnvStack`` names the pieces of a wrapped vector env the worker reads: the outermost env it steps, the observation
store whose ``obs`` / ``finals`` are what the replay records (the env-side observation, not the agent's view of it), the
action store whose ``actions`` are the raw agent actions, and the optional world-model wrapper of the real-env stack.

``Worker.rollout(agent, stop)`` steps the stack with ``agent.select_action`` until ``stop(ntimesteps, nstopped)`` holds
and returns the steps as a fresh ``ExperienceReplay``, one sub-environment per ``vindex`` slot.  The worker keeps the
last observation between calls, so consecutive rollouts continue the running episodes; ``reset()`` drops it and the next
rollout starts with ``envs.reset()``.

pdecontrol/mbrl/imagination_phase.py runs the same loop for the imagined-rollout stack with the closed loop kept in HBM.
"""
from typing import Any, Callable, List, NamedTuple

import torch

from pdecontrol.mbrl.replay import ExperienceReplay
from pdecontrol.mbrl.types import Sample


class PDEEnvStack(NamedTuple):
    envs: Any
    ostore: Any
    astore: Any
    world_wrapper: Any = None


def _stored(store, values):
    """A copy of a store's history reduced to its valid slots: ``[E, num_steps, ...][mask]``."""
    return values.copy()[store.mask]


class Worker:
    def __init__(self, stack: PDEEnvStack, callbacks: List[Any] = None):
        self.stack = stack
        self.callbacks = [] if callbacks is None else callbacks
        self._last_obs = None
        self._last_stored_obs = None

    def reset(self) -> None:
        self._last_obs = None
        self._last_stored_obs = None

    def start(self, **reset_kwargs) -> None:
        """The reset a fresh worker's first rollout makes, made now: ``envs.reset(**reset_kwargs)`` (``seed=`` for a
        reproducible first episode) and the stored observation that goes with it."""
        self._last_obs = self.stack.envs.reset(**reset_kwargs)
        self._last_stored_obs = _stored(self.stack.ostore, self.stack.ostore.obs)

    def rollout(self, agent, stop: Callable, deterministic: bool = False) -> ExperienceReplay:
        replay = ExperienceReplay()
        envs, ostore, astore = self.stack.envs, self.stack.ostore, self.stack.astore
        if self._last_obs is None:
            self.start()
        while not stop(replay.ntimesteps, replay.nstopped):
            with torch.no_grad():
                actions = agent.select_action(self._last_obs, deterministic=deterministic)
            self._last_obs, rewards, terminated, truncated, infos = envs.step(actions)
            # the replay records what the stores hold: env-side observations, the agent's raw actions
            obs = self._last_stored_obs.copy()
            self._last_stored_obs = _stored(ostore, ostore.obs)
            nxtobs = self._last_stored_obs.copy()
            actions = _stored(astore, astore.actions)
            # envs that finished were reset inside the step: their next observation is the stored final one
            if "final_observation" in infos:
                index = infos["_final_observation"]
                nxtobs[index] = ostore.finals[index].copy()[ostore.mask[index]]
            sample = Sample(obs, actions, nxtobs, rewards, terminated, truncated, infos["step"])
            replay.add(sample.split(axis=0))
        for callback in self.callbacks:
            callback.on_rollout_end(replay)
        return replay
