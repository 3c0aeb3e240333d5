"""The controller's two real-env stacks (reference pdecontrol/mbrl/mbrl.py:259-291) over a ``KSBatchedVecEnv``, with
``Tmax`` chosen so that ``max_episode_steps = 4``: the collection stack (running observation scaling) and the evaluation
stack (the same scaling, frozen), a seeded agent and a worker per stack.  Used by tests/test_collection_phase_*.py;
``device = -1`` builds the stacks over the stepper's CPU twin."""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sac_models as sm  # noqa: E402

MAX_EPISODE_STEPS = 4
FIELDS = ("obs", "actions", "nxtobs", "rewards", "terminated", "truncated", "steps")
STAGGER = (0, 1, 2, 3, 0)
BURN_IN_SUBSTEPS = 500            # a short burn-in: the autoreset runs its burn-in path without its 200 000 sub-steps


def transforms(env, agent_stride=1):
    """The controller's transforms (mbrl.py:146-175): the running observation scaling, the frozen action scaling, sensors."""
    from pdegym.common import transforms as T
    oscaling = T.ScaleTransform(batched=True, aggregate=True, frozen=False)
    low = np.asarray(env.single_action_space.low)[np.newaxis, ...]
    high = np.asarray(env.single_action_space.high)[np.newaxis, ...]
    ascaling = T.ScaleTransform(bounds=(low, high), aggregate=True, frozen=True, batched=True).Inverse
    agent_sensor = T.BatchTransform(T.SensorTransform(stride=agent_stride))
    world_sensor = T.BatchTransform(T.SensorTransform(stride=1))
    return types.SimpleNamespace(oscaling=oscaling, ascaling=ascaling, agent_sensor=agent_sensor, world_sensor=world_sensor)


def make_stack(env, tf, frozen, obs_steps=1, act_steps=1, store_on_top=False, obs_transforms=None, action_transforms=None):
    """mbrl.py:259-272 (``frozen = False``) / :275-291 (``frozen = True``).  ``obs_transforms``: (transform, frozen) pairs
    innermost first in place of the controller's; ``action_transforms`` likewise, outermost last."""
    from pdecontrol.mbrl.worker import PDEEnvStack
    from pdecontrol.mbrl.world.wrappers import BaseWorldVecEnvWrapper
    from pdegym.common import vec_wrappers as W
    ostore = W.StoreNObsVecWrapper(env, num_steps=obs_steps)
    envs = ostore
    if obs_transforms is None:
        obs_transforms = [(tf.oscaling, frozen), (tf.world_sensor, False), None, (tf.agent_sensor, False)]
    world_wrapper = None
    for entry in obs_transforms:
        if entry is None:
            envs = world_wrapper = BaseWorldVecEnvWrapper(env=envs, surrogate=None, tstep=env.cfg_steps * env.dt)
        else:
            envs = W.TransformObsWrapper(envs, entry[0], frozen=entry[1])
    if action_transforms is None:
        action_transforms = [(tf.ascaling, True)]
    if store_on_top:
        for t, fr in action_transforms:
            envs = W.TransformActionWrapper(envs, t, frozen=fr)
        envs = astore = W.StoreNActionsVecWrapper(envs, num_steps=act_steps)
    else:
        astore = W.StoreNActionsVecWrapper(envs, num_steps=act_steps)
        envs = astore
        for t, fr in action_transforms:
            envs = W.TransformActionWrapper(envs, t, frozen=fr)
    return PDEEnvStack(envs=envs, ostore=ostore, astore=astore, world_wrapper=world_wrapper)


def make_env(E, N=64, device=-1, step_mode="fast", tmax=1.0):
    from pdegym.kuramoto.batched import KSBatchedVecEnv
    env = KSBatchedVecEnv(E, dict(L=22.0 * N / 64, N=N, Tmax=tmax), device=device, step_mode=step_mode, burn_in=False)
    env.burn_in_substeps = BURN_IN_SUBSTEPS
    return env


def build(E=5, N=64, device=-1, agent_device="cpu", agent_stride=1, obs_steps=1, hidden=256, tmax=1.0, step_mode="fast"):
    """Envs, both stacks, the agent and a worker per stack; nothing is reset yet."""
    from pdecontrol.mbrl.worker import Worker
    env, eval_env = make_env(E, N, device, step_mode, tmax), make_env(E, N, device, step_mode, tmax)
    assert tmax != 1.0 or env.max_episode_steps == MAX_EPISODE_STEPS
    tf = transforms(env, agent_stride)
    stack = make_stack(env, tf, frozen=False, obs_steps=obs_steps)
    eval_stack = make_stack(eval_env, tf, frozen=True, obs_steps=obs_steps)
    agent = sm.build(hidden=hidden, obs_dim=len(range(agent_stride // 2, N, agent_stride)), act_dim=4, seed=7, device=agent_device)
    return types.SimpleNamespace(env=env, eval_env=eval_env, transforms=tf, stack=stack, eval_stack=eval_stack, agent=agent,
                                 worker=Worker(stack), eval_worker=Worker(eval_stack))


def seed():
    torch.manual_seed(123)
    np.random.seed(321)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(99)


def prime(worker, env_seed, stagger=True):
    """The reset ``Worker.rollout`` makes on a fresh worker, then the env counters staggered so that envs truncate at
    different steps."""
    from pdecontrol.mbrl.worker import _stored
    stack = worker.stack
    worker._last_obs = stack.envs.reset(seed=env_seed)
    worker._last_stored_obs = _stored(stack.ostore, stack.ostore.obs)
    ks = stack.ostore.env
    if stagger:
        ks.timestep[:] = np.resize(np.asarray(STAGGER), ks.num_envs)


def replay_record(replay):
    """Keys in order, vindex, and every item of every field of every episode (with its type and dtype)."""
    rec = {"keys": list(replay.episodes), "vindex": dict(replay.vindex), "ntimesteps": replay.ntimesteps,
           "nstopped": replay.nstopped, "capacity": replay.capacity}
    for name in FIELDS:
        store = getattr(replay, name)
        rec[f"{name}_keys"] = list(store.keys())
        for key, items in store.items():
            rec[f"{name}_{key}"] = list(items)
    return rec


def assert_same_replay(a, b):
    ra, rb = replay_record(a), replay_record(b)
    assert sorted(ra) == sorted(rb)
    for k in ra:
        if not isinstance(ra[k], list) or k.endswith("keys"):
            assert ra[k] == rb[k], k
            continue
        assert len(ra[k]) == len(rb[k]), k
        for u, v in zip(ra[k], rb[k]):
            assert type(u) is type(v) and np.asarray(u).dtype == np.asarray(v).dtype and np.shape(u) == np.shape(v), k
            np.testing.assert_array_equal(np.asarray(u), np.asarray(v), err_msg=k)


def state_record(worker, with_stepper=True):
    """Everything ``Worker.rollout`` mutates besides the replay it returns."""
    stack = worker.stack
    ks = stack.ostore.env
    scaling = next(w.transform for w in _wrappers(stack.envs) if hasattr(w, "transform") and hasattr(w.transform, "vmin"))
    rec = {"last_obs": worker._last_obs.copy(), "last_stored_obs": worker._last_stored_obs.copy(),
           "ostore_obs": stack.ostore.obs.copy(), "ostore_mask": stack.ostore.mask.copy(),
           "ostore_finals": stack.ostore.finals.copy(), "astore_actions": stack.astore.actions.copy(),
           "astore_mask": stack.astore.mask.copy(), "vmin": scaling.vmin.clone(), "vmax": scaling.vmax.clone(),
           "timestep": ks.timestep.copy(), "mt_state": ks._rng.state.copy(), "mt_pos": ks._rng.pos.copy(),
           "numpy": np.random.get_state(), "torch_cpu": torch.get_rng_state().clone()}
    if with_stepper:
        rec["stepper"] = ks.stepper.get_state()
    if torch.cuda.is_available():
        rec["torch_cuda"] = torch.cuda.get_rng_state(0).clone()
    return rec


def _wrappers(env):
    while hasattr(env, "env"):
        yield env
        env = env.env


def assert_same_state(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        if k == "numpy":
            assert a[k][0] == b[k][0] and np.array_equal(a[k][1], b[k][1]) and a[k][2:] == b[k][2:], k
        elif isinstance(a[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (k, a[k], b[k])
        else:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


class Callback:
    def __init__(self):
        self.seen = []

    def on_rollout_end(self, replay):
        self.seen.append(replay)
