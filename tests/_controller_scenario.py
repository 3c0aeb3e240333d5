"""A toy run of ``PDEModelBasedController`` for tests/test_controller_host.py and tests/test_controller_gpu.py: the
envs of tests/_collect_scenario.py (``Tmax = 1``: four steps per episode, a short burn-in) injected through ``make_env`` /
``make_envs``, the N = 64 ConvLSTM factory with two members, tau = 2 and a curriculum of one extrapolated step, so that a
four-step episode holds two training windows."""
import json
import os
import sys
from argparse import Namespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _collect_scenario as sc  # noqa: E402

ENV_ID = "KuramotoSivashinskyEnv-v0"
TAU = 2


def toy_args(**over):
    """The reference's flags (script.py) at toy sizes."""
    args = dict(
        agent_eval_freq=1, num_eval_episodes=3, status_report_freq=5, logging_freq=10, total_timesteps=18, cuda=False, seed=0,
        env_id=ENV_ID, cpus=3, gamma=0.99, capacity=1000000, rollout_length=1, learning_starts=12,
        policy_train_steps_per_sample=1, model_buffer_store_iterations=3, model_rollouts_per_sample=2,
        model_rollouts_batch_size=3, model_buffer_max_capacity=1000000, val_split_ratio=0.34,
        rollout_length_schedule=json.dumps(dict(scheduler="ConstantLengthScheduler", length=2)), surrogate_train_freq=3,
        loss="MSELoss", num_dynamics_models=2, num_elite_models=2, policy="Gaussian", policy_batch_size=8, tau=0.005,
        target_entropy=-3.0, lr=3e-4, alpha=0.2, target_update_interval=1, hidden_size=256, automatic_entropy_tuning=False,
        surrogate_eval_horizon=1, name=None)
    args.update(over)
    return Namespace(**args)


def toy_config(max_steps=2, patience=1000, batch_size=4):
    phase = dict(patience=patience, batch_size=batch_size, tbtt=10, lr=1e-3)
    steps = dict(max_steps=max_steps, min_steps=0)
    return Namespace(factory="KSAutoRegConvolutionalLSTM", model={}, surrogate={},
                     training=dict(tau=TAU, initial=dict(phase), iterations=dict(phase)),
                     curriculum=dict(scheduler="StepScheduler", steptype="epoch", steps=[], values=[1]),
                     trainer=dict(initial=dict(steps), iterations=dict(steps)), loss="MSELoss")


def seed():
    torch.manual_seed(123)
    np.random.seed(321)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(99)


def build(log_dir, args=None, config=None, N=64, device=-1, **kwargs):
    """The controller over injected envs (``device``: the stepper's; -1 is its CPU twin).  Seeds first: the members and
    the agent are initialised from torch's generator."""
    from pdecontrol import architectures
    from pdecontrol.mbrl.mbrl import PDEModelBasedController, RunLog
    args = toy_args() if args is None else args
    config = toy_config() if config is None else config
    seed()
    factory = getattr(architectures, config.factory)()
    return PDEModelBasedController(
        ENV_ID, factory, config, args, log=RunLog(log_dir), make_env=lambda: sc.make_env(1, N, -1).proto,
        make_envs=lambda n: sc.make_env(n, N, device), **kwargs)


def seed_spaces(controller):
    """What neither torch's nor numpy's seed reaches: the action space's own generator (the warm-up's draws) and the
    envs' MT streams (the workers' first reset, made here with a seed as ``Worker.rollout`` makes it without one)."""
    controller.envs.action_space.seed(7)
    sc.prime(controller.worker, 11, stagger=False)
    sc.prime(controller.eval_worker, 5, stagger=False)


def generators(controller):
    space = controller.envs.action_space
    rng = getattr(space, "_rng", None)
    rng = space.np_random if rng is None else rng
    ks = controller.stack.ostore.env
    rec = {"numpy": np.random.get_state(), "torch_cpu": torch.get_rng_state().clone(), "space": rng.bit_generator.state,
           "mt_state": ks._rng.state.copy(), "mt_pos": ks._rng.pos.copy()}
    if torch.cuda.is_available():
        rec["torch_cuda"] = torch.cuda.get_rng_state(0).clone()
    return rec


def same_generators(a, b, what=""):
    assert sorted(a) == sorted(b)
    for k in a:
        if k == "numpy":
            assert a[k][0] == b[k][0] and np.array_equal(a[k][1], b[k][1]) and a[k][2:] == b[k][2:], (what, k)
        elif k == "space":
            assert a[k] == b[k], (what, k)
        elif isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k]), (what, k)
        else:
            assert np.array_equal(a[k], b[k]), (what, k)


def slabs(replay):
    """The live rows of a ``DeviceExperienceReplay`` in packed order, as numpy, and its metadata."""
    store = replay.window_store()
    rows = [t.cpu().numpy() for t in store.gather(torch.arange(store.total, device=replay.device))]
    meta = dict(episodes=list(replay.episodes), vindex=dict(replay.vindex), ntimesteps=replay.ntimesteps,
                stopped=list(replay.stopped), starts=dict(store.starts))
    return rows, meta
