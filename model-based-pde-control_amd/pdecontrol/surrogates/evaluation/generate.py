"""The dataset of the offline surrogate evaluation (reference ``pdecontrol/surrogates/evaluation/generate.py``): complete
episodes of a random policy, saved as a ``TensorDataset`` of seven tensors,

    obs, actions, nxt   [E, T, 1, N], [E, T, 1, A], [E, T, 1, N]   float32
    rewards             [E, T]                                     float32
    terminated, truncated [E, T]                                   bool
    steps               [E, T]                                     long, arange(T) in every row

    python -m pdecontrol.surrogates.evaluation.generate --env KuramotoSivashinskyEnv-v0 --output KSattractor.pl \\
        --episodes 100 --device cuda --seed 0

The reference steps one env through ``episodes`` episodes.  Here the episodes are the envs of one ``KSBatchedVecEnv``
(``WAVE_EPISODES`` at a time), stepped from a fresh reset to their truncation by a ``RandomAgent`` through
``collect(..., sink=DeviceExperienceReplay)``: on a GPU that is the scripted tier of the collection phase (DESIGN.md 4.19:
``co_act_span`` -> T x ``ks_step_device`` -> ``ks_record_device``), so an episode's rows never leave HBM, and the
tensors are read from the sink's slabs through its row map.  The step at which the envs truncate is a host step of the
stack, so ``nxt`` of an episode's last step is the final observation, not the observation of the autoreset.  On the CPU
the same call runs the per-step loop over the stepper's CPU twin.

``--env BurgersEnv-v0`` (``pdegym.burgers.ENV_ID``) takes the same route over a ``BurgersBatchedVecEnv`` (``co_act_span`` ->
``bg_step_span`` -> ``bg_record``), on a GPU only: the Burgers stepper has no CPU twin and ``--device cpu`` is refused.
"""
import argparse
import json
import sys

import torch
from torch.utils.data import TensorDataset

#: envs of one ``KSBatchedVecEnv``: more episodes run in waves of this many.  A wave's slabs hold 2 N + A + 4 words per
#: step, 0.2 GB at N = 64 and 400 steps; the cap bounds that, not the stepper, which takes any batch.
WAVE_EPISODES = 1024


def _stack(envs):
    """The bare stack ``Worker`` and ``collect`` need: both stores, no transform (the dataset holds env-side values)."""
    from pdecontrol.mbrl.worker import PDEEnvStack
    from pdegym.common.vec_wrappers import StoreNActionsVecWrapper, StoreNObsVecWrapper
    ostore = StoreNObsVecWrapper(envs, num_steps=1)
    astore = StoreNActionsVecWrapper(ostore, num_steps=1)
    return PDEEnvStack(envs=astore, ostore=ostore, astore=astore, world_wrapper=None)


def _wave(envs, device, seed, tier):
    """One complete episode of every env of ``envs`` as the seven tensors, and the tier that ran."""
    from pdecontrol.mbrl.collection_phase import collect
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    from pdecontrol.mbrl.utils import RandomAgent
    from pdecontrol.mbrl.worker import Worker
    E, T = int(envs.num_envs), int(envs.max_episode_steps)
    stack = _stack(envs)
    worker = Worker(stack)
    if seed is not None:
        stack.envs.action_space.seed(int(seed))
    worker.start(**({} if seed is None else {"seed": int(seed)}))
    agent = RandomAgent(stack.envs.action_space)
    stop = lambda timesteps, _: timesteps >= E * T
    sink = DeviceExperienceReplay(device=device)
    if tier == "loop":
        rollout = worker.rollout(agent, stop)
        ran = "loop"
    else:
        rollout = collect(worker, agent, stop, sink=sink)
        ran = rollout.tier
    sink.extend(rollout)
    if sink.nepisodes != E or sink.ntimesteps != E * T:
        raise RuntimeError(f"{E} envs of {T} steps left {sink.nepisodes} episodes of {sink.ntimesteps} steps")
    obs, actions, nxt, rewards, terminated, truncated, _ = sink.window_store().tensors      # episodes in key order
    fold = lambda t: t.reshape((E, T) + tuple(t.shape[1:]))
    steps = torch.arange(T, dtype=torch.long, device=obs.device).repeat(E, 1)
    return (fold(obs), fold(actions), fold(nxt), fold(rewards), fold(terminated).to(torch.bool),
            fold(truncated).to(torch.bool), steps), ran


def generate_dataset(env_id, episodes, config=None, device=None, seed=None, tier=None, make_envs=None):
    """``episodes`` complete episodes of a uniform random policy on ``env_id`` as a ``TensorDataset`` (module docstring);
    its ``tier`` attribute names the collection tier that ran ("kernel" or "loop").

    ``env_id``: the KS env's id or ``pdegym.burgers.ENV_ID``; ``config``: the env's config dict; ``device``: None / "cpu"
    for the stepper's CPU twin (KS only), "cuda" or "cuda:i" for that GPU, where the tensors then stay; ``seed``: wave w seeds its envs' streams ``seed + first episode of w + i`` and its
    action space ``seed + first episode of w``; ``tier="loop"`` forces the per-step loop.  ``make_envs(n)`` replaces the
    vector env (tests: short episodes and a short burn-in)."""
    from pdegym import burgers
    from pdegym.kuramoto import ENV_ID, make_vec
    if tier not in (None, "loop"):
        raise ValueError(f"tier is {tier!r}: None or 'loop'")
    if env_id not in (ENV_ID, burgers.ENV_ID) and make_envs is None:
        raise ValueError(f"{env_id!r}: the offline evaluation is built for {ENV_ID}")
    if int(episodes) < 1:
        raise ValueError(f"{episodes} episodes (at least 1)")
    device = torch.empty(0, device="cpu" if device is None else device).device
    ordinal = device.index if device.type == "cuda" else -1
    if env_id == burgers.ENV_ID and make_envs is None:
        # the Burgers stepper has no CPU twin: its vector env lives on a GPU
        if device.type != "cuda":
            raise ValueError(f"{burgers.ENV_ID}: device={device.type!r} is refused, the Burgers stepper runs on a GPU only "
                             f"(device='cuda' or 'cuda:i')")
        ordinal = torch.cuda.current_device() if device.index is None else device.index
        make_vec = burgers.make_vec
    if make_envs is None:
        make_envs = lambda n: make_vec(n, config=dict(config or {}), device=ordinal)
    waves, tiers = [], set()
    for first in range(0, int(episodes), WAVE_EPISODES):
        envs = make_envs(min(WAVE_EPISODES, int(episodes) - first))
        fields, ran = _wave(envs, device, None if seed is None else int(seed) + first, tier)
        waves.append(fields)
        tiers.add(ran)
    data = TensorDataset(*(torch.cat(parts) for parts in zip(*waves)))
    data.tier = "kernel" if tiers == {"kernel"} else "loop"
    return data


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--env", type=str)
    parser.add_argument("--output", type=str)
    parser.add_argument("--episodes", type=int, default=100)
    parser.add_argument("--config", type=str, default="{}")
    parser.add_argument("--device", type=str, default="cpu")
    parser.add_argument("--seed", type=int, default=None)
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    data = generate_dataset(args.env, args.episodes, config=json.loads(args.config), device=args.device, seed=args.seed)
    torch.save(TensorDataset(*(t.cpu() for t in data.tensors)), args.output)
    return 0


if __name__ == "__main__":
    sys.exit(main())
