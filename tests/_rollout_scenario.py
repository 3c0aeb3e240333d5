"""Scripted imagined-rollout phase: the world of tests/_world_scenario.py (two seeded ensemble members, a replay of two
short episodes, tau = 3) under the controller's five-wrapper action stack and agent sensor (reference
pdecontrol/mbrl/mbrl.py:321-329), driven by a seeded SAC agent through ``Worker.rollout``.

Run against the reference's own Worker, wrappers, WorldVecEnv and SAC by tools/gen_rollout_golden.py
(tests/golden/rollout_golden.npz) and against this repository's by tests/test_imagination_phase_*.py.  All module objects
are passed in."""
import types

import numpy as np
import torch

NUM_ENVS, HORIZON, NUM_ROLLOUTS, TAU = 4, 3, 6, 3
FIELDS = ("obs", "actions", "nxtobs", "rewards", "terminated", "truncated", "steps")
PASSES = ("free", "limit")      # "limit": every replay step counter is max_episode_steps - 1, so the env limit cuts a round


def repo_namespace():
    """This repository's classes (the reference's come from tools/gen_rollout_golden.py)."""
    import pdegym  # noqa: F401
    from _oracle_stepper import OracleStepper
    from _sac_models import config, spaces
    from pdecontrol.architectures import KSAutoRegConvolutionalLSTM, KSAutoRegConvolutionalLSTMN
    from pdecontrol.mbrl.replay import ExperienceReplay
    from pdecontrol.mbrl.types import Sample
    from pdecontrol.mbrl.worker import PDEEnvStack, Worker
    from pdecontrol.mbrl.world.world import WorldVecEnv
    from pdecontrol.sac.sac import SAC
    from pdecontrol.surrogates.common import dataset as ds
    from pdecontrol.surrogates.surrogate import PDEEnsemble
    from pdecontrol.surrogates.training import PDETrainingModule
    from pdegym.common import transforms as T
    from pdegym.common import vec_wrappers as W
    from pdegym.kuramoto import KuramotoSivashinskyEnv
    env_cls = lambda **kw: KuramotoSivashinskyEnv(_stepper_cls=OracleStepper, **kw)   # never stepped
    return types.SimpleNamespace(Env=env_cls, T=T, W=W, Replay=ExperienceReplay, ds=ds, Sample=Sample,
                                 factory_cls=KSAutoRegConvolutionalLSTM, factory_n_cls=KSAutoRegConvolutionalLSTMN,
                                 TrainingModule=PDETrainingModule, Ensemble=PDEEnsemble, WorldVecEnv=WorldVecEnv,
                                 Worker=Worker, PDEEnvStack=PDEEnvStack, SAC=SAC, sac_config=config, sac_spaces=spaces)


def transforms(M, env, agent_stride=1):
    """The controller's transforms (pdecontrol/mbrl/mbrl.py:146-187; observation scaling frozen with fixed bounds)."""
    T = M.T
    oscaling = T.ScaleTransform(bounds=(np.full((1, 1, 1), -3.0, np.float32), np.full((1, 1, 1), 3.0, np.float32)),
                                batched=True, aggregate=True, frozen=True)
    low = np.asarray(env.action_space.low)[np.newaxis, ...]
    high = np.asarray(env.action_space.high)[np.newaxis, ...]
    ascaling = T.ScaleTransform(bounds=(low, high), aggregate=True, frozen=True, batched=True).Inverse
    forcing = T.BatchTransform(env.forcing)
    lo, hi = np.squeeze(forcing(low), axis=0), np.squeeze(forcing(high), axis=0)
    pdescaling = T.BatchTransform(T.ScaleTransform(bounds=(lo, hi), scale=(-1, 1), aggregate=True, frozen=True))
    agent_sensor = T.BatchTransform(T.SensorTransform(stride=agent_stride))
    world_sensor = T.BatchTransform(T.SensorTransform(stride=1))
    replay_to_world = T.SampleTransform([oscaling, world_sensor], [forcing, pdescaling, world_sensor])
    return types.SimpleNamespace(oscaling=oscaling, ascaling=ascaling, forcing=forcing, pdescaling=pdescaling,
                                 agent_sensor=agent_sensor, world_sensor=world_sensor, replay_to_world=replay_to_world)


def make_stack(M, world, obs_transforms, action_transforms):
    """The wrapper stack of the imagined rollouts (mbrl.py:321-329).  ``obs_transforms`` and ``action_transforms`` are
    listed innermost first; the latter as (transform, frozen)."""
    W = M.W
    ostore = W.StoreNObsVecWrapper(world, num_steps=1)
    envs = ostore
    for t in obs_transforms:
        envs = W.TransformObsWrapper(envs, t)
    for t, frozen in action_transforms:
        envs = W.TransformActionWrapper(envs, t, frozen=frozen)
    astore = W.StoreNActionsVecWrapper(envs, num_steps=1)
    return M.PDEEnvStack(envs=astore, ostore=ostore, astore=astore, world_wrapper=None)


def controller_action_transforms(t):
    return [(t.world_sensor, False), (t.pdescaling, True), (t.forcing, True), (t.ascaling, True)]


def build(M, device="cpu", limit=False, num_envs=NUM_ENVS, horizon=HORIZON, agent_stride=1, members=2, env_kwargs=None,
          world_kwargs=None):
    """World, wrapped stack and agent.  ``limit``: the second pass of the fixture.  ``env_kwargs`` (e.g. L = 88, N = 256)
    go to the env and select the any-N surrogate factory; ``world_kwargs`` as in tests/_world_scenario.py."""
    env = M.Env(**(env_kwargs or {}))
    N, tstep = env.N, env.cfg_steps * env.dt
    tf = transforms(M, env, agent_stride)
    replay_to_world = tf.replay_to_world

    # replay with two finished episodes of a smooth synthetic field
    rp = M.Replay()
    rs = np.random.RandomState(5)
    x = np.linspace(0, 2 * np.pi, N, endpoint=False)
    for ep_len in (7, 9):
        phase = rs.uniform(0, 6)
        for t in range(ep_len):
            mk = lambda tt: (np.sin(x + phase + 0.3 * tt) + 0.5 * np.cos(2 * x - 0.2 * tt)).astype(np.float32)[None, :]
            act = rs.uniform(-1, 1, (1, 4)).astype(np.float32)
            step = env.max_episode_steps - 1 if limit else t + 1
            rp.add([M.Sample(mk(t), act, mk(t + 1), np.float32(-1.0), False, t == ep_len - 1, np.int32(step))])

    modules = []
    for seed in range(members):
        torch.manual_seed(seed)
        f = M.factory_cls() if N == 64 else M.factory_n_cls()
        sur = f.surrogate(delta=tstep, dscaling=None, tau=TAU, **f.model(N=N))
        modules.append(M.TrainingModule(surrogate=sur, loss=torch.nn.MSELoss(reduction="none"), tstep=tstep, delta=tstep,
                                        tau=TAU, tbtt=10).to(device))
    ensemble = M.Ensemble(modules, num_elites=members)

    world = M.WorldVecEnv(surrogate=ensemble, observation_space=env.observation_space, action_space=env.action_space,
                          max_episode_steps=env.max_episode_steps, stransf=replay_to_world.Inverse,
                          reward_func=env.reward_func, num_envs=num_envs, horizon=horizon, tstep=tstep,
                          **{k: (v(env) if callable(v) else v) for k, v in (world_kwargs or {}).items()})
    starting = M.ds.StartingStateDataset(data=rp.data, length=TAU, stride=1, bootstrapping=False, stransf=replay_to_world)

    stack = make_stack(M, world, [tf.agent_sensor], controller_action_transforms(tf))

    torch.manual_seed(7)
    obs_space, act_space = M.sac_spaces(obs_dim=len(range(agent_stride // 2, N, agent_stride)), act_dim=4)
    agent = M.SAC(obs_space, act_space, M.sac_config(hidden=256, cuda=torch.device(device).type == "cuda"))
    return types.SimpleNamespace(env=env, world=world, starting=starting, stack=stack, agent=agent, replay=rp,
                                 ensemble=ensemble, transforms=tf)


def seed():
    torch.manual_seed(123)
    np.random.seed(321)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(99)


def stop(num_rollouts=NUM_ROLLOUTS):
    return lambda ts, eps: eps >= num_rollouts


def record(replay, tag):
    """The whole structure of an ``ExperienceReplay`` as arrays."""
    rec = {f"{tag}_keys": np.asarray(sorted(replay.episodes)), f"{tag}_ntimesteps": np.asarray(replay.ntimesteps),
           f"{tag}_nstopped": np.asarray(replay.nstopped)}
    for key in replay.episodes:
        for name in FIELDS:
            rec[f"{tag}_ep{key}_{name}"] = np.asarray(list(getattr(replay, name)[key]))
    return rec


def run(M, device="cpu", rollout=None, **build_kwargs):
    """Both passes through ``rollout(scene) -> ExperienceReplay`` (default: a fresh ``Worker``)."""
    rec = {}
    for tag in PASSES:
        s = build(M, device, limit=tag == "limit", **build_kwargs)
        s.world.setup(s.starting)
        seed()
        replay = (rollout or (lambda s: M.Worker(s.stack).rollout(s.agent, stop())))(s)
        rec.update(record(replay, tag))
    return rec


# ----------------------------------------------------------------------------------------------------------------------
# numpy twin of the forcing product of ro_act_chain (csrc/rollout.hip)
# ----------------------------------------------------------------------------------------------------------------------
def host_matmul_is_fma_chain(F, actions):
    """Whether torch's CPU matmul forms ``actions @ F`` as the fma chain in action order on this host (it does where MKL
    runs its fma sgemm; tests/conftest.py::require_fma_sgemm)."""
    got = (torch.from_numpy(actions) @ torch.from_numpy(F)).numpy()
    return np.array_equal(got, fma_chain(actions, F))


def fma32(a, b, c):
    """fp32 fma of fp32 arrays: the product is exact in fp64; the sum is rounded to odd in fp64 (TwoSum tells whether it
    was inexact), so that the final rounding to fp32 is the single rounding of the exact a * b + c."""
    p, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    s = p + c
    bp = s - p
    err = (p - (s - bp)) + (c - bp)
    bits = s.view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    toward = np.where((err > 0) == (s > 0), 1, -1)          # |s| grows when the error has s's sign
    toward = np.where(s == 0, 0, toward)
    s = np.where(fix, (bits + np.where(fix, toward, 0)).view(np.float64), s)
    return s.astype(np.float32)


def fma_chain(actions, F):
    """acc = a0 * F[0]; acc = fma(ak, F[k], acc): the forcing product of ro_act_chain, [..., A] x [A, L] -> [..., L]."""
    a = np.asarray(actions, dtype=np.float32)
    acc = (a[..., 0:1] * F[0]).astype(np.float32)
    for k in range(1, F.shape[0]):
        acc = fma32(np.broadcast_to(a[..., k:k + 1], acc.shape), np.broadcast_to(F[k], acc.shape), acc)
    return acc
