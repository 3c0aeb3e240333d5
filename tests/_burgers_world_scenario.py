"""Scripted imagined-rollout phase over the second PDE path: a ``WorldVecEnv`` over an ensemble of three seeded
``FNOAutoRegSurrogate`` members whose reward owner is a ``BurgersBatchedVecEnv`` (N = 256, 4 actuators), under the
controller's wrapper stack of tests/_rollout_scenario.py (forcing at full width, agent sensor of stride 4) and a seeded SAC
agent.  N = 256 and not 64: the fused SAC kernels take observation widths of 64, 128 and 256, so a stride-4 sensor needs 256
grid points for the agent to stay on them (as the b5_n256_stride4 case of tests/test_imagination_phase_gpu.py).  On a GPU
the env is a real one and the starting states come from a short scripted collection with it (made once per process);
without one the env carries its host attributes only (as ``_bare_env`` of tests/test_burgers_collect_host.py) and the
replay holds a smooth synthetic field."""
import math
import types

import numpy as np
import torch

import _rollout_scenario as rsc

NUM_ENVS, HORIZON, NUM_ROLLOUTS, TAU, N, AGENT_STRIDE, MEMBERS = 5, 3, 10, 3, 256, 4, 3     # 2 rounds of 5 envs
CFG = dict(L=2 * math.pi, N=N, cfg_steps=2, dt=1e-3, nu=0.01, Tmax=0.1, sigma=0.15)          # 50 steps per episode
FIELDS = rsc.FIELDS
seed, stop = rsc.seed, rsc.stop
_collected = None


def bare_env(E=NUM_ENVS, scenario=None, **over):
    """A ``BurgersBatchedVecEnv`` without its device side (the constructor allocates on the GPU): the spaces and the host
    attributes the world, the wrappers and the recognition read.  ``scenario`` replaces the class's ``scenario``."""
    from pdegym._gym import gym
    from pdegym.burgers.burgers import BurgersBatchedVecEnv
    from pdegym.common.transforms import FuncTransform, GaussianForcing
    cfg = {**CFG, **over}
    cls = BurgersBatchedVecEnv if scenario is None else type("ScenarioBurgersEnv", (BurgersBatchedVecEnv,),
                                                             {"scenario": property(lambda self: scenario)})
    env = cls.__new__(cls)
    n = cfg["N"]
    gym.vector.VectorEnv.__init__(env, E, gym.spaces.Box(-np.inf, np.inf, shape=(1, n), dtype=np.float32),
                                  gym.spaces.Box(-1.0, 1.0, shape=(1, 4), dtype=np.float32))
    for k, v in cfg.items():
        setattr(env, k, v)
    env.dx = env.L / n
    env.x = np.linspace(0.0, env.L - env.L / n, n, dtype=np.float32)
    env.max_episode_steps = math.ceil(env.Tmax / (env.dt * env.cfg_steps))
    env.forcing = GaussianForcing(env.x, env.Xi, env.sigma, env.L, n)
    env.reward_func = FuncTransform(lambda obs, *a, **k: (-1.0) * (1 / env.N) * torch.norm(obs) ** 2)
    env.timestep = np.zeros(E, dtype=np.int64)
    return env


def real_env(E=NUM_ENVS):
    from pdegym.burgers.burgers import BurgersBatchedVecEnv
    return BurgersBatchedVecEnv(E, device=0, **CFG)


def _synthetic_samples(env, limit):
    rs = np.random.RandomState(5)
    x = np.linspace(0, 2 * np.pi, env.N, endpoint=False)
    out = []
    for ep_len in (7, 9):
        phase = rs.uniform(0, 6)
        for t in range(ep_len):
            mk = lambda tt: (np.sin(x + phase + 0.3 * tt) + 0.5 * np.cos(2 * x - 0.2 * tt)).astype(np.float32)[None, :]
            act = rs.uniform(-1, 1, (1, 4)).astype(np.float32)
            out.append((mk(t), act, mk(t + 1), np.float32(-1.0), False, t == ep_len - 1, np.int32(t + 1)))
    return out


def _collected_samples(env):
    """Seven scripted steps of two envs of a real ``BurgersBatchedVecEnv``: two episodes of the world's replay."""
    global _collected
    if _collected is None:
        rs = np.random.RandomState(5)
        obs = env.reset(seed=11)
        eps = [[], []]
        for t in range(7):
            act = rs.uniform(-1, 1, (env.num_envs, 1, 4)).astype(np.float32)
            env.step_async(act)
            nxt, rew, _, _, info = env.step_wait()
            for b in range(2):
                eps[b].append((obs[b].copy(), act[b].copy(), nxt[b].copy(), np.float32(rew[b]), False, t == 6,
                               np.int32(info["step"][b])))
            obs = nxt
        _collected = eps[0] + eps[1]
    return _collected


def repo_namespace():
    from _sac_models import config, spaces
    from pdecontrol.architectures.fno import BurgersFNO
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
    return types.SimpleNamespace(T=T, W=W, Replay=ExperienceReplay, ds=ds, Sample=Sample, factory_cls=BurgersFNO,
                                 TrainingModule=PDETrainingModule, Ensemble=PDEEnsemble, WorldVecEnv=WorldVecEnv,
                                 Worker=Worker, PDEEnvStack=PDEEnvStack, SAC=SAC, sac_config=config, sac_spaces=spaces)


def fno_module(M, tstep, seed_, device, **model_kwargs):
    torch.manual_seed(seed_)
    f = M.factory_cls()
    sur = f.surrogate(delta=tstep, dscaling=None, tau=TAU, **f.model(**model_kwargs))
    return M.TrainingModule(surrogate=sur, loss=torch.nn.MSELoss(reduction="none"), tstep=tstep, delta=tstep, tau=TAU,
                            tbtt=10).to(device)


def build(M, device="cpu", env=None, num_envs=NUM_ENVS, horizon=HORIZON, modules=None, members=MEMBERS):
    """World, wrapped stack and agent.  ``env``: the reward owner (default: a real env on a GPU, a bare one otherwise);
    ``modules``: the ensemble's training modules (default: ``members`` seeded FNOs of the kernels' geometry)."""
    device = torch.device(device)
    if env is None:
        env = real_env(num_envs) if device.type == "cuda" else bare_env(num_envs)
    tstep = env.cfg_steps * env.dt
    # the transforms read the single env's action box and forcing
    tf = rsc.transforms(M, types.SimpleNamespace(action_space=env.single_action_space, forcing=env.forcing), AGENT_STRIDE)
    samples = _collected_samples(env) if hasattr(env, "stepper") else _synthetic_samples(env, False)
    rp = M.Replay()
    for s in samples:
        rp.add([M.Sample(*s)])
    if modules is None:
        modules = [fno_module(M, tstep, s, device) for s in range(members)]
    ensemble = M.Ensemble(modules, num_elites=len(modules))
    world = M.WorldVecEnv(surrogate=ensemble, observation_space=env.single_observation_space,
                          action_space=env.single_action_space, max_episode_steps=env.max_episode_steps,
                          stransf=tf.replay_to_world.Inverse, reward_func=env.reward_func, num_envs=num_envs, horizon=horizon,
                          tstep=tstep, batched_reward_func=env.batched_reward_func)
    starting = M.ds.StartingStateDataset(data=rp.data, length=TAU, stride=1, bootstrapping=False, stransf=tf.replay_to_world)
    stack = rsc.make_stack(M, world, [tf.agent_sensor], rsc.controller_action_transforms(tf))
    torch.manual_seed(7)
    obs_space, act_space = M.sac_spaces(obs_dim=len(range(AGENT_STRIDE // 2, env.N, AGENT_STRIDE)), act_dim=4)
    agent = M.SAC(obs_space, act_space, M.sac_config(hidden=256, cuda=device.type == "cuda"))
    return types.SimpleNamespace(env=env, world=world, starting=starting, stack=stack, agent=agent, replay=rp,
                                 ensemble=ensemble, transforms=tf)
