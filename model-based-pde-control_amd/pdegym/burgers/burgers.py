"""Viscous-Burgers control environments on the MI355X HIP stepper (BASELINE configs[4]).

There is nothing to mirror: the reference imports ``pdegym.burgers`` (pdegym/__init__.py:2) but ships no such module.
What the reference does fix is the discretisation -- ``BurgersPhyPDELoss`` (pdecontrol/surrogates/phyloss/phyloss.py:36-86):
``u_t = nu u_xx - u u_x`` with the 2nd-order central gradient, the 4th-order central Laplacian, periodic, stepped by
the explicit midpoint rule -- and that arithmetic is what ``libburgers_hip.so`` implements (pinned to the reference
class's own outputs in tests/test_burgers.py).  Everything around the step follows the Kuramoto-Sivashinsky env of the
same package: four Gaussian actuators (``GaussianForcing``), ``cfg_steps`` sub-steps per ``step`` with the forcing held,
a reward averaged over the sub-steps (taken before each update), truncation at ``Tmax``, fp32 observations ``[1, N]``.
**Parity unpinned** for all of that (no reference to compare with).

Two objectives (``objective=``), as the KS env has them: ``"l2control"``, the reward ``-(1/N) |u|^2``, and
``"dissipation"``, the energy budget of the forced equation ``d/dt 1/2 <u^2> = -nu <u_x^2> + <u phi>`` turned into the
reward ``-(nu <u_x^2> + <u phi>)``: shrink the field at low dissipation and low actuation power.  The name selects it (no
truthiness rule: there is no reference to mirror).  The step's reward comes from the stepper kernel itself
(include/burgers/objective.h), the reward of given rows from ``bg_reward_rows`` on the device and from
``dissipation_rows`` on the host.

``BurgersBatchedVecEnv`` is the vector env (one HBM-resident fp32 batch, one launch per step, gym autoreset
semantics); ``BurgersEnv`` is the single-env view of it that ``gym.make`` returns.
"""
import math
from typing import Optional

import numpy as np
import torch

from hipbind import ptr as _ptr
from pdegym._gym import gym
from pdegym.burgers import _hip
from pdegym.common.transforms import FuncTransform, GaussianForcing


OBJECTIVES = ("l2control", "dissipation")


def _checked_objective(objective):
    if objective not in OBJECTIVES:
        raise ValueError(f"objective must be one of {OBJECTIVES}, not {objective!r}")
    return objective


def dissipation_rows(u, phi, dx, nu):
    """The dissipation reward of fp32 rows ``u`` [M, N] under the fp32 forcing field ``phi`` [M, N], fp64 [M]: the fp64
    spelling of ``bg_reward_rows`` with every row summed in index order, the bits of ``bg_reward_rows_host``."""
    u = np.asarray(u, dtype=np.float32).astype(np.float64)
    p = np.asarray(phi, dtype=np.float32).astype(np.float64)
    n = u.shape[1]
    ux = (np.roll(u, -1, axis=1) - np.roll(u, 1, axis=1)) / (2.0 * dx)
    # cumsum adds in index order (from 0.0, as the kernel's accumulator starts), where sum() adds pairwise
    in_order = lambda t: np.cumsum(np.concatenate((np.zeros((t.shape[0], 1)), t), axis=1), axis=1)[:, -1]
    return (-1.0) * (float(np.float32(nu)) * (in_order(ux * ux) / n) + in_order(u * p) / n)


def _stream(dev):
    return _hip.ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(dev.index if dev.index is not None else 0))


class BurgersStepper:
    """The stepper face of a ``BurgersBatchedVecEnv`` as the collection phase talks to it (what it uses of
    ``kspde.KSStepper``): raw device pointers (ints, 0 = NULL), every launch asynchronous on torch's current stream of the
    env's device, on the env's live state ``env.u`` and forcing matrix."""

    def __init__(self, env):
        self._env, self._lib = env, env._lib
        self.device, self.num_envs, self.N, self.n_act = env.device.index, env.num_envs, env.N, len(env.Xi)

    def _step_args(self):
        env = self._env
        return _stream(env.device), _ptr(env.u), _ptr(env._F)

    def step_device(self, d_actions=0, n_substeps=50, d_obs=0, d_ssq=0, d_status=0):
        """One ``bg_step`` launch (``bg_step_objective`` under the dissipation objective, whose sum ``d_ssq`` then
        receives): ``d_actions`` [E, A] (0: no forcing), ``d_obs`` [E, N], ``d_ssq`` fp64 [E], ``d_status`` [E]."""
        env, vp = self._env, _void_p
        stream, u, F = self._step_args()
        if env.objective != "l2control":
            _hip.check_objective(self._lib.bg_step_objective(
                stream, u, vp(d_actions), F, self.n_act, self.num_envs, self.N, env.dx, env.dt, env.nu, int(n_substeps),
                vp(d_obs), vp(d_ssq), vp(d_status), _hip.OBJECTIVES[env.objective]))
            return
        _hip.check(self._lib.bg_step(stream, u, vp(d_actions), F, self.n_act, self.num_envs, self.N, env.dx, env.dt, env.nu,
                                     int(n_substeps), vp(d_obs), vp(d_ssq), vp(d_status)))

    def step_span(self, d_actions, T, n_substeps, d_traj, d_ssq=0, d_status=0):
        """``T`` steps in one ``bg_step_span`` launch: ``d_actions`` [T, E, A], ``d_traj`` [T + 1, E, N] (slots 1 ... T are
        written), ``d_ssq`` fp64 [T, E], ``d_status`` [T, E].  Under the dissipation objective: ``bg_step_span_objective``."""
        env, vp = self._env, _void_p
        stream, u, F = self._step_args()
        if env.objective != "l2control":
            _hip.check_objective(self._lib.bg_step_span_objective(
                stream, u, vp(d_actions), F, self.n_act, self.num_envs, self.N, int(T), env.dx, env.dt, env.nu,
                int(n_substeps), vp(d_traj), vp(d_ssq), vp(d_status), _hip.OBJECTIVES[env.objective]))
            return
        _hip.check(self._lib.bg_step_span(stream, u, vp(d_actions), F, self.n_act, self.num_envs, self.N, int(T), env.dx,
                                          env.dt, env.nu, int(n_substeps), vp(d_traj), vp(d_ssq), vp(d_status)))

    def record_device(self, d_traj, d_actions, A, d_ssq, d_steps, T, n_substeps, d_dst, dst_host, slabs):
        """The ``T * num_envs`` transitions of ``T`` steps without a truncation into replay rows; see ``bg_record``.
        ``dst_host`` a C-contiguous int64 array [T, num_envs]; ``slabs`` a ``hipbind.Slabs`` (``_hip.Slabs``)."""
        vp = _void_p
        if dst_host is not None:
            assert dst_host.dtype == np.int64 and dst_host.flags["C_CONTIGUOUS"] and dst_host.size == int(T) * self.num_envs, \
                (dst_host.dtype, dst_host.shape, T, self.num_envs)
        _hip.check(self._lib.bg_record(_stream(self._env.device), vp(d_traj), vp(d_actions), self.num_envs, self.N, int(A),
                                       vp(d_ssq), vp(d_steps), int(T), int(n_substeps), vp(d_dst),
                                       None if dst_host is None else dst_host.ctypes.data_as(_hip.ctypes.c_void_p),
                                       None if slabs is None else _hip.ctypes.byref(slabs)))


def _void_p(x):
    return _hip.ctypes.c_void_p(int(x)) if x else None


class BurgersBatchedVecEnv(gym.vector.VectorEnv):
    Xi = [0, 0.25, 0.5, 0.75]
    objective = "l2control"

    def __init__(self, num_envs: int, L: float = 2 * math.pi, N: int = 512, cfg_steps: int = 50, dt: float = 1e-3,
                 nu: float = 0.01, Tmax: float = 10.0, sigma: float = 0.15, ic_modes: int = 4, device: int = 0,
                 objective: str = "l2control"):
        self.objective = _checked_objective(objective)
        self.L, self.N, self.cfg_steps, self.dt, self.nu, self.Tmax, self.sigma = L, N, cfg_steps, dt, nu, Tmax, sigma
        self.ic_modes = ic_modes
        self.dx = L / N
        self.x = np.linspace(0.0, L - L / N, N, dtype=np.float32)
        self.max_episode_steps = math.ceil(Tmax / (dt * cfg_steps))
        self.forcing = GaussianForcing(self.x, self.Xi, sigma, L, N)
        self.reward_func = self._reward_transform()
        obs_space = gym.spaces.Box(-np.inf, np.inf, shape=(1, N), dtype=np.float32)
        act_space = gym.spaces.Box(-1.0, 1.0, shape=(1, len(self.Xi)), dtype=np.float32)
        super().__init__(num_envs, obs_space, act_space)
        self.device = torch.device("cuda", device)
        self._lib = _hip.load()
        self.u = torch.zeros((num_envs, N), dtype=torch.float32, device=self.device)
        self._F = self.forcing.forcing.to(self.device).contiguous()
        self._ssq = torch.zeros(num_envs, dtype=torch.float64, device=self.device)
        self._status = torch.zeros(num_envs, dtype=torch.int32, device=self.device)
        self.timestep = np.zeros(num_envs, dtype=np.int64)
        self._rngs = [np.random.RandomState() for _ in range(num_envs)]
        self._actions = None
        self.stepper = BurgersStepper(self)

    @property
    def scenario(self):
        return {"cfg_steps": self.cfg_steps, "L": self.L, "N": self.N, "dx": self.dx, "Tmax": self.Tmax, "dt": self.dt,
                "nu": self.nu, "Xi": self.Xi, "objective": self.objective}

    # -- rewards of given rows ----------------------------------------------------------------------------------
    def _reward_transform(self):
        """``reward_func`` of the env's objective: ``reward_func(obs, phi)`` of one row, a torch scalar."""
        if self.objective == "l2control":
            return FuncTransform(lambda obs, *a, **k: (-1.0) * (1 / self.N) * torch.norm(obs) ** 2)
        return FuncTransform(self._dissipation)

    def _forcing_field(self, phi):
        """phi as a forcing field: actions ``[..., n_act]`` go through ``forcing`` (fp32 ``[..., N]``); the rule of
        ``KuramotoSivashinskyEnv._forcing_field``."""
        if phi.shape[-1] == len(self.Xi) and phi.shape[-1] != self.N:
            return self.forcing(phi)
        return phi

    def _dissipation(self, obs, phi=None, *args, **kwargs):
        if phi is None:
            raise ValueError("the dissipation reward needs the forcing (phi or actions)")
        as_np = lambda v: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        u, p = as_np(obs).reshape(1, self.N), np.asarray(self._forcing_field(as_np(phi))).reshape(1, self.N)
        return torch.as_tensor(np.float32(dissipation_rows(u, p, self.dx, self.nu)[0]))

    def _batched_dissipation(self, obs, phi):
        """``_dissipation`` of every row of ``obs [B, ..., N]`` in the input's dtype; ``phi`` is ``[B, ..., N]`` or actions
        ``[B, ..., n_act]``.  CUDA tensors by ``bg_reward_rows`` on torch's current stream (actions through the kernel's
        own forcing chain), numpy and CPU tensors by ``dissipation_rows``."""
        if phi is None:
            raise ValueError("the dissipation reward needs the forcing (phi or actions)")
        b = obs.shape[0]
        if isinstance(obs, torch.Tensor) and obs.is_cuda:
            u = obs.reshape(b, self.N).to(torch.float32).contiguous()
            p = torch.as_tensor(phi, device=obs.device).reshape(b, -1).to(torch.float32).contiguous()
            out = torch.empty(b, dtype=torch.float64, device=obs.device)
            if p.shape[1] == len(self.Xi) and p.shape[1] != self.N:
                field, actions, F = None, p, self._F if self._F.device == obs.device else self._F.to(obs.device)
            else:
                field, actions, F = p.reshape(b, self.N), None, None
            _hip.check_objective(self._lib.bg_reward_rows(_stream(obs.device), _ptr(u), _ptr(field), _ptr(actions), _ptr(F), b,
                                                          self.N, len(self.Xi), self.dx, self.nu, _ptr(out)))
            return out.to(obs.dtype)
        as_np = lambda v: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        u = as_np(obs).reshape(b, self.N)
        p = np.asarray(self._forcing_field(as_np(phi))).reshape(b, self.N)
        rew = dissipation_rows(u, p, self.dx, self.nu)
        if isinstance(obs, torch.Tensor):
            return torch.as_tensor(rew).to(obs.dtype)
        return rew.astype(obs.dtype)

    def batched_reward_func(self, obs, phi=None):
        """``reward_func`` for a whole batch ``[B, ..., N]`` at once (numpy or torch, host or device): the reward of every
        row, in the input's dtype.  Dissipation: ``phi`` is ``[B, ..., N]`` or actions ``[B, ..., n_act]``."""
        if self.objective != "l2control":
            return self._batched_dissipation(obs, phi)
        flat = obs.reshape(obs.shape[0], -1)
        if isinstance(obs, np.ndarray):
            return ((-1.0) * (1 / self.N) * np.linalg.norm(flat, axis=1) ** 2).astype(obs.dtype)
        return (-1.0) * (1 / self.N) * torch.linalg.vector_norm(flat, dim=1) ** 2

    # -- initial conditions: smooth random Fourier series (amplitude O(1)), per-env generator -----------------------
    def _initial(self, ids):
        rows = []
        for i in ids:
            rs = self._rngs[i]
            amp = rs.uniform(-1.0, 1.0, self.ic_modes) / np.arange(1, self.ic_modes + 1)
            ph = rs.uniform(0.0, 2 * np.pi, self.ic_modes)
            k = np.arange(1, self.ic_modes + 1)[:, None] * (2 * np.pi / self.L)
            rows.append((amp[:, None] * np.sin(k * self.x[None, :].astype(np.float64) + ph[:, None])).sum(0))
        return np.asarray(rows, dtype=np.float32)

    def _fresh_rows(self, ids):
        ids = np.asarray(ids, dtype=np.int64)
        u0 = torch.from_numpy(self._initial(ids)).to(self.device)
        self.u[torch.from_numpy(ids).to(self.device)] = u0
        self.timestep[ids] = 0
        return u0.cpu().numpy()

    # -- device-resident stepping -------------------------------------------------------------------------------
    def step_torch(self, actions: Optional[torch.Tensor], n_substeps: Optional[int] = None):
        """One env.step of the whole batch on torch's current stream: ``actions`` CUDA fp32 [E, 4] (or [E, 1, 4]) or
        None (no forcing).  Returns (state [E, N] fp32 -- the live buffer --, rewards [E] fp64); no host sync."""
        n = self.cfg_steps if n_substeps is None else int(n_substeps)
        a = None if actions is None else actions.reshape(self.num_envs, -1).contiguous()
        if self.objective != "l2control":
            self.stepper.step_device(0 if a is None else a.data_ptr(), n, 0, self._ssq.data_ptr(), self._status.data_ptr())
            return self.u, self._ssq * self.reward_scale(n)
        _hip.check(self._lib.bg_step(_stream(self.device), _ptr(self.u), _ptr(a), _ptr(self._F), len(self.Xi), self.num_envs,
                                     self.N, self.dx, self.dt, self.nu, n, None, _ptr(self._ssq), _ptr(self._status)))
        return self.u, self._ssq * self.reward_scale(n)

    def reward_scale(self, n_substeps: Optional[int] = None):
        """The fp64 factor ``c`` of a step's reward ``ssq * c``: minus the mean over the grid, averaged over the sub-steps
        (of the squares under l2control, of ``nu u_x^2 + u phi`` under dissipation: the stepper's sum follows the objective)."""
        n = self.cfg_steps if n_substeps is None else int(n_substeps)
        return -(1.0 / self.N) / max(n, 1)

    def rewards_of(self, ssq):
        """The rewards of steps of ``cfg_steps`` sub-steps from their fp64 sums ``ssq`` on the host (any shape)."""
        return ssq * self.reward_scale()

    def bind_stream(self, stream):
        """Nothing to bind: every launch takes torch's current stream by itself, and ``step_device`` / ``step_span`` pick
        the entry of the env's objective on every call."""

    def _raise_on(self, status):
        """``status`` [E] of one step: the ``FloatingPointError`` of ``step_wait`` when any env's state is non-finite."""
        if np.any(status):
            raise FloatingPointError(f"non-finite Burgers state in envs {np.nonzero(status)[0].tolist()}")

    def residual(self, u, phi=None):
        """nu u_xx - u u_x (+ phi) of fp32 rows [M, N] on the device (test hook of the kernel's stencils)."""
        u = torch.as_tensor(u, dtype=torch.float32, device=self.device).contiguous()
        phi_t = None if phi is None else torch.as_tensor(phi, dtype=torch.float32, device=self.device).contiguous()
        out = torch.empty_like(u)
        _hip.check(self._lib.bg_residual(_stream(self.device), _ptr(u), _ptr(phi_t), u.shape[0], u.shape[1], self.dx, self.nu,
                                         _ptr(out)))
        return out

    def derivatives(self, u):
        """(u_x, u_xx) of fp32 rows [M, N] on the device, fp64 device tensors [M, N]: ``bg_derivatives``, the stencils of
        the stepper taken in fp64 from the widened values."""
        u = torch.as_tensor(u, dtype=torch.float32, device=self.device).contiguous()
        ux, uxx = (torch.empty(u.shape, dtype=torch.float64, device=self.device) for _ in range(2))
        _hip.check_eval(self._lib.bg_derivatives(_stream(self.device), _ptr(u), u.shape[0], u.shape[1], self.dx, _ptr(ux),
                                                 _ptr(uxx)))
        return ux, uxx

    def rhs(self, u, phi=None):
        """``(residual, (u_x, u_xx))`` of numpy or tensor rows ``[..., N]``, as ``KuramotoSivashinskyEnv.rhs`` hands them to
        ``test_step``'s host lines: numpy arrays of the input's shape, the residual fp32 (``bg_residual``), the
        derivatives fp64 (``bg_derivatives``)."""
        host = lambda v: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        rows = np.ascontiguousarray(host(u), dtype=np.float32)
        shape = rows.shape
        if not shape or shape[-1] != self.N:
            raise ValueError(f"rhs takes rows of {self.N} points, not an array of shape {shape}")
        flat = torch.from_numpy(rows.reshape(-1, self.N)).to(self.device)
        phi_t = None
        if phi is not None:
            phi_rows = np.array(np.broadcast_to(np.asarray(host(phi), dtype=np.float32), shape), order="C")
            phi_t = torch.from_numpy(phi_rows.reshape(-1, self.N)).to(self.device)
        res = self.residual(flat, phi_t)
        ux, uxx = self.derivatives(flat)
        return res.cpu().numpy().reshape(shape), (ux.cpu().numpy().reshape(shape), uxx.cpu().numpy().reshape(shape))

    # -- test phase: the metric section of PDETrainingModule.test_step (include/burgers/eval.h) ---------------------
    def eval_rows_device(self, batch, B, T, d_rowstats):
        """The 14 fp64 sums of every (b, t) row of a test batch (``batch`` an ``_hip.EvalBatch`` of raw device pointers)
        into ``d_rowstats`` [B, T, 14]; see ``bg_eval_rows``.  Enqueued on torch's current stream of the env's device."""
        _hip.check_eval(self._lib.bg_eval_rows(_stream(self.device), None if batch is None else _hip.ctypes.byref(batch),
                                               int(B), int(T), self.N, self.dx, _void_p(d_rowstats)))

    def eval_fold_device(self, d_rowstats, B, T, d_tables, d_accum=0):
        """``d_rowstats`` [B, T, 14] folded into the MSE and the 20 per-step tables, ``d_tables`` [1 + 20 T], and
        ``d_accum`` (same shape, 0 = NULL) += B * tables; see ``bg_eval_fold``.  Enqueued on torch's current stream."""
        _hip.check_eval(self._lib.bg_eval_fold(_stream(self.device), _void_p(d_rowstats), int(B), int(T), self.N,
                                               _void_p(d_tables), _void_p(d_accum)))

    # -- gym.vector API ---------------------------------------------------------------------------------------------
    def reset_wait(self, seed=None, return_info: bool = False, options=None, **kwargs):
        if seed is None:
            seeds = [None] * self.num_envs
        elif isinstance(seed, (int, np.integer)):
            seeds = [int(seed) + i for i in range(self.num_envs)]
        else:
            seeds = list(seed)
        self._rngs = [np.random.RandomState(s) for s in seeds]
        obs = self._fresh_rows(np.arange(self.num_envs)).reshape(self.num_envs, 1, self.N)
        if return_info:
            return obs, {"step": self.timestep.copy()}
        return obs

    def reset(self, **kwargs):
        return self.reset_wait(**kwargs)

    def step_async(self, actions):
        self._actions = np.ascontiguousarray(np.asarray(actions, dtype=np.float32).reshape(self.num_envs, -1))

    def step_wait(self, **kwargs):
        assert self._actions is not None, "step_wait() without step_async()"
        a = torch.from_numpy(self._actions).to(self.device, non_blocking=True)
        self._actions = None
        u, rewards = self.step_torch(a)
        obs = u.cpu().numpy().reshape(self.num_envs, 1, self.N)
        rewards = rewards.cpu().numpy()
        if bool(self._status.any()):
            self._raise_on(self._status.cpu().numpy())
        self.timestep += 1
        truncated = self.timestep >= self.max_episode_steps
        infos = {"step": self.timestep.copy()}
        if truncated.any():
            done = np.nonzero(truncated)[0]
            finals = np.full(self.num_envs, None, dtype=object)
            for i in done:
                finals[i] = obs[i].copy()
            infos["final_observation"], infos["_final_observation"] = finals, truncated.copy()
            obs[done] = self._fresh_rows(done).reshape(len(done), 1, self.N)
        return obs, rewards, np.zeros(self.num_envs, dtype=bool), truncated, infos


class BurgersEnv(gym.Env):
    """Single environment = a batch of one (same kernel, same arithmetic)."""

    def __init__(self, **config):
        super().__init__()
        self._config = dict(config)
        self._vec = None
        probe = {k: v for k, v in config.items() if k != "device"}
        self.objective = _checked_objective(probe.get("objective", "l2control"))
        L, N = probe.get("L", 2 * math.pi), probe.get("N", 512)
        self.L, self.N = L, N
        self.cfg_steps, self.dt = probe.get("cfg_steps", 50), probe.get("dt", 1e-3)
        self.max_episode_steps = math.ceil(probe.get("Tmax", 10.0) / (self.dt * self.cfg_steps))
        self.observation_space = gym.spaces.Box(-np.inf, np.inf, shape=(1, N), dtype=np.float32)
        self.action_space = gym.spaces.Box(-1.0, 1.0, shape=(1, 4), dtype=np.float32)

    @property
    def vec(self):
        if self._vec is None:   # constructing the env must not touch the GPU
            self._vec = BurgersBatchedVecEnv(1, **self._config)
        return self._vec

    def __getattr__(self, name):
        if name in ("forcing", "reward_func", "scenario", "dx", "x", "nu", "batched_reward_func", "rhs", "derivatives",
                    "eval_rows_device", "eval_fold_device"):
            return getattr(self.vec, name)
        raise AttributeError(name)

    def reset(self, seed=None, return_info=False, **kwargs):
        out = self.vec.reset(seed=seed, return_info=return_info)
        if return_info:
            return out[0][0], {"step": int(out[1]["step"][0])}
        return out[0]

    def step(self, action):
        self.vec.step_async(np.asarray(action, dtype=np.float32).reshape(1, -1))
        v = self.vec
        a = torch.from_numpy(v._actions).to(v.device)
        v._actions = None
        u, rewards = v.step_torch(a)
        if bool(v._status.any()):
            raise FloatingPointError("non-finite Burgers state")
        v.timestep += 1
        truncated = bool(v.timestep[0] >= v.max_episode_steps)
        return u.cpu().numpy().reshape(1, self.N), float(rewards[0]), False, truncated, {"step": int(v.timestep[0])}
