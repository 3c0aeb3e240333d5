"""The SAC agent on its gfx950 kernels (C ABI: include/sac_hip.h ``sac_*``; kernels: csrc/sac.hip).

``FusedSAC`` holds what the kernels need beside the agent's own tensors: the host structs with one device pointer per
parameter and Adam moment, the device counters, the entropy coefficient as a device scalar, the workspace and the
statistics buffer.  Parameters stay the modules' parameters and the moments stay the ``torch.optim.Adam`` state
(``exp_avg``, ``exp_avg_sq``; created here exactly as Adam's first ``step()`` creates it), so ``state_dict()`` /
``load_state_dict()`` are the torch ones and a run may change path between any two updates.  Adam's ``step`` is a host
scalar in torch's default layout: the kernels count in device memory (a captured graph must not freeze the count), the
host scalars are advanced alongside, and the device counters are re-seeded whenever the two disagree (after a torch-path
update or ``load_state_dict``).

The CPU path, ``PDECONTROL_FUSED=0`` / ``ops.fused(False)`` and whatever ``unsupported`` names run the torch spelling of
pdecontrol/sac/sac.py, the last with one logged notice per reason.  A missing library raises: there is no silent fallback.
"""
import ctypes
import os

import torch

import hipbind
from pdecontrol.surrogates import ops

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.abspath(os.path.join(_HERE, "..", "..", "lib", "libsac_hip.so"))

N_POLICY, N_CRITIC = 8, 12
_p, _i, _l, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float


class Config(ctypes.Structure):
    """``sac_config`` of include/sac_hip.h"""
    _fields_ = [("obs_dim", _i), ("act_dim", _i), ("hidden", _i), ("auto_alpha", _i), ("target_update_interval", _i),
                ("gamma", _f), ("tau", _f), ("target_entropy", _f),
                ("lr", _f * 3), ("beta1", _f * 3), ("beta2", _f * 3), ("eps", _f * 3)]


class State(ctypes.Structure):
    """``sac_state`` of include/sac_hip.h"""
    _fields_ = [("policy", _p * N_POLICY), ("policy_m", _p * N_POLICY), ("policy_v", _p * N_POLICY),
                ("critic", _p * N_CRITIC), ("critic_m", _p * N_CRITIC), ("critic_v", _p * N_CRITIC),
                ("target", _p * N_CRITIC),
                ("log_alpha", _p), ("log_alpha_m", _p), ("log_alpha_v", _p), ("alpha", _p), ("counters", _p),
                ("act_scale", _p), ("act_bias", _p)]


_cfg, _st = ctypes.POINTER(Config), ctypes.POINTER(State)
SYMBOLS = (
    ("sac_supported", _i, [_i, _i, _i]),
    ("sac_workspace_floats", _l, [_i, _i, _i, _i]),
    ("sac_policy_forward", _i, [_p, _cfg, _st, _i, _p, _p, _p, _p, _p]),
    ("sac_update", _i, [_p, _cfg, _st, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    ("sac_grads", _i, [_p, _cfg, _st, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, ctypes.POINTER(_p), ctypes.POINTER(_p), _p]),
    ("sac_last_error", ctypes.c_char_p, []),
)
STAT_KEYS = ("critic_loss", "policy_loss", "alpha_loss", "alpha", "reward_mean", "terminated")
_lib = None


class SacHipError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is None:
        _lib = hipbind.open_library(LIB_PATH, SYMBOLS, SacHipError, "The fused SAC path has no fallback.")
    return _lib


def last_error():
    return load().sac_last_error().decode(errors="replace")


_check = hipbind.checker(SacHipError, "libsac_hip", "sac_last_error", lambda: load())
_stream, _ptr = hipbind.stream, hipbind.ptr


def _adam_reason(opt, what):
    if type(opt) is not torch.optim.Adam or len(opt.param_groups) != 1:
        return f"SAC {what} optimizer that is not one-group torch.optim.Adam"
    g = opt.param_groups[0]
    if (g.get("weight_decay", 0) != 0 or g.get("amsgrad") or g.get("maximize") or g.get("capturable") or g.get("fused")
            or g.get("differentiable") or isinstance(g["lr"], torch.Tensor)):
        return f"SAC {what} Adam with options the kernels do not implement (weight decay, amsgrad, maximize, capturable, fused)"
    return None


def unsupported(agent, obs=None, batch=None):
    """None when the kernels run this agent (on ``obs``, squeezed [B, channels, height], and the ``(actions, rewards,
    terminated)`` of an update batch), else the reason."""
    params = list(agent.policy.parameters()) + list(agent.critic.parameters()) + list(agent.critic_target.parameters())
    tensors = params + ([] if obs is None else [obs]) + ([] if batch is None else list(batch[:2]))
    if any(t.dtype != torch.float32 for t in tensors):
        bad = next(t.dtype for t in tensors if t.dtype != torch.float32)
        return f"SAC agent in {str(bad).replace('torch.', '')} (the kernels are fp32)"
    if type(agent.policy).__name__ != "GaussianPolicy" or type(agent.critic).__name__ != "QNetwork":
        return f"SAC networks {type(agent.policy).__name__} / {type(agent.critic).__name__} (the kernels implement GaussianPolicy / QNetwork)"
    obs_dim, hidden = agent.policy.linear1.in_features, agent.policy.linear1.out_features
    act_dim = agent.policy.mean_linear.out_features
    if agent.policy.action_scale.numel() != act_dim or agent.policy.action_bias.numel() != act_dim:
        return "SAC policy without a per-component action scale (the kernels take one scale and bias per action component)"
    if load().sac_supported(obs_dim, act_dim, hidden) != 0:
        return "SAC " + last_error()
    if obs is not None and (obs.dim() != 3 or obs.shape[1] * obs.shape[2] != obs_dim or obs.shape[0] < 1):
        return f"SAC observations of shape {tuple(obs.shape)} (the kernels take [B, channels, height] with {obs_dim} values)"
    if batch is not None:
        actions, rewards, terminated = batch
        B = obs.shape[0]
        if actions.dim() != 3 or actions.shape[1] * actions.shape[2] != act_dim or rewards.numel() != B or terminated.numel() != B:
            return (f"SAC batch with actions {tuple(actions.shape)}, rewards {tuple(rewards.shape)}, terminated "
                    f"{tuple(terminated.shape)} (the kernels take [B, channels, height] actions and one reward and flag per sample)")
    for opt, what in ((agent.critic_optim, "critic"), (agent.policy_optim, "policy")) + (
            ((agent.alpha_optim, "log_alpha"),) if agent.automatic_entropy_tuning else ()):
        reason = _adam_reason(opt, what)
        if reason:
            return reason
    return None


def use_kernels(agent, obs=None, batch=None):
    """True when ``agent`` acts and trains on the HIP kernels: on CUDA, fp32, a supported geometry, and not opted out
    (``ops.fused(False)`` / ``PDECONTROL_FUSED=0``).  What the kernels refuse runs the torch spelling on PyTorch-ROCm
    kernels, announced once per reason (the ``ops._use_fused_layout`` convention)."""
    if agent.device.type != "cuda" or not ops.fused_enabled():
        return False
    load()                                      # raises when the library has not been built: no silent fallback
    reason = unsupported(agent, obs, batch)
    if reason is None:
        return True
    if reason not in ops._NOTIFIED:
        ops._NOTIFIED.add(reason)
        ops._LOG.warning("the fused HIP kernels do not implement the %s: it runs on plain PyTorch-ROCm kernels", reason)
    return False


def _ensure_adam_state(opt):
    """The state ``torch.optim.Adam`` creates in its first ``step()`` (``_init_group``), for every parameter that has none."""
    for group in opt.param_groups:
        for p in group["params"]:
            state = opt.state[p]
            if len(state) == 0:
                state["step"] = torch.tensor(0.0, dtype=torch.get_default_dtype())
                state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)


def _steps(opt):
    return opt.state.get(opt.param_groups[0]["params"][0], {}).get("step", 0)


class FusedSAC:
    """The device-side companion of one ``SAC`` agent (see the module docstring)."""

    def __init__(self, agent):
        self.agent = agent
        dev = agent.device
        pol = agent.policy
        self.obs_dim, self.act_dim = pol.linear1.in_features, pol.mean_linear.out_features
        self.counters = torch.zeros(8, dtype=torch.int32, device=dev)
        self.mirror = None                       # host copy of counters[0:4]; None: not seeded yet
        self.alpha_buf = torch.zeros(1, dtype=torch.float32, device=dev)
        self._alpha_seen = None
        self.stats = torch.zeros(8, dtype=torch.float32, device=dev)
        self.scale = pol.action_scale.detach().reshape(-1).to(dev, torch.float32).contiguous()
        self.bias = pol.action_bias.detach().reshape(-1).to(dev, torch.float32).contiguous()
        self.work = {}
        self.version = 0
        self._keys = None
        self.cfg = None
        self.state = None
        self.graphs = {}

    # ---- host structs ---------------------------------------------------------------------------------------------
    def _identity(self):
        a = self.agent
        opts = [a.critic_optim, a.policy_optim] + ([a.alpha_optim] if a.automatic_entropy_tuning else [])
        key = []
        for opt in opts:
            ps = opt.param_groups[0]["params"]
            for p in (ps[0], ps[-1]):
                st = opt.state.get(p, {})
                key += [p.data_ptr(), id(st.get("exp_avg")), id(st.get("exp_avg_sq"))]
        g = [(o.param_groups[0]["lr"], tuple(o.param_groups[0]["betas"]), o.param_groups[0]["eps"]) for o in opts]
        return (tuple(key), tuple(g), a.gamma, a.tau, a.target_update_interval, next(a.critic_target.parameters()).data_ptr())

    def refresh(self, need_adam=True):
        """(Re)build the host structs when a tensor they point at has been replaced (``load_state_dict`` of an optimizer
        replaces the moments) or a hyper-parameter changed.  Captured graphs carry them by value and are dropped."""
        a = self.agent
        if need_adam:
            _ensure_adam_state(a.critic_optim)
            _ensure_adam_state(a.policy_optim)
            if a.automatic_entropy_tuning:
                _ensure_adam_state(a.alpha_optim)
        key = (self._identity(), need_adam)
        if key == self._keys:
            return
        self._keys = key
        self.version += 1
        self.graphs.clear()
        cfg = Config(self.obs_dim, self.act_dim, a.policy.linear1.out_features, int(bool(a.automatic_entropy_tuning)),
                     int(a.target_update_interval), float(a.gamma), float(a.tau),
                     float(a.target_entropy) if a.automatic_entropy_tuning else 0.0)
        opts = [a.critic_optim, a.policy_optim, a.alpha_optim if a.automatic_entropy_tuning else a.policy_optim]
        for i, opt in enumerate(opts):
            g = opt.param_groups[0]
            cfg.lr[i], cfg.beta1[i], cfg.beta2[i], cfg.eps[i] = float(g["lr"]), g["betas"][0], g["betas"][1], g["eps"]
        st = State()
        for name, module, opt in (("policy", a.policy, a.policy_optim), ("critic", a.critic, a.critic_optim)):
            for i, p in enumerate(module.parameters()):
                assert p.is_contiguous()
                getattr(st, name)[i] = p.data_ptr()
                if need_adam:
                    getattr(st, name + "_m")[i] = opt.state[p]["exp_avg"].data_ptr()
                    getattr(st, name + "_v")[i] = opt.state[p]["exp_avg_sq"].data_ptr()
        for i, p in enumerate(a.critic_target.parameters()):
            st.target[i] = p.data_ptr()
        if a.automatic_entropy_tuning:
            st.log_alpha = a.log_alpha.data_ptr()
            if need_adam:
                st.log_alpha_m = a.alpha_optim.state[a.log_alpha]["exp_avg"].data_ptr()
                st.log_alpha_v = a.alpha_optim.state[a.log_alpha]["exp_avg_sq"].data_ptr()
        st.alpha, st.counters = self.alpha_buf.data_ptr(), self.counters.data_ptr()
        st.act_scale, st.act_bias = self.scale.data_ptr(), self.bias.data_ptr()
        self.cfg, self.state = cfg, st

    def refresh_current(self):
        """``refresh`` for a launch that needs the Adam moments only where the structs already hold them."""
        self.refresh(need_adam=self._keys[1] if self._keys else False)

    def workspace(self, B):
        if B not in self.work:
            n = load().sac_workspace_floats(self.obs_dim, self.act_dim, self.cfg.hidden, B)
            if n < 0:
                raise SacHipError(last_error())
            self.work[B] = torch.empty(n, dtype=torch.float32, device=self.agent.device)
        return self.work[B]

    # ---- host / device bookkeeping ----------------------------------------------------------------------------------
    def sync_in(self):
        """Seed the device counters and the device alpha from the agent's host-side state where they disagree."""
        a = self.agent
        want = [int(_steps(a.critic_optim)), int(_steps(a.policy_optim)),
                int(_steps(a.alpha_optim)) if a.automatic_entropy_tuning else 0, int(a.updates)]
        if want != self.mirror:
            self.counters[:4].copy_(torch.tensor(want, dtype=torch.int32))
            self.mirror = want
        if a.alpha is not self.alpha_buf and a.alpha is not self._alpha_seen:
            if isinstance(a.alpha, torch.Tensor):
                self.alpha_buf.copy_(a.alpha.detach().reshape(1))
            else:
                self.alpha_buf.fill_(float(a.alpha))
            self._alpha_seen = a.alpha

    def sync_out(self):
        """What one ``sac_update`` did to the counters, on the host: Adam's ``step`` scalars, ``updates``, ``alpha``."""
        a = self.agent
        opts = [a.critic_optim, a.policy_optim] + ([a.alpha_optim] if a.automatic_entropy_tuning else [])
        for opt in opts:
            for st in opt.state.values():
                st["step"] += 1
        a.updates += 1
        self.mirror = [self.mirror[0] + 1, self.mirror[1] + 1, self.mirror[2] + (1 if a.automatic_entropy_tuning else 0),
                       self.mirror[3] + 1]
        if a.automatic_entropy_tuning:
            a.alpha = self.alpha_buf        # a view of the device scalar the kernels keep current

    # ---- launches ---------------------------------------------------------------------------------------------------
    def forward(self, obs, noise, want_logp=False, want_mean=False):
        """obs [B, obs_dim] fp32 on the device; noise [B, act_dim] or None.  Returns (action, logp or None, mean or None)."""
        self.refresh_current()
        B = obs.shape[0]
        action = torch.empty((B, self.act_dim), dtype=torch.float32, device=obs.device)
        logp = torch.empty((B, 1), dtype=torch.float32, device=obs.device) if want_logp else None
        mean = torch.empty_like(action) if want_mean else None
        _check(load().sac_policy_forward(_stream(), ctypes.byref(self.cfg), ctypes.byref(self.state), B, _ptr(obs), _ptr(noise),
                                         _ptr(action), _ptr(logp), _ptr(mean)))
        return action, logp, mean

    def forward_launcher(self, B, obs, noise, action):
        """A zero-argument callable that launches the policy forward of ``B`` rows from the static buffers ``obs`` and
        ``noise`` into ``action`` (no log-probability, no mean) and raises on a non-zero status.  The structs as they
        stand (``refresh_current`` first), the pointers and the raw handle of torch's current stream are resolved here,
        once: a call costs the launch alone."""
        forward, stream = load().sac_policy_forward, _stream()
        cfg, state = ctypes.byref(self.cfg), ctypes.byref(self.state)
        p_obs, p_noise, p_action = _ptr(obs), _ptr(noise), _ptr(action)

        def launch():
            rc = forward(stream, cfg, state, B, p_obs, p_noise, p_action, None, None)
            if rc != 0:
                _check(rc)
        return launch

    def launch_update(self, obs, actions, nxtobs, rewards, terminated, noise_next, noise_cur):
        """The five launches of one update on the current stream (no host bookkeeping: ``update`` / ``update_many`` do it)."""
        B = obs.shape[0]
        _check(load().sac_update(_stream(), ctypes.byref(self.cfg), ctypes.byref(self.state), B, _ptr(obs), _ptr(actions),
                                 _ptr(nxtobs), _ptr(rewards), _ptr(terminated), _ptr(noise_next), _ptr(noise_cur),
                                 _ptr(self.stats), _ptr(self.workspace(B))))

    def update(self, obs, actions, nxtobs, rewards, terminated, noise_next, noise_cur):
        self.refresh()
        self.sync_in()
        self.launch_update(obs, actions, nxtobs, rewards, terminated, noise_next, noise_cur)
        self.sync_out()

    def grads(self, obs, actions, nxtobs, rewards, terminated, noise_next, noise_cur):
        """The test hook ``sac_grads``: ({critic name: grad}, {policy name: grad}, log_alpha grad or None, statistics);
        no parameter, moment, counter or target is written."""
        a = self.agent
        self.refresh_current()
        self.sync_in()
        gc = [torch.zeros_like(p) for p in a.critic.parameters()]
        gp = [torch.zeros_like(p) for p in a.policy.parameters()]
        gl = torch.zeros(1, dtype=torch.float32, device=a.device) if a.automatic_entropy_tuning else None
        arr_c = (_p * N_CRITIC)(*[t.data_ptr() for t in gc])
        arr_p = (_p * N_POLICY)(*[t.data_ptr() for t in gp])
        B = obs.shape[0]
        _check(load().sac_grads(_stream(), ctypes.byref(self.cfg), ctypes.byref(self.state), B, _ptr(obs), _ptr(actions),
                                _ptr(nxtobs), _ptr(rewards), _ptr(terminated), _ptr(noise_next), _ptr(noise_cur),
                                _ptr(self.stats), _ptr(self.workspace(B)), arr_c, arr_p, _ptr(gl)))
        return (dict(zip((n for n, _ in a.critic.named_parameters()), gc)),
                dict(zip((n for n, _ in a.policy.named_parameters()), gp)), gl, self.stats.clone())

    # ---- the captured update ------------------------------------------------------------------------------------------
    def graph_for(self, shapes):
        """Static input buffers and the captured graph of one update for these (obs, actions) shapes."""
        self.refresh()
        key = tuple(shapes)
        g = self.graphs.get(key)
        if g is None:
            g = self.graphs[key] = _GraphedUpdate(self, *shapes)
        return g


class _GraphedUpdate:
    def __init__(self, fused, B, act_shape):
        from pdecontrol.surrogates.graph_step import capture_graph
        from pdecontrol.surrogates.hipops import pooled_streams
        dev = fused.agent.device
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
        self.obs, self.nxtobs = z(B, fused.obs_dim), z(B, fused.obs_dim)
        self.actions, self.rewards, self.terminated = z(B, fused.act_dim), z(B), z(B)
        self.noise_next, self.noise_cur = z(B, *act_shape), z(B, *act_shape)
        self.inputs = (self.obs, self.actions, self.nxtobs, self.rewards, self.terminated, self.noise_next, self.noise_cur)
        fused.workspace(B)
        (stream,) = pooled_streams(dev, 1, "capture")
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            fused.grads(*self.inputs)            # warm-up of every kernel that writes no state
        torch.cuda.current_stream(dev).wait_stream(stream)
        self.graph = torch.cuda.CUDAGraph()
        capture_graph(self.graph, lambda: fused.launch_update(*self.inputs), stream)
