"""Shared pieces of the SAC tests and of tools/gen_sac_golden.py: spaces, configurations, seeded batches and the scenario
the fixture tests/golden/sac_golden.npz records (run there on the reference's class, in tests/test_sac_host.py on ours)."""
from argparse import Namespace

import numpy as np
import torch

# tag -> (hidden, B, updates, automatic entropy tuning, target_update_interval, seed)
CASES = {"h32": (32, 16, 3, False, 1, 101), "h32_auto": (32, 16, 3, True, 2, 102), "h256": (256, 256, 2, False, 1, 103)}
OBS, ACT, N_ACT_OBS = 64, 4, 10
LOG_KEYS = ("Pol. Rew. Mean", "SAC/Qloss", "SAC/PolicyLoss", "SAC/entropy_loss", "SAC/alpha_loss")
NETS = ("critic", "critic_target", "policy")


class Box:
    """The three attributes of gym.spaces.Box the agent reads."""

    def __init__(self, low, high, shape):
        self.low = np.full(shape, low, dtype=np.float32)
        self.high = np.full(shape, high, dtype=np.float32)
        self.shape = shape


def spaces(obs_dim=OBS, act_dim=ACT, low=-1.0, high=1.0):
    return Box(-np.inf, np.inf, (1, obs_dim)), Box(low, high, (1, act_dim))


def config(hidden=256, auto=False, interval=1, cuda=False, **over):
    cfg = dict(gamma=0.99, tau=0.005, alpha=0.2, policy="Gaussian", target_update_interval=interval,
               automatic_entropy_tuning=auto, cuda=cuda, hidden_size=hidden, lr=3e-4)
    cfg.update(over)
    return Namespace(**cfg)


def smooth_fields(B, N, seed):
    """[B, 1, 1, N] fp32: per sample a sum of four sines, amplitudes uniform(-1, 1), phases uniform(0, 6)."""
    rs = np.random.RandomState(seed)
    x = np.linspace(0, 2 * np.pi, N, endpoint=False)
    rows = [sum(rs.uniform(-1, 1) * np.sin((k + 1) * x + rs.uniform(0, 6)) for k in range(4)) for _ in range(B)]
    return np.stack(rows).astype(np.float32).reshape(B, 1, 1, N)


def make_batch(B, seed, obs_dim=OBS, act_dim=ACT, dtype=torch.float32):
    """The 7-tuple of ``SAC.update``: obs, actions, nxtobs [B, 1, 1, n]; rewards in (-1, 0), flags and steps [B, 1]."""
    rs = np.random.RandomState(seed + 1000)
    obs = torch.from_numpy(smooth_fields(B, obs_dim, seed)).to(dtype)
    nxt = torch.from_numpy(smooth_fields(B, obs_dim, seed + 1)).to(dtype)
    act = torch.from_numpy(rs.uniform(-1, 1, (B, 1, 1, act_dim)).astype(np.float32)).to(dtype)
    rew = torch.from_numpy(-rs.uniform(0.01, 0.99, (B, 1)).astype(np.float32)).to(dtype)
    flags = torch.zeros((B, 1), dtype=torch.bool)
    steps = torch.from_numpy(rs.randint(0, 100, (B, 1)))
    return obs, act, nxt, rew, flags, flags.clone(), steps


def noise_pair(B, seed, act_dim=ACT, dtype=torch.float32):
    """Two stored standard-normal tensors [B, 1, act_dim] (next-state draw, current-state draw)."""
    rs = np.random.RandomState(seed + 2000)
    return tuple(torch.from_numpy(rs.standard_normal((B, 1, act_dim)).astype(np.float32)).to(dtype) for _ in range(2))


def snapshot(out, tag, k, agent, whole):
    for net in NETS:
        for name, p in getattr(agent, net).state_dict().items():
            v = p.detach().cpu().numpy()
            if whole:
                out[f"{tag}_u{k}_{net}.{name}"] = v.copy()
            else:
                out[f"{tag}_u{k}_{net}.{name}_sum"] = np.asarray(v.astype(np.float64).sum())
                out[f"{tag}_u{k}_{net}.{name}_head"] = v.reshape(-1)[:8].copy()
    if getattr(agent, "automatic_entropy_tuning", False):
        out[f"{tag}_u{k}_log_alpha"] = agent.log_alpha.detach().cpu().numpy().copy()


def scenario(tag, make_agent, logs):
    """Seed, build the agent, act, update ``updates`` times on the case's batch, act again.  ``make_agent(obs_space,
    act_space, cfg)`` builds it; ``logs`` is the list the agent's logger appends (dict, commit) to.  Returns {key: array}."""
    hidden, B, updates, auto, interval, seed = CASES[tag]
    whole = hidden <= 32
    out = {}
    batch = make_batch(B, seed)
    act_obs = smooth_fields(N_ACT_OBS, OBS, seed + 7)[:, 0]
    torch.manual_seed(seed)
    agent = make_agent(*spaces(), config(hidden, auto, interval))
    for name, t in zip(("obs", "actions", "nxtobs", "rewards", "terminated", "truncated", "steps"), batch):
        out[f"{tag}_batch_{name}"] = t.numpy().copy()
    out[f"{tag}_act_obs"] = act_obs.copy()
    snapshot(out, tag, 0, agent, whole)
    out[f"{tag}_action_before"] = np.asarray(agent.select_action(act_obs)).copy()
    for k in range(1, updates + 1):
        del logs[:]
        agent.update(batch)
        merged = {}
        for entry, _commit in logs:
            merged.update(entry)
        out[f"{tag}_u{k}_logged"] = np.asarray([float(merged[key]) for key in LOG_KEYS], dtype=np.float64)
        snapshot(out, tag, k, agent, whole)
    out[f"{tag}_action_after"] = np.asarray(agent.select_action(act_obs)).copy()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# helpers of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
class stored_noise:
    """``with stored_noise([n1, n2, ...]):`` -- every standard-normal draw of the agent (torch spelling and fused path
    alike) takes the next stored tensor instead, cast to the dtype and device asked for."""

    def __init__(self, tensors):
        self.queue = list(tensors)

    def _draw(self, like):
        t = self.queue.pop(0)
        assert t.shape == like.shape, (t.shape, like.shape)
        return t.to(device=like.device, dtype=like.dtype)

    def __enter__(self):
        from pdecontrol.sac import policies, sac
        self.saved = (policies.draw_noise, sac.draw_noise)
        policies.draw_noise = sac.draw_noise = self._draw
        return self

    def __exit__(self, *exc):
        from pdecontrol.sac import policies, sac
        policies.draw_noise, sac.draw_noise = self.saved


def build(hidden=256, auto=False, interval=1, obs_dim=OBS, act_dim=ACT, seed=0, device="cpu", logs=None, low=-1.0, high=1.0, **over):
    """A freshly seeded agent of this repository's class."""
    from pdecontrol.sac.sac import SAC
    torch.manual_seed(seed)
    logger = None if logs is None else (lambda entry, commit=True: logs.append((dict(entry), commit)))
    cfg = config(hidden, auto, interval, device=device, **over)
    return SAC(*spaces(obs_dim, act_dim, low, high), cfg, logger=logger)


def twin(agent, dtype, logs=None):
    """A CPU agent in ``dtype`` with the parameters, target and entropy coefficient of ``agent`` (optimizers fresh)."""
    from pdecontrol.sac.sac import SAC
    pol = agent.policy
    hidden = pol.linear1.out_features
    auto = bool(agent.automatic_entropy_tuning)
    cfg = config(hidden, auto, agent.target_update_interval, gamma=agent.gamma, tau=agent.tau,
                 alpha=float(agent.alpha) if not isinstance(agent.alpha, torch.Tensor) else float(agent.alpha.item()),
                 lr=agent.critic_optim.param_groups[0]["lr"])
    logger = None if logs is None else (lambda entry, commit=True: logs.append((dict(entry), commit)))
    out = SAC(*spaces(pol.linear1.in_features, pol.mean_linear.out_features), cfg, logger=logger)
    for net in NETS:
        getattr(out, net).load_state_dict({k: v.detach().cpu() for k, v in getattr(agent, net).state_dict().items()})
        getattr(out, net).to(dtype)
    out.policy.action_scale = pol.action_scale.detach().cpu().to(dtype)
    out.policy.action_bias = pol.action_bias.detach().cpu().to(dtype)
    if auto:
        with torch.no_grad():
            out.log_alpha.copy_(agent.log_alpha.detach().cpu())
        out.log_alpha.data = out.log_alpha.data.to(dtype)
    out.updates = agent.updates
    return out


def cast_batch(batch, dtype=None, device=None):
    return tuple(t.to(device=device, dtype=dtype if t.is_floating_point() else None) for t in batch)


def terms(agent, batch, noises, terminated=None):
    """Losses and gradients of one update of ``agent`` at its current state, in its own dtype on its own device, with the
    policy gradient taken against the not-yet-updated critic (what ``sac_grads`` computes).  ``terminated`` (a float [B]
    vector such as ``flagged(B)``) replaces the batch's flags past the host assert of ``_prepare``."""
    obs, actions, nxtobs, rewards, flags, _ = agent._prepare(batch)
    terminated = flags if terminated is None else terminated.to(device=obs.device).reshape(flags.shape)
    n_next, n_cur = (n.to(device=obs.device, dtype=obs.dtype) for n in noises)
    with torch.no_grad():
        a2, lp2, _ = agent.policy.sample(nxtobs, noise=n_next)
        q1t, q2t = agent.critic_target(nxtobs, a2)
        y = rewards + (1.0 - terminated.to(obs.dtype)) * agent.gamma * (torch.min(q1t, q2t) - agent.alpha * lp2)
    q1, q2 = agent.critic(obs, actions)
    qloss = torch.nn.functional.mse_loss(q1, y) + torch.nn.functional.mse_loss(q2, y)
    names_c = [n for n, _ in agent.critic.named_parameters()]
    gc = dict(zip(names_c, torch.autograd.grad(qloss, list(agent.critic.parameters()))))
    pi, lp, mean = agent.policy.sample(obs, noise=n_cur)
    q1p, q2p = agent.critic(obs, pi)
    ploss = (agent.alpha * lp - torch.min(q1p, q2p)).mean()
    names_p = [n for n, _ in agent.policy.named_parameters()]
    gp = dict(zip(names_p, torch.autograd.grad(ploss, list(agent.policy.parameters()))))
    gla = -(lp + agent.target_entropy).mean().detach() if agent.automatic_entropy_tuning else None
    gap = (q1p - q2p).detach().abs().min() / torch.cat([q1p, q2p]).detach().abs().max()
    return dict(critic=gc, policy=gp, log_alpha=gla, qloss=qloss.detach(), ploss=ploss.detach(), q_gap=float(gap),
                action=pi.detach(), logp=lp.detach(), mean=mean.detach())


def tensor_dev(got, ref):
    """max over tensors of max|got - ref| / max|ref|"""
    worst = 0.0
    for k, r in ref.items():
        r = r.detach().cpu().double()
        worst = max(worst, float((got[k].detach().cpu().double() - r).abs().max() / r.abs().max()))
    return worst


def full_state(agent):
    """Every parameter, Adam moment, step count and the entropy state, as CPU tensors."""
    out = {}
    for net in NETS:
        for k, v in getattr(agent, net).state_dict().items():
            out[f"{net}.{k}"] = v.detach().cpu().clone()
    opts = [("critic_optim", agent.critic_optim), ("policy_optim", agent.policy_optim)]
    if agent.automatic_entropy_tuning:
        opts.append(("alpha_optim", agent.alpha_optim))
        out["log_alpha"] = agent.log_alpha.detach().cpu().clone()
    for name, opt in opts:
        for i, p in enumerate(opt.param_groups[0]["params"]):
            for k, v in opt.state.get(p, {}).items():
                out[f"{name}.{i}.{k}"] = torch.as_tensor(v).detach().cpu().clone()
    out["alpha"] = torch.as_tensor(agent.alpha).detach().cpu().clone().reshape(-1).float()
    out["updates"] = torch.tensor(agent.updates)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the optimizer half: an fp64 replay of one Adam step and of the Polyak average, and the units they are judged in
# ---------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24             # fp32 unit roundoff
UNIT_BOUND = 4.0           # m' sees at most 3 fp32 roundings, v' 4, target' 3, p' 8 on the step and one on the result
#: three optimizers that share no hyper-parameter: an index into sac_config's lr[3], beta1[3], beta2[3], eps[3] that is
#: off by one, or two betas swapped, changes a step by far more than a unit
HYPERS = {"critic_optim": dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8),
          "policy_optim": dict(lr=1e-4, betas=(0.8, 0.99), eps=1e-6),
          "alpha_optim": dict(lr=1e-3, betas=(0.7, 0.95), eps=1e-7)}


def optimizers(agent):
    names = ("critic_optim", "policy_optim") + (("alpha_optim",) if agent.automatic_entropy_tuning else ())
    return [(name, getattr(agent, name)) for name in names]


def set_distinct_hypers(agent):
    """HYPERS on ``param_groups[0]`` of the agent's optimizers (before the first fused call, or between two updates)."""
    for name, opt in optimizers(agent):
        opt.param_groups[0].update(HYPERS[name])


def hypers_of(opt):
    g = opt.param_groups[0]
    return dict(lr=float(g["lr"]), beta1=float(g["betas"][0]), beta2=float(g["betas"][1]), eps=float(g["eps"]))


def _f64(x):
    return (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).astype(np.float64)


def adam_replay(p, m, v, g, t, lr, beta1, beta2, eps, fp32_hyper=False):
    """One step of torch.optim.Adam (no weight decay, no amsgrad) in fp64 numpy from fp32 inputs: (p', m', v').
    ``fp32_hyper`` rounds lr, beta1, beta2 and eps to fp32 first, which is what the C ABI hands the kernels."""
    if fp32_hyper:
        lr, beta1, beta2, eps = (float(np.float32(x)) for x in (lr, beta1, beta2, eps))
    p, m, v, g = (_f64(x) for x in (p, m, v, g))
    m1 = m + (g - m) * (1.0 - beta1)
    v1 = beta2 * v + (1.0 - beta2) * g * g
    p1 = p - lr / (1.0 - beta1 ** t) * (m1 / (np.sqrt(v1) / np.sqrt(1.0 - beta2 ** t) + eps))
    return p1, m1, v1


def polyak_replay(target, p_new, tau, fp32_hyper=True):
    """target (1 - tau) + p_new tau in fp64 numpy from fp32 inputs (``tau`` rounded to fp32 first unless told otherwise)."""
    tau = float(np.float32(tau)) if fp32_hyper else float(tau)
    return _f64(target) * (1.0 - tau) + _f64(p_new) * tau


def _worst_units(got, ref, unit):
    """max |got - ref| / unit; an element whose unit is zero (a quantity that is exactly zero and stays so) must match."""
    err = np.abs(_f64(got) - ref)
    assert err.shape == unit.shape
    assert not np.any((unit == 0) & (err != 0)), "a zero quantity moved"
    if err.size == 0:
        return 0.0
    return float(np.max(np.where(unit > 0, err / np.where(unit > 0, unit, 1.0), 0.0)))


def adam_units(p, m, v, g, got_p, got_m, got_v, ref):
    """How far (p', m', v') = ``got_*`` sits from ``ref = adam_replay(...)``, in units: u max(|m|, |g|) for m',
    u max(v, g^2) for v', u |p| + 16 u |p'_ref - p| for p'.  Returns {"m": .., "v": .., "p": ..} (the worst element)."""
    p, m, v, g = (_f64(x) for x in (p, m, v, g))
    p1, m1, v1 = ref
    return {"m": _worst_units(got_m, m1, U * np.maximum(np.abs(m), np.abs(g))),
            "v": _worst_units(got_v, v1, U * np.maximum(v, g * g)),
            "p": _worst_units(got_p, p1, U * np.abs(p) + 16 * U * np.abs(p1 - p))}


def polyak_units(target, p_new, got, ref):
    target, p_new = _f64(target), _f64(p_new)
    return _worst_units(got, ref, U * np.maximum(np.abs(target), np.abs(p_new)))


# ---------------------------------------------------------------------------------------------------------------------
# the head where it clamps and saturates: regimes, a cancellation-free yardstick, terminated flags
# ---------------------------------------------------------------------------------------------------------------------
_F32 = np.float32
#: regime -> (log_std bias pattern, mean bias pattern), cycled over the action components (component j takes entry j % 4)
HEAD_REGIMES = {
    # clamped below, inside, clamped above, inside; a standard deviation of e^2 carries the pre-tanh value to |x| ~ 30
    "mixed": ([-25.0, -1.0, 3.5, 0.5], [0.0, 6.0, -9.0, 0.3]),
    # nothing clamped; |x| ~ 6 ... 9 in both signs, where scale * sech^2 crosses the 1e-6 floor inside the logarithm
    "knee": ([-1.0, -2.0, -1.5, -3.0], [7.0, -6.5, 8.0, -7.5]),
    # with log_std_linear.weight zeroed the raw log_std is the bias bit for bit: two components on the clamp's edges, two
    # one fp32 ulp outside
    "boundary": ([_F32(-20.0), _F32(2.0), np.nextafter(_F32(-20.0), _F32(-np.inf)), np.nextafter(_F32(2.0), _F32(np.inf))],
                 [0.2, -0.4, 1.0, -1.5]),
}
#: (obs_dim, act_dim, B, seed) of the regime tests: test_sac_gpu.py's gradient geometries and one 33-sample batch
HEAD_GEOMETRIES = [(64, 4, 256, 0), (256, 1, 37, 3), (64, 7, 129, 1), (64, 4, 1, 1), (128, 16, 130, 34), (64, 4, 33, 5)]
#: the boundary case's floor on min |Q1 - Q2| over the Q scale.  A tie in min(Q1, Q2) flips when the fp32 Q values are off
#: by the gap; three layers of dot products over K <= 272 terms leave about sqrt(K) 2^-24 ~ 1e-6 of the Q scale, and this
#: is ten times that (the (64, 4, 33, 5) batch has 2.8e-5 there; the gradient tests keep test_sac_gpu.py's 1e-4)
BOUNDARY_Q_GAP = 1e-5
#: (log_std bias, mean bias) of the one-component agents at SINGLE_GEOMETRY: one regime each
SINGLE_HEADS = [(-25.0, 0.0), (3.5, -9.0), (-1.0, 6.0), (-2.0, -6.5), (0.5, 0.3)]
SINGLE_GEOMETRY = (64, 1, 17, 2)           # one full 16-sample tile and a one-sample tail
#: (obs_dim, act_dim, B) of the one-update cases; the agent, batch and noise seeds are B, as in test_one_update_against_fp64
HEAD_UPDATES = [(64, 4, 256), (128, 16, 100)]


def action_box(A):
    """A box that differs per component: (lo, hi) fp32 [A]."""
    return np.linspace(-2.0, -0.25, A, dtype=np.float32), np.linspace(0.5, 3.0, A, dtype=np.float32)


def set_head(agent, log_std_bias, mean_bias, zero_log_std_weight=False):
    """Overwrite the policy's two head biases with the patterns cycled over the components and give it the box of
    ``action_box``.  Call before the first fused call: ``FusedSAC`` copies scale and bias at construction."""
    pol = agent.policy
    A = pol.mean_linear.out_features
    dev, dtype = pol.mean_linear.bias.device, pol.mean_linear.bias.dtype
    cycle = lambda pattern: torch.tensor([float(_F32(pattern[j % len(pattern)])) for j in range(A)], dtype=torch.float64).to(dev, dtype)
    with torch.no_grad():
        pol.log_std_linear.bias.copy_(cycle(log_std_bias))
        pol.mean_linear.bias.copy_(cycle(mean_bias))
        if zero_log_std_weight:
            pol.log_std_linear.weight.zero_()
    lo, hi = (torch.from_numpy(v) for v in action_box(A))
    pol.action_scale = ((hi - lo) / 2).reshape(1, A).to(dev, dtype)
    pol.action_bias = ((hi + lo) / 2).reshape(1, A).to(dev, dtype)
    return agent


def head_regime(agent, name):
    ls, mean = HEAD_REGIMES[name]
    return set_head(agent, ls, mean, zero_log_std_weight=name == "boundary")


class _Squash(torch.autograd.Function):
    """x -> (tanh x, sech^2 x) from e = exp(-2|x|), with d tanh / dx = sech^2 and d sech^2 / dx = -2 tanh sech^2: no
    difference of nearly equal numbers on the way there or back."""

    @staticmethod
    def forward(ctx, x):
        e = torch.exp(-2.0 * x.abs())
        d = 1.0 / (1.0 + e)
        y, om = torch.sign(x) * (1.0 - e) * d, 4.0 * e * d * d
        ctx.save_for_backward(y, om)
        return y, om

    @staticmethod
    def backward(ctx, gy, gom):
        y, om = ctx.saved_tensors
        return gy * om - 2.0 * gom * y * om


def stable_sample(policy, state, noise=None):
    """``GaussianPolicy.sample`` written cancellation-free: Normal.log_prob(mean + noise std) is -noise^2 / 2 - log_std -
    log(2 pi) / 2 without forming x - mean, and 1 - tanh^2 comes from ``_Squash``.  The yardstick of the regime tests, on an
    fp32 CPU twin only."""
    from pdecontrol.sac import policies
    mean, log_std = policy.forward(state)
    if noise is None:
        noise = policies.draw_noise(mean)
    y, om = _Squash.apply(mean + noise * log_std.exp())
    action = y * policy.action_scale + policy.action_bias
    log_prob = -0.5 * noise * noise - log_std - 0.5 * float(np.log(2.0 * np.pi)) - torch.log(policy.action_scale * om + policies.epsilon)
    return action, log_prob.sum((1, 2)).reshape(-1, 1), torch.tanh(mean) * policy.action_scale + policy.action_bias


def stable_twin(agent, logs=None):
    """The fp32 CPU twin of ``agent`` whose policy samples through ``stable_sample``."""
    out = twin(agent, torch.float32, logs)
    pol = out.policy
    pol.sample = lambda state, noise=None: stable_sample(pol, state, noise)
    return out


def flagged(B):
    """A float [B] vector of ``terminated`` flags: every third sample (0, 3, 6, ...) is set."""
    out = torch.zeros(B, dtype=torch.float32)
    out[::3] = 1.0
    return out


def head_inputs(agent, batch, noises):
    """(raw log_std, pre-tanh x) of ``agent``'s policy over both samples of an update (next state with the first noise,
    current state with the second), each [2 B, A], in the agent's dtype."""
    pol = agent.policy
    raw, xs = [], []
    with torch.no_grad():
        for state, noise in ((batch[2], noises[0]), (batch[0], noises[1])):
            state = state.squeeze(1).to(pol.linear1.weight.dtype)
            h = torch.relu(pol.linear2(torch.relu(pol.linear1(state.reshape(state.shape[0], -1)))))
            ls, mean = pol.log_std_linear(h), pol.mean_linear(h)
            raw.append(ls)
            xs.append(mean + noise.reshape(ls.shape).to(ls.dtype) * ls.clamp(-20, 2).exp())
    return torch.cat(raw), torch.cat(xs)


def steps_off(before, after, before64, after64, net, lr):
    """The share of ``net``'s elements whose step differs from the fp64 step by more than 0.1 lr."""
    bad = total = 0
    for k in before:
        if k.startswith(net + "."):
            d = (after[k] - before[k]).double() - (after64[k] - before64[k]).double()
            bad += int((d.abs() > 0.1 * lr).sum())
            total += d.numel()
    return bad / total


def one_update(agent, batch, noises):
    """(state before, state after) of one ``update`` of ``agent`` on ``batch`` (cast to the agent's dtype) with stored noise."""
    dtype = agent.policy.linear1.weight.dtype
    pre = full_state(agent)
    with stored_noise(list(noises)):
        agent.update(cast_batch(batch, dtype))
    return pre, full_state(agent)


def regime_case(regime, obs_dim, act_dim, B, seed, auto=True, device="cpu", flags=None):
    """An agent in ``regime`` on ``device`` with its fp64 twin, its yardstick twin, the seeded batch and noise, the flags
    (``flagged(B)`` unless given) and both twins' ``terms`` under them."""
    agent = head_regime(build(256, auto=auto, obs_dim=obs_dim, act_dim=act_dim, seed=seed, device=device), regime)
    ref64, yard = twin(agent, torch.float64), stable_twin(agent)
    batch, noises = make_batch(B, seed, obs_dim, act_dim), noise_pair(B, seed, act_dim)
    flags = flagged(B) if flags is None else flags
    t64 = terms(ref64, cast_batch(batch, torch.float64), noises, terminated=flags)
    ty = terms(yard, batch, noises, terminated=flags)
    dev = {net: tensor_dev(ty[net], t64[net]) for net in ("critic", "policy")}
    return Namespace(agent=agent, ref64=ref64, yard=yard, batch=batch, noises=noises, flags=flags, t64=t64, ty=ty, dev=dev)
