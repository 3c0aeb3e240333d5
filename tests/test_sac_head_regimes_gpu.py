"""The tanh-Gaussian head of csrc/sac.hip (``policy_head`` and its backward pieces in ``sac_policy_pass``) where it clamps
and saturates, and the ``(1 - terminated)`` mask of ``sac_critic_pass``, on an MI355X against the CPU module in fp64.

The regimes are those of tests/_sac_models.py (``head_regime``): head biases that push the raw log_std past both clamp edges
and the pre-tanh value to |x| ~ 6 ... 30, and a per-component action box.  There the fp32 torch spelling of the class loses
1e-2 of its gradients to cancellation, so the yardstick that sizes a bound is ``stable_sample`` on an fp32 CPU twin, measured
inside each test before the kernels are judged; tests/test_sac_head_regimes_host.py shows on the CPU that the regimes are
reached and that the yardstick holds.  ``terminated`` flags reach the kernels through ``fused.grads``, past the host assert.

What each one-line change of csrc/sac.hip would trip (each compiled on a scratch copy; the consequences read off the code and
off an fp32 torch emulation of the head's backward on the CPU, deviation of the policy gradients from fp64 in brackets):

  no clamp mask on ``dls``             test_one_component_per_regime[-25.0-0.0] and [3.5--9.0] "the clamped log_std must pass
                                       no gradient"; check_grads (policy) of every ``mixed`` gradient case [2.4]
  ``om = 1 - y * y``                   the log-probability bar of test_forward_in_the_regimes[knee-*] (2e-3 to 4e-3 of its
                                       scale against 2e-5); check_grads (policy) in both regimes [2e-2 to 6e-2]
  ``gpi * om`` without ``h.sc``        check_grads (policy) of the ``mixed`` gradient cases and of the ``boundary`` case [3e-2 to
                                       5e-2]; invisible in ``knee``, where sech^2 ~ 1e-6
  ``scale[0]`` for every component     the action bar and the box assertion of test_forward_in_the_regimes at A = 4 and 16
                                       (action off by 0.13 of its scale); check_grads (policy) [3e-2 to 7e-2]
  no ``(1 - term)`` on the target      check_grads (critic) of every gradient case (the flags move the fp64 critic gradients
                                       by more than 100 GRAD_TOL: test_sac_head_regimes_host.py); the bit-for-bit comparison
                                       of test_a_fully_terminated_batch_has_the_reward_as_its_target
  a strict clamp mask (``>``, ``<``)   test_clamp_edges_pass_the_gradient_and_one_ulp_outside_does_not, "got[0] != 0 and
                                       got[1] != 0" [1.0]

Observed figures are appended to sac_head_regimes_observed.jsonl next to conftest's gradient parity log; one run's copy is
profiles/sac_head_regimes_observed.json."""
import json
import os

import numpy as np
import pytest
import torch

import _sac_models as sm
from conftest import GRAD_LOG, GRAD_TOL, check_grads

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FWD = dict(rtol=2e-4, atol_scale=2e-5)     # test_sac_gpu.py's file-wide forward bars
LOSS_REL = 1e-4                            # test_one_update_against_fp64's bound on the losses
OBSERVED = os.path.join(os.path.dirname(GRAD_LOG), "sac_head_regimes_observed.jsonl")
SEED_OF = {geom[:3]: geom[3] for geom in sm.HEAD_GEOMETRIES}


def _record(**rec):
    print("sac head regimes", json.dumps(rec))
    try:
        os.makedirs(os.path.dirname(OBSERVED), exist_ok=True)
        with open(OBSERVED, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


def _assert_forward(got, ref, msg):
    got_n, ref_n = got.detach().cpu().double().numpy(), ref.detach().cpu().double().numpy()
    assert got_n.shape == ref_n.shape, (msg, got_n.shape, ref_n.shape)
    scale = float(np.abs(ref_n).max())
    err = float(np.abs(got_n - ref_n).max()) / scale
    np.testing.assert_allclose(got_n, ref_n, rtol=FWD["rtol"], atol=FWD["atol_scale"] * scale, err_msg=msg)
    return err


def _rel(a, b):
    a, b = (float(v.detach()) if isinstance(v, torch.Tensor) else float(v) for v in (a, b))
    return abs(a - b) / abs(b)


def _same(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


def _forward(agent, obs, noise):
    """(action, log-probability, mean action) of the fused forward launch and of the fp64 twin's ``policy.sample``."""
    B = obs.shape[0]
    ref = sm.twin(agent, torch.float64)
    want = ref.policy.sample(obs.double(), noise=noise.double())
    fused = agent._fused_for(obs.to(DEV))
    assert fused is not None
    got = fused.forward(obs.reshape(B, -1).to(DEV), noise.reshape(B, -1).to(DEV), want_logp=True, want_mean=True)
    torch.cuda.synchronize(DEV)
    return [g.reshape(w.shape) for g, w in zip(got, want)], [w.detach() for w in want]


def _grad_args(agent, batch, noises, flags):
    """The arguments of ``fused.grads`` for ``batch`` with ``flags`` as the terminated vector."""
    B = batch[0].shape[0]
    obs, actions, nxtobs, rewards, _, _ = agent._prepare(sm.cast_batch(batch, device=DEV))
    flat = lambda t: t.reshape(B, -1).contiguous()
    return (flat(obs), flat(actions), flat(nxtobs), flat(rewards).reshape(B), flags.to(DEV).reshape(B).contiguous(),
            flat(noises[0].to(DEV)), flat(noises[1].to(DEV)))


def _fused(agent, batch):
    fused = agent._fused_for(agent._prepare(sm.cast_batch(batch, device=DEV))[0])
    assert fused is not None
    return fused


def _judge_grads(case, c, gc, gp, gl, stats, auto):
    """Gradients, losses and the log-alpha gradient of one ``fused.grads`` call against ``c.t64``, bounded by the yardstick
    ``c.ty`` as measured; returns the per-network tolerance."""
    assert all(v <= GRAD_TOL / 4 for v in c.dev.values()), ("the yardstick leaves GRAD_TOL / 4 on these inputs", c.dev)
    tol = {net: max(4 * c.dev[net], GRAD_TOL) for net in c.dev}
    got = {"critic": sm.tensor_dev(gc, c.t64["critic"]), "policy": sm.tensor_dev(gp, c.t64["policy"])}
    loss = {"qloss": _rel(stats[0], c.t64["qloss"]), "ploss": _rel(stats[1], c.t64["ploss"])}
    loss_yard = {k: _rel(c.ty[k], c.t64[k]) for k in loss}
    gla = _rel(gl, c.t64["log_alpha"]) if auto else None
    # recorded, not judged: what the fp32 class (the torch tier's spelling) loses to cancellation on the same inputs
    t32 = sm.terms(sm.twin(c.agent, torch.float32), c.batch, c.noises, terminated=c.flags)
    cls = {net: sm.tensor_dev(t32[net], c.t64[net]) for net in c.dev}
    cls["logp"] = float((t32["logp"].double() - c.t64["logp"]).abs().max() / c.t64["logp"].abs().max())
    _record(case=case, yardstick_vs_fp64=c.dev, fused_vs_fp64=got, fp32_class_vs_fp64=cls, tol=tol, q_gap=c.t64["q_gap"], loss_rel=loss,
            yardstick_loss_rel=loss_yard, log_alpha_rel=gla, yardstick_log_alpha_rel=_rel(c.ty["log_alpha"], c.t64["log_alpha"]) if auto else None)
    for net, grads in (("critic", gc), ("policy", gp)):
        check_grads(f"SAC {net} gradient vs CPU fp64 ({case})", {k: v.cpu().numpy() for k, v in grads.items()},
                    {k: v.numpy() for k, v in c.t64[net].items()}.__getitem__, tol=tol[net])
    assert all(v <= LOSS_REL / 4 for v in loss_yard.values()), ("the yardstick's losses leave a quarter of the bound", loss_yard)
    assert all(v <= LOSS_REL for v in loss.values()), loss
    if auto:
        assert gla <= 1e-5, (float(gl), float(c.t64["log_alpha"]))
    return tol


# ---------------------------------------------------------------------------------------------------------------------
# a. forward, f. the deterministic action
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obs_dim,act_dim,B", [(64, 4, 33), (128, 16, 130), (256, 1, 37)])
@pytest.mark.parametrize("regime", ["mixed", "knee"])
def test_forward_in_the_regimes(regime, obs_dim, act_dim, B):
    seed = SEED_OF[(obs_dim, act_dim, B)]
    agent = sm.head_regime(sm.build(256, obs_dim=obs_dim, act_dim=act_dim, seed=seed, device=DEV), regime)
    obs = torch.from_numpy(sm.smooth_fields(B, obs_dim, seed)[:, 0])
    noise = sm.noise_pair(B, seed, act_dim)[1]
    got, want = _forward(agent, obs, noise)
    errs = [_assert_forward(g, w, name) for g, w, name in zip(got, want, ("action", "log-probability", "mean action"))]
    # every action inside its own component's box.  The kernel holds the box as (scale, bias): its edges are the fp32
    # bias -+ scale, which fma(+-1, scale, bias) returns exactly and which sit within one ulp of action_box's
    scale, bias = agent.policy.action_scale.cpu().reshape(-1), agent.policy.action_bias.cpu().reshape(-1)
    lo, hi = bias - scale, bias + scale
    box_lo, box_hi = (torch.from_numpy(v) for v in sm.action_box(act_dim))
    assert float((lo - box_lo).abs().max()) <= 2.0 ** -22 and float((hi - box_hi).abs().max()) <= 2.0 ** -22
    for name, a in (("action", got[0]), ("mean action", got[2])):
        a = a.cpu().reshape(B, act_dim)
        assert bool((a >= lo).all()) and bool((a <= hi).all()), (name, "leaves its component's box")
    det = agent.act(obs.to(DEV), deterministic=True)
    det_err = _assert_forward(det, want[2], "act(deterministic=True)")
    _record(case=f"forward-{regime}-O{obs_dim}-A{act_dim}-B{B}", action=errs[0], logp=errs[1], mean=errs[2], deterministic=det_err,
            atol_scale=FWD["atol_scale"])


# ---------------------------------------------------------------------------------------------------------------------
# b. one component per regime, d. the clamp's zero branch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_std,mean", sm.SINGLE_HEADS)
def test_one_component_per_regime(log_std, mean):
    """A = 1 agents: clamped below, clamped above and saturated, saturated on either side, and the plain interior.  A
    failure here names the branch.  Where the log_std is clamped on every sample its layer's gradient is exactly zero, as
    fp64 autograd gives it (tests/test_sac_head_regimes_host.py::test_one_component_agents)."""
    obs_dim, act_dim, B, seed = sm.SINGLE_GEOMETRY
    agent = sm.set_head(sm.build(256, obs_dim=obs_dim, act_dim=act_dim, seed=seed, device=DEV), [log_std], [mean])
    batch, noises = sm.make_batch(B, seed, obs_dim, act_dim), sm.noise_pair(B, seed, act_dim)
    got, want = _forward(agent, batch[0][:, 0], noises[1])
    errs = [_assert_forward(g, w, name) for g, w, name in zip(got, want, ("action", "log-probability", "mean action"))]
    flags = sm.flagged(B)
    ref64, yard = sm.twin(agent, torch.float64), sm.stable_twin(agent)
    t64 = sm.terms(ref64, sm.cast_batch(batch, torch.float64), noises, terminated=flags)
    ty = sm.terms(yard, batch, noises, terminated=flags)
    dev = {net: sm.tensor_dev(ty[net], t64[net]) for net in ("critic", "policy")}
    assert all(v <= GRAD_TOL / 4 for v in dev.values()), dev
    gc, gp, _, stats = _fused(agent, batch).grads(*_grad_args(agent, batch, noises, flags))
    torch.cuda.synchronize(DEV)
    fused_dev = {"critic": sm.tensor_dev(gc, t64["critic"]), "policy": sm.tensor_dev(gp, t64["policy"])}
    _record(case=f"single-ls{log_std}-m{mean}", action=errs[0], logp=errs[1], mean=errs[2], yardstick_vs_fp64=dev, fused_vs_fp64=fused_dev)
    for net, grads in (("critic", gc), ("policy", gp)):
        check_grads(f"SAC {net} gradient vs CPU fp64 (A=1, log_std bias {log_std}, mean bias {mean})",
                    {k: v.cpu().numpy() for k, v in grads.items()}, {k: v.numpy() for k, v in t64[net].items()}.__getitem__,
                    tol=max(4 * dev[net], GRAD_TOL))
    for name in ("log_std_linear.weight", "log_std_linear.bias"):
        zero64 = not bool(t64["policy"][name].any())
        assert zero64 == (log_std in (-25.0, 3.5)), name
        if zero64:
            assert not bool(gp[name].any()), f"{name}: the clamped log_std must pass no gradient"
        else:
            assert bool(gp[name].any()), name


def test_clamp_edges_pass_the_gradient_and_one_ulp_outside_does_not():
    """``boundary``: the raw log_std is its bias bit for bit; components 0 and 1 sit on -20 and 2, where torch's clamp
    passes the gradient (tests/test_sac_head_regimes_host.py), components 2 and 3 one fp32 ulp outside."""
    obs_dim, act_dim, B, seed = sm.HEAD_GEOMETRIES[-1]
    c = sm.regime_case("boundary", obs_dim, act_dim, B, seed, device=DEV)
    assert c.t64["q_gap"] >= sm.BOUNDARY_Q_GAP, c.t64["q_gap"]
    gc, gp, gl, stats = _fused(c.agent, c.batch).grads(*_grad_args(c.agent, c.batch, c.noises, c.flags))
    torch.cuda.synchronize(DEV)
    tol = _judge_grads("grads-boundary", c, gc, gp, gl, stats, auto=True)
    got, want = gp["log_std_linear.bias"].cpu().double(), c.t64["policy"]["log_std_linear.bias"]
    assert want[0] != 0 and want[1] != 0 and want[2] == 0 and want[3] == 0, want
    assert got[2] == 0 and got[3] == 0, got
    assert got[0] != 0 and got[1] != 0, got
    assert float((got[:2] - want[:2]).abs().max()) <= tol["policy"] * float(want.abs().max()), (got, want)
    # ... and the rows of the weight gradient follow their components
    gw = gp["log_std_linear.weight"].cpu()
    assert not bool(gw[2:].any()) and bool(gw[0].any()) and bool(gw[1].any())


# ---------------------------------------------------------------------------------------------------------------------
# c. gradients under terminated flags
# ---------------------------------------------------------------------------------------------------------------------
GRAD_CASES = [pytest.param(regime, auto, *geom, id=f"{regime}-{'auto' if auto else 'fixed'}-O{geom[0]}-A{geom[1]}-B{geom[2]}")
              for regime in ("mixed", "knee") for geom in sm.HEAD_GEOMETRIES for auto in (False, True)]


@pytest.mark.parametrize("regime,auto,obs_dim,act_dim,B,seed", GRAD_CASES)
def test_gradients_in_the_regimes_against_fp64_autograd(regime, auto, obs_dim, act_dim, B, seed):
    """Bound per network: 4 x the yardstick's deviation from fp64 on the same inputs (measured here), never below GRAD_TOL;
    the yardstick must itself stay within GRAD_TOL / 4.  Every third sample is terminated."""
    c = sm.regime_case(regime, obs_dim, act_dim, B, seed, auto=auto, device=DEV)
    assert c.t64["q_gap"] >= 1e-4, f"|Q1 - Q2| comes within {c.t64['q_gap']:.1e} of the Q scale: pick another seed"
    before = sm.full_state(c.agent)
    fused = _fused(c.agent, c.batch)
    args = _grad_args(c.agent, c.batch, c.noises, c.flags)
    counters = fused.counters.clone()
    gc, gp, gl, stats = fused.grads(*args)
    gc2, gp2, gl2, stats2 = fused.grads(*args)
    torch.cuda.synchronize(DEV)
    _judge_grads(f"grads-{regime}-{'auto' if auto else 'fixed'}-O{obs_dim}-A{act_dim}-B{B}", c, gc, gp, gl, stats, auto)
    _same({**gc, **{"p." + k: v for k, v in gp.items()}, "stats": stats},
          {**gc2, **{"p." + k: v for k, v in gp2.items()}, "stats": stats2}, "two sac_grads runs")
    if auto:
        assert torch.equal(gl, gl2)
    assert float(stats[5]) == float(c.flags.sum()) == len(range(0, B, 3)), (float(stats[5]), B)
    _same(before, sm.full_state(c.agent), "sac_grads must leave parameters, targets and moments alone")
    assert torch.equal(counters, fused.counters), "sac_grads must leave the counters alone"


def test_a_fully_terminated_batch_has_the_reward_as_its_target():
    """All flags set: the critic target is the reward alone, so the critic's gradients do not see the next observation or
    the next-state noise -- bit for bit -- and match fp64 under the same flags."""
    obs_dim, act_dim, B, seed = sm.HEAD_GEOMETRIES[-1]
    c = sm.regime_case("mixed", obs_dim, act_dim, B, seed, device=DEV, flags=torch.ones(B))
    fused = _fused(c.agent, c.batch)
    gc, gp, gl, stats = fused.grads(*_grad_args(c.agent, c.batch, c.noises, c.flags))
    other = list(c.batch)
    other[2] = 3.0 * sm.make_batch(B, seed + 50, obs_dim, act_dim)[2]
    other_noises = (2.0 * sm.noise_pair(B, seed + 50, act_dim)[0], c.noises[1])
    assert not torch.equal(other[2], c.batch[2]) and not torch.equal(other_noises[0], c.noises[0])
    gc2, gp2, _, stats2 = fused.grads(*_grad_args(c.agent, tuple(other), other_noises, c.flags))
    torch.cuda.synchronize(DEV)
    _judge_grads("grads-mixed-all-terminated", c, gc, gp, gl, stats, auto=True)
    assert float(stats[5]) == B
    _same(gc, gc2, "critic gradients under another next observation and next-state noise")
    _same(gp, gp2, "policy gradients under another next observation and next-state noise")
    assert torch.equal(stats, stats2)
    # the mask is what did it: with no flag set the same swap moves the critic's gradients
    none = torch.zeros(B)
    ga = fused.grads(*_grad_args(c.agent, c.batch, c.noises, none))[0]
    gb = fused.grads(*_grad_args(c.agent, tuple(other), other_noises, none))[0]
    torch.cuda.synchronize(DEV)
    assert not torch.equal(ga["linear1.weight"], gb["linear1.weight"])


# ---------------------------------------------------------------------------------------------------------------------
# e. one update from a common state against fp64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obs_dim,act_dim,B", sm.HEAD_UPDATES)
def test_one_update_in_the_mixed_regime_against_fp64(obs_dim, act_dim, B):
    """test_one_update_against_fp64's construction with the yardstick twin in the fp32 class's place: per network at most
    5e-4 of the elements may differ from the fp64 step by more than 0.1 lr, and the yardstick must meet that cap first
    (tests/test_sac_head_regimes_host.py shows on the CPU that it does at these seeds)."""
    lr, cap = 3e-4, 5e-4
    logs, logs64 = [], []
    agent = sm.head_regime(sm.build(256, obs_dim=obs_dim, act_dim=act_dim, seed=B, device=DEV, logs=logs, lr=lr), "mixed")
    ref64, yard = sm.twin(agent, torch.float64, logs64), sm.stable_twin(agent)
    batch, noises = sm.make_batch(B, B, obs_dim, act_dim), sm.noise_pair(B, B, act_dim)
    states = {name: sm.one_update(a, batch, noises) for name, a in (("fp64", ref64), ("yardstick", yard), ("fused", agent))}
    torch.cuda.synchronize(DEV)
    share = {name: {net: sm.steps_off(*states[name], *states["fp64"], net, lr) for net in ("critic", "policy")}
             for name in ("yardstick", "fused")}
    pre, post = states["fused"]
    target_err = max(float((post[f"critic_target.{k}"] - ((1 - agent.tau) * pre[f"critic_target.{k}"] + agent.tau * post[f"critic.{k}"])).abs().max())
                     for k in agent.critic.state_dict())
    want = {k: v for e, _ in logs64 for k, v in e.items()}
    got = {k: v for e, _ in logs for k, v in e.items()}
    loss_rel = {k: _rel(got[k], want[k]) for k in ("SAC/Qloss", "SAC/PolicyLoss")}
    _record(case=f"update-mixed-O{obs_dim}-A{act_dim}-B{B}", share_outside_tenth_lr=share, cap=cap, target_err=target_err, loss_rel=loss_rel)
    assert all(v <= cap for v in share["yardstick"].values()), ("the yardstick misses the cap on these inputs", share)
    assert all(v <= cap for v in share["fused"].values()), share
    assert target_err <= 1e-6, target_err
    assert all(v <= LOSS_REL for v in loss_rel.values()), loss_rel
    assert int(post["critic_optim.0.step"]) == 1 and int(post["policy_optim.7.step"]) == 1 and agent.updates == 1
