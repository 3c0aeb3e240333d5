"""The inputs of tests/test_sac_head_regimes_gpu.py, judged on the CPU references alone: the head regimes of
tests/_sac_models.py reach the clamp's two branches, the saturated tail and the 1e-6 floor inside the logarithm; and the
yardstick of that file, ``stable_sample`` on an fp32 twin, stays within the project's bounds of the fp64 class there, where
the fp32 class itself does not.  A GPU test that passes can then not have passed by missing the regime."""
import numpy as np
import pytest
import torch

import _sac_models as sm
from conftest import GRAD_TOL

REGIMES = ("mixed", "knee")
CASES = [pytest.param(regime, *geom, id=f"{regime}-O{geom[0]}-A{geom[1]}-B{geom[2]}") for regime in REGIMES for geom in sm.HEAD_GEOMETRIES]


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


@pytest.mark.parametrize("regime,obs_dim,act_dim,B,seed", CASES)
def test_the_regime_is_reached_and_the_yardstick_holds(regime, obs_dim, act_dim, B, seed):
    c = sm.regime_case(regime, obs_dim, act_dim, B, seed)
    raw, x = sm.head_inputs(c.ref64, sm.cast_batch(c.batch, torch.float64), c.noises)
    ax = x.abs()
    counts = {"below": int((raw < -20).sum()), "inside": int(((raw >= -20) & (raw <= 2)).sum()), "above": int((raw > 2).sum()),
              "small": int((ax < 1).sum()), "knee": int(((ax >= 5) & (ax <= 10)).sum()), "far": int((ax > 12).sum())}
    signs = {"x>=5": int((x >= 5).sum()), "x<=-5": int((x <= -5).sum()), "x>12": int((x > 12).sum()), "x<-12": int((x < -12).sum())}
    # the clamp's branch is taken in the backward pass, which only the current-state sample (the second half) has
    margin = float(torch.minimum((raw[B:] + 20).abs(), (raw[B:] - 2).abs()).min())
    print("clamp margin over both samples:", float(torch.minimum((raw + 20).abs(), (raw - 2).abs()).min()))
    gla = _rel(c.ty["log_alpha"], c.t64["log_alpha"])
    print(regime, (obs_dim, act_dim, B, seed), counts, signs, "margin", margin, "q_gap", c.t64["q_gap"], "yardstick", c.dev, "log_alpha", gla)
    if act_dim >= 4:
        if regime == "mixed":
            # the far tail sits around the mean bias of -9 (x > 12 needs a draw of +2.8 standard deviations there), so
            # both signs are asked of the saturated components as a whole, and of the tail itself from 129 samples on
            assert all(v > 0 for v in counts.values()), counts
            assert signs["x>12"] > 0 and signs["x<-12"] > 0 or B < 129, signs
        else:
            assert counts["below"] == counts["above"] == 0 and 2 * counts["knee"] >= raw.numel(), counts
        assert signs["x>=5"] > 0 and signs["x<=-5"] > 0, signs
    if regime == "mixed":
        assert margin >= 0.1, f"a raw log_std comes within {margin:.2g} of a clamp edge: fp32 could take the other branch"
    assert c.t64["q_gap"] >= 1e-4, c.t64["q_gap"]
    assert all(v <= GRAD_TOL / 4 for v in c.dev.values()), ("the yardstick leaves GRAD_TOL / 4", c.dev)
    assert gla <= 1e-5, gla
    for key in ("qloss", "ploss"):
        assert _rel(c.ty[key], c.t64[key]) <= 1e-4 / 4, (key, float(c.ty[key]), float(c.t64[key]))
    # the flags are live: without them the critic's gradient is another one
    plain = sm.terms(c.ref64, sm.cast_batch(c.batch, torch.float64), c.noises)
    assert sm.tensor_dev(plain["critic"], c.t64["critic"]) > 100 * GRAD_TOL


def test_the_fp32_class_cannot_be_the_yardstick_here():
    """Normal.log_prob forms x - mean at a standard deviation of 2e-9 and the class takes 1 - tanh^2 by subtraction: in fp32
    both cancel.  Should the class ever be made stable this trips, and ``stable_sample`` can be retired."""
    c = sm.regime_case("mixed", 64, 4, 256, 0)
    t32 = sm.terms(sm.twin(c.agent, torch.float32), c.batch, c.noises, terminated=c.flags)
    dev = {net: sm.tensor_dev(t32[net], c.t64[net]) for net in ("critic", "policy")}
    print("fp32 class against fp64:", dev, "yardstick:", c.dev)
    assert max(dev.values()) > GRAD_TOL, dev


def test_stable_sample_is_the_class_where_nothing_cancels():
    """At the initial weights (|x| ~ 1, log_std ~ 0) the yardstick and the class agree in fp64 to rounding, values and
    gradients: it is the same head."""
    agent = sm.set_head(sm.build(256, seed=4), [0.0], [0.0])
    ref = sm.twin(agent, torch.float64)
    obs = torch.from_numpy(sm.smooth_fields(19, sm.OBS, 4)[:, 0]).double()
    (noise,) = sm.noise_pair(19, 4)[:1]
    outs = []
    for sample in (ref.policy.sample, lambda s, noise: sm.stable_sample(ref.policy, s, noise)):
        action, logp, mean = sample(obs, noise=noise.double())
        grads = torch.autograd.grad((action * action).sum() + (logp * torch.arange(1.0, 20.0, dtype=torch.float64).reshape(-1, 1)).sum(),
                                    list(ref.policy.parameters()))
        outs.append([action, logp, mean, *grads])
    for a, b in zip(*outs):
        np.testing.assert_allclose(b.detach().numpy(), a.detach().numpy(), rtol=1e-9, atol=1e-12 * float(a.detach().abs().max()))


def test_torch_clamp_passes_the_gradient_on_its_edges_and_not_one_ulp_outside():
    obs_dim, act_dim, B, seed = sm.HEAD_GEOMETRIES[-1]
    c = sm.regime_case("boundary", obs_dim, act_dim, B, seed)
    raw, _ = sm.head_inputs(c.ref64, sm.cast_batch(c.batch, torch.float64), c.noises)
    want = torch.tensor([float(np.float32(v)) for v in sm.HEAD_REGIMES["boundary"][0]], dtype=torch.float64)
    assert torch.equal(raw, want.expand_as(raw)), "the raw log_std is the bias bit for bit"
    assert want[2] < -20 < want[0] + 1e-9 and want[3] > 2 and want[0] == -20 and want[1] == 2
    for t in (c.t64, c.ty):
        g = t["policy"]["log_std_linear.bias"]
        assert g[0] != 0 and g[1] != 0, g
        assert g[2] == 0 and g[3] == 0, g
    assert all(v <= GRAD_TOL / 4 for v in c.dev.values()), c.dev
    assert c.t64["q_gap"] >= sm.BOUNDARY_Q_GAP, c.t64["q_gap"]


@pytest.mark.parametrize("log_std,mean", sm.SINGLE_HEADS)
def test_one_component_agents(log_std, mean):
    """The clamped agents (log_std bias -25 and 3.5) are clamped on every sample, so fp64 autograd gives their log_std
    layer a gradient of exactly zero; the yardstick holds on all five."""
    obs_dim, act_dim, B, seed = sm.SINGLE_GEOMETRY
    agent = sm.set_head(sm.build(256, obs_dim=obs_dim, act_dim=act_dim, seed=seed), [log_std], [mean])
    ref64, yard = sm.twin(agent, torch.float64), sm.stable_twin(agent)
    batch, noises = sm.make_batch(B, seed, obs_dim, act_dim), sm.noise_pair(B, seed, act_dim)
    raw, _ = sm.head_inputs(ref64, sm.cast_batch(batch, torch.float64), noises)
    t64 = sm.terms(ref64, sm.cast_batch(batch, torch.float64), noises, terminated=sm.flagged(B))
    ty = sm.terms(yard, batch, noises, terminated=sm.flagged(B))
    dev = {net: sm.tensor_dev(ty[net], t64[net]) for net in ("critic", "policy")}
    print((log_std, mean), "raw log_std", float(raw.min()), float(raw.max()), "yardstick", dev)
    assert all(v <= GRAD_TOL / 4 for v in dev.values()), dev
    if log_std in (-25.0, 3.5):
        assert bool((raw < -20.1).all() or (raw > 2.1).all())
        for name in ("log_std_linear.weight", "log_std_linear.bias"):
            assert not bool(t64["policy"][name].any()) and not bool(ty["policy"][name].any()), name
    else:
        assert bool(((raw > -19.9) & (raw < 1.9)).all())
        assert bool(t64["policy"]["log_std_linear.bias"].any())


@pytest.mark.parametrize("obs_dim,act_dim,B", sm.HEAD_UPDATES)
def test_the_yardstick_meets_the_one_update_cap(obs_dim, act_dim, B):
    """test_one_update_against_fp64's construction in the mixed regime, with the yardstick twin in the fp32 class's place:
    at most 5e-4 of a network's elements step more than 0.1 lr away from the fp64 step."""
    lr, cap = 3e-4, 5e-4
    logs, logs64 = [], []
    agent = sm.head_regime(sm.build(256, obs_dim=obs_dim, act_dim=act_dim, seed=B, lr=lr), "mixed")
    ref64, yard = sm.twin(agent, torch.float64, logs64), sm.stable_twin(agent, logs)
    batch, noises = sm.make_batch(B, B, obs_dim, act_dim), sm.noise_pair(B, B, act_dim)
    s64, sy = sm.one_update(ref64, batch, noises), sm.one_update(yard, batch, noises)
    share = {net: sm.steps_off(*sy, *s64, net, lr) for net in ("critic", "policy")}
    want, got = ({k: v for e, _ in lg for k, v in e.items()} for lg in (logs64, logs))
    loss_rel = {k: _rel(got[k], want[k]) for k in ("SAC/Qloss", "SAC/PolicyLoss")}
    print("yardstick share off the fp64 step:", share, "loss", loss_rel)
    assert all(v <= cap for v in share.values()), share
    assert all(v <= 1e-4 / 4 for v in loss_rel.values()), loss_rel
