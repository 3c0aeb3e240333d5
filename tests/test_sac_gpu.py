"""The SAC agent on an MI355X: ``act`` and ``update`` on csrc/sac.hip against this repository's own module in fp64 on the
CPU (which tests/test_sac_host.py ties bit for bit to the reference's class).

Inputs are seeded smooth fields (sums of four sines), uniform(-1, 1) actions, rewards in (-1, 0) and stored noise tensors
(tests/_sac_models.py).  Where a bound is derived from a measurement, the measurement is the fp32 torch spelling on the CPU
against fp64 on the same inputs, taken inside the test before the kernels are judged.  The observed values are appended to
sac_parity_observed.jsonl next to conftest's gradient parity log (tools/sac_bench.py --parity collects them into
profiles/sac_parity_observed.json)."""
import json
import logging
import os

import numpy as np
import pytest
import torch

import _sac_models as sm
from conftest import GRAD_LOG, GRAD_TOL, check_grads

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FWD = dict(rtol=2e-4, atol_scale=2e-5)
LOSS_REL = 1e-3            # test 9's bound on the losses of two fp32 trajectories
OBSERVED = os.path.join(os.path.dirname(GRAD_LOG), "sac_parity_observed.jsonl")


def _record(**rec):
    print("sac parity", json.dumps(rec))
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


class _Counting:
    """A stand-in for the loaded library that counts sac_update / sac_policy_forward / sac_grads calls."""

    def __init__(self, lib):
        self.lib, self.calls = lib, {"sac_update": 0, "sac_policy_forward": 0, "sac_grads": 0}

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name not in self.calls:
            return fn

        def counted(*a):
            self.calls[name] += 1
            return fn(*a)
        return counted


@pytest.fixture
def counting(monkeypatch):
    from pdecontrol.sac import sac_hip
    c = _Counting(sac_hip.load())
    monkeypatch.setattr(sac_hip, "load", lambda: c)
    return c


# ---------------------------------------------------------------------------------------------------------------------
# 6. policy forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obs_dim", [64, 256])
@pytest.mark.parametrize("B", [1, 10, 100, 256, 257])
def test_policy_forward_against_cpu_fp64(B, obs_dim, counting):
    act_dim = 4 if obs_dim == 64 else 7
    agent = sm.build(256, obs_dim=obs_dim, act_dim=act_dim, seed=B + obs_dim, device=DEV, low=-2.0, high=1.0)
    ref = sm.twin(agent, torch.float64)
    obs = torch.from_numpy(sm.smooth_fields(B, obs_dim, B)[:, 0])
    (noise,) = sm.noise_pair(B, B, act_dim)[:1]
    want = ref.policy.sample(obs.double(), noise=noise.double())
    fused = agent._fused_for(obs.to(DEV))
    assert fused is not None
    got = fused.forward(obs.reshape(B, -1).to(DEV), noise.reshape(B, -1).to(DEV), want_logp=True, want_mean=True)
    torch.cuda.synchronize(DEV)
    errs = [_assert_forward(g.reshape(w.shape), w, name) for g, w, name in zip(got, want, ("action", "log-probability", "mean action"))]
    _record(case=f"forward-B{B}-O{obs_dim}", action=errs[0], logp=errs[1], mean=errs[2], atol_scale=FWD["atol_scale"])
    # the public entry: one launch, the stored noise, the mean action when asked for it
    before = counting.calls["sac_policy_forward"]
    with sm.stored_noise([noise]):
        action = agent.act(obs.to(DEV))
    assert counting.calls["sac_policy_forward"] == before + 1 and action.shape == (B, 1, act_dim) and action.is_cuda
    _assert_forward(action, want[0], "act")
    _assert_forward(agent.act(obs.to(DEV), deterministic=True), want[2], "act(deterministic=True)")
    torch.manual_seed(5)
    a = agent.select_action(obs.numpy(), deterministic=True)
    torch.manual_seed(5)
    b = agent.select_action(obs.numpy())
    assert isinstance(a, np.ndarray) and np.array_equal(a, b), "select_action ignores `deterministic`, as the reference does"


# ---------------------------------------------------------------------------------------------------------------------
# 7. gradients through sac_grads
# ---------------------------------------------------------------------------------------------------------------------
#: (obs_dim, act_dim, B, seed): today's geometry, then the edges of ``sac_wgrad``'s 128-sample batch loop and ragged K strip
#: at inputs on which the CPU fp32 spelling stays within GRAD_TOL / 4 of fp64 (no min(Q1, Q2) tie or ReLU that flips in
#: fp32), so the bound is GRAD_TOL itself.  At obs 128, act 16 most seeds miss that condition (CPU fp32 deviations of 1e-4
#: to 4e-3); (128, 16, 130, 34) meets it with 2.6e-6 / 1.5e-5.
GRAD_GEOMETRIES = [
    ((64, 4, 256, 0), ""),
    ((256, 1, 37, 3), "-O256-A1-B37"),         # B < 128: the batch loop's only pass is masked
    ((64, 7, 129, 1), "-O64-A7-B129"),         # one full pass plus a one-sample tail
    ((64, 4, 1, 1), "-O64-A4-B1"),             # a single sample
    ((128, 16, 130, 34), "-O128-A16-B130"),    # K = 144: the bias column opens a strip of its own; a two-sample tail
]
GRAD_CASES = [pytest.param(auto, *geom, id=("auto-alpha" if auto else "fixed-alpha") + tag)
              for geom, tag in GRAD_GEOMETRIES for auto in (False, True)]


@pytest.mark.parametrize("auto,obs_dim,act_dim,B,seed", GRAD_CASES)
def test_gradients_against_fp64_autograd(auto, obs_dim, act_dim, B, seed):
    """Bound per network: 4 x the deviation of the fp32 torch spelling on the CPU from fp64 on the same inputs (measured
    here), never below GRAD_TOL.  The factor 4 covers another summation order over the samples and the MFMA accumulation
    order.  The CPU fp32 deviation must itself stay within GRAD_TOL / 4, so that the bound is GRAD_TOL: a min(Q1, Q2) tie
    that flips in fp32 would otherwise inflate it."""
    agent = sm.build(256, auto=auto, obs_dim=obs_dim, act_dim=act_dim, seed=seed, device=DEV)
    ref64, ref32 = sm.twin(agent, torch.float64), sm.twin(agent, torch.float32)
    batch, noises = sm.make_batch(B, seed, obs_dim, act_dim), sm.noise_pair(B, seed, act_dim)
    t64 = sm.terms(ref64, sm.cast_batch(batch, torch.float64), noises)
    t32 = sm.terms(ref32, batch, noises)
    assert t64["q_gap"] >= 1e-4, f"|Q1 - Q2| comes within {t64['q_gap']:.1e} of the Q scale: pick another seed"
    dev = {net: sm.tensor_dev(t32[net], t64[net]) for net in ("critic", "policy")}
    print("cpu fp32 against fp64:", dev, "q_gap", t64["q_gap"])
    assert all(v <= GRAD_TOL / 4 for v in dev.values()), ("the CPU fp32 spelling leaves GRAD_TOL / 4 on these inputs", dev)
    tol = {net: max(4 * dev[net], GRAD_TOL) for net in dev}
    before = sm.full_state(agent)
    fused = agent._fused_for(agent._prepare(sm.cast_batch(batch, device=DEV))[0])
    obs, actions, nxtobs, rewards, terminated, _ = agent._prepare(sm.cast_batch(batch, device=DEV))
    flat = lambda t: t.reshape(B, -1).contiguous()
    args = (flat(obs), flat(actions), flat(nxtobs), flat(rewards).reshape(B), flat(terminated).reshape(B),
            flat(noises[0].to(DEV)), flat(noises[1].to(DEV)))
    counters = fused.counters.clone()
    gc, gp, gl, stats = fused.grads(*args)
    gc2, gp2, _, stats2 = fused.grads(*args)
    torch.cuda.synchronize(DEV)
    got = {"critic": sm.tensor_dev(gc, t64["critic"]), "policy": sm.tensor_dev(gp, t64["policy"])}
    geometry = "" if (obs_dim, act_dim, B) == (64, 4, 256) else f"-O{obs_dim}-A{act_dim}-B{B}"
    _record(case=f"grads-{'auto' if auto else 'fixed'}{geometry}", cpu_fp32_vs_fp64=dev, fused_vs_fp64=got, tol=tol, q_gap=t64["q_gap"],
            qloss_rel=_rel(stats[0], t64["qloss"]), ploss_rel=_rel(stats[1], t64["ploss"]))
    for net, grads in (("critic", gc), ("policy", gp)):
        check_grads(f"SAC {net} gradient vs CPU fp64 (B={B}, auto={auto})", {k: v.cpu().numpy() for k, v in grads.items()},
                    {k: v.numpy() for k, v in t64[net].items()}.__getitem__, tol=tol[net])
    _same({**gc, **{"p." + k: v for k, v in gp.items()}, "stats": stats},
          {**gc2, **{"p." + k: v for k, v in gp2.items()}, "stats": stats2}, "two sac_grads runs")
    if auto:
        assert _rel(gl, t64["log_alpha"]) <= 1e-5, (float(gl), float(t64["log_alpha"]))
    _same(before, sm.full_state(agent), "sac_grads must leave parameters, targets and moments alone")
    assert torch.equal(counters, fused.counters), "sac_grads must leave the counters alone"


# ---------------------------------------------------------------------------------------------------------------------
# 8. one update from a common state against fp64
# ---------------------------------------------------------------------------------------------------------------------
def _steps_off(before, after, before64, after64, net, lr):
    bad = total = 0
    for k in before:
        if not k.startswith(net + "."):
            continue
        d = (after[k] - before[k]).double() - (after64[k] - before64[k]).double()
        bad += int((d.abs() > 0.1 * lr).sum())
        total += d.numel()
    return bad / total


@pytest.mark.parametrize("obs_dim,act_dim,B", [(64, 4, 256), (128, 16, 100), (256, 1, 37)])
def test_one_update_against_fp64(obs_dim, act_dim, B):
    """Adam's first step is +-lr whatever the gradient's size, so an element whose gradient is at rounding level may flip:
    per network at most 5e-4 of the elements may differ from the fp64 step by more than 0.1 lr.  The fp32 torch spelling on
    the CPU must meet that cap on these inputs before the kernels are judged by it."""
    lr, cap = 3e-4, 5e-4
    logs, logs64 = [], []
    agent = sm.build(256, obs_dim=obs_dim, act_dim=act_dim, seed=B, device=DEV, logs=logs, lr=lr)
    ref64, ref32 = sm.twin(agent, torch.float64, logs64), sm.twin(agent, torch.float32)
    batch, noises = sm.make_batch(B, B, obs_dim, act_dim), sm.noise_pair(B, B, act_dim)
    states = {}
    for name, a, b in (("fp64", ref64, sm.cast_batch(batch, torch.float64)), ("fp32", ref32, batch), ("fused", agent, batch)):
        pre = sm.full_state(a)
        with sm.stored_noise(list(noises)):
            a.update(b)
        states[name] = (pre, sm.full_state(a))
    torch.cuda.synchronize(DEV)
    share = {name: {net: _steps_off(*states[name], *states["fp64"], net, lr) for net in ("critic", "policy")}
             for name in ("fp32", "fused")}
    pre, post = states["fused"]
    target_err = max(float((post[f"critic_target.{k}"] - ((1 - agent.tau) * pre[f"critic_target.{k}"] + agent.tau * post[f"critic.{k}"])).abs().max())
                     for k in agent.critic.state_dict())
    want = {k: v for e, _ in logs64 for k, v in e.items()}
    got = {k: v for e, _ in logs for k, v in e.items()}
    loss_rel = {k: _rel(got[k], want[k]) for k in ("SAC/Qloss", "SAC/PolicyLoss")}
    _record(case=f"update-O{obs_dim}-A{act_dim}-B{B}", share_outside_tenth_lr=share, cap=cap, target_err=target_err, loss_rel=loss_rel)
    assert all(v <= cap for v in share["fp32"].values()), ("the CPU fp32 spelling misses the cap on these inputs", share)
    assert all(v <= cap for v in share["fused"].values()), share
    assert target_err <= 1e-6, target_err
    assert all(v <= 1e-4 for v in loss_rel.values()), loss_rel
    assert _rel(got["Pol. Rew. Mean"], want["Pol. Rew. Mean"]) <= 1e-5 and got["SAC/alpha_loss"] == pytest.approx(0.2)
    assert int(post["critic_optim.0.step"]) == 1 and int(post["policy_optim.7.step"]) == 1 and agent.updates == 1


# ---------------------------------------------------------------------------------------------------------------------
# 9. five updates against the torch spelling on the same GPU
# ---------------------------------------------------------------------------------------------------------------------
def _run(agent, batches, fused_flags, seed):
    """``update`` per batch with the CUDA path of ``fused_flags``; returns the noise drawn."""
    from pdecontrol.sac import policies, sac
    from pdecontrol.surrogates import ops
    drawn, orig = [], policies.draw_noise
    spy = lambda like: (drawn.append(orig(like)), drawn[-1])[1]
    policies.draw_noise = sac.draw_noise = spy
    try:
        torch.manual_seed(seed)
        for batch, flag in zip(batches, fused_flags):
            with ops.fused(flag):
                agent.update(batch)
    finally:
        policies.draw_noise = sac.draw_noise = orig
    torch.cuda.synchronize(DEV)
    return drawn


def _losses(logs):
    return [(e["SAC/Qloss"], e["SAC/PolicyLoss"], e["SAC/alpha_loss"]) for e, _ in logs if "SAC/Qloss" in e]


@pytest.mark.parametrize("auto", [False, True], ids=["fixed-alpha", "auto-alpha"])
def test_updates_against_the_torch_spelling_on_the_gpu(auto, counting):
    """Tests 9 and 11: five (three with entropy tuning, which is then pinned end to end) updates on both CUDA paths from the
    same state and generator state."""
    n = 3 if auto else 5
    batches = [sm.cast_batch(sm.make_batch(256, 40 + i), device=DEV) for i in range(n)]
    runs = {}
    for fused in (True, False):
        logs = []
        agent = sm.build(256, auto=auto, interval=2 if auto else 1, seed=9, device=DEV, logs=logs)
        noise = _run(agent, batches, [fused] * n, seed=77)
        runs[fused] = (agent, _losses(logs), noise)
    assert counting.calls["sac_update"] == n
    assert len(runs[True][2]) == len(runs[False][2]) == 2 * n
    for a, b in zip(runs[True][2], runs[False][2]):
        assert torch.equal(a, b), "both CUDA paths must see the same noise"
    rel = [[_rel(x, y) for x, y in zip(f, t)] for f, t in zip(runs[True][1], runs[False][1])]
    la = _rel(runs[True][0].log_alpha, runs[False][0].log_alpha) if auto else 0.0
    _record(case=f"fused-vs-torch-gpu-{'auto' if auto else 'fixed'}", loss_rel=rel, log_alpha_rel=la, tol=LOSS_REL)
    assert len(rel) == n and all(v <= LOSS_REL for row in rel for v in row), rel
    if auto:
        assert la <= LOSS_REL and runs[True][0].alpha is not None
        assert _rel(runs[True][0].alpha, runs[False][0].alpha) <= LOSS_REL


# ---------------------------------------------------------------------------------------------------------------------
# 10. determinism, capture, path switching
# ---------------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical():
    batches = [sm.cast_batch(sm.make_batch(100, 60 + i, 128, 6), device=DEV) for i in range(3)]
    out = []
    for _ in range(2):
        agent = sm.build(256, auto=True, obs_dim=128, act_dim=6, seed=3, device=DEV)
        _run(agent, batches, [True] * 3, seed=1)
        state = sm.full_state(agent)
        state["stats"] = agent._fused.stats.cpu().clone()
        out.append(state)
    _same(out[0], out[1], "two runs from the same state")


@pytest.mark.parametrize("interval", [1, 2])
def test_update_many_replays_a_captured_graph_bit_for_bit(interval, counting):
    batches = [sm.cast_batch(sm.make_batch(256, 80 + i), device=DEV) for i in range(8)]
    out = []
    for many in (False, True):
        logs = []
        agent = sm.build(256, auto=True, interval=interval, seed=4, device=DEV, logs=logs)
        torch.manual_seed(21)
        if many:
            calls = counting.calls["sac_update"]
            agent.update_many(batches)
            assert counting.calls["sac_update"] == calls + 1, "one capture, eight replays"
        else:
            for b in batches:
                agent.update(b)
        torch.cuda.synchronize(DEV)
        state = sm.full_state(agent)
        state["logged"] = torch.tensor([list(row) for row in _losses(logs)])
        out.append(state)
    assert out[0]["logged"].shape == (8, 3)
    _same(out[0], out[1], "update_many against the update loop")
    assert int(out[1]["updates"]) == 8 and int(out[1]["critic_optim.0.step"]) == 8


def test_a_run_may_switch_path_between_updates():
    batches = [sm.cast_batch(sm.make_batch(256, 90 + i), device=DEV) for i in range(3)]
    runs = {}
    for name, flags in (("mixed", [True, False, True]), ("torch", [False] * 3)):
        logs = []
        agent = sm.build(256, auto=True, seed=6, device=DEV, logs=logs)
        _run(agent, batches, flags, seed=8)
        runs[name] = (agent, _losses(logs))
    rel = [[_rel(x, y) for x, y in zip(f, t)] for f, t in zip(runs["mixed"][1], runs["torch"][1])]
    _record(case="path-switching", loss_rel=rel, tol=LOSS_REL)
    assert len(rel) == 3 and all(v <= LOSS_REL for row in rel for v in row), rel
    sd, sd_torch = runs["mixed"][0].critic_optim.state_dict(), runs["torch"][0].critic_optim.state_dict()
    assert sd["param_groups"] == sd_torch["param_groups"] and set(sd["state"]) == set(sd_torch["state"]) == set(range(12))
    for i, st in sd["state"].items():
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 3.0
        assert st["step"].device == sd_torch["state"][i]["step"].device and st["step"].dtype == sd_torch["state"][i]["step"].dtype
        assert st["exp_avg"].shape == sd_torch["state"][i]["exp_avg"].shape
    # and the state round-trips into an agent that continues on either path
    other = sm.build(256, auto=True, seed=7, device=DEV)
    for name in ("critic", "critic_target", "policy"):
        getattr(other, name).load_state_dict(getattr(runs["mixed"][0], name).state_dict())
    other.critic_optim.load_state_dict(sd)
    other.policy_optim.load_state_dict(runs["mixed"][0].policy_optim.state_dict())
    other.update(batches[0])
    torch.cuda.synchronize(DEV)
    assert float(other.critic_optim.state_dict()["state"][0]["step"]) == 4.0


# ---------------------------------------------------------------------------------------------------------------------
# 12. fallback, 13. it learns
# ---------------------------------------------------------------------------------------------------------------------
def test_what_the_kernels_refuse_runs_the_torch_spelling_with_one_notice(counting, caplog):
    from pdecontrol.surrogates import ops
    batch = sm.make_batch(32, 3)
    for what, hidden, dtype in (("hidden = 128", 128, torch.float32), ("fp64 agent", 256, torch.float64)):
        ops._NOTIFIED.clear()
        caplog.clear()
        agent = sm.build(hidden, seed=1, device=DEV)
        if dtype is torch.float64:
            for net in sm.NETS:
                getattr(agent, net).to(dtype)
        before = sm.full_state(agent)
        with caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
            for _ in range(2):
                agent.update(sm.cast_batch(batch, dtype))
            agent.act(sm.cast_batch(batch, dtype, DEV)[0].squeeze(1))
        notices = [r for r in caplog.records if "plain PyTorch-ROCm" in r.message]
        assert len(notices) == 1, (what, [r.message for r in caplog.records])
        assert counting.calls == {"sac_update": 0, "sac_policy_forward": 0, "sac_grads": 0}, what
        after = sm.full_state(agent)
        assert agent.updates == 2 and not torch.equal(before["critic.linear1.weight"], after["critic.linear1.weight"])
    caplog.clear()
    agent = sm.build(256, seed=1, device=DEV)
    with caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        agent.update(batch)
        with ops.fused(False):
            agent.update(batch)
    assert counting.calls["sac_update"] == 1, "a supported agent under the defaults trains on the kernels"
    assert not [r for r in caplog.records if "plain PyTorch-ROCm" in r.message]


def test_a_terminated_sample_raises_on_the_host_or_at_the_next_fetch():
    logs = []
    agent = sm.build(256, seed=2, device=DEV, logs=logs)
    batch = list(sm.make_batch(32, 4))
    batch[4] = batch[4].clone()
    batch[4][5] = True
    with pytest.raises(AssertionError):
        agent.update(tuple(batch))                        # a host batch is checked on the host
    assert agent.updates == 0
    with pytest.raises(AssertionError):
        agent.update(sm.cast_batch(tuple(batch), device=DEV))   # a device batch at the fetch of the statistics


def test_it_learns():
    logs = []
    agent = sm.build(256, seed=0, device=DEV, logs=logs)
    batch = sm.cast_batch(sm.make_batch(256, 0), device=DEV)
    torch.manual_seed(0)
    for _ in range(200):
        agent.update(batch)
    torch.cuda.synchronize(DEV)
    losses = [row[0] for row in _losses(logs)]
    _record(case="learns", first=losses[0], last=losses[-1])
    assert len(losses) == 200 and losses[-1] < 0.1 * losses[0], (losses[0], losses[-1])
    assert all(bool(torch.isfinite(v).all()) for v in sm.full_state(agent).values())
