"""The optimizer half of ``sac_update`` on an MI355X, update by update: Adam inside ``sac_wgrad``, the Polyak average on the
same tile, ``log_alpha``'s Adam step in ``sac_finalize``, the device counters and the host ``step`` scalars.

Every update k of a run is replayed from the kernels' own gradients through the fp64 oracle of tests/_sac_models.py
(``adam_replay`` with ``fp32_hyper=True``, ``polyak_replay``; tests/test_sac_optimizer_host.py checks the oracle against
torch.optim.Adam and shows that the kernels' expression in plain fp32 meets the bound):

1. S = full_state(agent); ``fused.grads`` at S gives the critic and ``log_alpha`` gradients the update will use (the same
   five launches with every state write replaced by a store of the gradient);
2. ``agent.update`` gives S';
3. the policy gradient was taken against the *updated* critic: a second, fixed-alpha probe agent is loaded with S's policy,
   S''s critic and the entropy coefficient update k used, and its ``fused.grads`` gives it;
4. every ``exp_avg``, ``exp_avg_sq``, parameter, ``log_alpha`` and target tensor of S' must sit within 4 units of the oracle
   at t = step_S + 1 with that optimizer's own hyper-parameters, a target that is not due must be bit-equal, and the device
   counters, the host ``step`` scalars and ``agent.updates`` must agree.

Units (u = 2^-24): m' u max(|m|, |g|); v' u max(v, g^2); p' u |p| + 16 u |p'_ref - p|; target' u max(|target|, |p'|).
m' sees at most 3 fp32 roundings, v' 4, target' 3, p' 8 on the step and one on the result; FMA contraction removes some.

The three optimizers carry the distinct hyper-parameters of ``sm.HYPERS``, so an index into ``sac_config.lr[3]`` ... ``eps[3]``
that is off, two betas swapped, a bias-correction exponent off by one or a Polyak average on the wrong phase each move a
quantity by far more than 4 units from the second step on.  The worst units per run are appended to
sac_parity_observed.jsonl (tools/sac_bench.py --parity collects them into profiles/sac_parity_observed.json).
"""
import numpy as np
import pytest
import torch

import _sac_models as sm
from test_sac_gpu import _record, _same

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ALPHA_RTOL = 8 * sm.U


def _flat_args(agent, batch, noises):
    """(the fused companion, the seven flat device tensors of ``FusedSAC.grads``) for one batch and its stored noise pair"""
    obs, actions, nxtobs, rewards, terminated, _ = agent._prepare(sm.cast_batch(batch, device=DEV))
    fused = agent._fused_for(obs, (actions, rewards, terminated))
    assert fused is not None
    B = obs.shape[0]
    flat = lambda t: t.reshape(B, -1).contiguous()
    return fused, (flat(obs), flat(actions), flat(nxtobs), rewards.reshape(B).contiguous(), terminated.reshape(B).contiguous(),
                   flat(noises[0].to(DEV)), flat(noises[1].to(DEV)))


def _probe_for(agent):
    pol = agent.policy
    return sm.build(256, auto=False, obs_dim=pol.linear1.in_features, act_dim=pol.mean_linear.out_features, seed=12345, device=DEV)


def _policy_grad_used(probe, S, S1, batch, noises):
    """The policy gradient of the update S -> S': S's policy and entropy coefficient against S''s critic."""
    with torch.no_grad():
        for name, p in probe.policy.named_parameters():
            p.copy_(S[f"policy.{name}"])
        for name, p in probe.critic.named_parameters():
            p.copy_(S1[f"critic.{name}"])
    probe.alpha = float(S["alpha"])
    fused, args = _flat_args(probe, batch, noises)
    _, gp, _, _ = fused.grads(*args)
    return gp


def _worst_element(p, m, v, g, got_p, ref):
    """The element of a parameter furthest from the oracle in p-units, spelled out (for the failure message)."""
    P, M, G = (sm._f64(x) for x in (p, m, g))
    unit = sm.U * np.abs(P) + 16 * sm.U * np.abs(ref[0] - P)
    err = np.abs(sm._f64(got_p) - ref[0])
    j = np.unravel_index(np.argmax(np.where(unit > 0, err / np.where(unit > 0, unit, 1.0), 0.0)), err.shape)
    return dict(index=[int(i) for i in j], p=float(P[j]), step_ref=float(ref[0][j] - P[j]), got=float(sm._f64(got_p)[j]),
                m=float(M[j]), g=float(G[j]), m1_ref=float(ref[1][j]), v1_ref=float(ref[2][j]))


def _replayed_update(agent, probe, batch, noises, worst, notes):
    """One update of ``agent`` with every check of the module docstring; the worst units go into ``worst`` (max), whatever
    exceeds the bound into ``notes``."""
    batch = sm.cast_batch(batch, device=DEV)
    S = sm.full_state(agent)
    fused, args = _flat_args(agent, batch, noises)
    gc, _, gl, _ = fused.grads(*args)
    torch.cuda.synchronize(DEV)
    opts = sm.optimizers(agent)
    auto = bool(agent.automatic_entropy_tuning)
    t0 = {name: int(S.get(f"{name}.0.step", 0)) for name, _ in opts}
    updates = int(S["updates"])
    want = [t0["critic_optim"], t0["policy_optim"], t0.get("alpha_optim", 0), updates]
    assert fused.counters.tolist()[:5] == want + [0], "the device counters must carry the host's step counts before the update"
    hyper = {name: sm.hypers_of(opt) for name, opt in opts}

    agent.update(batch, noise=noises)
    torch.cuda.synchronize(DEV)
    S1 = sm.full_state(agent)
    gp = _policy_grad_used(probe, S, S1, batch, noises)
    torch.cuda.synchronize(DEV)

    def judge(what, opt, i, p_key, g):
        p = S[p_key]
        m, v = (S.get(f"{opt}.{i}.{k}", torch.zeros_like(p)) for k in ("exp_avg", "exp_avg_sq"))
        g = g.detach().cpu().reshape(p.shape)
        ref = sm.adam_replay(p, m, v, g, t0[opt] + 1, fp32_hyper=True, **hyper[opt])
        got = (S1[p_key], S1[f"{opt}.{i}.exp_avg"], S1[f"{opt}.{i}.exp_avg_sq"])
        units = sm.adam_units(p, m, v, g, *got, ref)
        for q, x in units.items():
            key = f"{what}.{q}"
            worst[key] = max(worst.get(key, 0.0), x)
            if not x <= sm.UNIT_BOUND:
                notes.append((updates, p_key, q, x, _worst_element(p, m, v, g, got[0], ref) if q == "p" else None))
        assert int(S1[f"{opt}.{i}.step"]) == t0[opt] + 1, (opt, i)

    for i, (name, g) in enumerate(gc.items()):
        judge("critic", "critic_optim", i, f"critic.{name}", g)
    for i, (name, g) in enumerate(gp.items()):
        judge("policy", "policy_optim", i, f"policy.{name}", g)
    if auto:
        judge("log_alpha", "alpha_optim", 0, "log_alpha", gl)
        alpha_want = float(np.exp(np.float64(S1["log_alpha"].item())))
        alpha_rel = abs(float(S1["alpha"]) - alpha_want) / alpha_want
        worst["alpha.rel"] = max(worst.get("alpha.rel", 0.0), alpha_rel)
        assert alpha_rel <= ALPHA_RTOL, (updates, float(S1["alpha"]), alpha_want)
    else:
        assert torch.equal(S1["alpha"], S["alpha"]), "a fixed entropy coefficient must not move"

    due = updates % agent.target_update_interval == 0
    for name in gc:
        tk, ck = f"critic_target.{name}", f"critic.{name}"
        if due:
            x = sm.polyak_units(S[tk], S1[ck], S1[tk], sm.polyak_replay(S[tk], S1[ck], agent.tau))
            worst["target"] = max(worst.get("target", 0.0), x)
            if not x <= sm.UNIT_BOUND:
                notes.append((updates, tk, "target", x, None))
            assert not torch.equal(S1[tk], S[tk]), (updates, tk, "the target is due and did not move")
        else:
            assert torch.equal(S1[tk], S[tk]), (updates, tk, "the target moved on an update where it is not due")

    after = [t0["critic_optim"] + 1, t0["policy_optim"] + 1, t0["alpha_optim"] + 1 if auto else 0, updates + 1]
    assert fused.counters.tolist()[:5] == after + [0], (fused.counters.tolist(), after)
    assert agent.updates == updates + 1
    return due


def _finish(case, worst, notes, **more):
    _record(case=case, units=worst, bound=sm.UNIT_BOUND, **more)
    assert not notes, (case, notes)
    assert all(x <= sm.UNIT_BOUND for k, x in worst.items() if k != "alpha.rel"), (case, worst)


def test_run_a_entropy_tuning_and_interval_three():
    """obs 64, act 4, B = 100, seven updates: the Polyak average fires at updates 0, 3 and 6 and at no other."""
    agent = sm.build(256, auto=True, interval=3, seed=21, device=DEV)
    sm.set_distinct_hypers(agent)
    probe = _probe_for(agent)
    worst, notes, fired = {}, [], []
    for k in range(7):
        fired.append(_replayed_update(agent, probe, sm.make_batch(100, 200 + k), sm.noise_pair(100, 200 + k), worst, notes))
    assert fired == [True, False, False, True, False, False, True]
    assert int(sm.full_state(agent)["alpha_optim.0.step"]) == 7
    _finish("adam-replay-a", worst, notes)


def test_run_b_fixed_alpha_interval_two_and_an_lr_changed_between_updates():
    """obs 256, act 1, B = 37 (less than one pass of the 128-sample batch loop), five updates; the policy's lr changes
    before update 3, and updates 3 and 4 must step with the new one (``FusedSAC.refresh`` rebuilds the host structs)."""
    O, A, B = 256, 1, 37
    agent = sm.build(256, auto=False, interval=2, obs_dim=O, act_dim=A, seed=22, device=DEV)
    sm.set_distinct_hypers(agent)
    probe = _probe_for(agent)
    worst, notes, fired, versions = {}, [], [], []
    for k in range(5):
        if k == 3:
            agent.policy_optim.param_groups[0]["lr"] = 2.5e-5
        fired.append(_replayed_update(agent, probe, sm.make_batch(B, 300 + k, O, A), sm.noise_pair(B, 300 + k, A), worst, notes))
        versions.append(agent._fused.version)
        assert sm.hypers_of(agent.policy_optim)["lr"] == (2.5e-5 if k >= 3 else 1e-4)
    assert fired == [True, False, True, False, True]
    assert versions[0] == versions[2] < versions[3] == versions[4], versions
    _finish("adam-replay-b", worst, notes)


def test_run_c_three_batch_passes_with_a_ragged_tail_and_a_bias_strip_of_its_own():
    """obs 128, act 16, B = 300, interval 1, entropy tuning, four updates: the wgrad batch loop runs 128 + 128 + 44 samples
    and the critic's first layer has K = 144, so its bias column opens a tenth 16-wide strip."""
    O, A, B = 128, 16, 300
    agent = sm.build(256, auto=True, interval=1, obs_dim=O, act_dim=A, seed=23, device=DEV)
    sm.set_distinct_hypers(agent)
    probe = _probe_for(agent)
    worst, notes, fired = {}, [], []
    for k in range(4):
        fired.append(_replayed_update(agent, probe, sm.make_batch(B, 400 + k, O, A), sm.noise_pair(B, 400 + k, A), worst, notes))
    assert fired == [True] * 4
    _finish("adam-replay-c", worst, notes)


def test_run_d_continues_from_torch_moments():
    """Two updates on the torch spelling leave Adam moments with step = 2 and updates = 2; three fused updates follow at
    t = 3, 4, 5 with interval 3: the target moves on the second of them only."""
    from pdecontrol.surrogates import ops
    agent = sm.build(256, auto=True, interval=3, seed=24, device=DEV)
    sm.set_distinct_hypers(agent)
    probe = _probe_for(agent)
    with ops.fused(False):
        for k in range(2):
            agent.update(sm.cast_batch(sm.make_batch(100, 500 + k), device=DEV), noise=sm.noise_pair(100, 500 + k))
    assert agent._fused is None and agent.updates == 2 and int(sm.full_state(agent)["critic_optim.0.step"]) == 2
    worst, notes, fired = {}, [], []
    for k in range(2, 5):
        fired.append(_replayed_update(agent, probe, sm.make_batch(100, 500 + k), sm.noise_pair(100, 500 + k), worst, notes))
    assert fired == [False, True, False]
    state = sm.full_state(agent)
    assert [int(state[f"{name}.0.step"]) for name, _ in sm.optimizers(agent)] == [5, 5, 5] and agent.updates == 5
    _finish("adam-replay-d", worst, notes)


def test_update_many_sees_a_hyper_parameter_change():
    """A captured graph carries the hyper-parameters by value: after the critic's lr changes, ``update_many`` must drop it
    and capture again.  Bit-equal to the ``update`` loop with the same change under the same seed."""
    batches = [sm.cast_batch(sm.make_batch(64, 600 + i), device=DEV) for i in range(8)]
    out = []
    for many in (False, True):
        agent = sm.build(256, auto=True, interval=2, seed=25, device=DEV)
        sm.set_distinct_hypers(agent)
        torch.manual_seed(31)
        for i, half in enumerate((batches[:4], batches[4:])):
            if i == 1:
                version = agent._fused.version
                agent.critic_optim.param_groups[0]["lr"] = 1e-4
            if many:
                agent.update_many(half)
            else:
                for b in half:
                    agent.update(b)
        torch.cuda.synchronize(DEV)
        assert agent._fused.version > version, "a changed lr must rebuild the host structs and drop the captured graphs"
        out.append(sm.full_state(agent))
    _same(out[0], out[1], "update_many against the update loop across a change of the critic's lr")
    assert int(out[1]["updates"]) == 8 and int(out[1]["critic_optim.0.step"]) == 8
    # and the change took: the same run without it ends elsewhere
    agent = sm.build(256, auto=True, interval=2, seed=25, device=DEV)
    sm.set_distinct_hypers(agent)
    torch.manual_seed(31)
    agent.update_many(batches[:4])
    agent.update_many(batches[4:])
    torch.cuda.synchronize(DEV)
    assert not torch.equal(sm.full_state(agent)["critic.linear1.weight"], out[1]["critic.linear1.weight"])
