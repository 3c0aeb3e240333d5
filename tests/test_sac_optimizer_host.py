"""The fp64 Adam / Polyak oracle of tests/_sac_models.py (``adam_replay``, ``polyak_replay``), checked without a GPU before
tests/test_sac_optimizer_gpu.py judges csrc/sac.hip by it.

One run of the CPU agent feeds every check: entropy tuning on, target_update_interval 3, B = 100, seven updates, the three
optimizers on the distinct hyper-parameters of ``sm.HYPERS``.  Every ``optimizer.step()`` is recorded with the gradients it
consumed (``p.grad`` after the update is not them: the policy loss's backward accumulates into the critic's ``.grad`` too).

Units (u = 2^-24): m' u max(|m|, |g|); v' u max(v, g^2); p' u |p| + 16 u |p'_ref - p|; target' u max(|target|, |p'|).  The
bound is 4 units each: m' sees at most 3 fp32 roundings, v' 4, target' 3, p' 8 on the step and one on the result.
"""
import math

import numpy as np
import pytest
import torch

import _sac_models as sm

UPDATES, INTERVAL, B = 7, 3, 100


@pytest.fixture(scope="module")
def run():
    """[{optimizer name: (t, hypers, [(p, m, v, g, p', m', v') per tensor])} per update], [(target before, critic after,
    target after) per update]"""
    agent = sm.build(256, auto=True, interval=INTERVAL, seed=3)
    sm.set_distinct_hypers(agent)
    steps, current = [], {}

    def recording(name, opt):
        step = opt.step

        def wrapped(*a, **kw):
            params = opt.param_groups[0]["params"]
            pre = []
            for p in params:
                st = opt.state.get(p, {})
                zero = torch.zeros_like(p)
                pre.append((p.detach().clone(), st.get("exp_avg", zero).clone(), st.get("exp_avg_sq", zero).clone(),
                            p.grad.detach().clone()))
            t = int(opt.state.get(params[0], {}).get("step", 0)) + 1
            out = step(*a, **kw)
            post = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in params]
            assert int(opt.state[params[0]]["step"]) == t
            current[name] = (t, sm.hypers_of(opt), [a + b for a, b in zip(pre, post)])
            return out
        opt.step = wrapped

    for name, opt in sm.optimizers(agent):
        recording(name, opt)
    targets = []
    for k in range(UPDATES):
        before = [p.detach().clone() for p in agent.critic_target.parameters()]
        agent.update(sm.make_batch(B, 30 + k), noise=sm.noise_pair(B, 30 + k))
        steps.append(dict(current))
        current.clear()
        targets.append((before, [p.detach().clone() for p in agent.critic.parameters()],
                        [p.detach().clone() for p in agent.critic_target.parameters()]))
    assert all(set(s) == set(sm.HYPERS) for s in steps) and agent.updates == UPDATES
    return steps, targets


def _kernel_spelling(p, m, v, g, t, lr, beta1, beta2, eps):
    """csrc/sac.hip's Adam in fp32 numpy, operation by operation (the bias corrections in double, cast to float)."""
    f = np.float32
    lr, beta1, beta2, eps = f(lr), f(beta1), f(beta2), f(eps)
    step_size = f(float(lr) / (1.0 - math.pow(float(beta1), float(t))))
    bc2_sqrt = f(math.sqrt(1.0 - math.pow(float(beta2), float(t))))
    p, m, v, g = (x.numpy() for x in (p, m, v, g))
    m1 = m + (g - m) * (f(1.0) - beta1)
    v1 = v * beta2 + (f(1.0) - beta2) * g * g
    p1 = p - step_size * (m1 / (np.sqrt(v1) / bc2_sqrt + eps))
    assert m1.dtype == v1.dtype == p1.dtype == np.float32
    return p1, m1, v1


def _worst(steps, got_of, fp32_hyper):
    worst = {name: {"m": 0.0, "v": 0.0, "p": 0.0} for name in sm.HYPERS}
    for rec in steps:
        for name, (t, hyper, tensors) in rec.items():
            for p, m, v, g, p1, m1, v1 in tensors:
                ref = sm.adam_replay(p, m, v, g, t, fp32_hyper=fp32_hyper, **hyper)
                got = got_of(p, m, v, g, t, hyper, (p1, m1, v1))
                units = sm.adam_units(p, m, v, g, *got, ref)
                worst[name] = {q: max(worst[name][q], units[q]) for q in units}
    return worst


def test_the_run_uses_the_distinct_hyper_parameters_and_counts_its_steps(run):
    steps, _ = run
    for k, rec in enumerate(steps):
        for name, (t, hyper, tensors) in rec.items():
            want = sm.HYPERS[name]
            assert t == k + 1 and hyper == dict(lr=want["lr"], beta1=want["betas"][0], beta2=want["betas"][1], eps=want["eps"])
            assert len(tensors) == {"critic_optim": 12, "policy_optim": 8, "alpha_optim": 1}[name]
            assert all(float(g.abs().max()) > 0 for *_, g, _p1, _m1, _v1 in tensors), "a gradient that is all zero pins nothing"


def test_oracle_reproduces_torch_adam(run):
    """torch.optim.Adam computes its bias corrections from the double hyper-parameters: the oracle with
    ``fp32_hyper=False`` must reproduce every moment and parameter of all seven updates within 4 units.  Observed on an
    x86-64 CPU: at most 1.0 / 2.1 / 1.1 units for m / v / p.  How near p' comes to the bound depends on the inputs: where a
    new gradient all but cancels the moment (say 0.8 m + 0.2 g = -7.8e-6 from m = 3.0e-3, g = -1.2e-2) m' is right to a
    fraction of its unit and still 6e-6 off in relative terms, and the step inherits that; with other seeds of this run
    single policy bias elements reached 3.2 units (torch) and 3.5 (the kernels' spelling)."""
    worst = _worst(run[0], lambda p, m, v, g, t, hyper, torch_result: torch_result, fp32_hyper=False)
    print("torch Adam against the fp64 oracle, units:", worst)
    assert all(x <= sm.UNIT_BOUND for w in worst.values() for x in w.values()), worst


def test_the_kernels_fp32_spelling_meets_the_bound_the_kernels_are_held_to(run):
    """The expression of ``sac_wgrad`` / ``sac_finalize`` in fp32 numpy (no FMA contraction: contraction only removes
    roundings) against the oracle with ``fp32_hyper=True``, on the same inputs: the GPU test's bound is achievable.
    Observed: at most 1.25 / 1.89 / 1.08 units for m / v / p."""
    worst = _worst(run[0], lambda p, m, v, g, t, hyper, _torch: _kernel_spelling(p, m, v, g, t, **hyper), fp32_hyper=True)
    print("the kernels' fp32 spelling against the fp32-hyper oracle, units:", worst)
    assert all(x <= sm.UNIT_BOUND for w in worst.values() for x in w.values()), worst


def test_distance_between_the_two_oracles_is_recorded(run):
    """The ABI carries lr, betas and eps as fp32, so the kernels' 1 - beta2^t at beta2 = 0.999 is about 1.3e-5 (relative)
    off torch's, which computes it from the double: torch's own fp32 Adam sits several p-units from the fp32-hyper oracle
    and the two oracles sit as far apart (observed: torch up to 8.9 p-units from the fp32-hyper oracle and 1.1 from the
    double-hyper one, the two oracles 9.4 apart; with other seeds up to 15 and 12).  A note, not a defect; what
    is asserted is that the switch is live for all three optimizers and that torch's Adam is nearer the double-hyper oracle, the one it implements."""
    steps, _ = run
    between = _worst(steps, lambda p, m, v, g, t, hyper, _torch: sm.adam_replay(p, m, v, g, t, fp32_hyper=False, **hyper),
                     fp32_hyper=True)
    torch32 = _worst(steps, lambda p, m, v, g, t, hyper, torch_result: torch_result, fp32_hyper=True)
    torch64 = _worst(steps, lambda p, m, v, g, t, hyper, torch_result: torch_result, fp32_hyper=False)
    print("double-hyper oracle against the fp32-hyper oracle, units:", between)
    print("torch Adam against the fp32-hyper oracle, units:", torch32)
    for name in sm.HYPERS:
        assert between[name]["p"] > 0 and between[name]["m"] > 0 and between[name]["v"] > 0, (name, between)
    assert torch64["critic_optim"]["p"] < torch32["critic_optim"]["p"], (torch64, torch32)


def test_interval_phase_of_the_cpu_agent(run):
    """With interval 3 the target moves after updates 0, 3 and 6, to the Polyak average with the updated critic, and is
    bit-equal to its old value after the others: the phase the GPU test demands of ``sac_wgrad``."""
    _, targets = run
    agent_tau = sm.config().tau
    worst = 0.0
    for k, (before, critic, after) in enumerate(targets):
        if k % INTERVAL == 0:
            for t0, p1, t1 in zip(before, critic, after):
                assert not torch.equal(t0, t1), k
                worst = max(worst, sm.polyak_units(t0, p1, t1, sm.polyak_replay(t0, p1, agent_tau)))
        else:
            assert all(torch.equal(t0, t1) for t0, t1 in zip(before, after)), k
    print("soft_update against the fp64 Polyak oracle, units:", worst)
    assert worst <= sm.UNIT_BOUND, worst
