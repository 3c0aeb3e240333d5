"""csrc/delay.hip (dly_forward, dly_backward) per cotangent, per slice and at the extremes, on an MI355X.

tests/test_delay_surrogate_gpu.py compares the delay rollout with the fp64 CPU module on one grid: every returned tensor
in the loss at once, S <= K, K never 2, weights at initialisation, white-noise states, one bar per tensor.  Here, with the
cases, inputs, operating points and bars of tests/_delay_models.py (tests/test_delay_regimes_host.py shows on the CPU that
the regimes are reached and measures the fp32 yardstick):

* one cotangent at a time (``_DelayRolloutFn`` does not materialise undefined cotangents, so each of d_out, d_del, d_inl,
  d_outl, d_cs_out, d_ca_out has a null branch in dly_bwd_kernel), three pairs, each run twice bit for bit;
* S > K, K = 2 with and without a given context, K = 1 from three given states; rows su..S of d_states and the given
  context's slot 0 exactly zero;
* the ``saturated`` and ``elu_deep`` operating points and smooth states of amplitude 1e-2, 1e-3 and 1e-4, where the first
  encoder LayerNorm's variance is below its eps;
* three cases of the base grid again, per slice;
* one rollout against the same rollout split in two with the context carried, bit for bit;
* one step of a three-member ensemble from a carried context, as WorldVecEnv.step asks for it.

Every case is compared with the same module as ``deepcopy(...).double()`` on the CPU and also runs the fp32 module on the
CPU as the yardstick.  Bars (``_delay_models.judge``): forward rtol 2e-4 / atol 2e-5 of the tensor's scale; every gradient
within max(GRAD_TOL, 4 x the yardstick's error on that tensor) of the tensor's scale (``check_grads``); every slice --
inputs per step, contexts per slot, the first MLP weight per window column block -- within max(GRAD_TOL, 4 x the
yardstick's error on that tensor's slices) of the SLICE's scale, and slices that are zero in fp64 on the zero rule
(``check_slices``).  The yardstick is measured in the test, against fp64, never against the kernels; where it stays
below GRAD_TOL / 4, as it did on every case when this was written, the bar is GRAD_TOL itself.
Every case appends the kernels' and the yardstick's figures to delay_regimes_observed.jsonl next to the gradient parity
log (profiles/delay_regimes_observed.json is that file of one run).

Faults emulated in fp32 torch by the host file, and the assertion here that fails on each:

  (a)  LayerNorm eps dropped / 1e-6     forward bar of the small-amplitude cases (error above 500 x the floor; the old
                                        grid's forward bar fails too, by less than 50 x: it was not blind to this one)
  (b)  exp(x) - 1 for expm1             check_grads of the amplitude-1e-4 case (first encoder LayerNorm gain, 1.7e-3)
  (b') ELU slope floored at 1e-3        check_grads of the elu_deep case (0.17 of scale)
  (c)  tanh slope 1 - |y|               check_grads of every case (and of the old grid: off at mid-range, not only at +-1)
  (c') tanh slope floored at 1e-3       check_grads of the two saturated cases (5e-3 of scale)
  (d)  states indexed with stride su    forward bar of the edge case (3, 6, 4) and of the grid row (5, 6, 4)
  (e)  null d_ctx_s_out read as d_out   check_grads of the cotangent case ``outputs`` alone
  (f)  K = 2 context from ring slots i  forward bar on context_s of the edge cases (3, 1, 2), (3, 2, 2), grid row (7, 1, 2)

Of these only (a) and (c) fail the nine cases the grid had before."""
import copy
import logging

import numpy as np
import pytest
import torch

import _delay_models as dm
import _grad_contract_models as gm

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
_GPU = {}


def _gpu(scaled, regime=None):
    """The fp32 CPU surrogate of ``dm.modules`` copied to the GPU, once."""
    if (scaled, regime) not in _GPU:
        _GPU[scaled, regime] = copy.deepcopy(dm.modules(scaled, regime)[1]).to(DEV)
    return _GPU[scaled, regime]


class _Counting:
    """A stand-in for the loaded library that counts dly_forward / dly_backward calls."""

    def __init__(self, lib):
        self.lib, self.calls = lib, {"dly_forward": 0, "dly_backward": 0}

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
    from pdecontrol.surrogates import delay_hip
    c = _Counting(delay_hip.load())
    monkeypatch.setattr(delay_hip, "load", lambda: c)
    return c.calls


def _plain_notices(caplog):
    return [r for r in caplog.records if "plain PyTorch-ROCm" in r.message]


def _kernels(case, counting, caplog, runs=1):
    """``runs`` rollouts and backwards of ``case`` on the kernels; one dly_forward and one dly_backward each."""
    sur = _gpu(case.scaled, case.regime)
    out = []
    with caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        for i in range(runs):
            out.append(dm.run_case(sur, case, device=DEV))
            torch.cuda.synchronize(DEV)
            assert counting == {"dly_forward": i + 1, "dly_backward": i + 1}, counting
    assert not _plain_notices(caplog)
    return out


def _compare(case, counting, caplog, runs=1):
    """The kernels against fp64 on ``judge``'s bars, the figures recorded first; returns (kernels' results, fp64 result)."""
    ref, yard = dm.reference(case)
    assert counting == {"dly_forward": 0, "dly_backward": 0}, "the references run on the CPU"
    got = _kernels(case, counting, caplog, runs)
    dm.record(case, ref, yard, got[0])
    dm.judge(case.name, got[0], ref, yard)
    return got, ref


@pytest.mark.parametrize("case", dm.COTANGENT_CASES, ids=lambda c: c.name)
def test_one_cotangent_at_a_time(case, counting, caplog):
    got, ref = _compare(case, counting, caplog, runs=2)
    for name in got[0]["grads"]:
        assert np.array_equal(got[0]["grads"][name], got[1]["grads"][name]), f"{name} differs between two runs"
    reached = {n for n, g in ref["grads"].items() if g.any()}
    assert reached, "the loss reaches nothing"
    for name in set(ref["grads"]) - reached:      # the zero rule at its strictest: an all-zero reference admits only zeros
        assert not got[0]["grads"][name].any(), f"{name}: no path from {case.cot}, yet the kernels wrote a gradient"


@pytest.mark.parametrize("case", dm.EDGE_CASES, ids=lambda c: c.name)
def test_edge_shapes(case, counting, caplog):
    got, ref = _compare(case, counting, caplog)
    grads, su = got[0]["grads"], min(case.S, case.K)
    assert grads["input.states"][:, :su].any() and not grads["input.states"][:, su:].any(), "rows su..S of d_states"
    if case.hidden:
        for tag in ("s", "a"):
            assert not grads[f"input.context_{tag}"][:, 0].any(), "slot 0 of the given context never reaches an output"
            assert grads[f"input.context_{tag}"][:, 1:].any()


@pytest.mark.parametrize("case", dm.REGIME_CASES, ids=lambda c: c.name)
def test_operating_points(case, counting, caplog):
    _compare(case, counting, caplog)


@pytest.mark.parametrize("case", dm.BASE_CASES, ids=lambda c: c.name)
def test_base_grid_per_slice(case, counting, caplog):
    _compare(case, counting, caplog)


@pytest.mark.parametrize("K1,given", [(3, False), (4, False), (5, False), (8, False), (4, True)],
                         ids=["K1=3", "K1=4", "K1=5", "K1=8", "K1=4-hidden"])
def test_a_split_rollout_is_the_same_arithmetic(K1, given, counting, caplog):
    """S = 3, K = 9 in one call against K1 steps, then the rest from outputs[:, -1:] and the carried context: bit for bit."""
    sur = _gpu(True)
    st, ac = dm.uniform_inputs(6, 3, 9, 41)
    st, ac = st.float().to(DEV), ac.float().to(DEV)
    hidden = tuple(t.float().to(DEV) for t in dm.context(6, 43)) if given else None
    grid = lambda k: gm.grid(k, "every", sur.delta)
    with torch.no_grad(), caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        whole = sur.rollout(st, ac, *grid(9), hidden=hidden)
        first = sur.rollout(st, ac[:, :K1], *grid(K1), hidden=hidden)
        second = sur.rollout(first.outputs[:, -1:], ac[:, K1:], *grid(9 - K1), hidden=first.hidden)
    torch.cuda.synchronize(DEV)
    assert counting == {"dly_forward": 3, "dly_backward": 0} and not _plain_notices(caplog)
    for name in ("outputs", "deltas", "inlatents", "outlatents"):
        halves = torch.cat((getattr(first, name), getattr(second, name)), dim=1)
        assert torch.equal(halves, getattr(whole, name)), name
    assert torch.equal(second.hidden[0], whole.hidden[0]) and torch.equal(second.hidden[1], whole.hidden[1])
    assert whole.outputs.shape == (6, 9, 1, 64) and torch.isfinite(whole.outputs).all()


def test_ensemble_step_from_a_carried_context_matches_the_cpu(counting, caplog):
    """What WorldVecEnv.step asks of the ensemble: three members, 100 rows, one step from a carried context."""
    from pdecontrol.surrogates.surrogate import PDEEnsemble
    members_cpu = [dm.build(seed=seed, perturb=True)[1] for seed in range(3)]
    members_gpu = [copy.deepcopy(m).to(DEV) for m in members_cpu]
    st, ac = dm.uniform_inputs(100, 1, 1, 17)
    times, targets = torch.zeros(1), torch.full((1,), 0.25)
    hidden = [dm.context(100, 30 + j) for j in range(3)]
    outs = []
    with caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        for members, dev, dtype in ((members_cpu, "cpu", torch.float64), (members_gpu, DEV, torch.float32)):
            ens = PDEEnsemble([m.double() if dtype is torch.float64 else m for m in members], num_elites=3)
            hid = [tuple(t.to(dev, dtype) for t in h) for h in hidden]
            torch.manual_seed(5)
            np.random.seed(5)
            with torch.no_grad():
                outs.append(ens.rollout(st.to(dev, dtype), ac.to(dev, dtype), times, targets, hidden=hid))
    torch.cuda.synchronize(DEV)
    assert counting == {"dly_forward": 3, "dly_backward": 0} and not _plain_notices(caplog)
    assert outs[1].outputs.shape == (100, 1, 1, 64)
    gm.assert_close(outs[1].outputs, outs[0].outputs, dm.FWD["rtol"], dm.FWD["atol_scale"], msg="elite choice or member outputs")
    for (s_cpu, a_cpu), (s_gpu, a_gpu), given in zip(outs[0].hidden, outs[1].hidden, hidden):
        assert s_gpu.shape == (100, 3, 8, 8) and a_gpu.shape == (100, 3, 4, 8)
        gm.assert_close(s_gpu, s_cpu, dm.FWD["rtol"], dm.FWD["atol_scale"], msg="carried state context")
        gm.assert_close(a_gpu, a_cpu, dm.FWD["rtol"], dm.FWD["atol_scale"], msg="carried action context")
        assert torch.equal(s_gpu[:, :2].cpu(), given[0][:, 1:].float()), "the two younger given slots move up unchanged"
