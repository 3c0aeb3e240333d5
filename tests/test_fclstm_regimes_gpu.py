"""csrc/sur_fclstm.hip (sur_fc_forward, sur_fc_backward) per cotangent, per gate quarter and at saturation, on an MI355X.

tests/test_fclstm_surrogate_gpu.py compares the FC-LSTM rollouts with the fp64 CPU module on one grid: every returned
tensor in the loss at once, weights at initialisation, white-noise states, one bar per tensor at GRAD_TOL -- about 140
times what the kernels were measured at.  Here, with the cases, inputs, operating points and bars of
tests/_fclstm_models.py (tests/test_fclstm_regimes_host.py shows on the CPU that the regimes are reached and measures
the fp32 yardstick), for both factories:

* one cotangent at a time (``_FCRolloutFn`` does not materialise undefined cotangents, so each of d_out, d_del, d_inl,
  d_outl, d_h_out, d_c_out has a null branch in fc_bwd_kernel) and three pairs at S = 2, K = 4 -- a cotangent on a given
  step at k = 0, on a given step at k > 0 and on free-running steps -- each run twice bit for bit; a gradient the loss
  does not reach is exactly zero;
* (B, S, K) = (3, 6, 4), (3, 3, 1), (3, 1, 2), (3, 2, 2), (4, 2, 3), (5, 1, 1), each with and without a given (H, C): rows
  su..S of d_states and d_h_in exactly zero, rows 0..su and d_c_in not;
* the ``saturated`` and ``deep`` operating points at (7, 3, 6), scaled and unscaled, and smooth states of amplitude 1e-3 and
  1e-4 at (6, 3, 5) with the first encoder bias zeroed;
* three rows of the base grid again (K = 10 cut to 8), on the tight bars and per slice;
* exact identities: bias_ih_l0.grad and bias_hh_l0.grad bit-equal in every case; the no-grad forward (``saved`` null)
  against the saving one; the autoregressive rollout with the re-encoding off (``inlatents`` null); the first K1 steps
  of a K = 8 rollout against the K1-step rollout; an all-teacher-forced autoregressive rollout against its two halves
  with (H, C) carried.

Every case is compared with the same module as ``deepcopy(...).double()`` on the CPU.  Bars (``_fclstm_models.judge``):
8 x the largest error of the fp32 CPU module against fp64 over ALL cases of this file (YARD_FWD, YARD_GRAD, YARD_SLICE;
measured in the session, never against the kernels), capped at the bars the suite had -- forward rtol 2e-4 and
min(2e-5, 8 YARD_FWD) of the tensor's scale; every gradient within min(GRAD_TOL, 8 YARD_GRAD) of the tensor's scale
(``check_grads``); every slice -- the four LSTM parameters per gate quarter, the inputs per step, the first encoder weight
per block of 16 columns -- within min(GRAD_TOL, 8 YARD_SLICE) of the SLICE's scale; a tensor or slice that is zero in fp64
admits only exact zeros.  When this was written: 1.4e-5, 1.0e-5 and 2.2e-5.  Every case appends the kernels' and the
yardstick's figures to fclstm_regimes_observed.jsonl next to the gradient parity log
(profiles/fclstm_regimes_observed.json is that file of one run).

Faults emulated in fp32 torch by the host file, the assertion here that fails on each, and whether the grid's bar did:

  (a)  null d_c_out read as d_h_out        check_grads of ``hidden_h`` alone and (deltas, hidden_h); grid: no null cotangent
  (b)  free-running d_inl dropped, latent  check_grads of ``inlatents`` alone and (inlatents, outlatents); the grid's rows
                                           with K > S fail too (inlatents is in its loss)
  (c)  forget-gate term with c' for c      check_grads (0.08 to 0.17 of a tensor's scale), the f-quarter slice bar by 3 to
                                           10 times more; GRAD_TOL on the whole tensor sees it: every grid row fails
  (d)  sigmoid slope floored at 1e-3       check_grads of the four saturated cases (2e-3 to 4e-3); grid: bit-identical
  (d') 1 - tanh(c)^2 floored at 1e-3       NOT separable: 7.8e-6 of scale at the saturated point against a bar of 1.0e-5
  (e)  last_slope as 1 - |y|, autoreg      check_grads of every case, the grid's too
  (f)  ELU slope floored at 1e-3, latent   check_grads of the two latent deep cases (7e-4 to 8e-4); grid: passes
  (f') exp(x) - 1 for expm1, latent        check_grads of the latent small cases: 2.3e-5 at amplitude 1e-3 (the tight bar
                                           only), 2.8e-4 at 1e-4; grid: passes
  (g)  states indexed with stride su       forward bar of the edge cases (3, 6, 4), (3, 3, 1); the grid's row (5, 6, 4) too
  (h)  g carried across a given step       check_grads of ``outputs`` alone and (outputs, hidden_c); the grid's rows with
                                           S >= 2 fail too

Of these (a), (d), (f) and (f') pass the grid the suite had; (b), (c), (e), (g) and (h) it caught already."""
import copy
import logging

import numpy as np
import pytest
import torch

import _fclstm_models as fm
import _grad_contract_models as gm
from test_fclstm_surrogate_gpu import _Counting, _plain_notices  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
LAUNCHES = ("sur_fc_forward", "sur_fc_backward")
_GPU = {}


def _gpu(factory, scaled, regime=None):
    """The fp32 CPU surrogate of ``fm.modules`` copied to the GPU, once."""
    if (factory, scaled, regime) not in _GPU:
        _GPU[factory, scaled, regime] = copy.deepcopy(fm.modules(factory, scaled, regime)[1]).to(DEV)
    return _GPU[factory, scaled, regime]


@pytest.fixture(autouse=True)
def _switch_on():
    from pdecontrol.surrogates import ops
    with ops.fused_fc(True):
        yield


@pytest.fixture
def counting(monkeypatch):
    from pdecontrol.surrogates import fclstm_hip
    c = _Counting(fclstm_hip.load())
    monkeypatch.setattr(fclstm_hip, "load", lambda: c)
    return c.calls


def _kernels(case, counting, caplog, runs=1):
    """``runs`` rollouts and backwards of ``case`` on the kernels; one sur_fc_forward and one sur_fc_backward each."""
    sur = _gpu(case.factory, case.scaled, case.regime)
    out = []
    with caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        for i in range(runs):
            out.append(fm.run_case(sur, case, device=DEV))
            torch.cuda.synchronize(DEV)
            assert counting == dict.fromkeys(LAUNCHES, i + 1), counting
    assert not _plain_notices(caplog)
    return out


def _compare(case, counting, caplog, runs=1):
    """The kernels against fp64 on ``fm.judge``'s bars, the figures recorded first; returns (kernels' results, fp64 result)."""
    ref, yard = fm.reference(case)
    fm.bars()
    assert counting == dict.fromkeys(LAUNCHES, 0), "the references run on the CPU"
    got = _kernels(case, counting, caplog, runs)
    fm.record(case, ref, yard, got[0])
    fm.judge(case.name, got[0], ref)
    ih, hh = (got[0]["grads"][fm.LSTM + n] for n in ("bias_ih_l0", "bias_hh_l0"))
    assert np.array_equal(ih, hh), "both biases sum row W_P3 in the same order"
    return got, ref


@pytest.mark.parametrize("case", fm.COTANGENT_CASES, ids=lambda c: c.name)
def test_one_cotangent_at_a_time(case, counting, caplog):
    got, ref = _compare(case, counting, caplog, runs=2)
    for name in got[0]["grads"]:
        assert np.array_equal(got[0]["grads"][name], got[1]["grads"][name]), f"{name} differs between two runs"
    assert any(g.any() for g in ref["grads"].values()), "the loss reaches nothing"


@pytest.mark.parametrize("case", fm.EDGE_CASES, ids=lambda c: c.name)
def test_edge_shapes(case, counting, caplog):
    got, _ = _compare(case, counting, caplog)
    grads, su = got[0]["grads"], min(case.S, case.K)
    assert grads["input.states"][:, :su].any() and not grads["input.states"][:, su:].any(), "rows su..S of d_states"
    if case.hidden:
        assert not grads["input.h_in"].any(), "the first step is teacher forced: no path from the incoming H"
        assert grads["input.c_in"].any()


@pytest.mark.parametrize("case", fm.REGIME_CASES + fm.SMALL_CASES, ids=lambda c: c.name)
def test_operating_points(case, counting, caplog):
    _compare(case, counting, caplog)


@pytest.mark.parametrize("case", fm.BASE_CASES, ids=lambda c: c.name)
def test_base_grid_per_slice(case, counting, caplog):
    _compare(case, counting, caplog)


# ---------------------------------------------------------------------------------------------------------------------
# exact identities
# ---------------------------------------------------------------------------------------------------------------------
def _inputs(B, S, K, seed, given=True):
    import _delay_models as dm
    st, ac = dm.uniform_inputs(B, S, K, seed)
    h = tuple(t.float().to(DEV) for t in fm.hidden(B, seed + 7)) if given else None
    return st.float().to(DEV), ac.float().to(DEV), h


def _same(a, b, names):
    for n in names:
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize("factory", fm.FACTORIES)
@pytest.mark.parametrize("B,S,K,given", [(5, 2, 4, True), (3, 6, 4, False)])
def test_the_forward_that_saves_nothing_is_the_saving_forward(factory, B, S, K, given, counting, caplog):
    """``saved`` null (no-grad) against the forward that writes the record: every returned tensor bit for bit."""
    sur = _gpu(factory, True)
    st, ac, h = _inputs(B, S, K, 51, given)
    grid = gm.grid(K, "every", sur.delta)
    with caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        with torch.no_grad():
            plain = fm.rollout_tensors(sur.rollout(st, ac, *grid, hidden=h))
        saving = fm.rollout_tensors(sur.rollout(st.clone().requires_grad_(True), ac, *grid, hidden=h))
    torch.cuda.synchronize(DEV)
    assert counting == {"sur_fc_forward": 2, "sur_fc_backward": 0} and not _plain_notices(caplog)
    assert saving["outputs"].grad_fn is not None and plain["outputs"].grad_fn is None
    assert set(plain) == set(saving) == set(fm.TENSORS)
    _same(plain, saving, fm.TENSORS)


def test_the_autoregressive_rollout_without_the_reencoding_is_the_same_arithmetic(counting, caplog):
    """``inlatents`` null against re-encoding on: outputs, deltas, outlatents and the hidden state bit for bit."""
    sur = _gpu(fm.AUTOREG, True)
    off = copy.deepcopy(sur)
    off.reencode_predictions = False
    st, ac, h = _inputs(5, 2, 6, 53)
    grid = gm.grid(6, "every", sur.delta)
    with torch.no_grad(), caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        a, b = sur.rollout(st, ac, *grid, hidden=h), off.rollout(st, ac, *grid, hidden=h)
    torch.cuda.synchronize(DEV)
    assert counting == {"sur_fc_forward": 2, "sur_fc_backward": 0} and not _plain_notices(caplog)
    assert a.inlatents is not None and b.inlatents is None
    _same(fm.rollout_tensors(a), fm.rollout_tensors(b), ("outputs", "deltas", "outlatents", "hidden_h", "hidden_c"))


@pytest.mark.parametrize("factory", fm.FACTORIES)
@pytest.mark.parametrize("K1", [1, 3, 4])
def test_the_first_steps_of_a_rollout_are_the_shorter_rollout(factory, K1, counting, caplog):
    """S = 2, K = 8 against K1 steps from the same inputs: the first K1 reported steps bit for bit."""
    sur = _gpu(factory, True)
    st, ac, h = _inputs(6, 2, 8, 55)
    with torch.no_grad(), caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        whole = fm.rollout_tensors(sur.rollout(st, ac, *gm.grid(8, "every", sur.delta), hidden=h))
        short = fm.rollout_tensors(sur.rollout(st, ac[:, :K1], *gm.grid(K1, "every", sur.delta), hidden=h))
    torch.cuda.synchronize(DEV)
    assert counting == {"sur_fc_forward": 2, "sur_fc_backward": 0} and not _plain_notices(caplog)
    for n in ("outputs", "deltas", "inlatents", "outlatents"):
        assert short[n].shape[1] == K1 and torch.equal(whole[n][:, :K1], short[n]), n
    assert whole["outputs"].shape == (6, 8, 1, 64) and torch.isfinite(whole["outputs"]).all()


def test_a_teacher_forced_autoregressive_rollout_is_its_two_halves(counting, caplog):
    """S = K = 6, every step teacher forced, in one call against steps 0..2, then steps 3..5 from states[:, 3:] with the
    first call's (H, C) carried: outputs, deltas, latents and the final hidden state bit for bit (c_in, h_out, c_out).
    The latent form restarts its running latent from the first given state, so it has no such split."""
    sur = _gpu(fm.AUTOREG, True)
    st, ac, h = _inputs(6, 6, 6, 57)
    grid = lambda k: gm.grid(k, "every", sur.delta)
    with torch.no_grad(), caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        whole = sur.rollout(st, ac, *grid(6), hidden=h)
        first = sur.rollout(st[:, :3], ac[:, :3], *grid(3), hidden=h)
        second = sur.rollout(st[:, 3:], ac[:, 3:], *grid(3), hidden=first.hidden)
    torch.cuda.synchronize(DEV)
    assert counting == {"sur_fc_forward": 3, "sur_fc_backward": 0} and not _plain_notices(caplog)
    for name in ("outputs", "deltas", "inlatents", "outlatents"):
        assert torch.equal(torch.cat((getattr(first, name), getattr(second, name)), dim=1), getattr(whole, name)), name
    assert torch.equal(second.hidden[0], whole.hidden[0]) and torch.equal(second.hidden[1], whole.hidden[1])
    assert not torch.equal(first.hidden[1], h[1]) and whole.outputs.shape == (6, 6, 1, 64)
