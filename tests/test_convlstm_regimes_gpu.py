"""The ConvLSTM surrogate's kernels (csrc/sur_encoder.h, sur_narrow.h, sur_layernorm.h, sur_cell.h, sur_chunk.h, sur_gemm.h
behind ``hipops.fused_rollout``) per cotangent, past the grid limits, at saturation, at small amplitudes and on an offset,
on an MI355X.

tests/test_surrogate_grad_contracts_gpu.py compares these rollouts with the fp64 CPU module in one regime: white-noise
states, weights at initialisation, B <= 5, every returned tensor in the loss at once, one bar per tensor at GRAD_TOL.
Here, with the cases, inputs, operating points and bars of tests/_convlstm_models.py (tests/test_convlstm_regimes_host.py
shows on the CPU that the regimes are reached and measures the fp32 yardstick):

* one cotangent at a time (``_ChunkFn`` does not materialise undefined cotangents, so dd_all, dout_all, dh_all and dc_all
  each have a null branch in chunks_backward_impl, dgrad_scan_kernel and cell_bwd_kernel) and three pairs at S = 2, K = 4,
  ``outputs`` alone also on the ``skip`` grid; each run twice, bit for bit;
* (B, S, K) = (1, 1, 1), (3, 6, 4), (3, 3, 3), (2, 1, 6), (4, 2, 3), (7, 3, 5), each with a given (H, C) and with the
  trainable H0 / C0: rows min(S, K)..S of d states and d h_in (d H0) exactly zero, rows 0..min(S, K) and d c_in (d C0) not;
* more (step, sample) pairs than workgroups: B = 513, S = K = 2 under no_grad (1026 pairs > the 1024 workgroups of
  enc_fwd_kernel and dec_fwd_kernel); B = 193, S = K = 4 with backward at N = 64 and N = 256 (772 pairs > ENCODER_ROWS = 768
  and > CHUNK_ROWS = 384), and the N = 64 one again with SUR_ACCUMULATE_IN_ROWS=1, on the bars;
* the ``saturated`` operating point (30 % of the gates within 1e-3 of 0 or 1, 26 % in [0.1, 0.9]) at (6, 3, 5), scaled and
  unscaled, N = 64 and 256; smooth states of amplitude 1e-3 and 1e-4 (every row of the first LayerNorm below LN_EPS);
* states ``offset + amp * smooth`` at (4, 0.01) and (8, 0.02), N = 64 and 256 (rows of the state encoder's first LayerNorm
  at mean^2 / var up to 4e7), and every second channel of the decoder's first deconvolution bias moved by 40 (those
  LayerNorm rows at mean^2 / var 7e4 to 4e5);
* three rows of the grid the suite had again, on the tight bars and per slice (the eight gate convolutions and every
  LayerNorm are tensors of their own; each gate convolution per kernel tap, d states and d actions per step);
* exact identities: the no-grad forward (``saved`` null) against the saving one; the first K1 steps of a K = 8 rollout
  against the K1-step rollout; an all-teacher-forced rollout against its two halves with (H, C) carried.

Every rollout is ``hipops.fused_rollout`` once: two encoder launches and one chunk launch forward, one chunk and two
encoder launches backward, no plain-torch notice.  Every case is compared with the same module as ``deepcopy(...).double()``
on the CPU.  Bars (``cm.judge``): 8 x the largest error of the fp32 CPU module against fp64 over the case's yardstick
group (measured in the session, never against the kernels), capped at the bars the suite has -- forward rtol 2e-4 and
min(2e-5, 8 YARD_FWD) of the tensor's scale, gradients and slices min(GRAD_TOL, 8 YARD) of the tensor's / the slice's scale,
the decoder bias in front of SiLU + LayerNorm min(2e-3, 8 x its own yardstick); a tensor or slice that is zero in fp64
admits only exact zeros.  When this was written (YARD_FWD / YARD_GRAD / YARD_SLICE / that bias -> bars):

  cotangent + edge + rounds + base   1.2e-6 / 2.6e-5 / 2.6e-5 / 1.3e-4  ->  9.6e-6, 2.0e-4, 2.0e-4, 1.0e-3
  saturated                          7.3e-6 / 8.4e-6 / 8.4e-6 / 3.1e-5  ->  2.0e-5, 6.7e-5, 6.7e-5, 2.5e-4
  small                              7.9e-7 / 2.7e-6 / 2.7e-6 / 2.6e-5  ->  6.3e-6, 2.1e-5, 2.1e-5, 2.1e-4
  offset                             1.0e-4 forward                      ->  8.0e-4 (the one bar above the suite's cap)

In the offset group fp32 torch itself is 1e-4 off forward, so its forward bar is 8 x its own yardstick; its gradients keep
GRAD_TOL per tensor unless fp32 torch itself is above GRAD_TOL / 8 on that tensor in the group, which is then held to 8 x
its OWN yardstick (2e-4 to 1.1e-3; the first encoder convolution, whose weight gradient cancels on a constant background,
0.27).  The one-pass variance these kernels had (var = E[y^2] - mean^2) was 7.6e-3 to 1.5e-2 of scale off on the five offset
cases, 9 to 19 x the bar; with the variance centred (two-pass in sur_layernorm.h, relative to the row's first value in
sur_narrow.h) they are at 3.2e-5 to 1.1e-4, where fp32 torch is.  Every case appends the kernels' and the yardstick's
figures to convlstm_regimes_observed.jsonl next to the gradient parity log (profiles/convlstm_regimes_observed.json is that
file of one run).

Faults emulated in fp32 torch by the host file, the assertion here that fails on each, and whether the grid's bar did:

  (a)  null dc_all read as dh_all          check_grads of ``hidden_h`` alone, ``outlatents`` alone, (deltas, hidden_h) and
                                           (outlatents, outputs): 2 to 2.5 of scale; grid: no null cotangent, passes
  (b)  dgrad_scan carry kept across a      check_grads of every case with S >= 2 (0.2 to 0.6 of scale); the grid's six rows
       forced step                         with S >= 2 fail too
  (c)  forget-gate term with c_k for       check_grads of every case (0.7 to 0.9 of scale on Wxf / Whf); every grid row
       c_(k-1)                             fails too
  (d)  sigmoid slope floored at 1e-3       check_grads of the saturated cases (8e-3 against 6.7e-5); grid: bit-identical
  (e)  1 - tanh(c)^2 floored at 1e-3       check_grads of the saturated cases (d c_in 2.4e-4 against 6.7e-5); grid:
                                           bit-identical
  (f)  one-pass LayerNorm variance         forward bar of all five offset cases (1.0e-2 to 2.1e-2 against 8.0e-4); grid: passes
  (g)  SiLU slope without v (1 - s)        check_grads of the two offset-8 cases (d states 2.7e-3 / 3.4e-3 against its bar
       beyond |v| > 8                      1.1e-3); grid: no |v| > 8, bit-identical.  At the decoder's shift of 40 the term
                                           is below an ulp: there the fault is no fault
  (h)  only the first 1024 / 768 / 384     forward bar of B = 513; check_grads of B = 193 (d states 0.4 of scale; the action
       pairs contributing                  encoder's first weight 1.5); grid: B <= 5, cannot reach it
  (i)  d states written for rows           the exact-zero rule of (3, 6, 4), even at 1e-6 of scale; the grid's two rows with
       >= min(S, K)                        S > K see it from 2e-4 of scale on

Of these (a), (d), (e), (f), (g), (h) and a small (i) pass the grid the suite had; (b), (c) and a large (i) it caught."""
import copy
import logging

import numpy as np
import pytest
import torch

import _convlstm_models as cm
import _grad_contract_models as gm
from test_fclstm_surrogate_gpu import _Counting as _FCCounting, _plain_notices

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FORWARD = {"sur_encoder_forward": 2, "sur_chunk_forward": 1}
BACKWARD = {"sur_chunk_backward": 1, "sur_encoder_backward": 2}
_GPU = {}


def _gpu(N, scaled, regime=None):
    """The fp32 CPU surrogate of ``cm.modules`` copied to the GPU, once."""
    if (N, scaled, regime) not in _GPU:
        _GPU[N, scaled, regime] = copy.deepcopy(cm.modules(N, scaled, regime)[1]).to(DEV)
    return _GPU[N, scaled, regime]


class _Counting(_FCCounting):
    """The loaded library, counting the launches of a rollout and its backward (the block-per-launch encoder backward
    counts as an encoder backward)."""

    def __init__(self, lib):
        self.lib, self.calls = lib, dict.fromkeys((*FORWARD, *BACKWARD, "sur_encoder_backward_multi"), 0)


@pytest.fixture
def counting(monkeypatch):
    """{launch: count} of libsurrogate_hip.so, and the calls of ``hipops.fused_rollout`` under ``fused_rollout``."""
    from pdecontrol.surrogates import hipops
    c = _Counting(hipops.load())
    monkeypatch.setattr(hipops, "load", lambda: c)
    orig = hipops.fused_rollout
    c.calls["fused_rollout"] = 0

    def fused_rollout(*a, **k):
        c.calls["fused_rollout"] += 1
        return orig(*a, **k)
    monkeypatch.setattr(hipops, "fused_rollout", fused_rollout)
    return c.calls


def _launches(calls):
    out = dict(calls)
    out["sur_encoder_backward"] += out.pop("sur_encoder_backward_multi")
    return out


def _expected(rollouts, backwards):
    return {"fused_rollout": rollouts, **{n: c * rollouts for n, c in FORWARD.items()},
            **{n: c * backwards for n, c in BACKWARD.items()}}


def _kernels(case, counting, caplog, runs=1):
    """``runs`` rollouts (and backwards) of ``case`` on the kernels: ``hipops.fused_rollout`` once each, two encoder
    launches and one chunk launch forward, one chunk and two encoder launches backward, no plain-torch notice."""
    sur = _gpu(case.N, case.scaled, case.regime)
    base, out = _launches(counting), []
    with caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        for i in range(runs):
            out.append(cm.run_case(sur, case, device=DEV))
            torch.cuda.synchronize(DEV)
            want = _expected(i + 1, 0 if case.forward_only else i + 1)
            assert {n: c - base[n] for n, c in _launches(counting).items()} == want, (counting, base)
    assert not _plain_notices(caplog)
    return out


def _compare(case, counting, caplog, runs=1):
    """The kernels against fp64 on ``cm.judge``'s bars, the figures recorded first; returns (kernels' results, fp64 result)."""
    ref, yard = cm.reference(case)
    cm.bars(cm.yard_group(case))
    assert not any(counting.values()), "the references run on the CPU"
    got = _kernels(case, counting, caplog, runs)
    cm.record(case, ref, yard, got[0])
    cm.judge(case, got[0], ref)
    return got, ref


@pytest.mark.parametrize("case", cm.COTANGENT_CASES, ids=lambda c: c.name)
def test_one_cotangent_at_a_time(case, counting, caplog):
    got, ref = _compare(case, counting, caplog, runs=2)
    for name in got[0]["grads"]:
        assert np.array_equal(got[0]["grads"][name], got[1]["grads"][name]), f"{name} differs between two runs"
    for name in got[0]["tensors"]:
        assert np.array_equal(got[0]["tensors"][name], got[1]["tensors"][name]), f"{name} differs between two runs"
    assert any(g.any() for g in ref["grads"].values()), "the loss reaches nothing"


@pytest.mark.parametrize("case", cm.EDGE_CASES, ids=lambda c: c.name)
def test_edge_shapes(case, counting, caplog):
    got, _ = _compare(case, counting, caplog)
    grads, su = got[0]["grads"], min(case.S, case.K)
    assert grads["input.states"][:, :su].any() and not grads["input.states"][:, su:].any(), "rows min(S, K)..S of d_states"
    if case.hidden:
        assert not grads["input.h_in"].any(), "the first step is teacher forced: no path from the incoming H"
        assert grads["input.c_in"].any()
    else:
        assert not grads["transition_model.H0"].any() and grads["transition_model.C0"].any()


@pytest.mark.parametrize("case", cm.ROUNDS_CASES, ids=lambda c: c.name)
def test_more_pairs_than_workgroups(case, counting, caplog):
    _compare(case, counting, caplog)


@pytest.mark.parametrize("case", cm.SATURATED_CASES + cm.SMALL_CASES, ids=lambda c: c.name)
def test_operating_points(case, counting, caplog):
    _compare(case, counting, caplog)


@pytest.mark.parametrize("case", cm.OFFSET_CASES, ids=lambda c: c.name)
def test_rows_riding_on_an_offset(case, counting, caplog):
    _compare(case, counting, caplog)


@pytest.mark.parametrize("case", cm.BASE_CASES, ids=lambda c: c.name)
def test_base_grid_per_slice(case, counting, caplog):
    _compare(case, counting, caplog)


def test_accumulators_in_partial_rows_stay_on_the_bars(counting, caplog, monkeypatch):
    """SUR_ACCUMULATE_IN_ROWS=1 (the GL = false instantiations) on the rounds case at N = 64: more (step, sample) pairs than
    workgroups, every workgroup adding several pairs straight into its partial row; held to the same bars against fp64."""
    case = cm.ROUNDS_CASES[1]
    ref, _ = cm.reference(case)
    monkeypatch.setenv("SUR_ACCUMULATE_IN_ROWS", "1")
    got = _kernels(case, counting, caplog)[0]
    cm.judge(case, got, ref, label=case.name + " accumulators in rows")


# ---------------------------------------------------------------------------------------------------------------------
# exact identities
# ---------------------------------------------------------------------------------------------------------------------
def _inputs(B, S, K, seed, N=64, given=True):
    st, ac = cm.noise(B, S, K, N, seed)
    h = tuple(t.float().to(DEV) for t in cm.hidden(B, N, seed + 7)) if given else None
    return st.float().to(DEV), ac.float().to(DEV), h


def _same(a, b, names):
    for n in names:
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize("N,B,S,K,given", [(64, 5, 2, 4, True), (256, 3, 6, 4, False)])
def test_the_forward_that_saves_nothing_is_the_saving_forward(N, B, S, K, given, counting, caplog):
    """``saved`` null (no-grad) against the forward that writes the record: every returned tensor bit for bit."""
    sur = _gpu(N, True)
    st, ac, h = _inputs(B, S, K, 51, N, given)
    grid = gm.grid(K, "every", sur.delta)
    with caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        with torch.no_grad():
            plain = cm.rollout_tensors(sur.rollout(st, ac, *grid, hidden=h))
        saving = cm.rollout_tensors(sur.rollout(st.clone().requires_grad_(True), ac.clone().requires_grad_(True), *grid, hidden=h))
    torch.cuda.synchronize(DEV)
    assert _launches(counting) == _expected(2, 0) and not _plain_notices(caplog)
    assert saving["outputs"].grad_fn is not None and plain["outputs"].grad_fn is None
    _same(plain, saving, cm.TENSORS)


@pytest.mark.parametrize("K1", [1, 3, 4])
def test_the_first_steps_of_a_rollout_are_the_shorter_rollout(K1, counting, caplog):
    """S = 2, K = 8 against K1 steps from the same inputs: the first K1 reported steps bit for bit."""
    sur = _gpu(64, True)
    st, ac, h = _inputs(6, 2, 8, 55)
    with torch.no_grad(), caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        whole = cm.rollout_tensors(sur.rollout(st, ac, *gm.grid(8, "every", sur.delta), hidden=h))
        short = cm.rollout_tensors(sur.rollout(st, ac[:, :K1], *gm.grid(K1, "every", sur.delta), hidden=h))
    torch.cuda.synchronize(DEV)
    assert _launches(counting) == _expected(2, 0) and not _plain_notices(caplog)
    for n in ("outputs", "deltas", "outlatents"):
        assert short[n].shape[1] == K1 and torch.equal(whole[n][:, :K1], short[n]), n
    assert whole["outputs"].shape == (6, 8, 1, 64) and torch.isfinite(whole["outputs"]).all()


def test_a_teacher_forced_rollout_is_its_two_halves(counting, caplog):
    """S = K = 6, every step teacher forced, in one call against steps 0..2, then steps 3..5 from states[:, 3:] with the
    first call's (H, C) carried: outputs, deltas, latents and the final hidden state bit for bit."""
    sur = _gpu(64, True)
    st, ac, h = _inputs(6, 6, 6, 57)
    grid = lambda k: gm.grid(k, "every", sur.delta)
    with torch.no_grad(), caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        whole = sur.rollout(st, ac, *grid(6), hidden=h)
        first = sur.rollout(st[:, :3], ac[:, :3], *grid(3), hidden=h)
        second = sur.rollout(st[:, 3:], ac[:, 3:], *grid(3), hidden=first.hidden)
    torch.cuda.synchronize(DEV)
    assert _launches(counting) == _expected(3, 0) and not _plain_notices(caplog)
    for name in ("outputs", "deltas", "outlatents"):
        assert torch.equal(torch.cat((getattr(first, name), getattr(second, name)), dim=1), getattr(whole, name)), name
    assert torch.equal(second.hidden[0], whole.hidden[0]) and torch.equal(second.hidden[1], whole.hidden[1])
    assert not torch.equal(first.hidden[1], h[1]) and whole.outputs.shape == (6, 6, 1, 64)
