"""The operating points, bars and mutations behind tests/test_delay_regimes_gpu.py, on the CPU only.

Three things are shown here, on the exact modules and inputs of the GPU file (tests/_delay_models.py holds both):

* every case reaches its regime on the fp64 module: the ``saturated`` point puts a share of ``outlatents`` and ``deltas``
  within 1e-3 of +-1 and leaves another share below 0.9, ``elu_deep`` puts ELU pre-activations below -5, ``small_states``
  puts the first encoder LayerNorm's variance below its eps;
* what fp32 PyTorch on the CPU loses against fp64 on every case, per tensor and per slice: the yardstick the GPU file
  takes its per-slice bars from (``_delay_models.bars``), written to delay_regimes_observed.jsonl;
* six faults a kernel could have, emulated in fp32 torch (a functional re-spelling of the one layer each touches, or of
  the one index it gets wrong), fail a named assertion of the new cases and none of the nine-case grid
  tests/test_delay_surrogate_gpu.py had before.  Nothing here runs a kernel: (d), (e) and (f) are faults of the kernel's
  indexing, emulated by what they would make it read or return."""
import copy
import os

import numpy as np
import pytest
import torch

import _delay_models as dm
from conftest import GRAD_TOL

ALL_NEW = dm.COTANGENT_CASES + dm.EDGE_CASES + dm.REGIME_CASES + dm.BASE_CASES
OLD_GRID = dm.GRID_CASES[:9]
_ref = dm.reference


def _share(a, cond):
    return float(np.mean(cond(np.abs(a))))


# ---------------------------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in dm.REGIME_CASES if c.regime == "saturated"], ids=lambda c: c.name)
def test_saturated_point_reaches_both_ends_of_the_tanh_slope(case):
    t = _ref(case)[0]["tensors"]
    assert _share(t["outlatents"], lambda y: y > 0.999) >= 0.10
    assert _share(t["deltas"], lambda y: y > 0.999) >= 0.10
    assert _share(t["outlatents"], lambda y: y < 0.9) >= 0.25


def test_the_grid_the_regimes_were_added_to_never_saturates():
    """The gap this file closes: at initialisation no tanh output of the old grid comes within 1e-3 of +-1."""
    for case in OLD_GRID[:3]:
        t = _ref(case)[0]["tensors"]
        assert _share(t["outlatents"], lambda y: y > 0.999) == 0 and _share(t["deltas"], lambda y: y > 0.999) == 0


def test_elu_deep_point_reaches_the_flat_end_of_the_elu():
    case = next(c for c in dm.REGIME_CASES if c.regime == "elu_deep")
    ref, _ = dm.modules(case.scaled, case.regime)
    pre = dm.elu_preactivations(ref, lambda: dm.run_case(ref, case, dtype=torch.float64))
    assert float((pre < -5).double().mean()) >= 0.05
    assert float((pre > 0).double().mean()) >= 0.25


def _first_layernorm_var_over_eps(states):
    ref, _ = dm.modules(True)
    ln = ref.state_encoder.model.block_l0.conv3x3_l1_norm
    seen = []
    hook = ln.register_forward_hook(lambda m, i, o: seen.append(i[0].detach()))
    try:
        with torch.no_grad():
            ref.state_encoder(states)
    finally:
        hook.remove()
    return (torch.cat([s.reshape(-1, s.shape[-1]) for s in seen]).var(dim=-1, unbiased=False) / ln.eps).numpy()


def test_small_states_put_the_first_layernorm_below_its_eps():
    small = next(c for c in dm.REGIME_CASES if c.states and c.states[0] == 1e-3)
    ratio = _first_layernorm_var_over_eps(small.inputs()[0])
    assert ratio.shape == (small.B * small.S,) and ratio.max() < 0.1, ratio.max()
    assert _first_layernorm_var_over_eps(dm.small_states(7, 3, 1e-3, small.seed)).max() < 0.1
    assert _first_layernorm_var_over_eps(dm.small_states(7, 3, 1.0, small.seed)).min() > 10


def test_small_states_are_smooth_fields_about_zero():
    s = dm.small_states(4, 2, 1e-2, 3)
    assert s.shape == (4, 2, 1, 64) and s.dtype == torch.float64
    assert float(s.mean(dim=-1).abs().max()) < 1e-17 and 0.5e-2 < float(s.abs().max()) <= 1.5e-2
    assert not torch.equal(s[0, 0], s[1, 0]) and torch.equal(s, dm.small_states(4, 2, 1e-2, 3))


# ---------------------------------------------------------------------------------------------------------------------
# slices and the yardstick
# ---------------------------------------------------------------------------------------------------------------------
def test_grad_slices_cover_every_element_once():
    grads = _ref(dm.EDGE_CASES[0])[0]["grads"]
    many = {"input.states": 6, "input.actions": 4, "input.context_s": 3, "input.context_a": 3, dm.MLP0: 6}
    for name, g in grads.items():
        count = np.zeros(g.shape, dtype=int)
        slices = dm.grad_slices(name, g)
        for _, idx in slices:
            count[idx] += 1
        assert (count == 1).all(), name
        assert len(slices) == many.get(name, 1), name
    w = dm.grad_slices(dm.MLP0, grads[dm.MLP0])
    assert [g for g, _ in w] == ["slot0.state", "slot0.action", "slot1.state", "slot1.action", "slot2.state", "slot2.action"]
    assert grads[dm.MLP0][w[3][1]].shape == (96, 32) and w[3][1][1] == slice(160, 192)


def test_check_slices_sees_what_the_tensor_bar_does_not():
    """A whole step of d_states off by 0.1 % sits under GRAD_TOL of the tensor's scale when the step is a tenth of the
    tensor's maximum; the slice bar catches it.  A zero slice that is written to fails the zero rule."""
    ref = {"input.states": np.zeros((2, 3, 1, 64)), "input.context_s": np.ones((2, 3, 8, 8))}
    ref["input.states"][:, 0], ref["input.states"][:, 1] = 1.0, 0.1
    ref["input.context_s"][:, 0] = 0.0
    got = copy.deepcopy(ref)
    assert dm.check_slices("exact", got, ref, GRAD_TOL) == (0.0, None)
    got["input.states"][:, 1] *= 1.001
    assert dm.tensor_errors(got, ref)["input.states"] < GRAD_TOL
    with pytest.raises(AssertionError, match=r"input.states\[step1\] off by 1.0"):
        dm.check_slices("one step off", got, ref, GRAD_TOL)
    got = copy.deepcopy(ref)
    got["input.states"][0, 2, 0, 5] = 1e-3           # a row su..S that is written to
    with pytest.raises(AssertionError, match=r"input.states\[step2\] is zero in fp64"):
        dm.check_slices("stray", got, ref, GRAD_TOL)
    got = copy.deepcopy(ref)
    got["input.context_s"][1, 0, 3, 3] = 1e-3
    with pytest.raises(AssertionError, match=r"input.context_s\[slot0\] is zero in fp64"):
        dm.check_slices("stray", got, ref, GRAD_TOL)
    with pytest.raises(AssertionError):
        dm.check_slices("missing", {"input.states": ref["input.states"]}, ref, GRAD_TOL)


def test_slices_sit_well_below_their_tensors_maximum():
    """Why the per-tensor bar is not enough: whole steps, slots and column blocks of these gradients sit about a factor
    of ten below their tensor's maximum."""
    smallest = 1.0
    for case in dm.BASE_CASES + dm.REGIME_CASES[:1]:
        grads = _ref(case)[0]["grads"]
        for name, g in grads.items():
            for _, idx in dm.grad_slices(name, g):
                if np.any(g[idx]):
                    smallest = min(smallest, float(np.abs(g[idx]).max() / np.abs(g).max()))
    assert smallest < 0.2, smallest


def _bounded(case):
    """The cases whose fp32 yardstick is asserted below GRAD_TOL / 4: the base grid's three, ``saturated``, S > K, K = 2,
    K = 1 from three states and K = 20."""
    return (case.group in ("base", "edge") or case.regime == "saturated"
            or (case.group == "grid" and (case.S > case.K or case.K in (2, 20))))


@pytest.mark.parametrize("case", ALL_NEW + dm.GRID_CASES, ids=lambda c: c.name)
def test_fp32_cpu_yardstick(case):
    """fp32 PyTorch on the CPU against fp64, per tensor and per slice, recorded for every GPU case.  On the base grid's
    three cases, at the ``saturated`` point, for S > K, K = 2 and K = 20 it stays below GRAD_TOL / 4 per tensor (measured:
    at most 2.1e-5, always a decoder bias in front of a LayerNorm or a first-block encoder weight), so the per-tensor
    bar of those cases is GRAD_TOL itself.  The others are recorded, not bounded -- their bars are whatever ``bars``
    makes of these figures: ``elu_deep`` 3.8e-5, the deltas-only loss 4.4e-5 (the scalar skip weight of the first
    encoder block), the small-amplitude states 0.7e-5 to 1.7e-5 at these phases and offsets."""
    ref, yard = _ref(case)
    rec = dm.record(case, ref, yard)
    tbar, sbar = dm.bars(yard["grads"], ref["grads"], GRAD_TOL)
    assert set(tbar) == set(sbar) == set(ref["grads"])
    assert rec["forward_err_of_scale"]["fp32_cpu"] < dm.FWD["atol_scale"]
    if _bounded(case):
        assert rec["gradient_err_of_scale"]["fp32_cpu"]["err"] < GRAD_TOL / 4, rec
        assert all(b == GRAD_TOL for b in tbar.values())
    dm.judge(case.name + " fp32 cpu", yard, ref, yard)      # the yardstick passes its own bars


def test_zero_rule_cases_have_the_zero_slices_they_are_there_for():
    by = {c.cot: _ref(c)[0]["grads"] for c in dm.COTANGENT_CASES}
    assert not by[("context_a",)]["input.states"].any() and not by[("context_a",)]["input.context_s"].any()
    assert not by[("context_a",)]["input.actions"][:, 0].any() and by[("context_a",)]["input.actions"][:, 1].any()
    assert not any(g.any() for n, g in by[("inlatents",)].items() if n.startswith(("action_encoder", "state_decoder")))
    assert by[("inlatents",)]["input.states"].any()
    edge = _ref(dm.EDGE_CASES[0])[0]["grads"]
    assert edge["input.states"][:, :4].any() and not edge["input.states"][:, 4:].any()
    assert not edge["input.context_s"][:, 0].any() and edge["input.context_s"][:, 1].any()


# ---------------------------------------------------------------------------------------------------------------------
# mutations
# ---------------------------------------------------------------------------------------------------------------------
# (b) exp(x) - 1 for expm1f, (b') the ELU slope floored at 1e-3, (c) the tanh slope as 1 - |y|, (c') the tanh slope floored
# at 1e-3: the emulations tests/test_fclstm_regimes_host.py shares (tests/_delay_models.py)
_EluByExp, _EluFlooredSlope, _TanhAbsSlope, _TanhFlooredSlope = dm.EluByExp, dm.EluFlooredSlope, dm.TanhAbsSlope, dm.TanhFlooredSlope
_swap = dm.swap_activation


def _layernorm_eps(sur, eps):
    for m in sur.modules():
        if isinstance(m, torch.nn.LayerNorm):
            m.eps = eps
    return sur


def _stride_su(case):
    """(d): what a forward that indexes the given states with stride su = min(S, K) reads."""
    st, ac, h = case.inputs()
    su, flat = min(case.S, case.K), st.reshape(case.B * case.S, 1, 64)
    read = st.clone()
    for b in range(case.B):
        for k in range(su):
            read[b, k] = flat[b * su + k]
    return read, ac, h


def _null_context_reads_outputs(case):
    """(e): a backward that reads the d_outputs buffer where d_ctx_s_out is null: the loss gains <context_s, the first
    192 values per sample offset b * 192 of d_outputs>.  It needs d_outputs itself: a null one is no buffer to read."""
    if "context_s" in case.cot or "outputs" not in case.cot or case.K < 3:
        return None
    import _grad_contract_models as gm

    def loss_of(tensors, weights):
        stray = weights["outputs"].reshape(-1)[:case.B * 192].reshape(case.B, 3, 8, 8)
        return gm.weighted_loss({**{n: tensors[n] for n in case.cot}, "stray": tensors["context_s"]},
                                {**weights, "stray": stray})
    return loss_of


def _ring_slots_unrotated(case):
    """(f): a K = 2 final context read from ring slots i where it sits in (K + i) % 3: slot i returns slot (i - K) % 3."""
    def tensors_of(ro):
        t = dm.rollout_tensors(ro)
        order = [(i - case.K) % 3 for i in range(3)]
        t["context_s"], t["context_a"] = t["context_s"][:, order], t["context_a"][:, order]
        return t
    return tensors_of if case.K == 2 else dm.rollout_tensors


MUTATIONS = ("a_eps_dropped", "a_eps_1e-6", "b_exp_minus_1", "b_elu_floored_slope", "c_tanh_abs_slope", "c_tanh_floored_slope", "d_stride_su", "e_null_ctx_reads_outputs",
             "f_k2_ring_unrotated")


def mutated(name, case):
    """The fp32 CPU module's result on ``case`` with fault ``name``."""
    sur = copy.deepcopy(dm.modules(case.scaled, case.regime)[1])
    kw = {}
    if name == "a_eps_dropped":
        _layernorm_eps(sur, 0.0)
    elif name == "a_eps_1e-6":
        _layernorm_eps(sur, 1e-6)
    elif name == "b_elu_floored_slope":
        _swap(sur, torch.nn.ELU, _EluFlooredSlope)
    elif name == "b_exp_minus_1":
        _swap(sur, torch.nn.ELU, _EluByExp)
    elif name == "c_tanh_abs_slope":
        _swap(sur, torch.nn.Tanh, _TanhAbsSlope)
    elif name == "c_tanh_floored_slope":
        _swap(sur, torch.nn.Tanh, _TanhFlooredSlope)
    elif name == "d_stride_su":
        kw["inputs"] = _stride_su(case)
    elif name == "e_null_ctx_reads_outputs":
        kw["loss_of"] = _null_context_reads_outputs(case)
    elif name == "f_k2_ring_unrotated":
        kw["tensors_of"] = _ring_slots_unrotated(case)
    else:
        raise ValueError(name)
    return dm.run_case(sur, case, **kw)


def _failed(case, got):
    """None, or which of ``judge``'s assertions ``got`` fails first on ``case``: "forward", "check_grads", "check_slices"."""
    import conftest
    ref, yard = _ref(case)
    log, conftest.GRAD_LOG = conftest.GRAD_LOG, os.devnull       # an emulated fault is no observation of the project's
    try:
        dm.judge(case.name + " emulated fault", got, ref, yard)
    except AssertionError as e:
        text = str(e)
        if "Not equal to tolerance" in text:
            return "forward"
        return "check_slices" if ("of the slice's scale" in text or "is zero in fp64" in text) else "check_grads"
    finally:
        conftest.GRAD_LOG = log
    return None


def _failed_old(case, got):
    """The same for the assertions the grid had before: forward bar and ``check_grads`` at GRAD_TOL, no slices."""
    kind = _failed(case, got)
    return None if kind == "check_slices" else kind


def _same(a, b):
    return all(np.array_equal(a[k][n], b[k][n]) for k in ("tensors", "grads") for n in a[k])


_MUTATED = {}


def _mutated(name, case):
    if (name, case.name) not in _MUTATED:
        _MUTATED[name, case.name] = mutated(name, case)
    return _MUTATED[name, case.name]


def _case(cases, **want):
    found = [c for c in cases if all(getattr(c, k) == v for k, v in want.items())]
    assert len(found) == 1, (want, [c.name for c in found])
    return found[0]


@pytest.mark.parametrize("name", ["a_eps_dropped", "a_eps_1e-6"])
def test_a_layernorm_eps_fails_the_forward_bar_by_orders_of_magnitude_below_eps(name):
    """(a) LayerNorm with eps dropped or 1e-6.  New assertion: the forward bar of the small-amplitude cases, where the
    first LayerNorm's variance is below eps and 1/sqrt(var + eps) is off by a factor, not by parts in 1e4: the error is
    above 500 x the bar's floor.  The grid had this one already: its forward bar fails too (the decoder's LayerNorms see
    rows of small variance at initialisation), by less than 50 x the floor -- the issue's expectation that a wrong eps
    would pass the nine cases does not hold, and this test says so."""
    for case in (c for c in dm.REGIME_CASES if c.group == "small"):
        got, ref = _mutated(name, case), _ref(case)[0]
        assert _failed(case, got) == "forward", case.name
        err = max(dm.scale_error(got["tensors"][n], ref["tensors"][n]) for n in dm.TENSORS)
        print(name, case.name, "forward error of scale", err)
        assert err > 500 * dm.FWD["atol_scale"], (case.name, err)
    worst = 0.0
    for case in OLD_GRID[:3]:
        got, ref = _mutated(name, case), _ref(case)[0]
        worst = max(worst, max(dm.scale_error(got["tensors"][n], ref["tensors"][n]) for n in dm.TENSORS))
    print(name, "old grid forward error of scale", worst)
    assert any(_failed_old(c, _mutated(name, c)) == "forward" for c in OLD_GRID[:3])
    assert worst < 50 * dm.FWD["atol_scale"], worst


def test_b_exp_minus_one_fails_check_grads_at_amplitude_1e_4_only():
    """(b) exp(x) - 1 rounded in fp32 in place of expm1.  New assertion: ``check_grads`` of the amp 1e-4 case, on the
    first encoder LayerNorm's gain (1.7e-3 of its scale against a bar of 2e-4; fp32 torch: 7e-6): the pre-activations
    are about 1e-4, exp(x) - 1 is off by up to 6e-8 of them, and the LayerNorm below its eps multiplies what is left by
    316.  At amp 1e-3 the same fault reaches 1.6e-4 and passes, which is why the 1e-4 case exists.  The nine grid cases
    pass (at most 2.3e-5)."""
    case = _case(dm.REGIME_CASES, states=(1e-4, 0.0))
    assert _failed(case, _mutated("b_exp_minus_1", case)) == "check_grads"
    for old in OLD_GRID:
        assert _failed_old(old, _mutated("b_exp_minus_1", old)) is None, old.name


def test_b_floored_elu_slope_fails_check_grads_at_the_elu_deep_point_only():
    """(b') the ELU slope y + 1 floored at 1e-3.  New assertion: ``check_grads`` of the ``elu_deep`` case (a decoder
    weight off by 0.17 of its scale).  The nine grid cases are bit-identical to the unmutated module's or pass: no
    pre-activation of theirs is below -6.9."""
    case = _case(dm.REGIME_CASES, regime="elu_deep")
    assert _failed(case, _mutated("b_elu_floored_slope", case)) == "check_grads"
    for old in OLD_GRID:
        assert _failed_old(old, _mutated("b_elu_floored_slope", old)) is None, old.name


def test_c_tanh_slopes():
    """(c) the tanh slope taken as 1 - |y|: it differs from 1 - y*y by up to 0.25 at mid-range, so every case fails
    ``check_grads``, the nine grid cases included -- this spelling never needed the saturated point.  (c') the slope
    floored at 1e-3 does: bit-identical wherever |y| < 0.9995, which is everywhere on the grid, and 5e-3 of scale off at
    the ``saturated`` point.  New assertion: ``check_grads`` of the two ``saturated`` cases."""
    for case in OLD_GRID[:3] + dm.REGIME_CASES[:2]:
        assert _failed_old(case, _mutated("c_tanh_abs_slope", case)) == "check_grads", case.name
    for case in (c for c in dm.REGIME_CASES if c.regime == "saturated"):
        assert _failed(case, _mutated("c_tanh_floored_slope", case)) == "check_grads", case.name
    for old in OLD_GRID:
        assert _failed_old(old, _mutated("c_tanh_floored_slope", old)) is None, old.name


def test_d_stride_su_fails_the_forward_bar_where_more_states_are_given_than_steps():
    """(d) the given states indexed with stride su = min(S, K) instead of S.  New assertion: the forward bar of the edge
    case (3, 6, 4) (and of the grid's new row (5, 6, 4)): every sample but the first reads another sample's states.
    No old grid case has S > K: there the fault reads what the kernel reads."""
    case = _case(dm.EDGE_CASES, S=6)
    assert _failed(case, _mutated("d_stride_su", case)) == "forward"
    assert _failed_old(dm.GRID_CASES[9], _mutated("d_stride_su", dm.GRID_CASES[9])) == "forward"
    for old in OLD_GRID:
        assert old.S <= old.K and all(torch.equal(a, b) for a, b in zip(_stride_su(old)[:2], old.inputs()[:2]))


def test_e_null_context_cotangent_fails_check_grads_under_the_outputs_only_loss():
    """(e) a null d_ctx_s_out read as the d_outputs buffer.  New assertion: ``check_grads`` of the cotangent case
    ``outputs`` alone (a first-block encoder weight off by 59 x its scale).  Every grid case back-propagates all six
    tensors, so none of its cotangents is null.  Emulated for a non-null d_outputs only: with both null the fault reads
    no buffer at all, which only the kernel could show."""
    case = _case(dm.COTANGENT_CASES, cot=("outputs",))
    assert _failed(case, _mutated("e_null_ctx_reads_outputs", case)) == "check_grads"
    for other in dm.COTANGENT_CASES:
        assert (_null_context_reads_outputs(other) is not None) == (other.cot == ("outputs",))
    for old in OLD_GRID:
        assert old.cot == dm.TENSORS and _null_context_reads_outputs(old) is None


def test_f_unrotated_ring_fails_the_forward_bar_of_the_returned_context_at_two_steps():
    """(f) the K = 2 final context taken from ring slots i instead of (K + i) % 3.  New assertion: the forward bar on
    ``context_s`` of the edge cases (3, 1, 2) and (3, 2, 2) (and of the grid's new row (7, 1, 2)).  No old grid case has
    K = 2."""
    for case in (c for c in dm.EDGE_CASES if c.K == 2):
        got = _mutated("f_k2_ring_unrotated", case)
        assert _failed(case, got) == "forward"
        ref = _ref(case)[0]["tensors"]
        assert dm.scale_error(got["tensors"]["context_s"], ref["context_s"]) > 0.1
        assert dm.scale_error(got["tensors"]["outputs"], ref["outputs"]) < dm.FWD["atol_scale"]
    assert _failed_old(dm.GRID_CASES[10], _mutated("f_k2_ring_unrotated", dm.GRID_CASES[10])) == "forward"
    assert all(old.K != 2 for old in OLD_GRID)
