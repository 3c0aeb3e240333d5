"""The operating points, bars and emulated faults behind tests/test_fclstm_regimes_gpu.py, on the CPU only.

On the exact modules and inputs of the GPU file (tests/_fclstm_models.py holds both):

* every case reaches its regime on the fp64 module: ``saturated`` puts a share of the gates within 1e-3 of 0 or 1 and
  leaves another share in [0.1, 0.9], |tanh(c)| above 0.999 and (autoregressive) a share of ``deltas`` within 1e-3 of +-1
  with another below 0.9; ``deep`` puts pre-activations of the three hidden Linear layers below -5 and leaves others
  above -1; ``small`` puts the first hidden pre-activations below 2e-2 in magnitude.  The grid the suite had reaches none;
* what fp32 PyTorch on the CPU loses against fp64 on every case, per tensor and per slice: the file-wide yardstick
  YARD_FWD / YARD_GRAD / YARD_SLICE that ``_fclstm_models.bars`` takes the GPU file's bars from;
* ten faults a kernel could have, emulated in fp32 torch, each against the GPU file's judge (``fm.judge``) and against the
  bar the grid had (forward atol 2e-5, ``check_grads`` at GRAD_TOL, no slices).  Nothing here runs a kernel: the LSTM
  cell is re-spelled as an autograd Function (``_Cell``) behind nn.LSTM's interface, the activations are those of
  tests/_delay_models.py, and the faults of indexing and wiring are emulated by what they would read or add."""
import copy
import os

import numpy as np
import pytest
import torch

import _delay_models as dm
import _fclstm_models as fm
from conftest import GRAD_TOL

_ref = fm.reference
OLD_GRID = fm.GRID_CASES


# ---------------------------------------------------------------------------------------------------------------------
# the LSTM cell, re-spelled: the probe of the operating points and the seat of the emulated cell faults
# ---------------------------------------------------------------------------------------------------------------------
class _Cell(torch.autograd.Function):
    """(pre [B, 64], c_prev [B, 16]) -> (h', c') as nn.LSTM's cell, the backward written out as fc_bwd_kernel's p3:
    ``fault`` None is the cell itself; "f_c_new" (c) takes c' for c in the forget-gate term; "sigmoid_floor" (d) floors
    g(1 - g) at 1e-3; "tanh_c_floor" (d') floors 1 - tanh(c')^2 at 1e-3."""

    @staticmethod
    def forward(ctx, pre, c_prev, fault):
        i, f, g, o = pre.chunk(4, dim=-1)
        i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
        c = f * c_prev + i * g
        tc = torch.tanh(c)
        ctx.save_for_backward(i, f, g, o, c_prev, c, tc)
        ctx.fault = fault
        return o * tc, c

    @staticmethod
    def backward(ctx, dh, dc_in):
        i, f, g, o, c_prev, c, tc = ctx.saved_tensors
        slope = (lambda s: torch.clamp(s * (1 - s), min=1e-3)) if ctx.fault == "sigmoid_floor" else (lambda s: s * (1 - s))
        tslope = 1 - tc * tc
        if ctx.fault == "tanh_c_floor":
            tslope = torch.clamp(tslope, min=1e-3)
        dc = dh * o * tslope + dc_in
        p = (dc * g * slope(i), dc * (c if ctx.fault == "f_c_new" else c_prev) * slope(f), dc * i * (1 - g * g),
             dh * tc * slope(o))
        return torch.cat(p, dim=-1), dc * f, None


class _FunctionalLSTM(torch.nn.Module):
    """nn.LSTM(4, 16, batch_first=True) on ``_Cell``, with the SAME four Parameters under the same names; ``seen`` gathers
    the gate activations and c' of every step."""

    def __init__(self, lstm, fault=None):
        super().__init__()
        for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
            setattr(self, n, getattr(lstm, n))
        self.fault, self.seen = fault, []

    def forward(self, x, hidden):
        h, c = hidden[0][0], hidden[1][0]
        out = []
        for t in range(x.shape[1]):
            pre = x[:, t] @ self.weight_ih_l0.T + self.bias_ih_l0 + h @ self.weight_hh_l0.T + self.bias_hh_l0
            h, c = _Cell.apply(pre, c, self.fault)
            gates = pre.detach().chunk(4, dim=-1)
            self.seen.append({"gates": torch.cat([torch.sigmoid(gates[0]), torch.sigmoid(gates[1]), torch.sigmoid(gates[3])], -1),
                              "c": c.detach()})
            out.append(h)
        return torch.stack(out, dim=1), (h[None], c[None])


def _functional(sur, fault=None):
    """A copy of ``sur`` whose nn.LSTM is ``_FunctionalLSTM``."""
    sur = copy.deepcopy(sur)
    sur.transition_model.lstm = _FunctionalLSTM(sur.transition_model.lstm, fault)
    return sur


def _probe(case):
    """What the fp64 module of ``case`` passes through: sigmoid gate activations, c', and the pre-activations of the three
    hidden Linear layers (both encoder layers, the first decoder layer), each as one flat array."""
    sur = _functional(fm.modules(case.factory, case.scaled, case.regime)[0])
    layers = {"enc0": sur.state_encoder.model[0].linear, "enc1": sur.state_encoder.model[1].linear,
              "dec0": sur.state_decoder.model[0].linear}
    pre = {n: [] for n in layers}
    hooks = [m.register_forward_hook(lambda m, i, o, n=n: pre[n].append(o.detach().reshape(-1))) for n, m in layers.items()]
    try:
        out = fm.run_case(sur, case, dtype=torch.float64)
    finally:
        for h in hooks:
            h.remove()
    seen = sur.transition_model.lstm.seen
    return {"gates": torch.cat([s["gates"].reshape(-1) for s in seen]).numpy(),
            "c": torch.cat([s["c"].reshape(-1) for s in seen]).numpy(),
            "pre": {n: torch.cat(v).numpy() for n, v in pre.items()}, "run": out}


def _shares(case):
    p = _probe(case)
    g, t = p["gates"], _ref(case)[0]["tensors"]
    out = {"gates_flat": float(np.mean((g < 1e-3) | (g > 1 - 1e-3))), "gates_mid": float(np.mean((g >= 0.1) & (g <= 0.9))),
           "tanh_c_max": float(np.abs(np.tanh(p["c"])).max()), "c_max": float(np.abs(p["c"]).max()),
           "h_max": float(np.abs(t["outlatents"]).max()),
           "deltas_flat": float(np.mean(np.abs(t["deltas"]) > 1 - 1e-3)), "deltas_mid": float(np.mean(np.abs(t["deltas"]) < 0.9))}
    for n, v in p["pre"].items():
        out[f"{n}_below_-5"], out[f"{n}_above_-1"], out[f"{n}_absmax"] = float(np.mean(v < -5)), float(np.mean(v > -1)), float(np.abs(v).max())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# coverage: the operating points are reached, and the grid the suite had reaches none of them
# ---------------------------------------------------------------------------------------------------------------------
def test_the_respelled_cell_is_the_module():
    """``_FunctionalLSTM`` against nn.LSTM in fp64: rounding apart (1e-13 of scale), values and every gradient agree."""
    for case in fm.BASE_CASES[:2] + fm.COTANGENT_CASES[4:6]:
        got, ref = _probe(case)["run"], _ref(case)[0]
        assert max(fm.forward_errors(got["tensors"], ref["tensors"]).values()) < 1e-13, case.name
        assert max(dm.tensor_errors(got["grads"], ref["grads"]).values()) < 1e-13, case.name


@pytest.mark.parametrize("case", [c for c in fm.REGIME_CASES if c.regime == "saturated"], ids=lambda c: c.name)
def test_saturated_point_reaches_both_ends_of_every_slope(case):
    s = _shares(case)
    print(case.name, s)
    assert s["gates_flat"] >= 0.05 and s["gates_mid"] >= 0.05, s
    assert s["tanh_c_max"] > 0.999, s
    if case.factory == fm.AUTOREG:
        assert s["deltas_flat"] >= 0.02 and s["deltas_mid"] >= 0.20, s


@pytest.mark.parametrize("case", [c for c in fm.REGIME_CASES if c.regime == "deep"], ids=lambda c: c.name)
def test_deep_point_reaches_the_flat_end_of_the_hidden_activation(case):
    s = _shares(case)
    print(case.name, s)
    for layer in ("enc0", "enc1", "dec0"):
        assert s[f"{layer}_below_-5"] >= 0.25 and s[f"{layer}_above_-1"] >= 0.25, (layer, s)


@pytest.mark.parametrize("case", fm.SMALL_CASES, ids=lambda c: c.name)
def test_small_states_put_the_first_hidden_layer_far_below_one(case):
    """The given states' first pre-activations: |x| <= 20 x the amplitude (64 inputs, weights within 1 / 8, no bias), where
    expm1f(x) and expf(x) - 1 differ.  The latent form encodes nothing else; the autoregressive one also re-encodes its
    predictions, which are of order 0.1."""
    sur = fm.modules(case.factory, case.scaled, case.regime)[0]
    states = case.inputs()[0]
    with torch.no_grad():
        x = float(sur.state_encoder.model[0].linear(states).abs().max())
    s = _shares(case)
    print(case.name, x, s)
    assert 0 < x <= 20 * case.states and float(states.abs().max()) <= 1.5 * case.states
    if case.factory == fm.LATENT:
        assert s["enc0_absmax"] == x


def test_the_grid_the_suite_had_reaches_none_of_the_operating_points():
    """The gap this file closes: at initialisation no gate of the old grid comes within 1e-3 of 0 or 1, no |tanh(c)|
    reaches 0.999, no delta comes within 1e-3 of +-1, no hidden pre-activation falls below -5 and the first hidden layer
    sees |x| of order one."""
    for case in OLD_GRID:
        if case.B > 7:
            continue
        s = _shares(case)
        assert s["gates_flat"] == 0 and s["tanh_c_max"] < 0.999, (case.name, s)
        assert case.factory == fm.LATENT or s["deltas_flat"] == 0, (case.name, s)     # the latent deltas are no tanh output
        assert all(s[f"{layer}_below_-5"] == 0 for layer in ("enc0", "enc1", "dec0")), (case.name, s)
        assert s["enc0_absmax"] > 0.5, (case.name, s)


# ---------------------------------------------------------------------------------------------------------------------
# slices and the yardstick
# ---------------------------------------------------------------------------------------------------------------------
def test_grad_slices_cover_every_element_once():
    grads = _ref(fm.EDGE_CASES[0])[0]["grads"]
    many = {"input.states": 6, "input.actions": 4, fm.ENC0: 4, **{fm.LSTM + n: 4 for n in
                                                                  ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")}}
    assert set(many) <= set(grads) and len(grads) == 16
    for name, g in grads.items():
        count = np.zeros(g.shape, dtype=int)
        slices = fm.grad_slices(name, g)
        for _, idx in slices:
            count[idx] += 1
        assert (count == 1).all(), name
        assert len(slices) == many.get(name, 1), name
    w = fm.grad_slices(fm.LSTM + "weight_hh_l0", grads[fm.LSTM + "weight_hh_l0"])
    assert [g for g, _ in w] == ["i", "f", "g", "o"] and grads[fm.LSTM + "weight_hh_l0"][w[1][1]].shape == (16, 16)
    assert w[1][1] == (slice(16, 32),)
    assert grads[fm.ENC0][fm.grad_slices(fm.ENC0, grads[fm.ENC0])[2][1]].shape == (32, 16)


def test_check_slices_sees_one_gate_quarter_that_the_tensor_bar_passes():
    """The forget-gate quarter of weight_hh off by 0.05 %: 1.3e-4 of the TENSOR's scale when the g quarter is 3.8 times
    larger, under GRAD_TOL; 5e-4 of the quarter's own scale.  A zero slice that is written to fails at any size."""
    name = fm.LSTM + "weight_hh_l0"
    ref = {name: np.ones((64, 16)), "input.states": np.ones((2, 3, 1, 64))}
    for q, m in enumerate((0.38, 0.48, 1.81, 0.54)):
        ref[name][16 * q:16 * (q + 1)] *= m
    ref["input.states"][:, 2] = 0.0
    got = copy.deepcopy(ref)
    assert dm.check_slices("exact", got, ref, GRAD_TOL, slices=fm.grad_slices, zero_tol=0.0) == (0.0, None)
    got[name][16:32] *= 1.0005
    assert dm.tensor_errors(got, ref)[name] < GRAD_TOL
    with pytest.raises(AssertionError, match=r"weight_hh_l0\[f\] off by 5.0"):
        dm.check_slices("one quarter off", got, ref, GRAD_TOL, slices=fm.grad_slices, zero_tol=0.0)
    got = copy.deepcopy(ref)
    got["input.states"][1, 2, 0, 7] = 1e-30
    with pytest.raises(AssertionError, match=r"input.states\[step2\] is zero in fp64"):
        dm.check_slices("stray", got, ref, GRAD_TOL, slices=fm.grad_slices, zero_tol=0.0)


def test_gate_quarters_sit_well_below_their_tensors_maximum():
    """Why the per-tensor bar is not enough: on the base grid a gate quarter of an LSTM gradient sits a factor of three
    or more below its tensor's maximum."""
    smallest = 1.0
    for case in fm.BASE_CASES:
        for name, g in _ref(case)[0]["grads"].items():
            if name.startswith(fm.LSTM):
                smallest = min(smallest, min(float(np.abs(g[idx]).max() / np.abs(g).max()) for _, idx in fm.grad_slices(name, g)))
    assert smallest < 1 / 3, smallest


def test_bars_come_from_the_yardstick_and_are_tighter_than_the_ones_the_suite_had():
    """fp32 torch on the CPU over every case of the file: measured 1.7e-6 forward (``deltas`` at the saturated point),
    1.3e-6 per tensor and 2.1e-6 to 2.8e-6 per slice, depending on the CPU (the figures are printed).  8 x each is below
    the old caps, so the caps do not bind: the bars are about 1.4e-5, 1.0e-5 and 2e-5."""
    y, bar = fm.yardstick(), fm.bars()
    print("fclstm regimes yardstick", y, bar)
    assert 0 < y["YARD_FWD"] and 0 < y["YARD_GRAD"] <= y["YARD_SLICE"]
    assert bar == {"forward": 8 * y["YARD_FWD"], "gradient": 8 * y["YARD_GRAD"], "slice": 8 * y["YARD_SLICE"]}
    assert bar["forward"] < 2e-5 and bar["gradient"] < GRAD_TOL and bar["slice"] < GRAD_TOL


@pytest.mark.parametrize("case", fm.ALL_CASES, ids=lambda c: c.name)
def test_fp32_cpu_yardstick(case):
    """fp32 PyTorch on the CPU against fp64, per tensor and per slice, recorded for every GPU case; the yardstick passes
    the judge it sets the bars of."""
    ref, yard = _ref(case)
    rec = fm.record(case, ref, yard)
    y = fm.yardstick()
    assert rec["forward_err_of_scale"]["fp32_cpu"]["err"] <= y["YARD_FWD"]
    assert rec["gradient_err_of_scale"]["fp32_cpu"]["err"] <= y["YARD_GRAD"]
    assert rec["worst_slice"]["fp32_cpu"]["err"] <= y["YARD_SLICE"]
    assert len(ref["grads"]) == (16 if case.hidden else 14)
    fm.judge(case.name + " fp32 cpu", yard, ref)


def _cot(factory, *cot):
    return _case(fm.COTANGENT_CASES, factory=factory, cot=cot)


def test_zero_rule_cases_have_the_zero_slices_they_are_there_for():
    g = _ref(_cot(fm.AUTOREG, "inlatents"))[0]["grads"]     # the re-encoded predictions are detached
    assert g["input.states"][:, :2].any() and not g["input.actions"].any()
    assert not any(v.any() for n, v in g.items() if n.startswith(("state_decoder", "transition_model")))
    assert all(v.any() for n, v in g.items() if n.startswith("state_encoder"))
    g = _ref(_cot(fm.LATENT, "inlatents"))[0]["grads"]      # the running latent is not: it reaches the cell
    assert g[fm.LSTM + "weight_hh_l0"].any() and not any(v.any() for n, v in g.items() if n.startswith("state_decoder"))
    assert g["input.actions"][:, :3].any() and not g["input.actions"][:, 3].any()
    for f in fm.FACTORIES:
        g = _ref(_cot(f, "hidden_c"))[0]["grads"]
        assert not g["input.h_in"].any() and g["input.c_in"].any() and g["input.states"].any()
        for case in fm.EDGE_CASES:
            g, su = _ref(case)[0]["grads"], min(case.S, case.K)
            assert g["input.states"][:, :su].any() and not g["input.states"][:, su:].any(), case.name
            assert ("input.c_in" in g) == case.hidden and (not case.hidden or (g["input.c_in"].any() and not g["input.h_in"].any()))


# ---------------------------------------------------------------------------------------------------------------------
# emulated faults
# ---------------------------------------------------------------------------------------------------------------------
def _null_c_reads_h(case):
    """(a): a backward that reads d_h_out where d_c_out is null: the loss gains <hidden_c, the weights of hidden_h>.  It
    needs d_h_out itself: a null one is no buffer to read."""
    if case.cot is None or "hidden_c" in case.cot or "hidden_h" not in case.cot:
        return None
    import _grad_contract_models as gm
    return lambda tensors, weights: gm.weighted_loss({**{n: tensors[n] for n in case.cot}, "stray": tensors["hidden_c"]},
                                                     {**weights, "stray": weights["hidden_h"]})


def _free_running_inlatents_dropped(case):
    """(b): d_inl of the free-running steps never added to the running latent's carry (latent form)."""
    su = min(case.S, case.K)

    def tensors_of(ro):
        t = fm.rollout_tensors(ro)
        if case.kind == "every":
            t["inlatents"] = torch.cat((t["inlatents"][:, :su], t["inlatents"][:, su:].detach()), dim=1)
        return t
    return tensors_of


def _stride_su(case):
    """(g): what a forward that indexes the given states with stride su = min(S, K) reads."""
    st, ac, h = case.inputs()
    su, flat = min(case.S, case.K), st.reshape(case.B * case.S, 1, 64)
    read = st.clone()
    for b in range(case.B):
        for k in range(su):
            read[b, k] = flat[b * su + k]
    return read, ac, h


def _autoreg_rollout(leak):
    """AutoRegPDESurrogate.rollout's torch loop re-spelled; ``leak`` (h): the integration base of a teacher-forced step
    k > 0 carries the gradient of the previous output (values unchanged: x + (o - o)), as a ``g`` carried across it would."""
    def rollout(sur, states, actions, times, targets, hidden):
        from pdecontrol.mbrl.types import ModelRollout
        from pdecontrol.surrogates.surrogate import action_and_target_indices, take_steps
        n_given, lstates = states.size(1), sur.state_encoder(states)
        aidx, tidx = action_and_target_indices(times, targets, sur.delta)
        lactions = take_steps(sur.action_encoder(actions), aidx.tolist())
        n_steps = lactions.size(1)
        inlatents, outlatents, outdeltas, outputs = [], [], [], []
        output, inlast = states[:, :1], lstates[:, :1]
        for k in range(n_steps):
            laction = lactions[:, k:k + 1]
            if k < n_given:
                inlatent, base = lstates[:, k:k + 1], states[:, k:k + 1]
                if leak and k > 0:
                    base = base + (output - output.detach())
                outlatent, hidden = sur.transition_model.teacherforcing(states=inlatent, actions=laction, hidden=hidden)
            else:
                inlatent, base = inlast, output
                outlatent, hidden = sur.transition_model.transition(states=inlatent, actions=laction, hidden=hidden)
            outdelta = sur.state_decoder(outlatent)
            output = base + sur.delta * sur.dscaling(outdelta)
            if n_given <= k + 1 < n_steps:
                inlast = sur.state_encoder(output).detach()
            inlatents.append(inlatent), outlatents.append(outlatent), outdeltas.append(outdelta), outputs.append(output)
        gather = lambda seq: take_steps(torch.cat(seq, dim=1), tidx.tolist())
        return ModelRollout(inlatents=gather(inlatents), outlatents=gather(outlatents), deltas=gather(outdeltas),
                            outputs=gather(outputs), hidden=hidden)
    return rollout


CELL_FAULTS = {"c_forget_c_new": "f_c_new", "d_sigmoid_floored": "sigmoid_floor", "d_tanh_c_floored": "tanh_c_floor"}
ACT_FAULTS = {"e_tanh_abs_slope": (torch.nn.Tanh, dm.TanhAbsSlope), "f_elu_floored_slope": (torch.nn.ELU, dm.EluFlooredSlope),
              "f_exp_minus_1": (torch.nn.ELU, dm.EluByExp)}


def mutated(name, case):
    """The fp32 CPU module's result on ``case`` with fault ``name``; "cell" is the re-spelled cell without a fault and
    "loop" the re-spelled autoregressive loop without one."""
    sur = fm.modules(case.factory, case.scaled, case.regime)[1]
    kw = {}
    if name == "cell" or name in CELL_FAULTS:
        sur = _functional(sur, CELL_FAULTS.get(name))
    elif name in ACT_FAULTS:
        sur = dm.swap_activation(copy.deepcopy(sur), *ACT_FAULTS[name])
    elif name == "a_null_c_reads_h":
        kw["loss_of"] = _null_c_reads_h(case)
    elif name == "b_free_inlatents_dropped":
        kw["tensors_of"] = _free_running_inlatents_dropped(case)
    elif name == "g_stride_su":
        kw["inputs"] = _stride_su(case)
    elif name in ("loop", "h_carry_across_given"):
        kw["rollout"] = _autoreg_rollout(leak=name != "loop")
    else:
        raise ValueError(name)
    return fm.run_case(sur, case, **kw)


_MUTATED = {}


def _mutated(name, case):
    if (name, case.name) not in _MUTATED:
        _MUTATED[name, case.name] = mutated(name, case)
    return _MUTATED[name, case.name]


def _quiet(fn):
    """Run ``fn`` with the gradient parity log switched off: an emulated fault is no observation of the project's."""
    import conftest
    log, conftest.GRAD_LOG = conftest.GRAD_LOG, os.devnull
    try:
        fn()
    except AssertionError as e:
        return str(e)
    finally:
        conftest.GRAD_LOG = log
    return None


def _failed(case, got):
    """None, or which of ``fm.judge``'s assertions ``got`` fails first on ``case``: "forward", "zero" (a gradient that is
    zero in fp64 was written), "check_grads", "check_slices" -- with the text of the failure."""
    text = _quiet(lambda: fm.judge(case.name + " emulated fault", got, _ref(case)[0]))
    if text is None:
        return None, ""
    if "Not equal to tolerance" in text:
        return "forward", text
    if "no path from the loss" in text:
        return "zero", text
    return ("check_slices" if ("of the slice's scale" in text or "is zero in fp64 but" in text) else "check_grads"), text


def _failed_old(case, got):
    """The same for the bar the grid had: forward rtol 2e-4 / atol 2e-5 of scale, ``check_grads`` at GRAD_TOL, no slices."""
    from conftest import check_grads
    ref = _ref(case)[0]

    def old():
        for n, r in ref["tensors"].items():
            np.testing.assert_allclose(got["tensors"][n], r, rtol=fm.FWD_RTOL, atol=fm.FWD_CAP * max(1.0, float(np.abs(r).max())))
        check_grads(case.name + " emulated fault, old bar", got["grads"], ref["grads"].__getitem__)
    text = _quiet(old)
    return None if text is None else ("forward" if "Not equal to tolerance" in text else "check_grads")


def _case(cases, **want):
    found = [c for c in cases if all(getattr(c, k) == v for k, v in want.items())]
    assert len(found) == 1, (want, [c.name for c in found])
    return found[0]


def _worst(case, got):
    ref = _ref(case)[0]["grads"]
    return dm.worst_of(dm.tensor_errors(got["grads"], ref)), dm.worst_slice(got["grads"], ref, fm.grad_slices)


def _autoreg(cases):
    return [c for c in cases if c.factory == fm.AUTOREG]


def _latent(cases):
    return [c for c in cases if c.factory == fm.LATENT]


def test_the_respellings_without_a_fault_pass_the_judge():
    """The seats of the emulations are clean: the re-spelled cell and the re-spelled autoregressive loop, in fp32 and
    without a fault, pass ``fm.judge`` on every case a fault below is judged on (the loop is bit for bit the module)."""
    for case in fm.REGIME_CASES + fm.BASE_CASES + OLD_GRID[:4]:
        assert _failed(case, _mutated("cell", case))[0] is None, case.name
    for case in _autoreg(fm.COTANGENT_CASES):
        got, yard = _mutated("loop", case), _ref(case)[1]
        assert all(np.array_equal(got[k][n], yard[k][n]) for k in ("tensors", "grads") for n in yard[k]), case.name


def test_a_null_cell_cotangent_read_from_the_hidden_one_fails_check_grads_under_hidden_h_alone():
    """(a) a null d_c_out read as the d_h_out buffer.  New assertion: ``check_grads`` of the cotangent cases ``hidden_h``
    alone and (deltas, hidden_h), both factories (2.4 to 2.8 x the scale of a gradient).  Every grid case back-propagates
    all returned tensors, so none of its cotangents is null: the fault has nothing to read there."""
    hit = [c for c in fm.COTANGENT_CASES if _null_c_reads_h(c) is not None]
    assert sorted(c.cot for c in hit) == [("deltas", "hidden_h")] * 2 + [("hidden_h",)] * 2
    for case in hit:
        assert _failed(case, _mutated("a_null_c_reads_h", case))[0] == "check_grads", case.name
    assert all(old.cot is None and _null_c_reads_h(old) is None for old in OLD_GRID)


def test_b_dropped_free_running_inlatents_cotangent_fails_check_grads_under_inlatents_alone():
    """(b) latent form: d_inl of the free-running steps never reaches the running latent's carry.  New assertion:
    ``check_grads`` of ``inlatents`` alone and (inlatents, outlatents) (a gradient off by its whole scale).  The grid
    had ``inlatents`` in its loss, so its rows with K > S fail too (0.6 of scale): it was not blind to this one, only to
    which of the three places d_inl is added in -- a given step at k = 0, a given step at k > 0, a free-running step --
    since no row isolates the cotangent."""
    for case in _latent(fm.COTANGENT_CASES):
        want = "check_grads" if "inlatents" in case.cot else None
        assert _failed(case, _mutated("b_free_inlatents_dropped", case))[0] == want, case.name
    for old in _latent(OLD_GRID):
        want = "check_grads" if old.K > old.S and old.kind == "every" else None
        assert _failed_old(old, _mutated("b_free_inlatents_dropped", old)) == want, old.name


def test_c_forget_gate_term_with_the_new_cell_state_fails_check_grads_and_the_f_quarter_by_more():
    """(c) the forget-gate gradient with c' for c (the ``rec[R_C + j - REC]`` look-back).  New assertions: ``check_grads``
    (0.08 to 0.17 of a tensor's scale on the base grid) and, had that passed, the slice bar on an f quarter (0.5 to 0.85
    of the quarter's scale: the error sits in rows 16:32 and is divided by the g quarter's maximum in the tensor
    figure).  GRAD_TOL on the whole tensor DOES see this one: every row of the grid fails ``check_grads`` -- the quarter
    bar matters for a fault 400 times smaller than this."""
    for case in fm.BASE_CASES:
        got, ref = _mutated("c_forget_c_new", case), _ref(case)[0]
        assert _failed(case, got)[0] == "check_grads", case.name
        lstm = lambda r: {n: g for n, g in r["grads"].items() if n.startswith(fm.LSTM)}
        with pytest.raises(AssertionError, match=r"l0\[f\] off by"):
            dm.check_slices(case.name, lstm(got), lstm(ref), fm.bars()["slice"], slices=fm.grad_slices, zero_tol=0.0)
        tensor = dm.worst_of(dm.tensor_errors(lstm(got), lstm(ref)))
        worst = dm.worst_slice(lstm(got), lstm(ref), fm.grad_slices)
        assert worst["name"].endswith("[f]") and worst["err"] > 3 * tensor["err"], (case.name, tensor, worst)
    for old in OLD_GRID:
        assert _failed_old(old, _mutated("c_forget_c_new", old)) == "check_grads", old.name


def test_d_floored_sigmoid_slope_fails_check_grads_at_the_saturated_point_only():
    """(d) the sigmoid slope g(1 - g) floored at 1e-3.  New assertion: ``check_grads`` of the four ``saturated`` cases
    (2e-3 to 4e-3 of a tensor's scale, 6e-3 to 8e-3 of a gate quarter's).  The grid passes: no gate of it comes within
    1e-3 of 0 or 1, so the floor never binds and the results are those of the cell without a fault, bit for bit."""
    for case in (c for c in fm.REGIME_CASES if c.regime == "saturated"):
        assert _failed(case, _mutated("d_sigmoid_floored", case))[0] == "check_grads", case.name
    for old in OLD_GRID:
        got, clean = _mutated("d_sigmoid_floored", old), _mutated("cell", old)
        assert _failed_old(old, got) is None, old.name
        assert all(np.array_equal(got["grads"][n], clean["grads"][n]) for n in clean["grads"]), old.name


def test_d_floored_cell_tanh_slope_is_below_what_fp32_can_show():
    """(d') 1 - tanh(c')^2 floored at 1e-3: NOT separable.  It binds where |tanh(c')| > 0.9995, and there it changes dc
    by at most 1e-3 dh o: measured at the ``saturated`` point 7.8e-6 of input.c_in's scale (autoregressive; 7e-7 latent)
    against a bar of 1.0e-5 and fp32 noise of the re-spelled cell of 3.7e-6.  Reported, not asserted; on the grid the
    floor never binds (bit for bit the cell without a fault)."""
    for case in (c for c in fm.REGIME_CASES if c.regime == "saturated"):
        print("d' tanh(c) slope floored", case.name, _worst(case, _mutated("d_tanh_c_floored", case)), fm.bars())
    for old in OLD_GRID:
        got, clean = _mutated("d_tanh_c_floored", old), _mutated("cell", old)
        assert all(np.array_equal(got["grads"][n], clean["grads"][n]) for n in clean["grads"]), old.name


def test_e_last_slope_as_one_minus_abs_fails_check_grads_everywhere():
    """(e) autoregressive form: ``last_slope`` taken as 1 - |y| where the kernel has 1 - y*y.  It differs by up to 0.25
    at mid-range, so ``check_grads`` fails on every case (0.2 to 0.5 of scale), the grid's included: this spelling never
    needed the saturated point."""
    for case in _autoreg(fm.REGIME_CASES[:4] + fm.BASE_CASES):
        assert _failed(case, _mutated("e_tanh_abs_slope", case))[0] == "check_grads", case.name
    for old in _autoreg(OLD_GRID):
        assert _failed_old(old, _mutated("e_tanh_abs_slope", old)) == "check_grads", old.name


def test_f_floored_elu_slope_fails_check_grads_at_the_deep_point_only():
    """(f) latent form: the ELU slope floored at 1e-3.  New assertion: ``check_grads`` of the two latent ``deep`` cases
    (7e-4 to 8e-4 of an encoder gradient's scale).  The grid passes: none of its pre-activations is below -6.9."""
    for case in _latent([c for c in fm.REGIME_CASES if c.regime == "deep"]):
        assert _failed(case, _mutated("f_elu_floored_slope", case))[0] == "check_grads", case.name
    for old in _latent(OLD_GRID):
        assert _failed_old(old, _mutated("f_elu_floored_slope", old)) is None, old.name


def test_f_exp_minus_one_fails_check_grads_at_both_small_amplitudes_on_the_tight_bar_only():
    """(f') latent form: exp(x) - 1 rounded in fp32 in place of expm1.  New assertion: ``check_grads`` of the two latent
    ``small`` cases, on the second encoder weight: 2.3e-5 of its scale at amplitude 1e-3 -- above the bar of 1.0e-5,
    below GRAD_TOL, so only the tight bar sees it -- and 2.8e-4 at amplitude 1e-4.  The grid passes (at most 1.2e-6: its
    pre-activations are of order one)."""
    for case in _latent(fm.SMALL_CASES):
        got = _mutated("f_exp_minus_1", case)
        assert _failed(case, got)[0] == "check_grads", case.name
        assert case.states != 1e-3 or _failed_old(case, got) is None, case.name
    for old in _latent(OLD_GRID):
        assert _failed_old(old, _mutated("f_exp_minus_1", old)) is None, old.name


def test_g_stride_su_fails_the_forward_bar_where_more_states_are_given_than_steps():
    """(g) the given states indexed with stride su = min(S, K) instead of S.  New assertion: the forward bar of the edge
    cases (3, 6, 4) and (3, 3, 1): every sample but the first reads another sample's states.  The grid's one row with
    S > K, (5, 6, 4), fails too; every other row has S <= K, where the fault reads what the kernel reads."""
    hit = [c for c in fm.EDGE_CASES if c.S > c.K]
    assert {(c.B, c.S, c.K) for c in hit} == {(3, 6, 4), (3, 3, 1)} and len(hit) == 8
    for case in hit:
        assert _failed(case, _mutated("g_stride_su", case))[0] == "forward", case.name
    for old in OLD_GRID:
        if old.S > old.K:
            assert (old.B, old.S, old.K) == (5, 6, 4) and _failed_old(old, _mutated("g_stride_su", old)) == "forward"
        else:
            assert all(torch.equal(a, b) for a, b in zip(_stride_su(old)[:2], old.inputs()[:2]))


def test_h_output_carry_across_a_teacher_forced_step_fails_check_grads_under_outputs_alone():
    """(h) autoregressive form: the output-gradient carry ``g`` taken across a teacher-forced step (``k + 1 >= su``
    dropped).  New assertion: ``check_grads`` of the cotangent cases ``outputs`` alone and (outputs, hidden_c) at S = 2,
    K = 4: d_states of step 0 gains d output_1 (the whole scale of the tensor).  The other cotangents put nothing into
    ``g`` before a given step and pass.  The grid's rows with S >= 2 fail too: it was not blind to this one."""
    for case in _autoreg(fm.COTANGENT_CASES):
        want = "check_grads" if "outputs" in case.cot else None
        assert _failed(case, _mutated("h_carry_across_given", case))[0] == want, case.name
    for old in _autoreg(OLD_GRID):
        want = "check_grads" if old.S >= 2 else None
        assert _failed_old(old, _mutated("h_carry_across_given", old)) == want, old.name
