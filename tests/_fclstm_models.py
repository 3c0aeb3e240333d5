"""Builders of the fully-connected LSTM surrogate tests (tests/test_fclstm_surrogate_host.py,
tests/test_fclstm_surrogate_gpu.py): both factories, KSAutoRegFullyConnectedLSTM and KSLatentLSTM; and the cases,
operating points, gate-quarter slices, file-wide bars and runner that tests/test_fclstm_regimes_host.py and
tests/test_fclstm_regimes_gpu.py share: the host file shows on the CPU that every case reaches its regime and what fp32
torch loses there; the GPU file runs the same cases, on the same inputs, through csrc/sur_fclstm.hip.  The error
measures, the slice judge and the observed-file writer are those of tests/_delay_models.py."""
import copy
import os

import numpy as np
import torch

import _delay_models as dm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FACTORIES = ("KSAutoRegFullyConnectedLSTM", "KSLatentLSTM")
AUTOREG, LATENT = FACTORIES
TENSORS = ("outputs", "deltas", "inlatents", "outlatents", "hidden_h", "hidden_c")
ENC0 = "state_encoder.model.0.linear.weight"
LSTM = "transition_model.lstm."
GATES = ("i", "f", "g", "o")
HID = 16


def golden():
    """(fclstm_golden.npz, latent_golden.npz, b8 states [8, 20, 1, 64], b8 actions [8, 20, 1, 4]): the autoregressive
    factory's fixture, the latent factory's (``lstm_*``), and the batch both were recorded on (the states of
    surrogate_golden.npz, the 4-actuator actions of latent_golden.npz)."""
    shared, latent = np.load(os.path.join(GOLDEN, "surrogate_golden.npz")), np.load(os.path.join(GOLDEN, "latent_golden.npz"))
    return (np.load(os.path.join(GOLDEN, "fclstm_golden.npz")), latent, torch.from_numpy(shared["b8_states"]),
            torch.from_numpy(latent["lstm_actions"]))


def build(factory="KSAutoRegFullyConnectedLSTM", scaled=False, seed=0, perturb=False, ssize=None, activation=None):
    """(surrogate, PDETrainingModule) of a factory on the CPU in fp32, as the fixtures: delta = tstep = 0.25, tau = 5,
    tbtt = 10, MSELoss(reduction="none").  ``perturb`` moves every bias (the LSTM's and the Linear layers').  ``ssize`` /
    ``activation`` rebuild the tree with another latent width / hidden activation: layouts the kernels refuse."""
    import _latent_models as lm
    import pdecontrol.architectures as arch
    from pdecontrol.surrogates.models.fcnn import LinearBlock
    from pdecontrol.surrogates.training import PDETrainingModule
    from pdecontrol.surrogates.transition import LSTMTransitionModel
    und, dsc = lm.normalize_pair() if scaled else (None, None)
    torch.manual_seed(seed)
    f = getattr(arch, factory)()
    model = f.model()
    if ssize is not None or activation is not None:
        w = 16 if ssize is None else ssize
        act = (torch.nn.SiLU if factory == FACTORIES[0] else torch.nn.ELU) if activation is None else activation
        last = torch.nn.Tanh if factory == FACTORIES[0] else torch.nn.Identity
        model["state_encoder"] = torch.nn.Sequential(LinearBlock(1, 64, 1, 32, activation=act),
                                                     LinearBlock(1, 32, 1, w, activation=act))
        model["state_decoder"] = torch.nn.Sequential(LinearBlock(1, w, 1, 32, activation=act),
                                                     LinearBlock(1, 32, 1, 64, activation=last))
        model["transition_model"] = LSTMTransitionModel(schannels=1, ssize=w, achannels=1, asize=4)
    sur = f.surrogate(delta=0.25, dscaling=dsc, tau=5, **model)
    module = PDETrainingModule(surrogate=sur, loss=torch.nn.MSELoss(reduction="none"), tstep=0.25, delta=0.25,
                               undscaling=und, tau=5, tbtt=10)
    if perturb:
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for name, p in sur.named_parameters():
                if ".bias" in name:            # Linear: .bias; nn.LSTM: .bias_ih_l0, .bias_hh_l0
                    p.add_(0.3 * torch.randn(p.shape, generator=g))
    return sur, module


# ---------------------------------------------------------------------------------------------------------------------
# operating points (tests/test_fclstm_regimes_host.py shows that each is reached)
# ---------------------------------------------------------------------------------------------------------------------
DEEP_BIASES = ("state_encoder.model.0.linear.bias", "state_encoder.model.1.linear.bias", "state_decoder.model.0.linear.bias")
# LSTM weights x 6, biases x 3, decoder weights x 4 reach |c| 3.4 and |h| 0.96 but put only 0.2 % of the gates and 0.15 % of
# the deltas at the flat end; these do (tuned on the fp64 CPU module, see ``regime``)
SAT = dict(lstm_weight=12.0, lstm_bias=6.0, decoder_weight=6.0)


def regime(module, name):
    """A copy of ``module`` (a surrogate or its training module) moved to an operating point.
    ``saturated``: LSTM weights x SAT["lstm_weight"], LSTM biases x SAT["lstm_bias"] and, for the autoregressive factory,
    decoder weights x SAT["decoder_weight"]: a share of the gates within 1e-3 of 0 or 1 (the slope g(1 - g) at its small
    end) while another share stays in [0.1, 0.9], |tanh(c)| above 0.999 and, for the autoregressive factory, a share of
    ``deltas`` within 1e-3 of +-1 (``last_slope`` 1 - y*y at its small end) while another stays below 0.9.
    ``deep``: every third bias of both encoder layers and of the first decoder layer lowered by 8, so that those
    pre-activations sit below -5: the flat end of the ELU (latent factory), SiLU's negative tail (autoregressive).
    ``small``: the first encoder bias set to zero; with ``small_states`` inputs of amplitude 1e-3 / 1e-4 the latent
    factory's first ELU then sees |x| << 1, where expm1f(x) and expf(x) - 1 differ.
    Shares reached at (7, 3, 6) on the fp64 module (tests/test_fclstm_regimes_host.py asserts the floors), autoregressive /
    latent.  ``saturated`` with SAT = 12, 6, 6: gates within 1e-3 of 0 or 1 14.8 % / 16.1 %, gates in [0.1, 0.9] 34.9 % /
    34.8 %, max |tanh(c)| 0.99994 / 0.99984 (|c| 5.2 / 4.7, |h| 0.994 / 0.993), deltas within 1e-3 of +-1 19.7 %, deltas
    below 0.9 40.0 % (autoregressive only; scaling does not move them).  ``deep``: pre-activations below -5 34.4 %, 37.5 %,
    34.4 % and above -1 64.4 %, 62.5 %, 65.6 % / 62.5 % in the two encoder layers and the first decoder layer.  ``small``:
    the given states' first pre-activations stay below 20 x the amplitude."""
    out = copy.deepcopy(module)
    sur = getattr(out, "surrogate", out)
    autoreg = type(sur).__name__ == "AutoRegPDESurrogate"
    with torch.no_grad():
        for pname, p in sur.named_parameters():
            if name == "saturated":
                if pname.startswith(LSTM + "weight"):
                    p.mul_(SAT["lstm_weight"])
                elif pname.startswith(LSTM + "bias"):
                    p.mul_(SAT["lstm_bias"])
                elif autoreg and pname.startswith("state_decoder") and pname.endswith(".weight"):
                    p.mul_(SAT["decoder_weight"])
            elif name == "deep":
                if pname in DEEP_BIASES:
                    p[::3] -= 8.0
            elif name == "small":
                if pname == DEEP_BIASES[0]:
                    p.zero_()
            else:
                raise ValueError(name)
    return out


def hidden(B, seed):
    """A carried (H, C), each [1, B, 16]: ``_hidden`` of tests/test_fclstm_surrogate_gpu.py."""
    g = torch.Generator().manual_seed(seed)
    return (0.5 * torch.randn(1, B, HID, generator=g, dtype=torch.float64),
            0.5 * torch.randn(1, B, HID, generator=g, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    """One rollout and one backward.  ``states``: None (white noise in [-1, 1]) or the amplitude of ``dm.small_states``;
    ``cot``: the returned tensors the loss <tensor, fixed random weights> is summed over (None: all of them)."""

    def __init__(self, factory, B, S, K, hidden, scaled, kind="every", cot=None, regime=None, states=None, group=""):
        self.factory, self.B, self.S, self.K, self.hidden, self.scaled = factory, B, S, K, hidden, scaled
        self.kind, self.cot, self.regime, self.states, self.group = kind, (None if cot is None else tuple(cot)), regime, states, group
        self.seed = S * 100 + K * 10 + B
        parts = ["autoreg" if factory == AUTOREG else "latent", f"B{B}-S{S}-K{K}", "hidden" if hidden else "zero",
                 "affine" if scaled else "identity"]
        if regime:
            parts.append(regime)
        if states:
            parts.append(f"amp{states:g}")
        if kind != "every":
            parts.append(kind)
        if self.cot is not None:
            parts.append("d_" + "+".join(self.cot))
        self.name = "-".join(parts)

    def inputs(self):
        """(states, actions, (H, C) or None) in fp64 on the CPU."""
        import _grad_contract_models as gm
        st, ac = dm.uniform_inputs(self.B, self.S, len(gm.grid(self.K, self.kind, 0.25)[0]), self.seed)
        if self.states:
            st = dm.small_states(self.B, self.S, self.states, self.seed)
        return st, ac, (hidden(self.B, self.seed + 7) if self.hidden else None)


def _both(*a, **kw):
    return [Case(f, *a, **kw) for f in FACTORIES]


COTANGENTS = [(n,) for n in TENSORS] + [("outputs", "hidden_c"), ("deltas", "hidden_h"), ("inlatents", "outlatents")]
# S = 2, K = 4: a cotangent on a given step at k = 0, on a given step at k > 0 and on two free-running steps
COTANGENT_CASES = [c for cot in COTANGENTS for c in _both(5, 2, 4, True, True, cot=cot, group="cotangent")]
# S > K (the b*S + k stride with su = K, rows su..S of d_states zeroed), S = K, K = 2 from one and from two given states,
# K = 3, K = 1 from three given states and from one; each with and without a given (H, C): c_in null or not
EDGE_SHAPES = ((3, 6, 4), (3, 3, 1), (3, 1, 2), (3, 2, 2), (4, 2, 3), (5, 1, 1))
EDGE_CASES = [c for i, shape in enumerate(EDGE_SHAPES) for given in (True, False)
              for c in _both(*shape, given, (i + given) % 2 == 0, group="edge")]
REGIME_CASES = [c for name in ("saturated", "deep") for scaled in (True, False)
                for c in _both(7, 3, 6, True, scaled, regime=name, group="regime")]
SMALL_CASES = [c for amp in (1e-3, 1e-4) for c in _both(6, 3, 5, True, True, regime="small", states=amp, group="small")]
# three rows of ROLLOUT_CASES of tests/test_fclstm_surrogate_gpu.py (K = 10 cut to 8), now on the tight bars and per slice
BASE_CASES = _both(7, 3, 3, True, True, group="base") + _both(1, 5, 8, True, False, group="base") + \
    _both(5, 6, 4, False, True, group="base")
ALL_CASES = COTANGENT_CASES + EDGE_CASES + REGIME_CASES + SMALL_CASES + BASE_CASES
# the grid of tests/test_fclstm_surrogate_gpu.py with B <= 64: what the suite had before (the host file's "old grid")
GRID_CASES = [c for row in ((1, 1, 1, False, False, "every"), (7, 3, 3, True, True, "every"), (64, 5, 10, False, True, "every"),
                            (1, 5, 10, True, False, "every"), (7, 1, 20, False, True, "every"), (64, 1, 1, True, True, "every"),
                            (7, 5, 10, True, True, "skip"), (5, 6, 4, False, True, "every"))
              for c in _both(*row[:5], kind=row[5], group="grid")]

_MODULES = {}


def modules(factory, scaled, regime_name=None):
    """(fp64 surrogate, fp32 surrogate) on the CPU at an operating point, built once: ``build(perturb=True)`` as the
    existing GPU tests, then ``regime``."""
    key = (factory, scaled, regime_name)
    if key not in _MODULES:
        sur, _ = build(factory, scaled=scaled, perturb=True)
        if regime_name:
            sur = regime(sur, regime_name)
        _MODULES[key] = (copy.deepcopy(sur).double(), sur)
    return _MODULES[key]


_REFERENCE = {}


def reference(case):
    """(fp64 result, fp32 CPU result) of a case, computed once and shared by every test that needs it; the fp32 CPU
    result is the yardstick."""
    if case.name not in _REFERENCE:
        ref, cpu = modules(case.factory, case.scaled, case.regime)
        _REFERENCE[case.name] = (run_case(ref, case, dtype=torch.float64), run_case(cpu, case))
    return _REFERENCE[case.name]


def rollout_tensors(ro):
    out = {"outputs": ro.outputs, "deltas": ro.deltas, "outlatents": ro.outlatents, "hidden_h": ro.hidden[0],
           "hidden_c": ro.hidden[1]}
    if ro.inlatents is not None:
        out["inlatents"] = ro.inlatents
    return out


def run_case(sur, case, device="cpu", dtype=torch.float32, inputs=None, tensors_of=rollout_tensors, loss_of=None,
             rollout=None):
    """One rollout of ``sur`` on ``case`` and the backward of its loss.  Returns {"tensors": {name: fp64 array},
    "grads": {name: fp64 array}}: ``input.states``, ``input.actions``, with a given hidden state ``input.h_in`` and
    ``input.c_in``, and the twelve parameters; an undefined gradient counts as zero.  ``inputs``, ``tensors_of``,
    ``loss_of(tensors, weights)`` and ``rollout(sur, states, actions, times, targets, hidden)`` replace the case's own
    (the host file's emulations)."""
    import _grad_contract_models as gm
    st, ac, h = case.inputs() if inputs is None else inputs
    mk = lambda t: t.to(device, dtype).clone().requires_grad_(True)
    st_l, ac_l, h_l = mk(st), mk(ac), (None if h is None else tuple(mk(t) for t in h))
    for p in sur.parameters():
        p.grad = None
    times, targets = gm.grid(case.K, case.kind, sur.delta)
    if rollout is None:
        ro = sur.rollout(st_l, ac_l, times, targets, hidden=h_l)
    else:
        ro = rollout(sur, st_l, ac_l, times, targets, h_l)
    tensors = tensors_of(ro)
    weights = gm.loss_weights({n: tensors[n] for n in TENSORS if n in tensors}, case.seed)
    cot = tuple(tensors) if case.cot is None else case.cot
    loss = gm.weighted_loss({n: tensors[n] for n in cot}, weights) if loss_of is None else loss_of(tensors, weights)
    loss.backward()
    grad = lambda t: (torch.zeros_like(t) if t.grad is None else t.grad).detach().cpu().double().numpy()
    grads = {"input.states": grad(st_l), "input.actions": grad(ac_l)}
    if h_l is not None:
        grads["input.h_in"], grads["input.c_in"] = grad(h_l[0]), grad(h_l[1])
    grads.update(gm.trainable_grads(sur))
    for p in sur.parameters():
        p.grad = None
    return {"tensors": {n: t.detach().cpu().double().numpy() for n, t in tensors.items()}, "grads": grads}


# ---------------------------------------------------------------------------------------------------------------------
# slices and bars
# ---------------------------------------------------------------------------------------------------------------------
def grad_slices(name, array):
    """[(label, index)] covering ``array``: the four LSTM parameters per gate quarter (rows 0:16 i, 16:32 f, 32:48 g,
    48:64 o -- the four branches of p3 in fc_bwd_kernel), the rollout's inputs per step, the first encoder weight per
    block of 16 input columns; every other gradient is one slice."""
    if name.startswith(LSTM):
        return [(g, (slice(HID * q, HID * (q + 1)),)) for q, g in enumerate(GATES)]
    if name in ("input.states", "input.actions"):
        return [(f"step{k}", (slice(None), k)) for k in range(array.shape[1])]
    if name == ENC0:
        return [(f"cols{c}:{c + 16}", (slice(None), slice(c, c + 16))) for c in range(0, array.shape[1], 16)]
    return [("all", Ellipsis)]


FWD_RTOL, FWD_CAP, MARGIN = 2e-4, 2e-5, 8.0       # the forward bar of tests/test_fclstm_surrogate_gpu.py; bars = 8 x yardstick
_BARS = {}


def forward_errors(got, ref):
    """{name: max |x - ref| / max(1, max |ref|)}: the figure of the forward bar's absolute floor."""
    return {n: dm.scale_error(np.asarray(got[n]), np.asarray(ref[n])) for n in ref}


def yardstick():
    """{"YARD_FWD", "YARD_GRAD", "YARD_SLICE"}: the largest error of the fp32 CPU module against fp64 over ALL_CASES --
    forward values of the tensor's scale, gradients of the tensor's scale, gradient slices of the slice's scale --
    computed once per session from the cached references.  Never from the kernels."""
    if not _BARS:
        y = {"YARD_FWD": 0.0, "YARD_GRAD": 0.0, "YARD_SLICE": 0.0}
        for case in ALL_CASES:
            ref, yard = reference(case)
            y["YARD_FWD"] = max(y["YARD_FWD"], *forward_errors(yard["tensors"], ref["tensors"]).values())
            y["YARD_GRAD"] = max(y["YARD_GRAD"], *dm.tensor_errors(yard["grads"], ref["grads"]).values())
            y["YARD_SLICE"] = max(y["YARD_SLICE"], *dm.slice_errors(yard["grads"], ref["grads"], grad_slices).values())
        _BARS.update(y)
    return dict(_BARS)


def bars():
    """{"forward", "gradient", "slice"}: MARGIN x the file-wide yardstick, capped at the bars the suite had: forward
    min(2e-5, 8 YARD_FWD) of the tensor's scale (with rtol 2e-4), gradients min(GRAD_TOL, 8 YARD_GRAD) of the tensor's
    scale, slices min(GRAD_TOL, 8 YARD_SLICE) of the slice's scale.  Why 8: the kernels' sums are fmaf chains in index
    order where torch runs blocked GEMMs, and the device's expf / tanhf differ from libm by a few ulp; on the MI355X run
    on record (profiles/fclstm_parity_observed.json) the kernels were at most 4.5 x the yardstick of the same case and
    1.5 x its worst over the grid."""
    from conftest import GRAD_TOL
    y = yardstick()
    return {"forward": min(FWD_CAP, MARGIN * y["YARD_FWD"]), "gradient": min(GRAD_TOL, MARGIN * y["YARD_GRAD"]),
            "slice": min(GRAD_TOL, MARGIN * y["YARD_SLICE"])}


OBSERVED = "fclstm_regimes"


def record(case, ref, yard, got=None, who="kernels", slices=grad_slices, figures=None, observed=OBSERVED):
    """The observed-file record of one case (fclstm_regimes_observed.jsonl next to the gradient parity log): the fp32 CPU
    module (``yard``) and, when given, the kernels (``got``) against the fp64 module (``ref``), with the bars.  ``slices``,
    ``figures`` ({"yardstick", "bars"}) and ``observed`` are another family's (tests/_convlstm_models.py)."""
    runs = {"fp32_cpu": yard} if got is None else {who: got, "fp32_cpu": yard}
    rec = {"case": case.name,
           "forward_err_of_scale": {w: dm.worst_of(forward_errors(r["tensors"], ref["tensors"])) for w, r in runs.items()},
           "gradient_err_of_scale": {w: dm.worst_of(dm.tensor_errors(r["grads"], ref["grads"])) for w, r in runs.items()},
           "worst_slice": {w: dm.worst_slice(r["grads"], ref["grads"], slices) for w, r in runs.items()}}
    rec.update({"yardstick": yardstick(), "bars": bars()} if figures is None else figures)
    dm.observe(rec, observed)
    return rec


def judge(label, got, ref, bar=None, slices=grad_slices, wider=None):
    """The assertions of a case, in this order: forward values within rtol 2e-4 / bars()["forward"] of the tensor's scale;
    a gradient that is identically zero in fp64 is exactly zero; every gradient within bars()["gradient"] of the tensor's
    scale (``check_grads``); every slice within bars()["slice"] of the SLICE's scale, and a slice that is identically zero
    in fp64 exactly zero (``dm.check_slices``).  Returns (worst slice error, "name[slice]").  ``bar`` and ``slices``
    replace this family's; ``wider`` {gradient name: bar} holds the named tensors, whole and per slice, to their own bar."""
    from conftest import check_grads
    bar, wider = bars() if bar is None else bar, wider or {}
    assert set(got["tensors"]) == set(ref["tensors"]), sorted(set(got["tensors"]) ^ set(ref["tensors"]))
    for n, r in ref["tensors"].items():
        np.testing.assert_allclose(got["tensors"][n], r, rtol=FWD_RTOL, atol=bar["forward"] * max(1.0, float(np.abs(r).max())),
                                   err_msg=f"{label}: {n}")
    assert set(got["grads"]) == set(ref["grads"]), sorted(set(got["grads"]) ^ set(ref["grads"]))
    for n, r in ref["grads"].items():
        if not r.any():
            assert not got["grads"][n].any(), f"{label}: {n} is zero in fp64 (no path from the loss), yet a gradient was written"
    check_grads(label, {n: g for n, g in got["grads"].items() if n not in wider}, ref["grads"].__getitem__, tol=bar["gradient"])
    for n, tol in wider.items():
        if n in got["grads"]:
            check_grads(f"{label} {n}", {n: got["grads"][n]}, ref["grads"].__getitem__, tol=tol)
    tol = {n: max(bar["slice"], wider.get(n, 0.0)) for n in ref["grads"]} if wider else bar["slice"]
    return dm.check_slices(label, got["grads"], ref["grads"], tol, slices=slices, zero_tol=0.0)
