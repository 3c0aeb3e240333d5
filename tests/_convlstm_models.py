"""Cases, operating points, slices and bars of the ConvLSTM surrogate's regime tests (tests/test_convlstm_regimes_host.py,
tests/test_convlstm_regimes_gpu.py): the host file shows on the CPU that every case reaches its regime, what fp32 torch
loses there and which emulated faults the bars catch; the GPU file runs the same cases, on the same inputs, through
csrc/sur_kernels.hip (``hipops.fused_rollout``).  The modules are ``gm.ks_module(N, scaled)`` of the gradient-contract
tests; the reference is ``deepcopy(...).double()`` on the CPU on the per-operator path, the yardstick the same module in
fp32 on the CPU; the runner, the judge and the observed-file writer are those of tests/_fclstm_models.py."""
import copy

import numpy as np
import torch

import _delay_models as dm
import _fclstm_models as fm
import _grad_contract_models as gm

TENSORS = ("outputs", "deltas", "outlatents", "hidden_h", "hidden_c")
CELL = "transition_model.cnnlstmcell."
DEC_BIAS = "state_decoder.model.block_l0.deconvolution.bias"
NOISY_BIAS, NOISY_BIAS_TOL = DEC_BIAS, 2e-3       # tests/test_surrogate_grad_contracts_gpu.py documents the wider bar
LN_EPS = 1e-5
# tuned on the fp64 CPU module (tests/test_convlstm_regimes_host.py asserts the floors): the eight gate convolutions x 8
# and the four biases x 4 put 10 % to 30 % of the sigmoid gates within 1e-3 of 0 or 1 and leave a quarter in [0.1, 0.9]
SAT = dict(weight=8.0, bias=4.0)
# every second channel of the decoder's first deconvolution bias moved by this: those SiLU + LayerNorm rows then have
# mean^2 / var >= 1e4.  The other channels keep the bias gradient's scale: a row-wide shift in front of a LayerNorm has
# next to no gradient of its own
DEC_SHIFT = 40.0


def regime(module, name):
    """A copy of ``module`` (the training module) moved to an operating point.  ``saturated``: the cell's gate
    convolutions x SAT["weight"], their biases x SAT["bias"].  ``decoder_offset``: DEC_BIAS[::2] + DEC_SHIFT."""
    out = copy.deepcopy(module)
    with torch.no_grad():
        for pname, p in out.surrogate.named_parameters():
            if name == "saturated":
                if pname.startswith(CELL) and pname.endswith(".weight"):
                    p.mul_(SAT["weight"])
                elif pname.startswith(CELL) and pname.endswith(".bias"):
                    p.mul_(SAT["bias"])
            elif name == "decoder_offset":
                if pname == DEC_BIAS:
                    p[::2] += DEC_SHIFT
            else:
                raise ValueError(name)
    return out


def smooth(B, S, N, seed):
    """[B, S, 1, N] fp64 fields sin(x + phi) + 0.5 sin(3 x + 2 phi), one random phase per field."""
    g = torch.Generator().manual_seed(seed)
    x = 2 * np.pi * torch.arange(N, dtype=torch.float64) / N
    phi = 2 * np.pi * torch.rand(B, S, 1, 1, generator=g, dtype=torch.float64)
    return torch.sin(x + phi) + 0.5 * torch.sin(3 * x + 2 * phi)


def noise(B, S, A, N, seed):
    """White noise in [-1, 1]: ``_inputs`` of tests/test_surrogate_grad_contracts_gpu.py."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, S, 1, N, generator=g, dtype=torch.float64) * 2 - 1,
            torch.rand(B, A, 1, N, generator=g, dtype=torch.float64) * 2 - 1)


def hidden(B, N, seed):
    """A carried (H, C), each [B, 16, N / 4]."""
    g = torch.Generator().manual_seed(seed)
    return (0.5 * torch.randn(B, 16, N // 4, generator=g, dtype=torch.float64),
            0.5 * torch.randn(B, 16, N // 4, generator=g, dtype=torch.float64))


class Case(fm.Case):
    """``fm.Case`` at grid width N.  ``states``: None (white noise in [-1, 1]) or (offset, amp) of ``offset + amp * smooth``;
    without a given hidden state H0 / C0 are trainable.  ``forward_only``: the rollout under no_grad, no backward."""

    def __init__(self, B, S, K, hidden, scaled, N=64, kind="every", cot=None, regime=None, states=None, group="",
                 forward_only=False):
        super().__init__("convlstm", B, S, K, hidden, scaled, kind=kind, cot=cot, regime=regime, group=group)
        self.N, self.states, self.forward_only = N, states, forward_only
        self.seed = N * 1000 + S * 100 + K * 10 + B
        parts = [f"N{N}", f"B{B}-S{S}-K{K}", "hidden" if hidden else "H0C0", "affine" if scaled else "identity"]
        if regime:
            parts.append(regime)
        if states:
            parts.append(f"{states[0]:g}+{states[1]:g}smooth")
        if kind != "every":
            parts.append(kind)
        if forward_only:
            parts.append("nograd")
        if self.cot is not None:
            parts.append("d_" + "+".join(self.cot))
        self.name = "-".join(parts)

    def inputs(self):
        st, ac = noise(self.B, self.S, len(gm.grid(self.K, self.kind, 0.25)[0]), self.N, self.seed)
        if self.states:
            st = self.states[0] + self.states[1] * smooth(self.B, self.S, self.N, self.seed)
        return st, ac, (hidden(self.B, self.N, self.seed + 7) if self.hidden else None)


COTANGENTS = [(n,) for n in TENSORS] + [("outputs", "hidden_c"), ("deltas", "hidden_h"), ("outlatents", "outputs")]
# S = 2, K = 4: dd_all, dout_all, dh_all (outlatents: every step; hidden_h: the last) and dc_all each alone
COTANGENT_CASES = [Case(5, 2, 4, True, True, cot=cot, group="cotangent") for cot in COTANGENTS] + \
    [Case(5, 2, 4, True, True, kind="skip", cot=("outputs",), group="cotangent")]
EDGE_SHAPES = ((1, 1, 1), (3, 6, 4), (3, 3, 3), (2, 1, 6), (4, 2, 3), (7, 3, 5))
EDGE_CASES = [Case(*shape, given, (i + given) % 2 == 0, group="edge") for i, shape in enumerate(EDGE_SHAPES)
              for given in (True, False)]
# the smallest batches past the grid limits: forward 2 * 513 = 1026 > 1024 (enc_fwd_kernel, dec_fwd_kernel); backward
# 4 * 193 = 772 > ENCODER_ROWS = 768 (both encoders) and > CHUNK_ROWS = 384 (dec_bwd_kernel, cell_wgrad_kernel)
ROUNDS_FORWARD = Case(513, 2, 2, True, True, group="rounds", forward_only=True)
ROUNDS_CASES = [ROUNDS_FORWARD, Case(193, 4, 4, True, True, group="rounds"), Case(193, 4, 4, False, True, N=256, group="rounds")]
SATURATED_CASES = [Case(6, 3, 5, True, scaled, N=N, regime="saturated", group="saturated")
                   for N in (64, 256) for scaled in (True, False)]
SMALL_CASES = [Case(6, 3, 5, True, True, states=(0.0, amp), group="small") for amp in (1e-3, 1e-4)]
OFFSET_POINTS = ((4.0, 0.01), (8.0, 0.02))
OFFSET_CASES = [Case(4, 2, 4, True, True, N=N, states=pt, group="offset") for N in (64, 256) for pt in OFFSET_POINTS] + \
    [Case(4, 2, 4, True, True, regime="decoder_offset", group="offset")]
# three rows of the grid of tests/test_surrogate_grad_contracts_gpu.py again, on the tight bars and per slice
BASE_CASES = [Case(5, 2, 5, True, True, group="base"), Case(5, 7, 4, False, False, N=128, group="base"),
              Case(1, 5, 5, True, False, N=256, kind="skip", group="base")]
YARD_GROUPS = {"main": COTANGENT_CASES + EDGE_CASES + ROUNDS_CASES + BASE_CASES, "saturated": SATURATED_CASES,
               "small": SMALL_CASES, "offset": OFFSET_CASES}
ALL_CASES = [c for cases in YARD_GROUPS.values() for c in cases]
# the grid the suite had at N = 64 (tests/test_surrogate_grad_contracts_gpu.py): the host file's "old grid"
GRID_CASES = [Case(B, S, K, given, scaled, kind=kind, group="grid") for S, K in ((1, 1), (2, 5), (5, 5), (7, 4))
              for B, scaled, kind, given in ((1, False, "every", False), (5, True, "skip", True))]


def yard_group(case):
    return case.group if case.group in YARD_GROUPS else "main"


_MODULES = {}


def modules(N, scaled, regime_name=None):
    """(fp64 surrogate, fp32 surrogate) on the CPU at an operating point, built once."""
    key = (N, scaled, regime_name)
    if key not in _MODULES:
        module = gm.ks_module(N, scaled)
        if regime_name:
            module = regime(module, regime_name)
        _MODULES[key] = (copy.deepcopy(module.surrogate).double(), module.surrogate)
    return _MODULES[key]


def rollout_tensors(ro):
    return {"outputs": ro.outputs, "deltas": ro.deltas, "outlatents": ro.outlatents, "hidden_h": ro.hidden[0],
            "hidden_c": ro.hidden[1]}


def run_case(sur, case, device="cpu", dtype=torch.float32, **kw):
    """``fm.run_case`` with the five tensors of the ConvLSTM rollout; H0 / C0 are trainable exactly when no hidden state
    is given.  A ``forward_only`` case runs under no_grad and has no gradients."""
    tm = sur.transition_model
    if case.forward_only:
        st, ac, h = case.inputs()
        to = lambda t: t.to(device, dtype)
        with torch.no_grad():
            ro = sur.rollout(to(st), to(ac), *gm.grid(case.K, case.kind, sur.delta), hidden=None if h is None else tuple(map(to, h)))
        return {"tensors": {n: t.cpu().double().numpy() for n, t in rollout_tensors(ro).items()}, "grads": {}}
    for p in (tm.H0, tm.C0):
        p.requires_grad_(not case.hidden)
    try:
        return fm.run_case(sur, case, device=device, dtype=dtype, tensors_of=rollout_tensors, **kw)
    finally:
        for p in (tm.H0, tm.C0):
            p.requires_grad_(False)
            p.grad = None


_REFERENCE = {}


def reference(case):
    """(fp64 result, fp32 CPU result) of a case, computed once and shared by every test that needs it; the fp32 CPU
    result is the yardstick."""
    if case.name not in _REFERENCE:
        ref, cpu = modules(case.N, case.scaled, case.regime)
        _REFERENCE[case.name] = (run_case(ref, case, dtype=torch.float64), run_case(cpu, case))
    return _REFERENCE[case.name]


# ---------------------------------------------------------------------------------------------------------------------
# slices and bars
# ---------------------------------------------------------------------------------------------------------------------
def grad_slices(name, array):
    """[(label, index)] covering ``array``.  The module keeps one tensor per gate convolution (Wxi .. Who) and per
    LayerNorm layer, so per gate and per layer is per tensor; each gate convolution is split further per kernel tap (the
    three circular shifts of cell_wgrad_kernel).  The rollout's inputs go per step.  Every other gradient is one slice."""
    if name.startswith(CELL) and name.endswith(".weight"):
        return [(f"tap{k}", (slice(None), slice(None), k)) for k in range(array.shape[2])]
    if name in ("input.states", "input.actions"):
        return [(f"step{k}", (slice(None), k)) for k in range(array.shape[1])]
    return [("all", Ellipsis)]


MARGIN = fm.MARGIN
_YARD = {}


def yardstick(group):
    """{"YARD_FWD", "YARD_GRAD", "YARD_SLICE", "YARD_NOISY", "YARD_TENSORS"} of a yardstick group (``YARD_GROUPS``): the
    largest error of the fp32 CPU module against fp64 over the group's cases -- forward values of the tensor's scale,
    gradients of the tensor's scale, gradient slices of the slice's scale; NOISY_BIAS apart, whole and sliced, as
    YARD_NOISY.  YARD_TENSORS: {gradient name: its own worst, whole or sliced} of the tensors on which fp32 torch itself
    is above GRAD_TOL / MARGIN.  Never from the kernels."""
    from conftest import GRAD_TOL
    if group not in _YARD:
        y, own = {"YARD_FWD": 0.0, "YARD_GRAD": 0.0, "YARD_SLICE": 0.0, "YARD_NOISY": 0.0}, {}
        for case in YARD_GROUPS[group]:
            ref, yard = reference(case)
            y["YARD_FWD"] = max(y["YARD_FWD"], *fm.forward_errors(yard["tensors"], ref["tensors"]).values())
            if case.forward_only:
                continue
            whole, sliced = dm.tensor_errors(yard["grads"], ref["grads"]), dm.slice_errors(yard["grads"], ref["grads"], grad_slices)
            for n in whole:
                own[n] = max(own.get(n, 0.0), whole[n], sliced[n])
            y["YARD_NOISY"] = max(y["YARD_NOISY"], whole.pop(NOISY_BIAS), sliced.pop(NOISY_BIAS))
            y["YARD_GRAD"], y["YARD_SLICE"] = max(y["YARD_GRAD"], *whole.values()), max(y["YARD_SLICE"], *sliced.values())
        y["YARD_TENSORS"] = {n: e for n, e in own.items() if MARGIN * e > GRAD_TOL and n != NOISY_BIAS}
        _YARD[group] = y
    return copy.deepcopy(_YARD[group])


def bars(group):
    """{"forward", "gradient", "slice", "noisy", "wider"} of a yardstick group: MARGIN = 8 x its yardstick (the margin of
    the FC-LSTM and delay pins: ~1-ulp hardware transcendentals, MFMA summation order), capped at the bars the suite has --
    forward 2e-5 of scale (with rtol 2e-4), GRAD_TOL for gradients and slices, NOISY_BIAS_TOL for NOISY_BIAS (never below
    the gradient bar).  The ``offset`` group is the one exception to the cap: there fp32 torch itself exceeds 2e-5 forward,
    and the bar is 8 x its own yardstick.  Its gradients: a large offset makes the first convolutions' weight gradients
    cancel, and fp32 torch is off by up to 2e-2 of scale on a handful of tensors; rather than lift every tensor to 8 x
    that, each tensor keeps GRAD_TOL unless fp32 torch itself is above GRAD_TOL / 8 on it somewhere in the group, and is
    then held to 8 x its OWN yardstick (``wider``, the rule of the delay pins' ``dm.bars``): never wider than the
    group-wide figure."""
    from conftest import GRAD_TOL
    y = yardstick(group)
    if group == "offset":
        out = {"forward": MARGIN * y["YARD_FWD"], "gradient": GRAD_TOL, "slice": GRAD_TOL,
               "noisy": max(GRAD_TOL, MARGIN * y["YARD_NOISY"]), "wider": {n: MARGIN * e for n, e in y["YARD_TENSORS"].items()}}
        return out
    out = {"forward": min(fm.FWD_CAP, MARGIN * y["YARD_FWD"]), "gradient": min(GRAD_TOL, MARGIN * y["YARD_GRAD"]),
           "slice": min(GRAD_TOL, MARGIN * y["YARD_SLICE"]), "wider": {}}
    out["noisy"] = max(out["gradient"], out["slice"], min(NOISY_BIAS_TOL, MARGIN * y["YARD_NOISY"]))
    return out


OBSERVED = "convlstm_regimes"


def figures(case):
    """The yardstick and the bars of the case's group as the observed file keeps them: of the per-tensor figures of the
    offset group their number and the largest only."""
    y, b = yardstick(yard_group(case)), bars(yard_group(case))
    own, wider = y.pop("YARD_TENSORS"), b.pop("wider")
    if wider:
        y["YARD_TENSORS"], b["wider"] = {"count": len(own), **dm.worst_of(own)}, {"count": len(wider), **dm.worst_of(wider)}
    return {"yardstick": y, "bars": b}


def record(case, ref, yard, got=None, who="kernels"):
    """The observed-file record of one case (convlstm_regimes_observed.jsonl next to the gradient parity log)."""
    if case.forward_only:
        runs = {"fp32_cpu": yard} if got is None else {who: got, "fp32_cpu": yard}
        rec = {"case": case.name, "forward_err_of_scale": {w: dm.worst_of(fm.forward_errors(r["tensors"], ref["tensors"]))
                                                           for w, r in runs.items()}, **figures(case)}
        dm.observe(rec, OBSERVED)
        return rec
    return fm.record(case, ref, yard, got, who, slices=grad_slices, figures=figures(case), observed=OBSERVED)


def judge(case, got, ref, label=None):
    """``fm.judge`` on the bars of the case's yardstick group, NOISY_BIAS on its own."""
    bar = bars(yard_group(case))
    return fm.judge(label or case.name, got, ref, bar=bar, slices=grad_slices, wider={NOISY_BIAS: bar["noisy"], **bar["wider"]})
