"""Builders of the delay-surrogate tests (tests/test_delay_surrogate_host.py, tests/test_delay_surrogate_gpu.py) and the
cases, operating points, slice bars and runner that tests/test_delay_regimes_host.py and tests/test_delay_regimes_gpu.py
share: the host file shows on the CPU that every case reaches its regime and what fp32 torch loses there; the GPU file
runs the same cases, on the same inputs, through csrc/delay.hip."""
import copy
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TENSORS = ("outputs", "deltas", "inlatents", "outlatents", "context_s", "context_a")
MLP0 = "transition_model.fwd_model.0.linear.weight"


def golden():
    """(delay_golden.npz, b8 states [8, 20, 1, 64], b8 actions [8, 20, 1, 4], surrogate_golden.npz): the delay fixture reuses
    the surrogate fixture's states and the latent fixture's 4-actuator actions."""
    shared, latent = np.load(os.path.join(GOLDEN, "surrogate_golden.npz")), np.load(os.path.join(GOLDEN, "latent_golden.npz"))
    return (np.load(os.path.join(GOLDEN, "delay_golden.npz")), torch.from_numpy(shared["b8_states"]),
            torch.from_numpy(latent["lstm_actions"]), shared)


def build(scaled=False, seed=0, perturb=False, delay=None):
    """(surrogate, PDETrainingModule) of KSDelayCNNSurrogateFactory on the CPU in fp32, as the fixture: delta = tstep = 0.25,
    tau = 5, tbtt = 10, MSELoss(reduction="none").  ``perturb``: non-trivial LayerNorm affine parameters and biases.
    ``delay``: rebuild the transition with another window length (a layout the kernels refuse)."""
    import _latent_models as lm
    import pdecontrol.architectures as arch
    from pdecontrol.surrogates.training import PDETrainingModule
    from pdecontrol.surrogates.transition import DelayTransitionModel
    from pdecontrol.surrogates.models.fcnn import LinearBlock
    und, dsc = lm.normalize_pair() if scaled else (None, None)
    torch.manual_seed(seed)
    f = arch.KSDelayCNNSurrogateFactory()
    model = f.model()
    if delay is not None:
        fwd = torch.nn.Sequential(LinearBlock(12 * delay, 8, 12, 8, activation=torch.nn.ELU),
                                  LinearBlock(12, 8, 8, 8, activation=torch.nn.ELU),
                                  LinearBlock(8, 8, 8, 8, activation=torch.nn.Tanh))
        model["transition_model"] = DelayTransitionModel(8, 8, 4, 8, fwd_model=fwd, delay=delay)
    sur = f.surrogate(delta=0.25, dscaling=dsc, tau=5, **model)
    module = PDETrainingModule(surrogate=sur, loss=torch.nn.MSELoss(reduction="none"), tstep=0.25, delta=0.25,
                               undscaling=und, tau=5, tbtt=10)
    if perturb:
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for name, p in sur.named_parameters():
                if "norm" in name or name.endswith(".bias"):
                    p.add_(0.3 * torch.randn(p.shape, generator=g))
    return sur, module


def stored(g, prefix, name, value):
    """Compare ``value`` with the fixture's record of it: the full tensor, or fp64 sum, sum of squares and every 97th element."""
    v = np.asarray(value)
    if f"{prefix}/{name}" in g.files:
        np.testing.assert_array_equal(v, g[f"{prefix}/{name}"], err_msg=name)
        return
    v64 = v.astype(np.float64)
    assert v64.sum() == g[f"{prefix}sum/{name}"] and (v64 * v64).sum() == g[f"{prefix}sq/{name}"], name
    np.testing.assert_array_equal(v.reshape(-1)[::97], g[f"{prefix}pick/{name}"], err_msg=name)


def recorded(g, prefix):
    """Names of the tensors the fixture records under ``prefix``."""
    out = set()
    for k in g.files:
        head, _, name = k.partition("/")
        if head in (prefix, prefix + "pick"):
            out.add(name)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# operating points (tests/test_delay_regimes_host.py shows that each is reached)
# ---------------------------------------------------------------------------------------------------------------------
def _surrogate(module):
    return getattr(module, "surrogate", module)


def regime(module, name):
    """A copy of ``module`` (a surrogate or its training module) moved to an operating point.
    ``saturated``: MLP weights x 3.5, decoder weights (LayerNorm gains included) x 2 -- a share of ``outlatents`` and
    ``deltas`` within 1e-3 of +-1 (the tanh slope 1 - y*y at its small end) while another share stays below 0.9.
    ``elu_deep``: every third bias in front of an ELU (MLP, action encoder, decoder channels) lowered by 8, so those
    pre-activations sit below -5 and the ELU slope y + 1 sits near 0."""
    out = copy.deepcopy(module)
    with torch.no_grad():
        for pname, p in _surrogate(out).named_parameters():
            if name == "saturated":
                if pname.startswith("transition_model.fwd_model") and pname.endswith(".weight"):
                    p.mul_(3.5)
                elif pname.startswith("state_decoder") and pname.endswith(".weight"):
                    p.mul_(2.0)
            elif name == "elu_deep":
                if pname in ("transition_model.fwd_model.0.linear.bias", "transition_model.fwd_model.1.linear.bias",
                             "action_encoder.model.0.linear.bias", "state_decoder.model.block_l0.deconvolution.bias",
                             "state_decoder.model.block_l1.deconvolution.bias"):
                    p[::3] -= 8.0
            else:
                raise ValueError(name)
    return out


def elu_preactivations(module, run):
    """Every value an nn.ELU of ``module`` receives while ``run()`` executes (forward hooks), as one flat tensor."""
    seen = []
    hooks = [m.register_forward_hook(lambda m, i, o: seen.append(i[0].detach().reshape(-1)))
             for m in module.modules() if type(m) is torch.nn.ELU]
    try:
        run()
    finally:
        for h in hooks:
            h.remove()
    return torch.cat(seen)


class EluByExp(torch.autograd.Function):
    """An emulated fault: exp(x) - 1 rounded in fp32 where a kernel has expm1f; the slope from the output, y + 1."""

    @staticmethod
    def forward(ctx, x):
        y = torch.where(x > 0, x, torch.exp(x) - 1)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        y, = ctx.saved_tensors
        return g * torch.where(y > 0, torch.ones_like(y), y + 1)


class EluFlooredSlope(torch.autograd.Function):
    """An emulated fault: the ELU slope y + 1 floored at 1e-3: bit-identical wherever the pre-activation is above
    log(1e-3) = -6.9."""

    @staticmethod
    def forward(ctx, x):
        y = torch.nn.functional.elu(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        y, = ctx.saved_tensors
        return g * torch.where(y > 0, torch.ones_like(y), torch.clamp(y + 1, min=1e-3))


class TanhAbsSlope(torch.autograd.Function):
    """An emulated fault: the tanh slope taken as 1 - |y| where a kernel has 1 - y*y."""

    @staticmethod
    def forward(ctx, x):
        y = torch.tanh(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        y, = ctx.saved_tensors
        return g * (1 - y.abs())


class TanhFlooredSlope(torch.autograd.Function):
    """An emulated fault: the tanh slope 1 - y*y floored at 1e-3, a "safety" clamp: bit-identical wherever |y| < 0.9995."""

    @staticmethod
    def forward(ctx, x):
        y = torch.tanh(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        y, = ctx.saved_tensors
        return g * torch.clamp(1 - y * y, min=1e-3)


class Act(torch.nn.Module):
    """An activation module around an autograd Function."""

    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x):
        return self.fn.apply(x)


def swap_activation(sur, cls, fn):
    """Replace every activation module of exactly type ``cls`` in ``sur`` by ``Act(fn)``."""
    for m in list(sur.modules()):
        for name, child in list(m.named_children()):
            if type(child) is cls:
                setattr(m, name, Act(fn))
    return sur


def small_states(B, S, amp, seed):
    """[B, S, 1, 64] fp64 smooth fields amp * (sin(x + phi) + 0.5 cos(2 x + psi)) about zero, random phases per field: the
    state near the fixed point the dissipation controller drives to."""
    g = torch.Generator().manual_seed(seed)
    x = 2 * np.pi * torch.arange(64, dtype=torch.float64) / 64
    phi, psi = (2 * np.pi * torch.rand(B, S, 1, 1, generator=g, dtype=torch.float64) for _ in range(2))
    return amp * (torch.sin(x + phi) + 0.5 * torch.cos(2 * x + psi))


def uniform_inputs(B, S, A, seed, amp=1.0):
    """White noise in [-amp, amp] / [-1, 1]: ``_inputs`` of tests/test_delay_surrogate_gpu.py."""
    g = torch.Generator().manual_seed(seed)
    st = (torch.rand(B, S, 1, 64, generator=g, dtype=torch.float64) * 2 - 1) * amp
    ac = torch.rand(B, A, 1, 4, generator=g, dtype=torch.float64) * 2 - 1
    return st, ac


def context(B, seed):
    """A carried context: ``_hidden`` of tests/test_delay_surrogate_gpu.py."""
    g = torch.Generator().manual_seed(seed)
    return (0.5 * torch.randn(B, 3, 8, 8, generator=g, dtype=torch.float64),
            0.5 * torch.randn(B, 3, 4, 8, generator=g, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    """One rollout and one backward.  ``states``: None (white noise in [-1, 1]) or (amp, offset) of ``small_states``;
    ``cot``: the returned tensors the loss <tensor, fixed random weights> is summed over."""

    def __init__(self, B, S, K, hidden, scaled, regime=None, states=None, cot=TENSORS, group="", kind="every"):
        self.B, self.S, self.K, self.hidden, self.scaled = B, S, K, hidden, scaled
        self.regime, self.states, self.cot, self.group, self.kind = regime, states, tuple(cot), group, kind
        self.seed = S * 100 + K * 10 + B
        parts = [f"B{B}-S{S}-K{K}", "hidden" if hidden else "zero", "affine" if scaled else "identity"]
        if regime:
            parts.append(regime)
        if states:
            parts.append(f"amp{states[0]:g}+{states[1]:g}")
        if kind != "every":
            parts.append(kind)
        if self.cot != TENSORS:
            parts.append("d_" + "+".join(self.cot))
        self.name = "-".join(parts)

    def inputs(self):
        """(states, actions, context or None) in fp64 on the CPU."""
        import _grad_contract_models as gm
        st, ac = uniform_inputs(self.B, self.S, len(gm.grid(self.K, self.kind, 0.25)[0]), self.seed)
        if self.states:
            st = small_states(self.B, self.S, self.states[0], self.seed) + self.states[1]
        return st, ac, (context(self.B, self.seed + 7) if self.hidden else None)


COTANGENTS = [(n,) for n in TENSORS] + [("outputs", "context_s"), ("deltas", "context_a"), ("inlatents", "outlatents")]
COTANGENT_CASES = [Case(5, 2, 4, True, True, cot=c, group="cotangent") for c in COTANGENTS]
# S > K (the b*S + k stride with su = K, rows su..S of d_states zeroed), K = 2 (the returned context mixes one given slot
# with two produced ones) with and without a given context, K = 1 from three given states
EDGE_CASES = [Case(3, 6, 4, True, True, group="edge"), Case(3, 1, 2, True, False, group="edge"),
              Case(3, 2, 2, False, True, group="edge"), Case(1, 3, 1, True, False, group="edge")]
# amp 1e-3 rides on an offset of 0.05, amp 1e-2 and 1e-4 on none: an exactly constant row, or a large offset, makes the
# first convolution's weight gradient cancel to nothing and fp32 torch itself is then off by orders of magnitude (offset
# 0.7 at amp 1e-3: 9e-4 of scale), so no bar could be taken from it.  amp 1e-4 is the amplitude at which exp(x) - 1 in
# place of expm1 shows (tests/test_delay_regimes_host.py): at 1e-3 that fault still passes
REGIME_CASES = [Case(7, 3, 6, True, True, regime="saturated", group="regime"),
                Case(7, 3, 12, True, True, regime="saturated", group="regime"),
                Case(7, 3, 6, True, True, regime="elu_deep", group="regime"),
                Case(7, 3, 6, True, True, states=(1e-3, 0.05), group="small"),
                Case(7, 3, 6, True, True, states=(1e-2, 0.0), group="small"),
                Case(7, 3, 6, True, True, states=(1e-4, 0.0), group="small")]
BASE_CASES = [Case(7, 3, 3, True, True, group="base"), Case(64, 5, 10, False, True, group="base"),
              Case(1, 5, 10, True, False, group="base")]
# the grid of tests/test_delay_surrogate_gpu.py (same modules, inputs and loss): its first nine rows are the grid the
# regimes were added to, the last two the rows it gained with them
GRID_CASES = [Case(*row[:5], kind=row[5], group="grid") for row in (
    (1, 1, 1, False, False, "every"), (7, 3, 3, True, True, "every"), (64, 5, 10, False, True, "every"),
    (300, 1, 20, True, False, "every"), (1, 5, 10, True, False, "every"), (7, 1, 20, False, True, "every"),
    (64, 1, 1, True, True, "every"), (300, 3, 3, False, False, "every"), (7, 5, 10, True, True, "skip"),
    (5, 6, 4, False, True, "every"), (7, 1, 2, True, False, "every"))]

_MODULES = {}


def modules(scaled, regime_name=None):
    """(fp64 surrogate, fp32 surrogate) on the CPU at an operating point, built once: ``build(perturb=True)`` as the
    existing GPU tests, then ``regime``."""
    key = (scaled, regime_name)
    if key not in _MODULES:
        sur, _ = build(scaled=scaled, perturb=True)
        if regime_name:
            sur = regime(sur, regime_name)
        _MODULES[key] = (copy.deepcopy(sur).double(), sur)
    return _MODULES[key]


_REFERENCE = {}


def reference(case):
    """(fp64 result, fp32 CPU result) of a case, computed once and shared by every test that needs it."""
    if case.name not in _REFERENCE:
        ref, cpu = modules(case.scaled, case.regime)
        _REFERENCE[case.name] = (run_case(ref, case, dtype=torch.float64), run_case(cpu, case))
    return _REFERENCE[case.name]


def rollout_tensors(ro):
    return {"outputs": ro.outputs, "deltas": ro.deltas, "inlatents": ro.inlatents, "outlatents": ro.outlatents,
            "context_s": ro.hidden[0], "context_a": ro.hidden[1]}


def run_case(sur, case, device="cpu", dtype=torch.float32, inputs=None, tensors_of=rollout_tensors, loss_of=None):
    """One rollout of ``sur`` on ``case`` and the backward of its loss.  Returns {"tensors": {name: fp64 array},
    "grads": {name: fp64 array}} with the inputs' gradients as ``input.*``; an undefined gradient counts as zero.
    ``inputs``, ``tensors_of`` and ``loss_of(tensors, weights)`` replace the case's own (the host file's emulations)."""
    import _grad_contract_models as gm
    st, ac, h = case.inputs() if inputs is None else inputs
    mk = lambda t: t.to(device, dtype).clone().requires_grad_(True)
    st_l, ac_l, h_l = mk(st), mk(ac), (None if h is None else tuple(mk(t) for t in h))
    for p in sur.parameters():
        p.grad = None
    times, targets = gm.grid(case.K, case.kind, sur.delta)
    tensors = tensors_of(sur.rollout(st_l, ac_l, times, targets, hidden=h_l))
    weights = gm.loss_weights(tensors, case.seed)
    loss = gm.weighted_loss({n: tensors[n] for n in case.cot}, weights) if loss_of is None else loss_of(tensors, weights)
    loss.backward()
    grad = lambda t: (torch.zeros_like(t) if t.grad is None else t.grad).detach().cpu().double().numpy()
    grads = {"input.states": grad(st_l), "input.actions": grad(ac_l)}
    if h_l is not None:
        grads["input.context_s"], grads["input.context_a"] = grad(h_l[0]), grad(h_l[1])
    grads.update(gm.trainable_grads(sur))
    for p in sur.parameters():
        p.grad = None
    return {"tensors": {n: t.detach().cpu().double().numpy() for n, t in tensors.items()}, "grads": grads}


# ---------------------------------------------------------------------------------------------------------------------
# slices and bars
# ---------------------------------------------------------------------------------------------------------------------
def grad_slices(name, array):
    """[(label, index)] covering ``array``: the rollout's inputs per step, the contexts per slot, the first MLP weight per
    window column block (3 slots x {64 state columns, 32 action columns}); every other gradient is one slice."""
    if name in ("input.states", "input.actions"):
        return [(f"step{k}", (slice(None), k)) for k in range(array.shape[1])]
    if name in ("input.context_s", "input.context_a"):
        return [(f"slot{s}", (slice(None), s)) for s in range(array.shape[1])]
    if name == MLP0:
        out = []
        for s in range(3):
            out.append((f"slot{s}.state", (slice(None), slice(96 * s, 96 * s + 64))))
            out.append((f"slot{s}.action", (slice(None), slice(96 * s + 64, 96 * s + 96))))
        return out
    return [("all", Ellipsis)]


def _rel(got, ref):
    scale = float(np.abs(ref).max())
    return float(np.abs(got - ref).max()) / scale if scale > 0 else float(np.abs(got).max())


def tensor_errors(got, ref):
    """{name: max |g - g_ref| / max |g_ref|}: check_grads's figure."""
    return {n: _rel(np.asarray(got[n]), np.asarray(ref[n])) for n in ref}


def slice_errors(got, ref, slices=grad_slices):
    """{name: worst over its non-zero slices of max |g - g_ref| / max |g_ref| over the SLICE}; ``slices``: the splitting
    rule (``grad_slices`` here, tests/_fclstm_models.py has its own)."""
    out = {}
    for n in ref:
        g, r = np.asarray(got[n]), np.asarray(ref[n])
        errs = [_rel(g[idx], r[idx]) for _, idx in slices(n, r) if np.any(r[idx])]
        out[n] = max(errs) if errs else 0.0
    return out


def bars(yardstick, ref, floor):
    """(per-tensor bar, per-slice bar), each {name: max(floor, 4 x the fp32 CPU module's error on this case and this
    tensor's slices)}: the yardstick is measured against fp64, never against the kernels; four is the margin
    conftest.GRAD_TOL documents (observed x 4: summation order decides which element is worst)."""
    return ({n: max(floor, 4 * e) for n, e in tensor_errors(yardstick, ref).items()},
            {n: max(floor, 4 * e) for n, e in slice_errors(yardstick, ref).items()})


def check_slices(label, got, ref, tol, slices=grad_slices, zero_tol=None):
    """Every slice (``slices``) of every gradient in ``ref``: one whose fp64 reference is non-zero lies within ``tol``
    (a number or {name: number}) of that SLICE's own maximum; one whose reference is identically zero (context slot 0,
    the d_states rows su..S, whatever the loss does not reach) is at most ``zero_tol`` (GRAD_TOL when None; 0 admits
    only exact zeros) x the reference tensor's scale, which is exactly zero where the whole tensor is.  No slice is left
    out.  Returns (worst error, "name[slice]")."""
    from conftest import GRAD_TOL
    zero_tol = GRAD_TOL if zero_tol is None else zero_tol
    assert set(got) == set(ref), (label, sorted(set(got) ^ set(ref)))
    worst, bad = (0.0, None), []
    for n in ref:
        g, r = np.asarray(got[n]), np.asarray(ref[n])
        assert g.shape == r.shape, (label, n, g.shape, r.shape)
        t = tol[n] if isinstance(tol, dict) else tol
        covered = np.zeros(r.shape, dtype=bool)
        for tag, idx in slices(n, r):
            covered[idx] = True
            if np.any(r[idx]):
                err = _rel(g[idx], r[idx])
                if err > worst[0]:
                    worst = (err, f"{n}[{tag}]")
                if not err <= t:
                    bad.append(f"{n}[{tag}] off by {err:.3e} of the slice's scale (tolerance {t:.1e})")
            else:
                stray, bound = float(np.abs(g[idx]).max()), zero_tol * float(np.abs(r).max())
                if not stray <= bound:
                    bad.append(f"{n}[{tag}] is zero in fp64 but reaches {stray:.3e} (at most {bound:.1e})")
        assert covered.all(), (label, n)
    assert not bad, f"{label}: " + "; ".join(bad)
    return worst


def scale_error(got, ref):
    """max |got - ref| / max(1, max |ref|): the figure of the forward bar's absolute floor."""
    return float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max()))


def observed_path(name="delay_regimes"):
    from conftest import GRAD_LOG
    return os.path.join(os.path.dirname(GRAD_LOG), f"{name}_observed.jsonl")


def observe(rec, name="delay_regimes"):
    """Append one record to ``name``_observed.jsonl next to the gradient parity log."""
    print(name.replace("_", " "), json.dumps(rec))
    try:
        os.makedirs(os.path.dirname(observed_path(name)), exist_ok=True)
        with open(observed_path(name), "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


def worst_of(errors):
    name = max(errors, key=errors.get)
    return {"name": name, "err": errors[name]}


def worst_slice(got, ref, slices=grad_slices):
    """{"name": "tensor[slice]", "err": ...} of the worst non-zero slice; judges nothing."""
    table = {}
    for n in ref:
        g, r = np.asarray(got[n]), np.asarray(ref[n])
        table.update({f"{n}[{tag}]": _rel(g[idx], r[idx]) for tag, idx in slices(n, r) if np.any(r[idx])})
    return worst_of(table)


FWD = dict(rtol=2e-4, atol_scale=2e-5)      # the forward bar of tests/test_delay_surrogate_gpu.py


def record(case, ref, yard, got=None, who="kernels"):
    """The observed-file record of one case: the fp32 CPU module (``yard``) and, when given, the kernels (``got``) against
    the fp64 module (``ref``); the bars that the yardstick lifts above GRAD_TOL are listed."""
    from conftest import GRAD_TOL
    runs = {"fp32_cpu": yard} if got is None else {who: got, "fp32_cpu": yard}
    tbar, sbar = bars(yard["grads"], ref["grads"], GRAD_TOL)
    rec = {"case": case.name,
           "forward_err_of_scale": {w: max(scale_error(r["tensors"][n], ref["tensors"][n]) for n in TENSORS)
                                    for w, r in runs.items()},
           "gradient_err_of_scale": {w: worst_of(tensor_errors(r["grads"], ref["grads"])) for w, r in runs.items()},
           "worst_slice": {w: worst_slice(r["grads"], ref["grads"]) for w, r in runs.items()},
           "yardstick": {"tensor_bars_above_grad_tol": {n: b for n, b in tbar.items() if b > GRAD_TOL},
                         "slice_bars_above_grad_tol": {n: b for n, b in sbar.items() if b > GRAD_TOL}}}
    observe(rec)
    return rec


def judge(label, got, ref, yard):
    """The assertions of a case, in this order: forward values on the FWD bar; every gradient within its per-tensor bar
    of the tensor's scale (``check_grads``); every slice within its per-slice bar of the slice's scale, zero slices on the
    zero rule (``check_slices``).  Both bars are ``bars``: GRAD_TOL unless fp32 torch itself is above GRAD_TOL / 4."""
    from conftest import GRAD_TOL, check_grads
    for n in TENSORS:
        r = ref["tensors"][n]
        np.testing.assert_allclose(got["tensors"][n], r, rtol=FWD["rtol"],
                                   atol=FWD["atol_scale"] * max(1.0, float(np.abs(r).max())), err_msg=f"{label}: {n}")
    tbar, sbar = bars(yard["grads"], ref["grads"], GRAD_TOL)
    assert set(got["grads"]) == set(ref["grads"]), sorted(set(got["grads"]) ^ set(ref["grads"]))
    check_grads(label, {n: g for n, g in got["grads"].items() if tbar[n] == GRAD_TOL}, ref["grads"].__getitem__)
    for n, bar in tbar.items():
        if bar > GRAD_TOL:
            check_grads(f"{label} {n}", {n: got["grads"][n]}, ref["grads"].__getitem__, tol=bar)
    return check_slices(label, got["grads"], ref["grads"], sbar)
