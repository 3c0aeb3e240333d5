"""Whole-rollout kernels behind the two fully-connected LSTM baselines (``KSAutoRegFullyConnectedLSTM``, ``KSLatentLSTM``;
C ABI: include/surrogate_hip.h ``sur_fc_*``; kernels: csrc/sur_fclstm.hip, part of libsurrogate_hip.so).

The rollout contract is the reference's (pdecontrol/surrogates/surrogate.py:79-206 with LSTMTransitionModel,
transition.py:34-109): teacher forced on the given states (H replaced by the encoded state, C kept), free running on the
LSTM's own state afterwards; the autoregressive form integrates the decoded, scaled delta in state space, the latent form
integrates h' in latent space and decodes the running latent.  Here a rollout call is

  forward   ONE launch: a wave per sample runs every step, the 6 672 weights staged in LDS once per workgroup;
  backward  TWO launches: the reverse walk (input gradients, one row of pre-activation gradients per sample and step),
            then the weight gradients as sums of outer products in a fixed order (bit-identical run to run).

``_FCRolloutFn`` is one autograd node per rollout call: the parameters go in as inputs and their gradients come out of
``backward``, so optimizers, frozen parameters and hipGraph capture see ordinary autograd.  The path is opt-in
(``ops.enable_fused_fc`` / ``ops.fused_fc`` / ``PDECONTROL_FUSED_FC=1``); off, and on the CPU, the torch spelling of
pdecontrol/surrogates/surrogate.py runs.
"""
import torch

from pdecontrol.surrogates import hipops

N, E1, HID, D1, NACT = 64, 32, 16, 32, 4
FORM_AUTOREG, FORM_LATENT = 0, 1
ACT_SILU_TANH, ACT_ELU_IDENTITY = 0, 1
NPARAM = 6672

_check = hipops._check
_stream, _ptr = hipops._stream, hipops._ptr


def load():
    return hipops.load()


# ---------------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------------
def _leaves(surrogate):
    """The modules the layout is read from, by their fixed paths (raises where the tree has another shape).  Plain
    ``_modules`` lookups: nn.Module's attribute fallback would make this walk cost more than the launch it guards."""
    top = surrogate._modules
    enc, dec = top["state_encoder"]._modules["model"]._modules, top["state_decoder"]._modules["model"]._modules
    tm = top["transition_model"]
    blocks = [enc["0"]._modules, enc["1"]._modules, dec["0"]._modules, dec["1"]._modules]
    return (*[m for blk in blocks for m in (blk["linear"], blk["activation"])], top["action_encoder"]._modules["model"], tm,
            tm._modules["lstm"])


def _kernel_parameters(surrogate):
    """The parameters of the flat vector: named_parameters() order without the frozen initial state H0 / C0 (``_examine``
    checks that these twelve, in this order, are what named_parameters() yields)."""
    leaves = _leaves(surrogate)
    lstm = leaves[-1]._parameters
    return [p for lin in leaves[0:8:2] for p in (lin._parameters["weight"], lin._parameters["bias"])] + \
        [lstm["weight_ih_l0"], lstm["weight_hh_l0"], lstm["bias_ih_l0"], lstm["bias_hh_l0"]]


def _form_and_act(surrogate):
    """(form, activation set) of a supported surrogate, or None.  A rollout asks several times per call and the walk over
    the tree costs more than the launch, so the answer is kept on the surrogate, keyed by the identity of every module it
    was read from: replacing a layer, an activation or the transition model examines the tree again."""
    try:
        key = (type(surrogate),) + tuple(map(id, _leaves(surrogate)))
    except (AttributeError, KeyError, TypeError):
        return None
    kept = surrogate.__dict__.get("_fc_layout")
    if kept is None or kept[0] != key:
        kept = (key, _examine(surrogate))
        object.__setattr__(surrogate, "_fc_layout", kept)
    return kept[1]


def _examine(surrogate):
    from torch import nn

    from pdecontrol.surrogates.delay_hip import _linear_blocks
    from pdecontrol.surrogates.surrogate import AutoRegPDESurrogate, LatentAutoRegPDESurrogate
    from pdecontrol.surrogates.transition import LSTMTransitionModel
    try:
        tm = surrogate.transition_model
        if type(tm) is not LSTMTransitionModel:
            return None
        if type(surrogate) is AutoRegPDESurrogate:
            form, act, hidden_act, last_act = FORM_AUTOREG, ACT_SILU_TANH, nn.SiLU, nn.Tanh
        elif type(surrogate) is LatentAutoRegPDESurrogate:
            form, act, hidden_act, last_act = FORM_LATENT, ACT_ELU_IDENTITY, nn.ELU, nn.Identity
        else:
            return None
        if (tm.schannels, tm.ssize, tm.achannels, tm.asize) != (1, HID, 1, NACT):
            return None
        lstm = tm.lstm
        if not (type(lstm) is nn.LSTM and (lstm.input_size, lstm.hidden_size, lstm.num_layers) == (NACT, HID, 1)
                and lstm.bias and lstm.batch_first and not lstm.bidirectional and lstm.proj_size == 0
                and lstm.dropout == 0.0):
            return None
        if tm.H0.requires_grad or tm.C0.requires_grad or tm.H0.shape != (HID,) or tm.C0.shape != (HID,):
            return None
        if type(surrogate.action_encoder.model) is not nn.Identity:
            return None
        if not _linear_blocks(surrogate.state_encoder.model, ((1, N, 1, E1, hidden_act), (1, E1, 1, HID, hidden_act))):
            return None
        if not _linear_blocks(surrogate.state_decoder.model, ((1, HID, 1, D1, hidden_act), (1, D1, 1, N, last_act))):
            return None
        named = [p for name, p in surrogate.named_parameters() if name not in ("transition_model.H0", "transition_model.C0")]
        mine = _kernel_parameters(surrogate)
        if len(named) != len(mine) or any(a is not b for a, b in zip(named, mine)) or len(list(surrogate.buffers())) != 0:
            return None
        if sum(p.numel() for p in mine) != NPARAM:
            return None
        return form, act
    except (AttributeError, KeyError, TypeError):
        return None


def fused_fc_supported(surrogate):
    """True when ``surrogate`` has exactly the module tree of KSAutoRegFullyConnectedLSTM or KSLatentLSTM: surrogate class,
    LinearBlock sizes 64 -> 32 -> 16 and 16 -> 32 -> 64, the factory's activations, an Identity action encoder and a
    one-layer nn.LSTM(4, 16) with both biases and a frozen H0 / C0."""
    return _form_and_act(surrogate) is not None


def geometry_unsupported(surrogate, tensor):
    """None when the kernels run this (layout-supported) surrogate on ``tensor`` (the states), else the reason."""
    if tensor.dtype != torch.float32 or any(p.dtype != torch.float32 for p in _kernel_parameters(surrogate)):
        return f"the FC-LSTM kernels are fp32 only (input {tensor.dtype})"
    form, act = _form_and_act(surrogate)
    if form == FORM_AUTOREG:
        try:
            hipops._dscale_constants(surrogate.dscaling)
        except hipops.SurrogateHipError as e:
            return f"the FC-LSTM kernels: {e}"
    lib = load()
    rc = lib.sur_fc_supported(int(tensor.shape[-1]), E1, HID, D1, NACT, form, act, NPARAM)
    return None if rc == 0 else lib.sur_last_error().decode(errors="replace")


# ---------------------------------------------------------------------------------------------------------------------
# the rollout node
# ---------------------------------------------------------------------------------------------------------------------
class _FCRolloutFn(torch.autograd.Function):
    """K rollout steps of B samples: sur_fc_forward now, sur_fc_backward when the caller's loss is back-propagated.
    states [B, S, 1, 64], actions [B, K, 4] (already mapped to the internal steps), h_in / c_in [B, 16]; returns outputs,
    deltas [B, K, 1, 64] (None in the latent form), inlatents (None when not asked for), outlatents [B, K, 1, 16] and the
    final h, c [B, 16]."""

    @staticmethod
    def forward(ctx, states, actions, h_in, c_in, form, act, with_inlatents, keep, delta, mul, add, *params):
        states, actions, c_in = states.contiguous(), actions.contiguous(), c_in.contiguous()
        flat = torch.cat([p.detach().reshape(-1) for p in params])
        b, s = states.shape[:2]
        k = actions.shape[1]
        dev = states.device
        new = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)
        outputs, outl = new(b, k, 1, N), new(b, k, 1, HID)
        deltas = new(b, k, 1, N) if form == FORM_AUTOREG else None
        inl = new(b, k, 1, HID) if with_inlatents else None
        h_out, c_out = new(b, HID), new(b, HID)
        needs_grad = keep and any(ctx.needs_input_grad)   # keep: grad mode at the call (it is off in here)
        lib = load()
        saved = new(lib.sur_fc_saved_floats(b, k)) if needs_grad else None
        _check(lib.sur_fc_forward(_stream(), _ptr(flat), form, act, b, s, k, _ptr(states), _ptr(actions), _ptr(h_in),
                                  _ptr(c_in), delta, mul, add, _ptr(outputs), _ptr(deltas), _ptr(inl), _ptr(outl),
                                  _ptr(h_out), _ptr(c_out), _ptr(saved)))
        if needs_grad:
            ctx.save_for_backward(flat, states, actions, c_in, saved)
        ctx.form, ctx.act, ctx.delta, ctx.mul = form, act, delta, mul
        ctx.shapes = [p.shape for p in params]
        ctx.set_materialize_grads(False)
        return outputs, deltas, inl, outl, h_out, c_out

    @staticmethod
    def backward(ctx, d_out, d_del, d_inl, d_outl, d_h, d_c):
        flat, states, actions, c_in, saved = ctx.saved_tensors
        needs = ctx.needs_input_grad
        cont = lambda t: None if t is None else t.contiguous()
        d_out, d_del, d_inl, d_outl, d_h, d_c = map(cont, (d_out, d_del, d_inl, d_outl, d_h, d_c))
        b, s = states.shape[:2]
        k = actions.shape[1]
        dev = states.device
        d_states = torch.empty_like(states) if needs[0] else None
        d_actions = torch.empty_like(actions) if needs[1] else None
        d_h_in = torch.empty((b, HID), device=dev, dtype=torch.float32) if needs[2] else None
        d_c_in = torch.empty((b, HID), device=dev, dtype=torch.float32) if needs[3] else None
        d_flat = torch.empty_like(flat) if any(needs[11:]) else None
        lib = load()
        work = torch.empty(lib.sur_fc_workspace_floats(b, k), device=dev, dtype=torch.float32)
        _check(lib.sur_fc_backward(_stream(), _ptr(flat), ctx.form, ctx.act, b, s, k, _ptr(states), _ptr(actions), _ptr(c_in),
                                   _ptr(saved), ctx.delta, ctx.mul, _ptr(d_out), _ptr(d_del), _ptr(d_inl), _ptr(d_outl),
                                   _ptr(d_h), _ptr(d_c), _ptr(d_states), _ptr(d_actions), _ptr(d_h_in), _ptr(d_c_in),
                                   _ptr(d_flat), _ptr(work)))
        grads, at = [], 0
        for shape, need in zip(ctx.shapes, needs[11:]):
            n = shape.numel()
            grads.append(d_flat[at:at + n].view(shape) if need else None)
            at += n
        return (d_states, d_actions, d_h_in, d_c_in, None, None, None, None, None, None, None, *grads)


def fused_fc_rollout(surrogate, states, actions, times, targets, hidden):
    """GPU rollout of the two FC-LSTM factories: the same ModelRollout as the torch spelling of
    AutoRegPDESurrogate.rollout / LatentAutoRegPDESurrogate.rollout, from one sur_fc_forward launch.
    states [B, S, 1, 64], actions [B, A, 1, 4]; ``hidden`` (H, C), each [1, B, 16], or None (the frozen H0 / C0)."""
    from pdecontrol.mbrl.types import ModelRollout
    from pdecontrol.surrogates.surrogate import action_and_target_indices, take_steps
    form, act = _form_and_act(surrogate)
    aidx, tidx = action_and_target_indices(times, targets, surrogate.delta)
    acts = take_steps(actions, aidx.tolist())
    b = states.shape[0]
    acts = acts.reshape(b, acts.shape[1], NACT)
    tm = surrogate.transition_model
    if hidden is None:
        h_in, c_in = tm.H0.expand(b, HID), tm.C0.expand(b, HID)
    else:
        h_in, c_in = hidden[0].reshape(b, HID), hidden[1].reshape(b, HID)
    if form == FORM_AUTOREG:
        mul, add = hipops._dscale_constants(surrogate.dscaling)
        with_inl = bool(surrogate.reencode_predictions)
    else:
        mul, add, with_inl = 1.0, 0.0, True
    outputs, deltas, inl, outl, h, c = _FCRolloutFn.apply(states, acts, h_in, c_in, form, act, with_inl, torch.is_grad_enabled(),
                                                          float(surrogate.delta), mul, add, *_kernel_parameters(surrogate))
    pick = tidx.tolist()
    if form == FORM_LATENT:    # the deltas stay in torch around the node, unpicked, as in the torch spelling
        deltas = surrogate.dscaling.Inverse(torch.diff(torch.cat((states[:, :1], outputs), dim=1), dim=1) / surrogate.delta)
    else:
        deltas = take_steps(deltas, pick)
    return ModelRollout(inlatents=take_steps(inl, pick) if inl is not None else None, outlatents=take_steps(outl, pick),
                        deltas=deltas, outputs=take_steps(outputs, pick), hidden=(h.unsqueeze(0), c.unsqueeze(0)))
