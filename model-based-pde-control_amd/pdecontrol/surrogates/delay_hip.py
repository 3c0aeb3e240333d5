"""Whole-rollout kernels behind the delay-embedding surrogate (``KSDelayCNNSurrogateFactory``; C ABI: include/delay_hip.h
``dly_*``; kernels: csrc/delay.hip).

The rollout contract is the reference's (pdecontrol/surrogates/surrogate.py:79-133 with DelayTransitionModel,
transition.py:299-382): teacher forced on the given states, free running on the re-encoded prediction afterwards,
``next = prev + delta * dscaling(decoder(MLP(window)))``.  Here a rollout call is

  forward   ONE launch: a workgroup per sample runs every step (encoders, the 3-slot window, MLP, decoder, integration);
  backward  TWO launches: a workgroup per sample walks the steps backwards into its own parameter-gradient row, then the
            rows are summed in sample order (bit-identical gradients run to run).

``_DelayRolloutFn`` is one autograd node per rollout call: the parameters go in as inputs and their gradients come out of
``backward``, so optimizers, frozen parameters and hipGraph capture see ordinary autograd.  The action-index map and the
target pick are ``take_steps`` on either side of the node.  The CPU path and ``PDECONTROL_FUSED=0`` run the torch
spelling of pdecontrol/surrogates/transition.py.
"""
import ctypes
import os

import torch

import hipbind

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.abspath(os.path.join(_HERE, "..", "..", "lib", "libdelay_hip.so"))

_p, _i, _l, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
SYMBOLS = (
    ("dly_param_count", _i, []),
    ("dly_supported", _i, [_i, _i, _i, _i, _i, _i, _i, _i]),
    ("dly_workspace_floats", _l, [_i]),
    ("dly_forward", _i, [_p, _p, _i, _i, _i, _p, _p, _p, _p, _f, _f, _f, _p, _p, _p, _p, _p, _p]),
    ("dly_backward", _i, [_p, _p, _i, _i, _i, _p, _p, _p, _p, _p, _p, _f, _f, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                          _p]),
    ("dly_last_error", ctypes.c_char_p, []),
)
N, DELAY, NACT = 64, 3, 4
_lib = None


class DelayHipError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is None:
        _lib = hipbind.open_library(LIB_PATH, SYMBOLS, DelayHipError, "The fused delay surrogate path has no fallback.")
    return _lib


_check = hipbind.checker(DelayHipError, "libdelay_hip", "dly_last_error", lambda: load())
_stream, _ptr = hipbind.stream, hipbind.ptr


# ---------------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------------
def _ln_width(ln):
    if ln is None:
        return None
    if not (isinstance(ln, torch.nn.LayerNorm) and ln.elementwise_affine and ln.eps == 1e-5 and ln.bias is not None
            and len(ln.normalized_shape) == 1):
        return -1
    return int(ln.normalized_shape[0])


def _act(m, cls):
    return type(m) is cls and (cls is not torch.nn.ELU or m.alpha == 1.0)


def _conv(c, cls, cin, cout, k, stride, pad, mode, bias, output_padding=0):
    return (type(c) is cls and c.in_channels == cin and c.out_channels == cout and c.kernel_size == (k,)
            and c.stride == (stride,) and c.padding == (pad,) and c.dilation == (1,) and c.groups == 1
            and c.padding_mode == mode and (c.bias is not None) == bias
            and (cls is not torch.nn.ConvTranspose1d or c.output_padding == (output_padding,)))


def _linear_blocks(seq, shapes):
    from pdecontrol.surrogates.models.fcnn import LinearBlock
    if type(seq) is not torch.nn.Sequential or len(seq) != len(shapes):
        return False
    for blk, (cin, sin, cout, sout, act) in zip(seq, shapes):
        if not (type(blk) is LinearBlock and (blk.in_channels, blk.in_size, blk.out_channels, blk.out_size) == (cin, sin, cout, sout)
                and type(blk.linear) is torch.nn.Linear and blk.linear.bias is not None
                and blk.linear.in_features == cin * sin and blk.linear.out_features == cout * sout and _act(blk.activation, act)):
            return False
    return True


def fused_delay_supported(surrogate):
    """True when ``surrogate`` has exactly the KSDelayCNNSurrogateFactory layout csrc/delay.hip implements: module types,
    channels, kernel sizes, strides, paddings, output paddings, activations, LayerNorm placement and widths, Linear shapes,
    delay = 3, N = 64 and 4 raw actuator values."""
    from torch import nn

    from pdecontrol.surrogates.models.cnn import ConvBlock, ConvNet, DeConvolutionBlock, ResidualBlock
    from pdecontrol.surrogates.surrogate import AutoRegPDESurrogate
    from pdecontrol.surrogates.transition import DelayTransitionModel
    try:
        tm = surrogate.transition_model
        if not (type(surrogate) is AutoRegPDESurrogate and type(tm) is DelayTransitionModel):
            return False
        if (tm.delay, tm.schannels, tm.ssize, tm.achannels, tm.asize) != (DELAY, 8, 8, 4, 8):
            return False
        enc, dec = surrogate.state_encoder.model, surrogate.state_decoder.model
        if not (type(enc) is ConvNet and enc.layers == ["block_l0", "block_l1", "block_l2"]):
            return False
        for name, (cin, cout, ln, act) in zip(enc.layers, ((1, 1, 32, nn.ELU), (1, 4, 16, nn.ELU), (4, 8, None, nn.Tanh))):
            b = getattr(enc, name)
            if not (type(b) is ResidualBlock and _act(b.activation, act)
                    and _conv(b.conv3x3_l1, nn.Conv1d, cin, cout, 3, 2, 1, "circular", False)
                    and _conv(b.conv3x3_l2, nn.Conv1d, cout, cout, 3, 1, 1, "circular", False)
                    and _conv(b.skip, nn.Conv1d, cin, cout, 1, 2, 0, "circular", False)
                    and all(_ln_width(getattr(b, n)) == ln for n in ("conv3x3_l1_norm", "conv3x3_l2_norm", "skip_norm"))):
                return False
        if not (type(dec) is ConvNet and dec.layers == ["block_l0", "block_l1", "block_l2", "block_l3"]):
            return False
        for name, (cin, cout, ln) in zip(dec.layers[:3], ((8, 8, 16), (8, 4, 32), (4, 1, None))):
            b = getattr(dec, name)
            if not (type(b) is DeConvolutionBlock and _act(b.activation, nn.ELU) and _ln_width(b.layernorm) == ln
                    and _conv(b.deconvolution, nn.ConvTranspose1d, cin, cout, 3, 2, 1, "zeros", True, output_padding=1)):
                return False
        b = dec.block_l3
        if not (type(b) is ConvBlock and _act(b.activation, nn.Tanh) and b.layernorm is None
                and _conv(b.convolution, nn.Conv1d, 1, 1, 5, 1, 2, "circular", True)):
            return False
        if not _linear_blocks(surrogate.action_encoder.model, ((1, 4, 4, 4, nn.ELU), (4, 4, 4, 8, nn.Tanh))):
            return False
        if not _linear_blocks(tm.fwd_model, ((36, 8, 12, 8, nn.ELU), (12, 8, 8, 8, nn.ELU), (8, 8, 8, 8, nn.Tanh))):
            return False
        return sum(p.numel() for p in surrogate.parameters()) == 39830 and len(list(surrogate.buffers())) == 0
    except AttributeError:
        return False


def geometry_unsupported(surrogate, tensor):
    """None when the kernels run this (layout-supported) surrogate on ``tensor`` (the states), else the reason."""
    if tensor.dtype != torch.float32 or any(p.dtype != torch.float32 for p in surrogate.parameters()):
        return f"the delay kernels are fp32 only (input {tensor.dtype})"
    from pdecontrol.surrogates import hipops
    try:
        hipops._dscale_constants(surrogate.dscaling)
    except hipops.SurrogateHipError as e:
        return f"the delay kernels: {e}"
    tm = surrogate.transition_model
    rc = load().dly_supported(int(tensor.shape[-1]), tm.delay, tm.schannels, tm.ssize, tm.achannels, tm.asize, NACT,
                              sum(p.numel() for p in surrogate.parameters()))
    return None if rc == 0 else load().dly_last_error().decode(errors="replace")


# ---------------------------------------------------------------------------------------------------------------------
# the rollout node
# ---------------------------------------------------------------------------------------------------------------------
class _DelayRolloutFn(torch.autograd.Function):
    """K rollout steps of B samples: dly_forward now, dly_backward when the caller's loss is back-propagated.
    states [B, S, 1, 64], actions [B, K, 4] (already mapped to the internal steps), context (S [B, 3, 8, 8], A [B, 3, 4, 8])
    or None; returns outputs, deltas [B, K, 1, 64], inlatents, outlatents [B, K, 8, 8] and the final context."""

    @staticmethod
    def forward(ctx, states, actions, cs, ca, delta, mul, add, *params):
        states, actions = states.contiguous(), actions.contiguous()
        cs = None if cs is None else cs.contiguous()
        ca = None if ca is None else ca.contiguous()
        flat = torch.cat([p.detach().reshape(-1) for p in params])
        b, s = states.shape[:2]
        k = actions.shape[1]
        dev = states.device
        outputs = torch.empty((b, k, 1, N), device=dev, dtype=torch.float32)
        deltas = torch.empty_like(outputs)
        inl = torch.empty((b, k, 8, 8), device=dev, dtype=torch.float32)
        outl = torch.empty_like(inl)
        cs_out = torch.empty((b, DELAY, 8, 8), device=dev, dtype=torch.float32)
        ca_out = torch.empty((b, DELAY, 4, 8), device=dev, dtype=torch.float32)
        _check(load().dly_forward(_stream(), _ptr(flat), b, s, k, _ptr(states), _ptr(actions), _ptr(cs), _ptr(ca), delta,
                                  mul, add, _ptr(outputs), _ptr(deltas), _ptr(inl), _ptr(outl), _ptr(cs_out), _ptr(ca_out)))
        ctx.save_for_backward(flat, states, actions, cs, ca, inl, outl)
        ctx.delta, ctx.mul = delta, mul
        ctx.shapes = [p.shape for p in params]
        ctx.set_materialize_grads(False)
        return outputs, deltas, inl, outl, cs_out, ca_out

    @staticmethod
    def backward(ctx, d_out, d_del, d_inl, d_outl, d_cs, d_ca):
        flat, states, actions, cs, ca, inl, outl = ctx.saved_tensors
        needs = ctx.needs_input_grad
        cont = lambda t: None if t is None else t.contiguous()
        d_out, d_del, d_inl, d_outl, d_cs, d_ca = map(cont, (d_out, d_del, d_inl, d_outl, d_cs, d_ca))
        b, s = states.shape[:2]
        k = actions.shape[1]
        d_states = torch.empty_like(states) if needs[0] else None
        d_actions = torch.empty_like(actions) if needs[1] else None
        d_cs_in = torch.empty((b, DELAY, 8, 8), device=states.device, dtype=torch.float32) if needs[2] else None
        d_ca_in = torch.empty((b, DELAY, 4, 8), device=states.device, dtype=torch.float32) if needs[3] else None
        d_flat = torch.empty_like(flat)
        work = torch.empty(load().dly_workspace_floats(b), device=states.device, dtype=torch.float32)
        _check(load().dly_backward(_stream(), _ptr(flat), b, s, k, _ptr(states), _ptr(actions), _ptr(cs), _ptr(ca), _ptr(inl),
                                   _ptr(outl), ctx.delta, ctx.mul, _ptr(d_out), _ptr(d_del), _ptr(d_inl), _ptr(d_outl),
                                   _ptr(d_cs), _ptr(d_ca), _ptr(d_states), _ptr(d_actions), _ptr(d_cs_in), _ptr(d_ca_in),
                                   _ptr(d_flat), _ptr(work)))
        grads, at = [], 0
        for shape, need in zip(ctx.shapes, needs[7:]):
            n = shape.numel()
            grads.append(d_flat[at:at + n].view(shape) if need else None)
            at += n
        return (d_states, d_actions, d_cs_in, d_ca_in, None, None, None, *grads)


def fused_delay_rollout(surrogate, states, actions, times, targets, hidden):
    """GPU rollout of the KSDelayCNNSurrogateFactory layout: the same ModelRollout as AutoRegPDESurrogate.rollout's torch
    spelling (inlatents included), from one dly_forward launch.  states [B, S, 1, 64], actions [B, A, 1, 4]."""
    from pdecontrol.mbrl.types import ModelRollout
    from pdecontrol.surrogates import hipops
    from pdecontrol.surrogates.surrogate import action_and_target_indices, take_steps
    aidx, tidx = action_and_target_indices(times, targets, surrogate.delta)
    acts = take_steps(actions, aidx.tolist())
    acts = acts.reshape(acts.shape[0], acts.shape[1], NACT)
    mul, add = hipops._dscale_constants(surrogate.dscaling)
    cs, ca = (None, None) if hidden is None else hidden
    outputs, deltas, inl, outl, cs_out, ca_out = _DelayRolloutFn.apply(states, acts, cs, ca, float(surrogate.delta), mul, add,
                                                                       *surrogate.parameters())
    pick = tidx.tolist()
    return ModelRollout(inlatents=take_steps(inl, pick), outlatents=take_steps(outl, pick), deltas=take_steps(deltas, pick),
                        outputs=take_steps(outputs, pick), hidden=(cs_out, ca_out))
