"""Functional layer between the surrogate modules and the kernels that execute them.

Every block of the surrogate goes through one of the functions below.  On CPU tensors they are
plain torch (this is also the fp32 torch reference the HIP kernels are tested against).  On CUDA
tensors the hand-written gfx950 kernels of libsurrogate_hip.so are THE path for the architecture they implement
(``hipops.fused_supported``: the reference's KSAutoRegConvolutionalLSTM layout, at the grid widths whose LayerNorm rows
the kernels reduce -- N = 64, 128, 256, ``hipops.geometry_unsupported``; any other width is announced once and runs on torch
kernels like an uncovered architecture): they are on by default and the library's absence raises at the first CUDA tensor.  Every call site asks ``use_fused_for(surrogate, tensor)``: an
architecture the kernels do not cover -- the reference also ships ``KSAutoRegFullyConnectedLSTM`` and trains it on the
GPU as it is -- runs the plain PyTorch-ROCm path, announced ONCE per class through ``logging`` (never silently, and
never the other way round: a covered architecture cannot end up on torch kernels without the explicit opt-out).  The
plain torch-on-GPU path also exists as an explicit opt-out (``enable_fused(False)``, the
``fused(False)`` context manager or ``PDECONTROL_FUSED=0``): it is the same-device cross-check of the
parity tests and the "hipGraph over torch kernels" leg of the benchmark.

The two fully-connected LSTM baselines (``KSAutoRegFullyConnectedLSTM``, ``KSLatentLSTM``) have whole-rollout kernels of
their own (``fclstm_hip``, ``sur_fc_*``) behind a second, opt-in switch: ``enable_fused_fc(True)``, the ``fused_fc(True)``
context manager or ``PDECONTROL_FUSED_FC=1``.  It is off by default -- then they run on PyTorch-ROCm kernels with the
notice above, exactly as before -- and the opt-out above overrides it.
"""
import logging
import os

import torch

_LOG = logging.getLogger("pdecontrol.surrogates")
_NOTIFIED = set()
_DEFAULT = os.environ.get("PDECONTROL_FUSED", "1") != "0"
_FUSED = {"enabled": _DEFAULT, "lib": None}
_DEFAULT_FC = os.environ.get("PDECONTROL_FUSED_FC", "0") == "1"
_FUSED_FC = {"enabled": _DEFAULT_FC}


def enable_fused(flag=True):
    """Select the CUDA code path: True = fused HIP kernels (loads the library; raises if absent)."""
    if flag:
        from pdecontrol.surrogates import hipops
        _FUSED["lib"] = hipops.load()
    _FUSED["enabled"] = bool(flag)


def reset_fused():
    """Back to the process defaults (fused unless PDECONTROL_FUSED=0; the FC-LSTM kernels off unless
    PDECONTROL_FUSED_FC=1)."""
    _FUSED["enabled"] = _DEFAULT
    _FUSED_FC["enabled"] = _DEFAULT_FC


def enable_fused_fc(flag=True):
    """Opt the fully-connected LSTM baselines in to (or out of) their whole-rollout kernels (``fclstm_hip``)."""
    _FUSED_FC["enabled"] = bool(flag)


def fused_fc_enabled():
    return _FUSED_FC["enabled"]


class fused_fc:
    """``with ops.fused_fc(True): ...`` -- run a block with the FC-LSTM kernels switched on (or off) and restore the
    previous choice."""

    def __init__(self, flag):
        self.flag = bool(flag)

    def __enter__(self):
        self.prev = _FUSED_FC["enabled"]
        enable_fused_fc(self.flag)
        return self

    def __exit__(self, *exc):
        _FUSED_FC["enabled"] = self.prev


def fused_enabled():
    return _FUSED["enabled"]


class fused:
    """``with ops.fused(False): ...`` -- run a block on the other CUDA path and restore the previous choice."""

    def __init__(self, flag):
        self.flag = bool(flag)

    def __enter__(self):
        self.prev = _FUSED["enabled"]
        enable_fused(self.flag)
        return self

    def __exit__(self, *exc):
        _FUSED["enabled"] = self.prev


def use_fused(tensor):
    """True when the fused HIP kernels handle this tensor (any CUDA tensor unless opted out)."""
    if not (_FUSED["enabled"] and tensor.is_cuda):
        return False
    if _FUSED["lib"] is None:
        from pdecontrol.surrogates import hipops
        _FUSED["lib"] = hipops.load()   # raises when the library has not been built: no silent fallback
    return True


def use_fused_for(surrogate, tensor):
    """``use_fused(tensor)`` for a surrogate the fused kernels implement; for any other architecture False, with one
    logged notice per class (it then runs on PyTorch-ROCm kernels, as in the reference)."""
    if is_delay(surrogate):
        return False   # its own kernels and its own notice: use_fused_delay_for
    if _fc_layout(surrogate, tensor):
        return False   # its own kernels and its own notice: use_fused_fc_for
    from pdecontrol.surrogates import hipops
    return _use_fused_layout(surrogate, tensor, hipops.fused_supported, "KSAutoRegConvolutionalLSTM")


def is_delay(surrogate):
    """True for a surrogate with a DelayTransitionModel (the KSDelayCNNSurrogateFactory ablation)."""
    from pdecontrol.surrogates.transition import DelayTransitionModel
    return isinstance(getattr(surrogate, "transition_model", None), DelayTransitionModel)


def use_fused_delay_for(surrogate, tensor):
    """``use_fused_for`` of a delay-embedding surrogate: True for the KSDelayCNNSurrogateFactory layout on fp32 CUDA
    tensors of width 64 (``delay_hip.fused_delay_rollout``); any other delay model, fp64 input or an unsupported dscaling
    form runs on PyTorch-ROCm kernels, announced once.  False without a notice for any other transition model."""
    if not is_delay(surrogate):
        return False
    from pdecontrol.surrogates import delay_hip
    return _use_fused_layout(surrogate, tensor, delay_hip.fused_delay_supported, "KSDelayCNNSurrogateFactory",
                             geometry=lambda sur, t: delay_hip.geometry_unsupported(sur, t), lib=delay_hip.load)


def use_fused_latent_for(surrogate, tensor):
    """``use_fused_for`` of the latent-space rollout (LatentAutoRegPDESurrogate): True for the KSLatentConvolutionalLSTM
    layout at a supported grid width; any other latent architecture (KSLatentLSTM) runs on PyTorch-ROCm kernels, announced
    once per class."""
    if _fc_layout(surrogate, tensor):
        return False   # its own kernels and its own notice: use_fused_fc_for
    from pdecontrol.surrogates import hipops
    return _use_fused_layout(surrogate, tensor, hipops.fused_latent_supported, "KSLatentConvolutionalLSTM")


def is_fc_lstm(surrogate):
    """True for a surrogate around an LSTMTransitionModel (the two fully-connected baselines and their variants)."""
    from pdecontrol.surrogates.transition import LSTMTransitionModel
    return isinstance(getattr(surrogate, "transition_model", None), LSTMTransitionModel)


def _fc_layout(surrogate, tensor):
    """True when the FC-LSTM switch decides the path of ``surrogate`` on ``tensor``: the switch is on (and
    ``PDECONTROL_FUSED`` / ``fused(False)`` does not override it), the tensor is on the GPU and the module tree is one of
    the two factories'.  With the switch off this is False before it looks at anything."""
    if not (_FUSED_FC["enabled"] and _FUSED["enabled"] and tensor.is_cuda and is_fc_lstm(surrogate)):
        return False
    from pdecontrol.surrogates import fclstm_hip
    return fclstm_hip.fused_fc_supported(surrogate)


def use_fused_fc_for(surrogate, tensor):
    """True when the rollout of ``surrogate`` on ``tensor`` (the states) runs on the FC-LSTM kernels
    (``fclstm_hip.fused_fc_rollout``): ``_fc_layout`` and a geometry the kernels take.  A supported tree they refuse for
    this input (fp64, another width, an unknown dscaling) is announced once per reason and runs on PyTorch-ROCm kernels;
    any other tree returns False silently (``use_fused_for`` / ``use_fused_latent_for`` announce it as before)."""
    if not _fc_layout(surrogate, tensor):
        return False
    from pdecontrol.surrogates import fclstm_hip, hipops
    hipops.load()           # raises when the library has not been built: no silent fallback
    reason = fclstm_hip.geometry_unsupported(surrogate, tensor)
    if reason is None:
        return True
    if reason not in _NOTIFIED:
        _NOTIFIED.add(reason)
        _LOG.warning("the FC-LSTM HIP kernels do not take this input (%s): it runs on plain PyTorch-ROCm kernels", reason)
    return False


def _use_fused_layout(surrogate, tensor, supported, layout, geometry=None, lib=None):
    if not (_FUSED["enabled"] and tensor.is_cuda):
        return False
    from pdecontrol.surrogates import hipops
    if supported(surrogate):
        if lib is not None:
            lib()           # raises when the library has not been built: no silent fallback
        elif not use_fused(tensor):
            return False
        reason = (hipops.geometry_unsupported(surrogate, tensor.shape[-1]) if geometry is None
                  else geometry(surrogate, tensor))
        if reason is None:
            return True
        if reason not in _NOTIFIED:
            _NOTIFIED.add(reason)
            _LOG.warning("the fused HIP kernels do not implement this grid width (%s): it runs on plain PyTorch-ROCm kernels", reason)
        return False
    name = type(surrogate).__name__ + "/" + type(getattr(surrogate, "transition_model", None)).__name__
    if name not in _NOTIFIED:
        _NOTIFIED.add(name)
        _LOG.warning("%s is not the architecture the fused HIP kernels implement (%s layout): "
                     "it runs on plain PyTorch-ROCm kernels", name, layout)
    return False


def conv_act_norm(x, conv, activation, layernorm):
    """layernorm(activation(conv(x))) for nn.Conv1d (circular) / nn.ConvTranspose1d modules."""
    y = activation(conv(x))
    return y if layernorm is None else layernorm(y)


def lstm_cell(x, h, c, cell):
    """Convolutional LSTM cell (transition.py CNNLSTMCell.forward): returns (h', c')."""
    gi = cell.Wxi(x) + cell.Whi(h)
    gf = cell.Wxf(x) + cell.Whf(h)
    gc = cell.Wxc(x) + cell.Whc(h)
    go = cell.Wxo(x) + cell.Who(h)
    c_new = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gc)
    h_new = torch.sigmoid(go) * torch.tanh(c_new)
    return h_new, c_new
