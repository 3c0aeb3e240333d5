"""1-D spectral convolution -- the core of a Fourier-Neural-Operator layer.

The reference has no FNO (BASELINE configs[4] names one, the repository contains none); the operator is the
published one (Li et al. 2021):  ``y = irfft(W . rfft(x)[..., :modes], n=N)`` with complex weights ``W [Cin, Cout, modes]``.

* CPU tensors (and CUDA tensors after ``ops.enable_fused(False)``): ``torch.fft`` -- this is also the fp32 reference the
  kernel is tested against.
* CUDA tensors: ``libspectral_hip.so`` (include/spectral_hip.h): truncated-DFT GEMM -> complex mode mixing -> inverse-DFT
  GEMM fused in one launch per direction, one workgroup per sample, MFMA fp32.  A missing library raises.  The kernel
  takes every fp32 geometry that ``spec_conv_supported`` accepts for BOTH directions (channels multiples of 16, N a power
  of two in [32, 2048], modes a multiple of 8 below N/2, channels x modes <= 1024, LDS <= 160 KiB); any other dtype or
  geometry runs the torch.fft spelling on the GPU, announced once per geometry through the ``pdecontrol.surrogates``
  logger -- so a module that trains on the CPU also trains on the GPU, and a geometry whose backward launch would not fit
  never fails mid-step.  **Parity unpinned** against the reference (nothing there to compare with); pinned against the
  dense DFT definition in tests/test_fno.py and tests/test_spectral_geometry.py.
"""
import ctypes
import logging
import os

import torch
from torch import nn

import hipbind

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.abspath(os.path.join(_HERE, "..", "..", "lib", "libspectral_hip.so"))
_p, _i = ctypes.c_void_p, ctypes.c_int
SYMBOLS = (
    ("spec_conv_forward", _i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p]),
    ("spec_conv_backward", _i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p]),
    ("spec_conv_supported", _i, [_i, _i, _i, _i]),
    ("spec_last_error", ctypes.c_char_p, []),
)
_lib = None
_LOG = logging.getLogger("pdecontrol.surrogates")
_GEOMETRY = {}      # (cin, cout, n, modes) -> None (the kernel runs both directions) or the library's refusal
_NOTIFIED = set()


class SpectralHipError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is None:
        _lib = hipbind.open_library(LIB_PATH, SYMBOLS, SpectralHipError, "The fused spectral convolution has no fallback.")
    return _lib


_check = hipbind.checker(SpectralHipError, "libspectral_hip", "spec_last_error", lambda: load())
_stream, _ptr = hipbind.stream, hipbind.ptr


def unsupported(cin, cout, n, modes):
    """None when both kernel launches accept this geometry, else the refusing call's message (asked once per geometry)."""
    key = (int(cin), int(cout), int(n), int(modes))
    if key not in _GEOMETRY:
        lib = load()
        rc = lib.spec_conv_supported(*key)
        _GEOMETRY[key] = None if rc == 0 else f"error {rc}: {lib.spec_last_error().decode(errors='replace')}"
    return _GEOMETRY[key]


def spectral_conv1d_reference(x, wr, wi):
    """torch.fft spelling: x [B, Cin, N], wr / wi [Cin, Cout, modes] -> [B, Cout, N]."""
    n, modes = x.shape[-1], wr.shape[-1]
    xf = torch.fft.rfft(x, dim=-1)[..., :modes]
    yf = torch.einsum("bim,iom->bom", xf, torch.complex(wr, wi))
    out = torch.zeros(x.shape[0], wr.shape[1], n // 2 + 1, dtype=yf.dtype, device=x.device)
    out[..., :modes] = yf
    return torch.fft.irfft(out, n=n, dim=-1)


class _SpectralConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, wr, wi):
        x, wr, wi = x.contiguous(), wr.contiguous(), wi.contiguous()
        b, cin, n = x.shape
        cout, modes = wr.shape[1], wr.shape[2]
        if wr.shape != (cin, cout, modes) or wi.shape != wr.shape or wr.device != x.device or wi.device != x.device:
            raise SpectralHipError(f"weights {tuple(wr.shape)} / {tuple(wi.shape)} on {wr.device} / {wi.device} do not fit "
                                   f"x {tuple(x.shape)} on {x.device}")
        y = torch.empty((b, cout, n), device=x.device, dtype=torch.float32)
        need = any(ctx.needs_input_grad)
        xft = torch.empty((b, cin, 2, modes), device=x.device, dtype=torch.float32) if need else None
        _check(load().spec_conv_forward(_stream(), _ptr(x), _ptr(wr), _ptr(wi), b, cin, cout, n, modes, _ptr(y), _ptr(xft)))
        ctx.save_for_backward(wr, wi, xft)
        ctx.dims = (b, cin, cout, n, modes)
        return y

    @staticmethod
    def backward(ctx, dy):
        wr, wi, xft = ctx.saved_tensors
        b, cin, cout, n, modes = ctx.dims
        dy = dy.contiguous()
        dx = torch.empty((b, cin, n), device=dy.device, dtype=torch.float32)
        gy = torch.empty((b, cout, 2, modes), device=dy.device, dtype=torch.float32)
        _check(load().spec_conv_backward(_stream(), _ptr(dy), _ptr(wr), _ptr(wi), b, cin, cout, n, modes, _ptr(dx), _ptr(gy)))
        gwr = gwi = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            # contraction over the batch of two tiny tensors ([B, C, modes] each): one batched GEMM per term
            xr, xi, gr, gi = xft[:, :, 0], xft[:, :, 1], gy[:, :, 0], gy[:, :, 1]
            gwr = torch.einsum("bom,bim->iom", gr, xr) + torch.einsum("bom,bim->iom", gi, xi)
            gwi = torch.einsum("bom,bim->iom", gi, xr) - torch.einsum("bom,bim->iom", gr, xi)
        return (dx if ctx.needs_input_grad[0] else None), gwr, gwi


def _refusal(x, wr, wi):
    """Why the kernel cannot take this call (None: it can)."""
    if x.dtype != torch.float32 or wr.dtype != torch.float32 or wi.dtype != torch.float32:
        return f"dtype {x.dtype} / {wr.dtype}: the kernel is fp32"
    return unsupported(wr.shape[0], wr.shape[1], x.shape[-1], wr.shape[-1])


def spectral_conv1d(x, wr, wi):
    from pdecontrol.surrogates import ops
    if ops.use_fused(x):
        reason = _refusal(x, wr, wi)
        if reason is None:
            return _SpectralConvFn.apply(x, wr, wi)
        key = (x.dtype, wr.dtype, tuple(wr.shape), x.shape[-1])
        if key not in _NOTIFIED:
            _NOTIFIED.add(key)
            _LOG.warning("spectral convolution Cin=%d, Cout=%d, N=%d, modes=%d (%s): the HIP kernel refuses it (%s); it runs "
                         "on torch.fft", wr.shape[0], wr.shape[1], x.shape[-1], wr.shape[-1], x.dtype, reason)
    return spectral_conv1d_reference(x, wr, wi)


class SpectralConv1d(nn.Module):
    """Fourier layer core: complex weights on the lowest ``modes`` frequencies (stored as two real tensors)."""

    def __init__(self, in_channels: int, out_channels: int, modes: int):
        super().__init__()
        self.in_channels, self.out_channels, self.modes = in_channels, out_channels, modes
        scale = 1.0 / (in_channels * out_channels)
        self.weight_real = nn.Parameter(scale * torch.rand(in_channels, out_channels, modes))
        self.weight_imag = nn.Parameter(scale * torch.rand(in_channels, out_channels, modes))

    def forward(self, x):
        return spectral_conv1d(x, self.weight_real, self.weight_imag)
