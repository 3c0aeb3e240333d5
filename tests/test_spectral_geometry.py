"""The fused spectral convolution (csrc/spectral.hip) across the geometry it accepts, and the torch.fft path for the
geometry it refuses.

* ``spec_conv_supported`` against a plain restatement of the rules in include/spectral_hip.h (host only, no GPU).
* The kernel against a dense fp64 DFT of the definition: y, dx, dWr, dWi and the two saved spectra, at N = 32 ... 2048,
  modes up to N/2 - 8 and Cin * modes = 1024, 1 to 4 row tiles, B = 1 and B above the CU count, both LDS paths in each
  direction and both ways of streaming the mixing weights.
* Geometries and dtypes the kernel refuses: the same module on the CPU in fp64, one logged notice per geometry.
"""
import copy
import ctypes
import logging
import math

import numpy as np
import pytest
import torch

from pdecontrol.architectures import BurgersFNO
from pdecontrol.surrogates import spectral
from pdecontrol.surrogates.spectral import SpectralConv1d
from pdecontrol.surrogates.training import PDETrainingModule

LDS_MAX = 160 * 1024


# ---------------------------------------------------------------------------------------------------------------------
# the documented rules, restated
# ---------------------------------------------------------------------------------------------------------------------
def lds_plan(c_in, c_out, n, modes):
    """(path, bytes) of one launch; c_in / c_out = channels of that launch's input / output tensor."""
    kp = 2 * modes + 4
    base = 4 * (c_in * (n + 4) + (c_in + c_out) * kp)
    dense, table = base + 4 * n * kp, base + 4 * n
    if dense <= LDS_MAX and n <= (c_in + c_out) * kp:
        return "dense", dense
    return "table", table


def mixing_plan(c_in, c_out, n, modes, backward):
    """Slab width of the staged mode-mixing weights (1 ... 8 channels), or "unstaged" when one slab does not fit the sample
    buffer and the weights are read straight from L2 (the two branches of phase B in spec_conv_kernel)."""
    lc_in, lc_out = (c_out, c_in) if backward else (c_in, c_out)
    per_ch = modes * lc_out if backward else c_out * modes
    ch = 8
    while ch > 1 and (2 * ch * per_ch > lc_in * (n + 4) or lc_in % ch):
        ch >>= 1
    return ch if 2 * ch * per_ch <= lc_in * (n + 4) else "unstaged"


def expected_refusal(cin, cout, n, modes):
    """None (both launches run), or (entry point that refuses, what its message must say)."""
    fwd = "spec_conv_forward"
    if cin % 16 or cout % 16:
        return fwd, f"channel counts ({cin}, {cout}) must be multiples of 16"
    if n < 32 or n > 2048 or n & (n - 1):
        return fwd, f"N = {n} must be a power of two in [32, 2048]"
    if modes % 8 or 2 * modes >= n:
        return fwd, f"modes = {modes} must be a multiple of 8 below N/2"
    if cin * modes > 1024 or cout * modes > 1024:
        return fwd, f"channels x modes ({cin * modes}, {cout * modes}) exceed 1024 mixing outputs"
    for who, (ci, co) in ((fwd, (cin, cout)), ("spec_conv_backward", (cout, cin))):
        _, nbytes = lds_plan(ci, co, n, modes)
        if nbytes > LDS_MAX:
            return who, f"needs {nbytes} B of LDS (> 160 KiB)"
    return None


def test_supported_query_matches_the_documented_rules():
    """Every (Cin, Cout, N, modes) of the grid: spec_conv_supported says what the rules say, and a refusal carries the code
    and text of the entry point that would refuse (that call is made too: it refuses on the host, before any launch)."""
    lib = spectral.load()
    one = ctypes.c_void_p(16)
    ns = [16, 32, 48, 64, 100, 128, 256, 512, 1024, 2048, 4096]
    chans = list(range(8, 81, 8))
    seen = {"ok": 0, "forward-only": 0}
    for n in ns:
        for modes in range(4, n // 2 + 1, 4):
            for cin in chans:
                for cout in chans:
                    want = expected_refusal(cin, cout, n, modes)
                    rc = lib.spec_conv_supported(cin, cout, n, modes)
                    geo = (cin, cout, n, modes)
                    if want is None:
                        assert rc == 0, (geo, lib.spec_last_error())
                        seen["ok"] += 1
                        continue
                    who, text = want
                    msg = lib.spec_last_error().decode()
                    assert rc == -4 and msg.startswith(who + ": ") and text in msg, (geo, rc, msg, want)
                    fn = getattr(lib, who)
                    assert fn(None, one, one, one, 3, cin, cout, n, modes, one, None) == rc, geo
                    assert lib.spec_last_error().decode() == msg, geo
                    if who == "spec_conv_backward":
                        seen["forward-only"] += 1
    assert seen == {"ok": 247, "forward-only": 23}, seen      # of 104 000 geometries
    # the table's forward-accepted, backward-refused module: 149 KiB forward, 277 KiB backward
    assert lib.spec_conv_supported(16, 32, 2048, 32) == -4
    assert lib.spec_last_error().decode() == "spec_conv_backward: needs 283904 B of LDS (> 160 KiB): channels x N too large"
    assert lds_plan(16, 32, 2048, 32) == ("table", 152576)
    assert spectral.unsupported(16, 32, 2048, 32).startswith("error -4: spec_conv_backward")
    assert spectral.unsupported(32, 32, 512, 16) is None


# (B, Cin, Cout, N, modes, forward LDS path, backward LDS path, forward mixing, backward mixing)
KERNEL_CASES = [
    (1, 16, 16, 32, 8, "dense", "dense", 2, 2),
    (3, 16, 16, 64, 24, "dense", "dense", 1, 1),              # modes = N/2 - 8
    (2, 16, 16, 256, 64, "table", "table", 2, 2),             # Cin * modes = 1024
    (4, 48, 32, 256, 16, "dense", "dense", 8, 4),             # 3 row tiles in, 2 out
    (4, 32, 48, 256, 16, "dense", "dense", 4, 8),
    (2, 64, 16, 256, 16, "dense", "dense", 8, 2),             # 4 row tiles
    (2, 64, 64, 512, 16, "table", "table", 8, 8),
    (2, 16, 16, 2048, 8, "table", "table", 8, 8),             # N at its maximum
    (2, 16, 16, 2048, 64, "table", "table", 8, 8),
    (2, 16, 32, 1024, 24, "table", "table", 8, 8),            # dense fits neither; the two tables differ in size
    (3, 16, 48, 512, 16, "dense", "table", 4, 8),             # forward and backward on different paths
    (3, 64, 32, 512, 16, "table", "dense", 8, 8),
    (2, 16, 64, 32, 8, "dense", "dense", "unstaged", 8),      # mixing weights straight from L2
    (2, 64, 16, 32, 8, "dense", "dense", 8, "unstaged"),
    (300, 32, 32, 512, 16, "dense", "dense", 8, 8),           # more workgroups than the MI355X has CUs (256)
]


def test_kernel_cases_cover_every_path():
    """The sweep below is what it claims: the LDS path and mixing branch of each case per the rules, and every
    combination (dense / table forward x dense / table backward, staged / unstaged mixing both ways) present."""
    for b, ci, co, n, m, pf, pb, mf, mb in KERNEL_CASES:
        assert expected_refusal(ci, co, n, m) is None
        assert (lds_plan(ci, co, n, m)[0], lds_plan(co, ci, n, m)[0]) == (pf, pb), (ci, co, n, m)
        assert (mixing_plan(ci, co, n, m, False), mixing_plan(ci, co, n, m, True)) == (mf, mb), (ci, co, n, m)
    paths = {(c[5], c[6]) for c in KERNEL_CASES}
    assert paths == {("dense", "dense"), ("table", "table"), ("dense", "table"), ("table", "dense")}
    assert {c[7] for c in KERNEL_CASES} >= {1, 8, "unstaged"} and {c[8] for c in KERNEL_CASES} >= {1, 8, "unstaged"}


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the kernel against the dense fp64 DFT of the definition
# ---------------------------------------------------------------------------------------------------------------------
def dense_dft_reference(x, wr, wi, dy):
    """fp64, CPU: y = sum_m s_m Re(e^{i th} sum_i X_i,m W_i,o,m) with X the truncated DFT of x; gradients by autograd of the
    same expression; the spectra the kernel saves: xft = (Re, Im) X, gyft = d loss / d (Re, Im) Y = s (.) DFT(dy)."""
    n, m = x.shape[-1], wr.shape[-1]
    x, wr, wi = (t.detach().double().requires_grad_(True) for t in (x, wr, wi))
    th = 2 * math.pi * torch.arange(m, dtype=torch.float64)[:, None] * torch.arange(n, dtype=torch.float64)[None, :] / n
    cos, sin = torch.cos(th), torch.sin(th)
    xr, xi = x @ cos.T, -(x @ sin.T)
    yr = torch.einsum("bim,iom->bom", xr, wr) - torch.einsum("bim,iom->bom", xi, wi)
    yi = torch.einsum("bim,iom->bom", xr, wi) + torch.einsum("bim,iom->bom", xi, wr)
    s = torch.full((m,), 2.0 / n, dtype=torch.float64)
    s[0] = 1.0 / n
    y = (s * yr) @ cos - (s * yi) @ sin
    dy = dy.double()
    y.backward(dy)
    xft = torch.stack((xr, xi), dim=2).detach()
    gyft = torch.stack((s * (dy @ cos.T), -s * (dy @ sin.T)), dim=2)
    return y.detach(), x.grad, wr.grad, wi.grad, xft, gyft


def _tol(ref):
    return 3e-5 * float(ref.detach().abs().max())   # fp32 sums of N (transforms) / B * N (weights) terms


def _count_apply(monkeypatch):
    calls = []
    orig = spectral._SpectralConvFn.apply
    monkeypatch.setattr(spectral._SpectralConvFn, "apply", lambda *a: (calls.append(1), orig(*a))[1])
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("b,ci,co,n,m", [c[:5] for c in KERNEL_CASES] + [pytest.param(3, 16, 32, 256, 16, id="transposed-x")])
def test_kernel_matches_dense_dft(b, ci, co, n, m, monkeypatch, request):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(b * 7 + ci + co + n + m)
    x = torch.randn(b, ci, n, generator=g)
    wr, wi = torch.randn(ci, co, m, generator=g) / ci, torch.randn(ci, co, m, generator=g) / ci
    dy = torch.randn(b, co, n, generator=g)
    y_ref, dx_ref, dwr_ref, dwi_ref, xft_ref, gyft_ref = dense_dft_reference(x, wr, wi, dy)

    transposed = "transposed" in request.node.name
    if transposed:                                   # x as a non-contiguous view: [N, Cin, B] storage
        leaf = x.permute(2, 1, 0).contiguous().to(dev).requires_grad_(True)
        xd = leaf.permute(2, 1, 0)
        assert not xd.is_contiguous()
    else:
        leaf = xd = x.to(dev).requires_grad_(True)
    wrd, wid = wr.to(dev).requires_grad_(True), wi.to(dev).requires_grad_(True)
    dyd = dy.to(dev)
    calls = _count_apply(monkeypatch)
    y = spectral.spectral_conv1d(xd, wrd, wid)
    assert len(calls) == 1, "a supported geometry must run on the kernel"
    xft = y.grad_fn.saved_tensors[2].detach().clone()
    y.backward(dyd)
    dx = leaf.grad.permute(2, 1, 0) if transposed else leaf.grad
    # the spectra the backward launch saves for the weight gradient, through the C ABI
    gyft = torch.empty((b, co, 2, m), device=dev)
    dx_abi = torch.empty((b, ci, n), device=dev)
    wrc, wic = wrd.detach().contiguous(), wid.detach().contiguous()
    lib = spectral.load()
    rc = lib.spec_conv_backward(spectral._stream(), spectral._ptr(dyd), spectral._ptr(wrc), spectral._ptr(wic), b, ci, co, n, m,
                                spectral._ptr(dx_abi), spectral._ptr(gyft))
    assert rc == 0, lib.spec_last_error()
    torch.cuda.synchronize(dev)

    observed = {}
    for name, got, ref in (("y", y, y_ref), ("dx", dx, dx_ref), ("dWr", wrd.grad, dwr_ref), ("dWi", wid.grad, dwi_ref),
                           ("xft", xft, xft_ref), ("gyft", gyft, gyft_ref)):
        got = got.detach().cpu().double()
        assert got.shape == ref.shape, name
        err = float((got - ref).abs().max())
        observed[name] = err / float(ref.abs().max())
        assert err <= _tol(ref), f"{name}: max error {err:.3e} > {_tol(ref):.3e} (= 3e-5 of max |ref| {float(ref.abs().max()):.3e})"
    print(f"spectral parity B={b} Cin={ci} Cout={co} N={n} modes={m}: max error / max |ref|",
          " ".join(f"{k} {v:.1e}" for k, v in observed.items()))
    np.testing.assert_array_equal(dx_abi.cpu().numpy(), dx.detach().cpu().numpy())   # same launch, same arguments
    # the DC imaginary part never reaches the output (irfft drops it): its weight gradient is exactly zero
    assert float(dwi_ref[..., 0].abs().max()) == 0.0
    assert float(wid.grad[..., 0].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# GPU: geometries and dtypes the kernel refuses run the torch.fft spelling
# ---------------------------------------------------------------------------------------------------------------------
# (Cin, Cout, N, modes) -> the refusal
REFUSED = [
    (24, 24, 64, 12, "spec_conv_forward: channel counts"),          # BurgersFNO width 24, 12 modes
    (48, 48, 128, 24, "spec_conv_forward: channels x modes"),       # width 48, 24 modes: Cin * modes = 1152
    (32, 32, 2048, 16, "spec_conv_forward: needs 280064 B"),        # width 32 at N = 2048
    (64, 64, 1024, 16, "spec_conv_forward: needs 285696 B"),        # width 64 at N = 1024
    (16, 32, 2048, 32, "spec_conv_backward: needs 283904 B"),       # the forward would launch (149 KiB), the backward not
]


@pytest.mark.gpu
@pytest.mark.parametrize("ci,co,n,m,why", REFUSED)
def test_refused_geometry_runs_torch_fft(ci, co, n, m, why, monkeypatch, caplog):
    dev = torch.device("cuda", 0)
    assert why in spectral.unsupported(ci, co, n, m)
    monkeypatch.setattr(spectral, "_NOTIFIED", set())
    torch.manual_seed(ci + co + n + m)
    ref_mod = SpectralConv1d(ci, co, m).double()
    mod = copy.deepcopy(ref_mod).float().to(dev)
    g = torch.Generator().manual_seed(n)
    x = torch.randn(3, ci, n, generator=g, dtype=torch.float64)
    dy = torch.randn(3, co, n, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    y_ref = ref_mod(xr)
    y_ref.backward(dy)
    calls = _count_apply(monkeypatch)
    xd = x.float().to(dev).requires_grad_(True)
    with caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        y = mod(xd)
        y.backward(dy.float().to(dev))              # the forward-only geometry must not fail here
        with torch.no_grad():
            mod(xd)                                 # a second call: no second notice
    torch.cuda.synchronize(dev)
    assert calls == [], "a refused geometry must not reach the kernel"
    notes = [r.getMessage() for r in caplog.records if "spectral convolution" in r.getMessage()]
    assert len(notes) == 1 and f"Cin={ci}, Cout={co}, N={n}, modes={m}" in notes[0] and why in notes[0], notes
    for name, got, ref in (("y", y, y_ref), ("dx", xd.grad, xr.grad), ("dWr", mod.weight_real.grad, ref_mod.weight_real.grad),
                           ("dWi", mod.weight_imag.grad, ref_mod.weight_imag.grad)):
        np.testing.assert_allclose(got.detach().cpu().double().numpy(), ref.detach().numpy(), rtol=0, atol=_tol(ref), err_msg=name)


@pytest.mark.gpu
def test_fp64_cuda_runs_torch_fft(monkeypatch, caplog):
    """fp64 on the GPU at a geometry the (fp32) kernel supports: torch.fft in fp64, equal to the CPU module to fp64 noise."""
    dev = torch.device("cuda", 0)
    monkeypatch.setattr(spectral, "_NOTIFIED", set())
    torch.manual_seed(5)
    ref_mod = SpectralConv1d(16, 32, 16).double()
    mod = copy.deepcopy(ref_mod).to(dev)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(4, 16, 256, generator=g, dtype=torch.float64)
    dy = torch.randn(4, 32, 256, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    y_ref = ref_mod(xr)
    y_ref.backward(dy)
    calls = _count_apply(monkeypatch)
    xd = x.to(dev).requires_grad_(True)
    with caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        y = mod(xd)
        y.backward(dy.to(dev))
    torch.cuda.synchronize(dev)
    assert calls == [] and y.dtype == torch.float64
    assert sum("torch.float64" in r.getMessage() for r in caplog.records) == 1
    for name, got, ref in (("y", y, y_ref), ("dx", xd.grad, xr.grad), ("dWr", mod.weight_real.grad, ref_mod.weight_real.grad),
                           ("dWi", mod.weight_imag.grad, ref_mod.weight_imag.grad)):
        np.testing.assert_allclose(got.detach().cpu().numpy(), ref.detach().numpy(), rtol=0, atol=1e-10 * float(ref.detach().abs().max()),
                                   err_msg=name)


@pytest.mark.gpu
@pytest.mark.parametrize("width,modes,n", [(24, 12, 64), (32, 16, 2048)])
def test_burgers_fno_at_refused_geometry_trains_on_cuda(width, modes, n):
    """An FNO that trains on the CPU trains on the GPU: training_step + backward against the same module on the CPU, with
    the bars of test_fno.py::test_fno_training_step_gpu_matches_cpu_and_trains."""
    from conftest import check_grads
    dev = torch.device("cuda", 0)
    mods = []
    for device in ("cpu", dev):
        torch.manual_seed(0)
        f = BurgersFNO()
        s = f.surrogate(delta=0.05, dscaling=None, tau=5, **f.model(width=width, modes=modes, layers=2))
        mods.append(PDETrainingModule(surrogate=s, loss=torch.nn.MSELoss(reduction="none"), tstep=0.05, delta=0.05, tau=5,
                                      tbtt=10).to(device))
    cpu, gpu = mods
    assert spectral.unsupported(width, width, n, modes) is not None
    g = torch.Generator().manual_seed(width + n)
    st, ac = torch.rand(3, 12, 1, n, generator=g) * 2 - 1, torch.rand(3, 12, 1, n, generator=g) * 2 - 1
    ref = cpu.training_step((st, ac), 0)
    ref["loss"].backward()
    out = gpu.training_step((st.to(dev), ac.to(dev)), 0)
    out["loss"].backward()
    torch.cuda.synchronize(dev)
    rel = abs(float(out["loss"].detach()) - float(ref["loss"].detach())) / abs(float(ref["loss"].detach()))
    assert rel < 1e-5, rel
    check_grads(f"BurgersFNO width {width}, {modes} modes, N = {n}: CUDA (torch.fft spectral path) vs CPU",
                {k: p.grad.detach().cpu().numpy() for k, p in gpu.surrogate.named_parameters()},
                dict((k, p.grad.numpy()) for k, p in cpu.surrogate.named_parameters()).__getitem__)
