"""fp64 reference of the whole-network FNO kernels (csrc/fno.hip), stage by stage -- CPU only.

``FNO1d(...).double()`` is the definition: the walk below calls the module's own submodules in the module's order and only
keeps what lies between them, which is what the kernels save (``pre``, ``xspec``) or emit per pair (``rows``, ``gspec``,
``dbase``, ``dact``).  Nothing here is a HIP kernel.

* ``walk(model, u, act, ...)``: the per-pair walk, for a stack of independent (u, act) pairs [P, N]; gradients by autograd,
  one pass per pair for the parameter rows.
* ``fp32_as_walk(...)``: the same walk in torch fp32 on the CPU, with the transforms spelled as dense cos / -sin
  contractions and the GELU as the kernels' Abramowitz & Stegun 7.1.26 formula.  It is the yardstick the measured
  tolerances are taken from: what a correct fp32 implementation of the same formulas loses against fp64.
* weight sets ``default`` (seed 0, as tests/test_fno.py) and ``stress`` (the same weights with per-layer gains, so that the
  GELU arguments leave |x| <= 1: ``STRESS_GAINS``, ``gelu_arguments``, ``coverage``).
"""
import math

import numpy as np
import torch

from pdecontrol.architectures.fno import FNO1d

WIDTH, MODES, LAYERS = 32, 16, 4
K2 = 2 * MODES
LAYER_SZ = WIDTH * WIDTH + WIDTH
ROW_DEFINED = 96 + LAYERS * LAYER_SZ + (WIDTH * WIDTH + WIDTH + WIDTH + 1)      # 5409; fno_row_width() pads beyond it


def row_slices():
    """name -> slice of a gradient row, in the kernels' layout."""
    s = {"lift.weight": slice(0, 64), "lift.bias": slice(64, 96)}
    off = 96
    for l in range(LAYERS):
        s[f"pointwise.{l}.weight"] = slice(off, off + 1024)
        s[f"pointwise.{l}.bias"] = slice(off + 1024, off + 1056)
        off += LAYER_SZ
    s["project.0.weight"] = slice(off, off + 1024)
    s["project.0.bias"] = slice(off + 1024, off + 1056)
    s["project.2.weight"] = slice(off + 1056, off + 1088)
    s["project.2.bias"] = slice(off + 1088, off + 1089)
    assert off + 1089 == ROW_DEFINED
    return s


def row_parameters(model):
    """The module's parameters in row order (everything but the spectral weights)."""
    ps = [model.lift.weight, model.lift.bias]
    for pw in model.pointwise:
        ps += [pw.weight, pw.bias]
    return ps + [model.project[0].weight, model.project[0].bias, model.project[2].weight, model.project[2].bias]


# ---------------------------------------------------------------------------------------------------------------------
# weight sets and inputs
# ---------------------------------------------------------------------------------------------------------------------
#: gain on every parameter of (lift, layer 0..3, project[0], project[2]).  A uniform 2.0 gives max |pre| of 4.3, 3.6, 2.2,
#: 1.5 at N = 64; the later layers get more so that every GELU argument set reaches [2, 4) on both signs (``coverage``).
STRESS_GAINS = {"lift": 2.0, "layers": (2.0, 2.2, 2.6, 2.6), "project.0": 2.6, "project.2": 2.0}
WEIGHT_SETS = ("default", "stress")


def make_model(weights="default", dtype=torch.float64):
    torch.manual_seed(0)
    model = FNO1d(in_channels=2, width=WIDTH, modes=MODES, layers=LAYERS)
    if weights == "stress":
        with torch.no_grad():
            g = STRESS_GAINS
            for p in model.lift.parameters():
                p.mul_(g["lift"])
            for l in range(LAYERS):
                for p in list(model.spectral[l].parameters()) + list(model.pointwise[l].parameters()):
                    p.mul_(g["layers"][l])
            for p in model.project[0].parameters():
                p.mul_(g["project.0"])
            for p in model.project[2].parameters():
                p.mul_(g["project.2"])
    elif weights != "default":
        raise ValueError(weights)
    return model.to(dtype)


def inputs(n, pairs, seed=0):
    """u, act [pairs, n] in [-1, 1] and gdelta, gout [pairs, n] standard normal, fp32 values (as float32 tensors)."""
    g = torch.Generator().manual_seed(1000 * seed + n + pairs)
    u, act = torch.rand(pairs, n, generator=g) * 2 - 1, torch.rand(pairs, n, generator=g) * 2 - 1
    return u, act, torch.randn(pairs, n, generator=g), torch.randn(pairs, n, generator=g)


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' GELU (Abramowitz & Stegun 7.1.26 from one exponential), in torch fp32
# ---------------------------------------------------------------------------------------------------------------------
_f32 = np.float32
AS_P = float(_f32(0.3275911) * _f32(0.70710678118654752))            # the kernel's compile-time fp32 product
AS_A = (1.061405429, -1.453152027, 1.421413741, -0.284496736, 0.254829592)
INV_SQRT_2PI = 0.3989422804014327


def _fmaf(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in fp64; one fp64 add, then one rounding to fp32."""
    c = torch.as_tensor(c, dtype=torch.float64)
    return (a.double() * torch.as_tensor(b, dtype=torch.float64) + c).float()


def as_gelu_parts(x):
    """(cdf, pdf) as ``gelu_parts`` of csrc/fno.hip computes them: same constants, same fma order, libm's exp."""
    assert x.dtype == torch.float32
    c = lambda v: torch.tensor(v, dtype=torch.float32)
    ax = x.abs()
    e = torch.exp((-0.5 * x) * x)
    t = 1.0 / _fmaf(ax, c(AS_P), 1.0)
    poly = _fmaf(t, c(AS_A[0]), c(AS_A[1]))
    for a in AS_A[2:]:
        poly = _fmaf(poly, t, c(a))
    erf_abs = _fmaf((-poly) * t, e, 1.0)
    cdf = 0.5 * (1.0 + torch.copysign(erf_abs, x))
    return cdf, c(INV_SQRT_2PI) * e


class _ASGelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return x * as_gelu_parts(x)[0]

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        cdf, pdf = as_gelu_parts(x)
        return g * _fmaf(x, pdf, cdf)           # gelu_grad: x * pdf + cdf


def as_gelu(x):
    return _ASGelu.apply(x)


def as_gelu_grad(x):
    cdf, pdf = as_gelu_parts(x)
    return _fmaf(x, pdf, cdf)


# ---------------------------------------------------------------------------------------------------------------------
# the walk
# ---------------------------------------------------------------------------------------------------------------------
class _Given(torch.autograd.Function):
    """Value of ``given``, gradient to ``computed``: the backward kernel takes its pre-activations as an input."""

    @staticmethod
    def forward(ctx, computed, given):
        return given.clone()

    @staticmethod
    def backward(ctx, g):
        return g, None


def twiddles(n, dtype):
    """tab[k][n]: k < 16 -> cos(2 pi k n / N), else -sin(2 pi (k - 16) n / N) (rfft's sign convention), from fp64."""
    pos, mode = torch.arange(n, dtype=torch.float64), torch.arange(MODES, dtype=torch.float64)
    th = 2 * math.pi * ((mode[:, None] * pos[None, :]) % n) / n
    return torch.cat((torch.cos(th), -torch.sin(th)), 0).to(dtype)


def mode_scale(n, dtype=torch.float64):
    s = torch.full((MODES,), 2.0 / n, dtype=dtype)
    s[0] = 1.0 / n
    return torch.cat((s, s))


def _spectrum(x, dense):
    """[P, 32 c, N] -> [P, 32 k, 32 c]: re | im of rfft(x)[..., :16], unscaled."""
    if dense:
        return torch.einsum("pcn,kn->pkc", x, twiddles(x.shape[-1], x.dtype))
    f = torch.fft.rfft(x, dim=-1)[..., :MODES]
    return torch.cat((f.real, f.imag), -1).transpose(1, 2)


def _dense_spectral(x, wr, wi):
    """The truncated-DFT spelling of the spectral convolution, as the kernel contracts it."""
    n = x.shape[-1]
    tab = twiddles(n, x.dtype)
    s = torch.einsum("pcn,kn->pck", x, tab)
    xr, xi = s[..., :MODES], s[..., MODES:]
    yr = torch.einsum("pim,iom->pom", xr, wr) - torch.einsum("pim,iom->pom", xi, wi)
    yi = torch.einsum("pim,iom->pom", xr, wi) + torch.einsum("pim,iom->pom", xi, wr)
    z = torch.cat((yr, yi), -1) * mode_scale(n, x.dtype)
    return torch.einsum("pok,kn->pon", z, tab)


def _forward(model, u, act, cscale, cshift, pre_given, dense, gelu):
    """One pass over [P, N] pairs with the graph kept; ``u`` / ``act`` may require grad."""
    t = {}
    x = model.lift(torch.stack((u, act), 1))
    xs, pres = [], []
    for l in range(LAYERS):
        xs.append(x)
        spec = model.spectral[l]
        y = _dense_spectral(x, spec.weight_real, spec.weight_imag) if dense else spec(x)
        pre = y + model.pointwise[l](x)
        if pre_given is not None:
            pre = _Given.apply(pre, pre_given[:, l])
        pres.append(pre)
        if l + 1 < LAYERS:
            x = gelu(pre) if gelu else model.activation(pre)
    z1 = model.project[0](pres[-1])
    h = gelu(z1) if gelu else model.project[1](z1)
    delta = model.project[2](h)[:, 0]
    t["x"], t["pre"], t["z1"], t["delta"] = xs, pres, z1, delta
    t["out"] = u + cscale * delta + cshift
    return t


def walk(model, u, act, cscale=1.0, cshift=0.0, gdelta=None, gout=None, pre_given=None, dense=False, gelu=None):
    """What the kernels save and emit for the pairs ``u``, ``act`` [P, N], as numpy arrays in the kernels' layouts.

    forward   x [P, 4, 32, N] (layer inputs), pre [P, 4, 32, N], z1 [P, 32, N], delta, out [P, N], xspec [4, 32 k, P, 32 c]
    backward  (with ``gdelta`` [P, N]; ``gout`` [P, N] or None, zero rows for pairs that receive none) of
              sum(gdelta * delta) + sum(gout * out), pair by pair: rows [P, 5409], gspec [4, 32 k, P, 32 c], dbase, dact,
              dpre [P, 4, 32, N].
    ``pre_given`` [P, 4, 32, N]: the pre-activations are taken from there (the backward kernel's view: they are its input),
    gradients still flow to the layer that computes them."""
    dt = model.lift.weight.dtype
    u, act = u.to(dt).clone(), act.to(dt).clone()
    back = gdelta is not None
    if back:
        u.requires_grad_(True)
        act.requires_grad_(True)
    if pre_given is not None:
        pre_given = pre_given.to(dt)
    with torch.enable_grad() if back else torch.no_grad():
        t = _forward(model, u, act, cscale, cshift, pre_given, dense, gelu)
    P, n = u.shape
    r = {"x": torch.stack(t["x"], 1), "pre": torch.stack(t["pre"], 1), "z1": t["z1"], "delta": t["delta"], "out": t["out"]}
    r["xspec"] = torch.stack([_spectrum(x.detach(), dense) for x in t["x"]], 0).transpose(1, 2)        # [4, k, P, c]
    if back:
        gdelta = gdelta.to(dt)
        loss_p = (gdelta * t["delta"]).sum(1)
        if gout is not None:
            loss_p = loss_p + (gout.to(dt) * t["out"]).sum(1)
        params = row_parameters(model)
        rows = []
        for p in range(P):
            g = torch.autograd.grad(loss_p[p], params, retain_graph=True)
            rows.append(torch.cat([x.reshape(-1) for x in g]))
        g = torch.autograd.grad(loss_p.sum(), t["pre"] + [u, act])
        dpre = torch.stack(g[:LAYERS], 1)
        r["rows"], r["dpre"], r["dbase"], r["dact"] = torch.stack(rows), dpre, g[LAYERS], g[LAYERS + 1]
        scale = mode_scale(n, dt)
        r["gspec"] = torch.stack([_spectrum(dpre[:, l], dense) * scale[None, :, None] for l in range(LAYERS)], 0).transpose(1, 2)
    return {k: v.detach().contiguous().numpy() for k, v in r.items()}


def fp32_as_walk(model32, u, act, **kw):
    """The yardstick: ``walk`` in fp32 with dense transforms and the kernels' GELU formula (never a HIP kernel)."""
    assert model32.lift.weight.dtype == torch.float32
    return walk(model32, u, act, dense=True, gelu=as_gelu, **kw)


def stage_local(model, u, act, pre, cscale=1.0, cshift=0.0):
    """fp64 recomputation of every stage from the fp32 stage before it: ``pre`` [P, 4, 32, N] are somebody's (a kernel's,
    the yardstick's) pre-activations; returns pre_l from THEIR pre_{l-1} (from u, act for l = 0), xspec_l from the same
    inputs, delta / out from THEIR pre_3.  A one-layer error then stays one layer's error."""
    dt = model.lift.weight.dtype
    pre = torch.as_tensor(pre).to(dt)
    u, act = u.to(dt), act.to(dt)
    with torch.no_grad():
        xs = [model.lift(torch.stack((u, act), 1))] + [model.activation(pre[:, l]) for l in range(LAYERS - 1)]
        loc = torch.stack([model.spectral[l](xs[l]) + model.pointwise[l](xs[l]) for l in range(LAYERS)], 1)
        delta = model.project(pre[:, LAYERS - 1])[:, 0]
        xspec = torch.stack([_spectrum(x, False) for x in xs], 0).transpose(1, 2)
    return {"pre": loc.numpy(), "xspec": xspec.contiguous().numpy(), "delta": delta.numpy(),
            "out": (u + cscale * delta + cshift).numpy()}


# ---------------------------------------------------------------------------------------------------------------------
# coverage of the GELU argument range
# ---------------------------------------------------------------------------------------------------------------------
def gelu_arguments(w):
    """The four argument sets that go through a GELU: pre_0, pre_1, pre_2 and z1 (pre_3 has no activation)."""
    return {"pre_0": w["pre"][:, 0], "pre_1": w["pre"][:, 1], "pre_2": w["pre"][:, 2], "z1": w["z1"]}


def coverage(w):
    """set -> {(lo, hi, sign): count} over the bands [1, 2), [2, 4), [4, 8)."""
    out = {}
    for name, x in gelu_arguments(w).items():
        out[name] = {(lo, hi, sg): int(np.count_nonzero((sg * x >= lo) & (sg * x < hi)))
                     for lo, hi in ((1, 2), (2, 4), (4, 8)) for sg in (1, -1)}
    return out
