"""The whole-network FNO kernels (csrc/fno.hip) through their C ABI, stage by stage against fp64 (tests/_fno_oracle.py).

What tests/test_fno.py cannot see from outside ``training_step``: the saved tensors (``pre``, ``xspec``, ``gspec``), the
per-pair gradient rows before they are summed, the spectra window, strided inputs, the NULL outputs, the ``gout`` gate, the
GELU approximation beyond |x| = 1 (the ``stress`` weight set), the remainder paths of the two reductions (exactly, on
integer-valued data) and run-to-run bit identity.

Tolerances are measured, not chosen: for every tensor, e = max |diff| / max |ref|; ``e_ref`` is what the fp32 yardstick
(``fp32_as_walk``: the same formulas in torch fp32 on the CPU) loses against the fp64 oracle on the same inputs, ``e_hip``
what the kernel loses; ``e_hip <= max(4 e_ref, 2^-22)``.  The factor 4 covers what the yardstick cannot reproduce (MFMA
K-split summation order against torch's blocked sums, ``__expf`` / ``__frcp_rn`` against libm, the 16-term ``row_dot``
chains); an index, sign, scale or conjugation error moves a tensor by its own scale.  Every (case, tensor, e_ref, e_hip) is
appended to fno_kernel_parity_observed.jsonl next to conftest's GRAD_LOG; the collected maxima are
profiles/fno_kernel_parity_observed.json.

What this criterion cannot see: a GELU coefficient off in its last digit (0.3275911 -> 0.3275912 is the only such change
that alters an fp32 constant) moves the activation by at most one ulp, below the floor and below the approximation's own
1.5e-7; a swapped s_0 / s_m scale or an off-by-one in a reduction's unrolled loop turns these tests red.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import _fno_oracle as fo
from conftest import GRAD_LOG

pytestmark = pytest.mark.gpu

NS = (64, 128, 512)        # half the waves without a position tile / one tile per wave / two tiles, LDS above 64 KB
NB, STEPS = 3, 2
PAIRS = NB * STEPS
SENT = -777.25             # sentinel: no kernel result is this value
FLOOR = 2.0 ** -22
FACTOR = 4.0
GRAD_CAP = 2e-4            # the outer caps of tests/test_fno.py, which must also hold at the default weights
LOG = os.path.join(os.path.dirname(GRAD_LOG), "fno_kernel_parity_observed.jsonl")      # the directory check_grads logs into
W, M, L = fo.WIDTH, fo.MODES, fo.LAYERS


def _dev():
    return torch.device("cuda", 0)


def _lib():
    from pdecontrol.surrogates import fno_hip
    return fno_hip.load()


def _full(shape, value=SENT):
    return torch.full(shape, value, device=_dev(), dtype=torch.float32)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _net(weights):
    from pdecontrol.surrogates import fno_hip
    m64, m32 = fo.make_model(weights), fo.make_model(weights, torch.float32)
    params = [p.detach().to(_dev()).contiguous() for p in fno_hip.parameters_of(m32)]
    w, keep = fno_hip._weights_struct(params)
    return {"m64": m64, "m32": m32, "w": w, "keep": (params, keep)}


def _view(t):
    """(pointer, stride_t, stride_b) of a [steps, nb, N] view (any strides; the last axis is contiguous)"""
    assert t.dim() == 3 and t.stride(2) == 1
    return ctypes.c_void_p(t.data_ptr()), t.stride(0), t.stride(1)


def forward(net, u, act, cscale=1.0, cshift=0.0, want_out=True, save=True, spec_pairs=None, pair0=0):
    """One fno_forward launch on [steps, nb, N] views ``u`` / ``act``; every output buffer starts as the sentinel."""
    from pdecontrol.surrogates import fno_hip
    import hipbind
    steps, nb, n = act.shape
    pairs = steps * nb
    spec_pairs = pairs if spec_pairs is None else spec_pairs
    r = {"delta": _full((pairs, n)), "out": _full((pairs, n)) if want_out else None,
         "pre": _full((pairs, L, W, n)) if save else None, "xspec": _full((L, 2 * M, spec_pairs, W)) if save else None}
    (up, ust, usb), (ap, ast, asb) = _view(u), _view(act)
    fno_hip._check(_lib().fno_forward(hipbind.stream(), ctypes.byref(net["w"]), W, M, L, n, nb, pairs, up, ust, usb, ap, ast, asb,
                                      cscale, cshift, hipbind.ptr(r["delta"]), hipbind.ptr(r["out"]), hipbind.ptr(r["pre"]),
                                      hipbind.ptr(r["xspec"]), spec_pairs, pair0))
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in r.items()}


def backward(net, u, act, cscale, gdelta, gout, gout_t, pre, spec_pairs=None, pair0=0, dbase="new", dact="new", bufs=None):
    """One fno_backward launch; ``dbase`` / ``dact``: "new" (a sentinel-filled buffer), None (NULL) or a tensor.  ``bufs``:
    rows / gspec / dbase / dact tensors to write into (the determinism test runs on the same buffers)."""
    from pdecontrol.surrogates import fno_hip
    import hipbind
    steps, nb, n = act.shape
    pairs = steps * nb
    spec_pairs = pairs if spec_pairs is None else spec_pairs
    width = _lib().fno_row_width()
    assert width >= fo.ROW_DEFINED
    bufs = bufs or {}
    r = {"rows": bufs.get("rows", None), "gspec": bufs.get("gspec", None)}
    if r["rows"] is None:
        r["rows"] = _full((pairs, width))
    if r["gspec"] is None:
        r["gspec"] = _full((L, 2 * M, spec_pairs, W))
    r["dbase"] = _full((pairs, n)) if isinstance(dbase, str) else dbase
    r["dact"] = _full((pairs, n)) if isinstance(dact, str) else dact
    assert r["rows"].shape == (pairs, width) and pre.shape == (pairs, L, W, n) and gdelta.shape == (pairs, n)
    assert gout is None or gout.shape == (nb, n)
    (up, ust, usb), (ap, ast, asb) = _view(u), _view(act)
    fno_hip._check(_lib().fno_backward(hipbind.stream(), ctypes.byref(net["w"]), W, M, L, n, nb, pairs, up, ust, usb, ap, ast, asb,
                                       cscale, hipbind.ptr(gdelta), hipbind.ptr(gout), gout_t, hipbind.ptr(pre),
                                       hipbind.ptr(r["gspec"]), spec_pairs, pair0, hipbind.ptr(r["rows"]), hipbind.ptr(r["dbase"]),
                                       hipbind.ptr(r["dact"])))
    torch.cuda.synchronize()
    out = {k: _np(v) for k, v in r.items()}
    out["rows"] = out["rows"][:, :fo.ROW_DEFINED]        # the padding columns are never initialised: never compared
    return out


@pytest.fixture(scope="module", autouse=True)
def _warm_up():
    """One eager call per N before anything else: the twiddle table of (device, N) is created on first use."""
    net = _net("default")
    for n in NS:
        z = torch.zeros((1, 1, n), device=_dev())
        forward(net, z, z, save=False)


# ---------------------------------------------------------------------------------------------------------------------
# the measured tolerance
# ---------------------------------------------------------------------------------------------------------------------
def _err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = float(np.abs(ref).max())
    return float(np.abs(got - ref).max()) / scale if scale > 0 else float(np.abs(got).max())


class Judge:
    def __init__(self, case):
        self.case, self.failures = case, []

    def __call__(self, tensor, hip, hip_ref, yard, yard_ref, cap=None):
        e_ref, e_hip = _err(yard, yard_ref), _err(hip, hip_ref)
        rec = {"case": self.case, "tensor": tensor, "e_ref": e_ref, "e_hip": e_hip}
        print("fno kernel parity", json.dumps(rec))
        try:
            os.makedirs(os.path.dirname(LOG), exist_ok=True)
            with open(LOG, "a") as f:
                f.write(json.dumps(rec) + "\n")
        except OSError:
            pass
        bound = max(FACTOR * e_ref, FLOOR)
        if not e_hip <= bound:
            self.failures.append(f"{tensor}: e_hip {e_hip:.3e} > max(4 x e_ref {e_ref:.3e}, 2^-22)")
        if cap is not None and not e_hip <= cap:
            self.failures.append(f"{tensor}: e_hip {e_hip:.3e} above the outer cap {cap:.1e}")

    def done(self):
        assert not self.failures, f"{self.case}:\n  " + "\n  ".join(self.failures)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b, what):
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=what)


def _written(r, keys, what):
    for k in keys:
        assert not (r[k] == SENT).any(), f"{what}: {k} has entries the kernel never wrote"


# ---------------------------------------------------------------------------------------------------------------------
# cases (computed once, shared, never modified)
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    """inputs, oracle walk, yardstick walk and the plain kernel launch of one (weight set, N, nb, steps)"""

    def __init__(self, weights, n, nb=NB, steps=STEPS):
        self.weights, self.n, self.nb, self.steps, self.pairs = weights, n, nb, steps, nb * steps
        self.net = _net(weights)
        self.label = f"{weights} N={n} pairs={self.pairs}"
        self.u, self.act, self.gdelta, gout = fo.inputs(n, self.pairs)          # pair p = t * nb + b
        self.gout = gout[:nb].contiguous()
        self.ref = fo.walk(self.net["m64"], self.u, self.act)
        self.yard = fo.fp32_as_walk(self.net["m32"], self.u, self.act)
        dev = _dev()
        self.u_dev, self.act_dev = self.u.view(steps, nb, n).to(dev), self.act.view(steps, nb, n).to(dev)
        self.hip = forward(self.net, self.u_dev, self.act_dev)


@functools.lru_cache(maxsize=None)
def _case(weights, n, nb=NB, steps=STEPS):
    return Case(weights, n, nb, steps)


def _judge_forward(j, tag, net, u, act, hip, ref, yard, cscale=1.0, cshift=0.0, outer_caps=False):
    """global and stage-local comparison of delta, out, pre and xspec"""
    for k in ("delta", "out"):
        j(f"{tag}{k}", hip[k], ref[k], yard[k], ref[k])
    for l in range(L):
        j(f"{tag}pre_{l}", hip["pre"][:, l], ref["pre"][:, l], yard["pre"][:, l], ref["pre"][:, l])
        j(f"{tag}xspec_{l}", hip["xspec"][l], ref["xspec"][l], yard["xspec"][l], ref["xspec"][l])
    loc_h = fo.stage_local(net["m64"], u, act, hip["pre"], cscale, cshift)
    loc_y = fo.stage_local(net["m64"], u, act, yard["pre"], cscale, cshift)
    for k in ("delta", "out"):
        j(f"{tag}local {k}", hip[k], loc_h[k], yard[k], loc_y[k])
    for l in range(L):
        j(f"{tag}local pre_{l}", hip["pre"][:, l], loc_h["pre"][:, l], yard["pre"][:, l], loc_y["pre"][:, l])
        j(f"{tag}local xspec_{l}", hip["xspec"][l], loc_h["xspec"][l], yard["xspec"][l], loc_y["xspec"][l])
    if outer_caps:
        np.testing.assert_allclose(hip["delta"], ref["delta"], rtol=1e-4, atol=2e-5)
        np.testing.assert_allclose(hip["out"], ref["out"], rtol=1e-4, atol=2e-5)


GRID = [(w, n) for w in fo.WEIGHT_SETS for n in NS]


@pytest.mark.parametrize("weights,n", GRID)
def test_forward_saved_tensors_against_the_oracle(weights, n):
    c = _case(weights, n)
    _written(c.hip, ("delta", "out", "pre", "xspec"), c.label)
    j = Judge(f"forward {c.label}")
    _judge_forward(j, "", c.net, c.u, c.act, c.hip, c.ref, c.yard, outer_caps=weights == "default")
    j.done()


@pytest.mark.parametrize("weights,n", GRID)
def test_forward_strided_rows_with_stride_t_zero(weights, n):
    """u as a slice of a wider buffer (stride_b > N) shared by every step (stride_t = 0: the form every free-running step
    uses), act in the rollout's [batch][step][N] layout."""
    c = _case(weights, n)
    dev = _dev()
    wide = torch.full((NB, n + 24), 55.5)
    wide[:, 4:4 + n] = c.u[:NB]
    wide_dev = wide.to(dev)
    u_view = wide_dev[:, 4:4 + n].unsqueeze(0).expand(STEPS, NB, n)              # stride_t = 0, stride_b = n + 24
    assert u_view.stride() == (0, n + 24, 1)
    acts = c.act.view(STEPS, NB, n).transpose(0, 1).contiguous().to(dev)          # [nb][steps][N]
    a_view = acts.transpose(0, 1)                                                # stride_t = n, stride_b = steps * n
    assert a_view.stride() == (n, STEPS * n, 1)
    cs, csh = 0.625, -0.25
    hip = forward(c.net, u_view, a_view, cscale=cs, cshift=csh)
    _written(hip, ("delta", "out", "pre", "xspec"), c.label)
    u = c.u[:NB].repeat(STEPS, 1)
    ref = fo.walk(c.net["m64"], u, c.act, cscale=cs, cshift=csh)
    yard = fo.fp32_as_walk(c.net["m32"], u, c.act, cscale=cs, cshift=csh)
    j = Judge(f"forward strided {c.label}")
    _judge_forward(j, "", c.net, u, c.act, hip, ref, yard, cs, csh, outer_caps=weights == "default")
    j.done()
    assert np.abs(ref["delta"][NB:] - c.ref["delta"][NB:]).max() > 1e-3 * np.abs(ref["delta"]).max(), "the shared base row matters"


@pytest.mark.parametrize("weights,n", GRID)
def test_forward_window_null_out_affine_and_inference_launch(weights, n):
    c = _case(weights, n)
    # the spectra window: this launch's pairs are pairs [3, 9) of a buffer spanning 11
    win = forward(c.net, c.u_dev, c.act_dev, spec_pairs=11, pair0=3)
    assert (win["xspec"][:, :, :3] == SENT).all() and (win["xspec"][:, :, 3 + PAIRS:] == SENT).all(), "written outside the window"
    _same_bits(win["xspec"][:, :, 3:3 + PAIRS], c.hip["xspec"], "spectra window")
    for k in ("delta", "out", "pre"):
        _same_bits(win[k], c.hip[k], f"window launch: {k}")
    # out = NULL
    nul = forward(c.net, c.u_dev, c.act_dev, want_out=False)
    for k in ("delta", "pre", "xspec"):
        _same_bits(nul[k], c.hip[k], f"out = NULL: {k}")
    # non-trivial cscale, cshift: out = u + cscale * delta + cshift on the same delta
    cs, csh = 0.03125 * 1.5, 0.0078125
    aff = forward(c.net, c.u_dev, c.act_dev, cscale=cs, cshift=csh)
    for k in ("delta", "pre", "xspec"):
        _same_bits(aff[k], c.hip[k], f"cscale, cshift: {k}")
    j = Judge(f"forward affine {c.label}")
    yard_out = (c.u.numpy() + np.float32(cs) * c.yard["delta"]).astype(np.float32) + np.float32(csh)
    j("out", aff["out"], c.u.double().numpy() + cs * c.ref["delta"] + csh, yard_out, c.u.double().numpy() + cs * c.ref["delta"] + csh)
    j.done()
    # the inference instantiation (pre = xspec = NULL) computes the same delta and out, bit for bit
    inf = forward(c.net, c.u_dev, c.act_dev, save=False)
    _same_bits(inf["delta"], c.hip["delta"], "inference launch: delta")
    _same_bits(inf["out"], c.hip["out"], "inference launch: out")
    inf = forward(c.net, c.u_dev, c.act_dev, cscale=cs, cshift=csh, save=False)
    _same_bits(inf["out"], aff["out"], "inference launch: out with cscale, cshift")


# ---------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------
CSCALE = 0.375


def _judge_backward(j, tag, hip, ref, yard, cap=None):
    for name, sl in fo.row_slices().items():
        j(f"{tag}rows {name}", hip["rows"][:, sl], ref["rows"][:, sl], yard["rows"][:, sl], ref["rows"][:, sl], cap)
    for l in range(L):
        j(f"{tag}gspec_{l}", hip["gspec"][l], ref["gspec"][l], yard["gspec"][l], ref["gspec"][l], cap)
    for k in ("dbase", "dact"):
        j(f"{tag}{k}", hip[k], ref[k], yard[k], ref[k], cap)


def _gout_full(c):
    g = torch.zeros(c.pairs, c.n)
    if c.steps > 1:
        g[c.nb:2 * c.nb] = c.gout               # the pairs of step gout_t = 1
    return g


@functools.lru_cache(maxsize=None)
def _backward_case(weights, n, nb=NB, steps=STEPS):
    """The backward kernel alone: fed the oracle's pre-activations rounded to fp32 (oracle and yardstick walk from the same
    values), a random gdelta and a gout for step 1."""
    c = _case(weights, n, nb, steps)
    dev = _dev()
    pre32 = torch.from_numpy(c.ref["pre"].astype(np.float32))
    kw = dict(cscale=CSCALE, gdelta=c.gdelta, pre_given=pre32)
    dv = {"pre": pre32.to(dev), "gdelta": c.gdelta.to(dev), "gout": c.gout.to(dev)}
    with_gout = steps > 1
    r = {"dev": dv,
         "hip": backward(c.net, c.u_dev, c.act_dev, CSCALE, dv["gdelta"], dv["gout"], 1, dv["pre"]),
         "ref": fo.walk(c.net["m64"], c.u, c.act, gout=_gout_full(c) if with_gout else None, **kw),
         "yard": fo.fp32_as_walk(c.net["m32"], c.u, c.act, gout=_gout_full(c) if with_gout else None, **kw)}
    return r


@pytest.mark.parametrize("weights,n", GRID)
def test_backward_rows_spectra_and_input_gradients_against_the_oracle(weights, n):
    c, b = _case(weights, n), _backward_case(weights, n)
    _written(b["hip"], ("rows", "gspec", "dbase", "dact"), c.label)
    j = Judge(f"backward {c.label}")
    _judge_backward(j, "", b["hip"], b["ref"], b["yard"], cap=GRAD_CAP if weights == "default" else None)
    j.done()


@pytest.mark.parametrize("weights,n", GRID)
def test_backward_gout_gate_and_gout_null(weights, n):
    c, b = _case(weights, n), _backward_case(weights, n)
    dv = b["dev"]
    hip = backward(c.net, c.u_dev, c.act_dev, CSCALE, dv["gdelta"], None, 1, dv["pre"])
    kw = dict(cscale=CSCALE, gdelta=c.gdelta, pre_given=dv["pre"].cpu())
    j = Judge(f"backward gout=NULL {c.label}")
    _judge_backward(j, "", hip, fo.walk(c.net["m64"], c.u, c.act, **kw), fo.fp32_as_walk(c.net["m32"], c.u, c.act, **kw),
                    cap=GRAD_CAP if weights == "default" else None)
    j.done()
    # pairs of a step other than gout_t show no trace of gout; the pairs of step gout_t do
    other, at = slice(0, NB), slice(NB, 2 * NB)
    for k in ("rows", "dbase", "dact"):
        _same_bits(b["hip"][k][other], hip[k][other], f"{k} of step 0 with and without gout")
        assert (_bits(b["hip"][k][at]) != _bits(hip[k][at])).mean() > 0.5, f"{k} of step 1 ignores gout"
    _same_bits(b["hip"]["gspec"][:, :, other], hip["gspec"][:, :, other], "gspec of step 0 with and without gout")
    assert (_bits(b["hip"]["gspec"][:, :, at]) != _bits(hip["gspec"][:, :, at])).mean() > 0.5
    # a gout_t that matches no step of the launch: the same as gout = NULL
    none = backward(c.net, c.u_dev, c.act_dev, CSCALE, dv["gdelta"], dv["gout"], STEPS, dv["pre"])
    for k in ("rows", "gspec", "dbase", "dact"):
        _same_bits(none[k], hip[k], f"gout_t outside the launch: {k}")


@pytest.mark.parametrize("weights,n", GRID)
def test_backward_null_input_gradients_and_spectra_window(weights, n):
    c, b = _case(weights, n), _backward_case(weights, n)
    dv = b["dev"]
    held_base, held_act = _full((PAIRS, n)), _full((PAIRS, n))        # passed only to the second call
    nul = backward(c.net, c.u_dev, c.act_dev, CSCALE, dv["gdelta"], dv["gout"], 1, dv["pre"], dbase=None, dact=None)
    assert nul["dbase"] is None and nul["dact"] is None
    assert (held_base == SENT).all() and (held_act == SENT).all(), "handed NULL, the kernel writes no input gradient"
    for k in ("rows", "gspec"):
        _same_bits(nul[k], b["hip"][k], f"dbase = dact = NULL: {k}")
    two = backward(c.net, c.u_dev, c.act_dev, CSCALE, dv["gdelta"], dv["gout"], 1, dv["pre"], dbase=held_base, dact=held_act)
    for k in ("rows", "gspec", "dbase", "dact"):
        _same_bits(two[k], b["hip"][k], f"second call: {k}")
    win = backward(c.net, c.u_dev, c.act_dev, CSCALE, dv["gdelta"], dv["gout"], 1, dv["pre"], spec_pairs=11, pair0=3)
    assert (win["gspec"][:, :, :3] == SENT).all() and (win["gspec"][:, :, 3 + PAIRS:] == SENT).all(), "written outside the window"
    _same_bits(win["gspec"][:, :, 3:3 + PAIRS], b["hip"]["gspec"], "spectra window")
    for k in ("rows", "dbase", "dact"):
        _same_bits(win[k], b["hip"][k], f"window launch: {k}")


@pytest.mark.parametrize("n", NS)
def test_backward_on_the_forward_kernels_own_pre_activations(n):
    """The production pairing at the default weights: fno_backward reads what fno_forward saved; oracle and yardstick walk
    back from those same fp32 pre-activations."""
    c = _case("default", n)
    dev = _dev()
    pre = torch.from_numpy(c.hip["pre"])
    hip = backward(c.net, c.u_dev, c.act_dev, CSCALE, c.gdelta.to(dev), c.gout.to(dev), 1, pre.to(dev))
    kw = dict(cscale=CSCALE, gdelta=c.gdelta, gout=_gout_full(c), pre_given=pre)
    j = Judge(f"backward own pre {c.label}")
    _judge_backward(j, "", hip, fo.walk(c.net["m64"], c.u, c.act, **kw), fo.fp32_as_walk(c.net["m32"], c.u, c.act, **kw), cap=GRAD_CAP)
    j.done()


def test_single_pair_launch():
    """nb = 1, pairs = 1 (one workgroup; step 0 only, so gout_t = 0 applies to it), stress weights."""
    c = Case("stress", 128, nb=1, steps=1)
    _written(c.hip, ("delta", "out", "pre", "xspec"), c.label)
    j = Judge(f"forward {c.label}")
    _judge_forward(j, "", c.net, c.u, c.act, c.hip, c.ref, c.yard)
    dev = _dev()
    pre32 = torch.from_numpy(c.ref["pre"].astype(np.float32))
    hip = backward(c.net, c.u_dev, c.act_dev, CSCALE, c.gdelta.to(dev), c.gout.to(dev), 0, pre32.to(dev))
    _written(hip, ("rows", "gspec", "dbase", "dact"), c.label)
    kw = dict(cscale=CSCALE, gdelta=c.gdelta, gout=c.gout, pre_given=pre32)
    _judge_backward(j, "backward ", hip, fo.walk(c.net["m64"], c.u, c.act, **kw), fo.fp32_as_walk(c.net["m32"], c.u, c.act, **kw))
    j.done()


# ---------------------------------------------------------------------------------------------------------------------
# the two reductions, exactly: integer-valued floats, every partial sum an integer below 2^24, so fp32 is exact in any order
# ---------------------------------------------------------------------------------------------------------------------
GUARD = 1.0e6          # rows / planes next to the operands hold this: an index one past the end reads it, in bounds


@pytest.mark.parametrize("pairs", [1, 7, 8, 9, 24, 25, 31, 32, 33, 40, 65])
def test_reduce_rows_exact(pairs):
    """8 interleaved chains, unrolled by 4, with a tail loop: every remainder path, bit for bit."""
    import hipbind
    from pdecontrol.surrogates import fno_hip
    lib = _lib()
    width = lib.fno_row_width()
    rs = np.random.RandomState(pairs)
    rows = rs.randint(-8, 9, size=(pairs, width)).astype(np.float32)
    buf = np.full((pairs + 2, width), GUARD, dtype=np.float32)          # one guard row on either side
    buf[1:pairs + 1] = rows
    dbuf = torch.from_numpy(buf).to(_dev())
    out = _full((width,))
    fno_hip._check(lib.fno_reduce_rows(hipbind.stream(), hipbind.ptr(dbuf[1:]), pairs, hipbind.ptr(out)))
    torch.cuda.synchronize()
    want = rows.astype(np.int64).sum(0)
    assert np.abs(want).max() < 2 ** 24
    np.testing.assert_array_equal(_np(out)[:fo.ROW_DEFINED], want[:fo.ROW_DEFINED].astype(np.float32))


@pytest.mark.parametrize("pairs", [1, 2, 3, 4, 5, 15, 16, 17, 33, 65])
def test_spec_wgrad_exact(pairs):
    """4 pairs per MFMA, 4 K-quarters, zero padding past the last pair: all four layers, all 16 modes, both outputs against
    dWr = sum_p Gr Xr + Gi Xi, dWi = sum_p Gi Xr - Gr Xi; every (layer, mode, pair, channel) entry is its own random draw."""
    import hipbind
    from pdecontrol.surrogates import fno_hip
    lib = _lib()
    rs = np.random.RandomState(100 + pairs)
    shape = (L, 2 * M, pairs, W)
    X, G = rs.randint(-4, 5, size=shape), rs.randint(-4, 5, size=shape)
    size = int(np.prod(shape))
    dev_bufs = []
    for a in (X, G):
        flat = np.full(size + 2 * pairs * W + 2 * W, GUARD, dtype=np.float32)      # guard planes before and after
        flat[pairs * W + W:pairs * W + W + size] = a.reshape(-1)
        dev_bufs.append(torch.from_numpy(flat).to(_dev()))
    xs, gs = (b[pairs * W + W:pairs * W + W + size] for b in dev_bufs)
    dwr, dwi = [_full((W, W, M)) for _ in range(L)], [_full((W, W, M)) for _ in range(L)]
    P4 = ctypes.c_void_p * 4
    fno_hip._check(lib.fno_spec_wgrad(hipbind.stream(), hipbind.ptr(xs), hipbind.ptr(gs), pairs, P4(*[t.data_ptr() for t in dwr]),
                                      P4(*[t.data_ptr() for t in dwi])))
    torch.cuda.synchronize()
    for l in range(L):
        xr, xi, gr, gi = X[l, :M], X[l, M:], G[l, :M], G[l, M:]          # [m, p, c], int64
        want_r = np.einsum("mpo,mpi->iom", gr, xr) + np.einsum("mpo,mpi->iom", gi, xi)
        want_i = np.einsum("mpo,mpi->iom", gi, xr) - np.einsum("mpo,mpi->iom", gr, xi)
        assert max(np.abs(want_r).max(), np.abs(want_i).max()) < 2 ** 24
        np.testing.assert_array_equal(_np(dwr[l]), want_r.astype(np.float32), err_msg=f"dWr of layer {l}")
        np.testing.assert_array_equal(_np(dwi[l]), want_i.astype(np.float32), err_msg=f"dWi of layer {l}")


# ---------------------------------------------------------------------------------------------------------------------
# determinism
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 512])
def test_backward_is_bit_identical_run_to_run(n):
    """The same backward launch five times on the same buffers (stress weights, 6 pairs): every defined column of the rows
    (the p2.weight columns, which the eight waves of a workgroup fold together, included), gspec, dbase and dact."""
    c, b = _case("stress", n), _backward_case("stress", n)
    dv = b["dev"]
    bufs = {"rows": _full((PAIRS, _lib().fno_row_width())), "gspec": _full((L, 2 * M, PAIRS, W))}
    held_base, held_act = _full((PAIRS, n)), _full((PAIRS, n))
    runs = [backward(c.net, c.u_dev, c.act_dev, CSCALE, dv["gdelta"], dv["gout"], 1, dv["pre"], dbase=held_base, dact=held_act,
                     bufs=bufs) for _ in range(5)]
    sl = fo.row_slices()["project.2.weight"]
    for k, r in enumerate(runs[1:], 1):
        moved = int((_bits(r["rows"][:, sl]) != _bits(runs[0]["rows"][:, sl])).sum())
        print(f"determinism N={n} run {k}: p2.weight entries that differ from run 0: {moved} of {PAIRS * W}")
    for k, r in enumerate(runs[1:], 1):
        for key in ("rows", "gspec", "dbase", "dact"):
            _same_bits(r[key], runs[0][key], f"run {k} against run 0: {key}")
