"""``fno_forward_chain`` (csrc/fno.hip, include/spectral/forward_chain.h) on the GPU: ``delta`` and ``out`` are, byte for byte,
what one ``fno_forward`` launch per step writes; the surroundings of both outputs stay as they were; a second launch and a
replayed hipGraph give the same bytes; every step is within the whole-network kernels' own bound of the fp64 walk
(tests/_fno_oracle.py); and with ``PDECONTROL_FNO_CHAIN=1`` ``rollout`` takes the chain exactly when nobody will ask for a
gradient, with the bytes of ``PDECONTROL_FNO_CHAIN=0`` and of the default, which keeps the per-step launches.  The per-step launches of a case are computed once and shared by its tests."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fno_oracle as fo  # noqa: E402

pytestmark = pytest.mark.gpu

# (n, nb, steps): one step (the chain degenerates to fno_forward), two, more steps than waves, one position tile per wave,
# two tiles per wave with the LDS layout above 64 KB
SHAPES = [(64, 1, 1), (64, 3, 2), (64, 3, 7), (128, 2, 5), (512, 2, 3)]
PAD = 37                       # floats of fill pattern before and after each output
FILL = -7.5
CSCALE, CSHIFT = 0.05 * 1.37, -0.01
FLOOR, FACTOR = 2.0 ** -22, 4.0                # tests/test_fno_kernels_gpu.py:38-39, the bound of fno_forward


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _net():
    from pdecontrol.surrogates import fno_hip
    m64, m32 = fo.make_model("default"), fo.make_model("default", torch.float32)
    params = [p.detach().to(_dev()).contiguous() for p in fno_hip.parameters_of(m32)]
    w, keep = fno_hip._weights_struct(params)
    return {"m64": m64, "m32": m32, "w": w, "keep": (params, keep)}


def _forward(net, u, act, delta, out):
    """One ``fno_forward`` launch through the C ABI: ``u``, ``act``, ``delta``, ``out`` contiguous [nb, n]."""
    from pdecontrol.surrogates import fno_hip
    nb, n = u.shape
    fno_hip._check(fno_hip.load().fno_forward(fno_hip._stream(), ctypes.byref(net["w"]), 32, 16, 4, n, nb, nb, fno_hip._ptr(u), 0, n,
                                              fno_hip._ptr(act), 0, n, CSCALE, CSHIFT, fno_hip._ptr(delta), fno_hip._ptr(out),
                                              None, None, 0, 0))


@functools.lru_cache(maxsize=None)
def _case(n, nb, steps):
    """Inputs on the device and the per-step launches' delta / out [steps, nb, n] (numpy); never modified."""
    net = _net()
    u, act, _, _ = fo.inputs(n, (steps + 1) * nb, seed=steps)
    u0 = u[:nb].contiguous().to(_dev())
    act = act[nb:].reshape(steps, nb, n).contiguous().to(_dev())
    delta, out = torch.empty((steps, nb, n), device=_dev()), torch.empty((steps, nb, n), device=_dev())
    for k in range(steps):
        _forward(net, u0 if k == 0 else out[k - 1], act[k], delta[k], out[k])
    torch.cuda.synchronize()
    ref = {"delta": delta.cpu().numpy(), "out": out.cpu().numpy()}
    assert np.isfinite(ref["delta"]).all() and np.isfinite(ref["out"]).all()
    if steps > 1:       # the steps differ: writing a step into another's slot cannot pass
        assert not np.array_equal(ref["delta"][0], ref["delta"][1])
    return {"n": n, "nb": nb, "steps": steps, "net": net, "u0": u0, "act": act, "ref": ref}


def _padded(floats):
    """(the flat fill-patterned buffer, the offset of ``floats`` floats inside it)"""
    return torch.full((2 * PAD + floats,), FILL, device=_dev(), dtype=torch.float32), PAD


class Launch:
    """The buffers and the argument struct of one chain call of a case.

    layout "plain":   u0 [nb, n] and act [steps, nb, n] time major in buffers of their own.
    layout "rollout": what ``_forward_launches`` passes -- act a [B, K, 1, N] batch-major tensor (step stride N, sample
                      stride K * N), u0 the row block just before ``out`` in the same [steps + 1, nb, n] buffer."""

    def __init__(self, case, layout):
        from pdecontrol.surrogates import fno_hip
        n, nb, steps = case["n"], case["nb"], case["steps"]
        whole = steps * nb * n
        self.case, self.whole = case, whole
        self.dflat, d0 = _padded(whole)
        self.delta = self.dflat[d0:d0 + whole].view(steps, nb, n)
        if layout == "rollout":
            self.oflat, o0 = _padded(whole + nb * n)
            rows = self.oflat[o0:o0 + whole + nb * n].view(steps + 1, nb, n)
            rows[0].copy_(case["u0"])
            self.u0, self.out = rows[0], rows[1:]
            self.out_slice = slice(o0 + nb * n, o0 + nb * n + whole)
            self.act = case["act"].transpose(0, 1).contiguous().unsqueeze(2)            # [B, K, 1, N]
            ast, asb = self.act.stride(1), self.act.stride(0)
            assert (steps == 1 or ast == n) and (nb == 1 or asb == steps * n)
            assert self.u0.data_ptr() + 4 * nb * n == self.out.data_ptr()
        else:
            self.oflat, o0 = _padded(whole)
            self.u0, self.out = case["u0"], self.oflat[o0:o0 + whole].view(steps, nb, n)
            self.out_slice = slice(o0, o0 + whole)
            self.act = case["act"]
            ast, asb = self.act.stride(0), self.act.stride(1)
        self.delta_slice = slice(d0, d0 + whole)
        self.args = fno_hip.FnoChainArgs(ctypes.pointer(case["net"]["w"]), CSCALE, CSHIFT, self.u0.data_ptr(), n, self.act.data_ptr(),
                                         ast, asb, self.delta.data_ptr(), self.out.data_ptr(), steps)

    def __call__(self):
        from pdecontrol.surrogates import fno_hip
        fno_hip.forward_chain(fno_hip._stream(), self.case["n"], self.case["nb"], self.args)

    def clear(self):
        self.dflat[self.delta_slice] = FILL
        self.oflat[self.out_slice] = FILL

    def check(self, what):
        """Both outputs are the per-step bytes and the fill pattern around them is intact."""
        torch.cuda.synchronize()
        ref = self.case["ref"]
        for name, flat, cut in (("delta", self.dflat, self.delta_slice), ("out", self.oflat, self.out_slice)):
            host = flat.cpu().numpy()
            got = host[cut].reshape(ref[name].shape)
            assert got.tobytes() == ref[name].tobytes(), (what, name, float(np.nanmax(np.abs(got - ref[name]))))
            around = np.ones(host.size, bool)
            around[cut] = False
            if name == "out" and self.u0.data_ptr() != self.case["u0"].data_ptr():   # the rollout layout: u0 in out's buffer
                first = cut.start - self.u0.numel()
                assert host[first:cut.start].tobytes() == self.case["u0"].cpu().numpy().tobytes(), (what, "u0 was written")
                around[first:cut.start] = False
            assert np.all(host[around] == np.float32(FILL)), (what, name, "the fill pattern around an output changed")


@pytest.mark.parametrize("n,nb,steps", SHAPES, ids=[f"n{n}_b{nb}_k{k}" for n, nb, k in SHAPES])
@pytest.mark.parametrize("layout", ("plain", "rollout"))
def test_the_chain_writes_the_bytes_of_the_per_step_launches(n, nb, steps, layout):
    case = _case(n, nb, steps)
    launch = Launch(case, layout)
    launch()
    launch.check((n, nb, steps, layout, "first launch"))
    launch.clear()
    launch()                                         # a second launch from the same inputs gives the same bytes
    launch.check((n, nb, steps, layout, "second launch"))
    # one launch captured into a hipGraph (the twiddle matrix of this width exists: the eager calls above) and replayed
    launch.clear()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side):
        launch()
    torch.cuda.synchronize()
    launch.clear()
    graph.replay()
    launch.check((n, nb, steps, layout, "graph replay"))


def _err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = float(np.abs(ref).max())
    return float(np.abs(got - ref).max()) / scale if scale > 0 else float(np.abs(got).max())


def test_every_step_is_within_the_forward_kernels_bound_of_fp64():
    """(64, 3, 7), chained step by step: step k's fp64 walk and its fp32 yardstick both start from the base row the kernel
    itself started from (u0, then the kernel's own out[k - 1]), so that a step's error is that step's;
    ``e_hip <= max(4 e_ref, 2^-22)`` on each step's delta and out, the bound tests/test_fno_kernels_gpu.py holds
    ``fno_forward`` to."""
    case = _case(64, 3, 7)
    net = case["net"]
    launch = Launch(case, "plain")
    launch()
    torch.cuda.synchronize()
    delta, out = launch.delta.cpu(), launch.out.cpu()
    act, failures = case["act"].cpu(), []
    for k in range(case["steps"]):
        base = case["u0"].cpu() if k == 0 else out[k - 1]
        ref = fo.walk(net["m64"], base, act[k], CSCALE, CSHIFT)
        yard = fo.fp32_as_walk(net["m32"], base, act[k], cscale=CSCALE, cshift=CSHIFT)
        for name, got in (("delta", delta[k].numpy()), ("out", out[k].numpy())):
            e_ref, e_hip = _err(yard[name], ref[name]), _err(got, ref[name])
            print(f"fno chain parity step {k} {name}: e_ref {e_ref:.3e} e_hip {e_hip:.3e}")
            if not e_hip <= max(FACTOR * e_ref, FLOOR):
                failures.append(f"step {k} {name}: e_hip {e_hip:.3e} > max(4 x e_ref {e_ref:.3e}, 2^-22)")
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------------------------------
# the default route against the switch
# ---------------------------------------------------------------------------------------------------------------------
N, B, TAU, K = 64, 3, 2, 6
TSTEP = 0.05


def _surrogate(seed=3):
    from pdecontrol.architectures.fno import BurgersFNO
    torch.manual_seed(seed)
    f = BurgersFNO()
    return f.surrogate(delta=TSTEP, dscaling=None, **f.model()).to(_dev())


def _rollout(sur, grad, switch, monkeypatch):
    """(outputs, deltas, chain launches, parameter gradients or None) of one ``rollout`` call."""
    from pdecontrol.surrogates import fno_hip
    u, act, g_d, g_o = fo.inputs(N, B * K, seed=9)
    states = u.view(B, K, 1, N)[:, :TAU].contiguous().to(_dev())
    actions = act.view(B, K, 1, N).to(_dev())
    k = torch.arange(K)
    calls, real = [], fno_hip.forward_chain
    with monkeypatch.context() as m:
        m.setattr(fno_hip, "forward_chain", lambda *a, **kw: (calls.append(a[1:3]), real(*a, **kw))[1])
        if switch is None:
            m.delenv("PDECONTROL_FNO_CHAIN", raising=False)
        else:
            m.setenv("PDECONTROL_FNO_CHAIN", switch)
        for p in sur.parameters():
            p.grad = None
        with torch.enable_grad() if grad else torch.no_grad():
            out = sur.rollout(states=states, actions=actions, times=TSTEP * k, targets=TSTEP * (k + 1))
            grads = None
            if grad:
                loss = (out.deltas * g_d.view(B, K, 1, N).to(_dev())).sum() + (out.outputs * g_o.view(B, K, 1, N).to(_dev())).sum()
                loss.backward()
                grads = [p.grad.detach().cpu().numpy().copy() for p in sur.parameters()]
    torch.cuda.synchronize()
    return out.outputs.detach().cpu().numpy(), out.deltas.detach().cpu().numpy(), calls, grads


def test_rollout_takes_the_chain_without_a_gradient_and_never_with_one(monkeypatch):
    sur = _surrogate()
    outputs, deltas, calls, _ = _rollout(sur, False, "1", monkeypatch)
    assert calls == [(N, B)], "one chain launch for the K - tau free-running steps"
    assert outputs.shape == deltas.shape == (B, K, 1, N) and np.isfinite(outputs).all()
    for switch in ("0", None):                       # the switch off, and the default (off: profiles/fno_chain_bench.json)
        off_outputs, off_deltas, off_calls, _ = _rollout(sur, False, switch, monkeypatch)
        assert off_calls == []
        assert outputs.tobytes() == off_outputs.tobytes() and deltas.tobytes() == off_deltas.tobytes()
    # parameters that require grad under no_grad: still nobody to ask for a gradient
    assert all(p.requires_grad for p in sur.parameters())
    # grad mode on: the per-step launches (they save what the backward pass reads), with the switch either way
    g_outputs, g_deltas, g_calls, grads = _rollout(sur, True, "1", monkeypatch)
    assert g_calls == []
    assert g_outputs.tobytes() == outputs.tobytes() and g_deltas.tobytes() == deltas.tobytes()
    _, _, g_off_calls, grads_off = _rollout(sur, True, "0", monkeypatch)
    assert g_off_calls == [] and len(grads) == len(grads_off) > 0
    assert all(np.abs(g).max() > 0 for g in grads)
    for a, b in zip(grads, grads_off):
        assert a.tobytes() == b.tobytes()
    # a single free-running step is no chain: the launch it would replace is one launch (``fno_hip.rollout`` itself:
    # ``surrogate.rollout`` may append a trailing internal step to the action list)
    from pdecontrol.surrogates import fno_hip
    u, act, _, _ = fo.inputs(N, B * K, seed=9)
    states, acts = u.view(B, K, 1, N)[:, :TAU].contiguous().to(_dev()), act.view(B, K, 1, N)[:, :TAU + 1].contiguous().to(_dev())
    calls, real = [], fno_hip.forward_chain
    with monkeypatch.context() as m, torch.no_grad():
        m.setattr(fno_hip, "forward_chain", lambda *a, **kw: (calls.append(a[1:3]), real(*a, **kw))[1])
        m.setenv("PDECONTROL_FNO_CHAIN", "1")
        d, o = fno_hip.rollout(sur.model, states, acts, TAU, TSTEP, sur.dscaling)
    assert calls == [] and o.shape == (B, TAU + 1, 1, N)
    assert o.cpu().numpy().tobytes() == outputs[:, :TAU + 1].tobytes(), "the first free-running step of the longer rollout"
