"""The decoded-mode TBPTT loss on an MI355X: decoded_loss_kernel and latent_deltas_kernel (csrc/sur_decoded.hip) at their own
entry points against the oracle of tests/_sur_decoded_oracle.py, on the cases, storages and scalings the delta loss is held to
(tests/test_surrogate_tail_gpu.py).  Bounds:
  dout_all, outdeltas, deltas, d_all   bit-equal to the fp32 numpy spelling (one rounding per operation, nothing contracted)
  loss, hsteploss[1:], means, stds     within one fp32 rounding (relative 2^-24) of the fp64 sums: each is ONE rounding of an fp64
                                       value whose own error is far below that; the precondition |mean| <= std keeps the
                                       variance free of cancellation
  hsteploss[0], row T-1 of dout_all    exactly zero"""
import ctypes
import math

import numpy as np
import pytest
import torch

import _sur_decoded_oracle as do
import _sur_tail_oracle as so
from test_surrogate_tail_gpu import LOSS_CASES, _device_view

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DELTA = 0.25
SENT = so.bits(np.float32(so.SENTINEL).reshape(1))[0]


def _lib():
    from pdecontrol.surrogates import hipops
    return hipops.load()


def _stream():
    import hipbind
    return hipbind.stream()


def _ok(rc):
    assert rc == 0, (rc, _lib().sur_last_error().decode())


def _host(t):
    return t.detach().cpu().numpy().copy()


class _Out:
    """The outputs of one loss, each between guard sentinels."""
    NAMES = ("outdeltas", "deltas", "dout_all", "hstep", "loss", "stats")

    def __init__(self, B, T, N):
        sizes = (B * (T - 1) * N, B * (T - 1) * N, T * B * N, T, 1, 4)
        self.flat, self.view = {}, {}
        for name, n in zip(self.NAMES, sizes):
            self.flat[name], self.view[name] = so.guarded(n, DEV)

    def host(self):
        return {k: _host(v) for k, v in self.view.items()}

    def gaps_intact(self):
        return all(bool(np.all(so.bits(x[:so.GAP]) == SENT) and np.all(so.bits(x[-so.GAP:]) == SENT)) for x in self.flat.values())


def _loss(states, out_all, B, T, N, mean, stdv, out, partial, ticket, dout=True):
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _ok(_lib().sur_tbptt_decoded_loss(_stream(), p(states), states.stride(0), states.stride(1), p(out_all), B, T, N, DELTA, mean, stdv,
                                      *(p(out.view[k]) if k != "dout_all" or dout else None for k in _Out.NAMES), p(partial), p(ticket)))


@pytest.mark.parametrize("mean,stdv", [(0.0, 1.0), (0.01, math.sqrt(0.5))], ids=["identity", "scaled"])
@pytest.mark.parametrize("storage", ["batch", "time", "padded"])
@pytest.mark.parametrize("B,T,N", LOSS_CASES)
def test_decoded_loss_against_fp64(B, T, N, storage, mean, stdv):
    s_np, o_np = do.decoded_inputs(B, T, N, 40, storage)
    ref = do.decoded_loss_oracle(s_np, o_np, DELTA, mean, stdv)
    alt = do.decoded_loss_oracle(s_np, o_np, DELTA, mean, stdv, order=1)
    assert abs(ref["stats"][0]) <= ref["stats"][1] and abs(ref["stats"][2]) <= ref["stats"][3], "|mean| <= std for both populations"
    for key, pick in (("loss", ...), ("hsteploss", slice(1, None)), ("stats", ...)):
        assert so.rel_err(np.asarray(alt[key])[pick].astype(np.float32), np.asarray(ref[key])[pick]) <= so.U, \
            f"the bound holds for another summation order: {key}"
    keep, states = _device_view(s_np)
    keep_bits = so.bits(keep)
    out_all = torch.from_numpy(o_np).to(DEV)
    pflat, partial = so.guarded(40 * T, DEV, dtype=torch.float64, fill=float("nan"))
    tflat, ticket = so.guarded(1, DEV, dtype=torch.int32, fill=0)
    runs = []
    for _ in range(2):
        partial.fill_(float("nan"))
        out = _Out(B, T, N)
        _loss(states, out_all, B, T, N, mean, stdv, out, partial, ticket)
        torch.cuda.synchronize(DEV)
        assert int(ticket) == 0 and out.gaps_intact()
        assert np.all(_host(tflat)[[0, 1, 2, -3, -2, -1]] == int(np.int32(float(so.SENTINEL))))
        assert np.all(_host(pflat)[:so.GAP] == float(so.SENTINEL)) and np.all(_host(pflat)[-so.GAP:] == float(so.SENTINEL))
        runs.append(out.host())
    assert np.array_equal(so.bits(keep), keep_bits) and np.array_equal(so.bits(out_all), so.bits(o_np)), "the inputs are read only"
    one, two = runs
    for key in _Out.NAMES:
        assert np.array_equal(so.bits(one[key]), so.bits(two[key])), f"two runs differ in {key}"
    for key in ("dout_all", "outdeltas", "deltas"):
        assert np.array_equal(so.bits(one[key]), so.bits(ref[key].reshape(-1))), f"{key}: the fp32 spelling, bit for bit"
    assert not so.bits(one["dout_all"].reshape(T, -1)[T - 1]).any(), "row T - 1 of dout_all is exactly zero"
    assert so.bits(one["hstep"][:1])[0] == 0, "hsteploss[0] is exactly zero"
    errs = dict(loss=so.rel_err(one["loss"], [ref["loss"]]), hsteploss=so.rel_err(one["hstep"][1:], ref["hsteploss"][1:]),
                means=so.rel_err(one["stats"][[0, 2]], ref["stats"][[0, 2]]), stds=so.rel_err(one["stats"][[1, 3]], ref["stats"][[1, 3]]))
    so.record(case=f"decoded-loss-B{B}-T{T}-N{N}-{storage}-mean{mean}", **{k: v / so.U for k, v in errs.items()}, unit="2^-24 relative")
    for key, e in errs.items():
        assert e <= so.U, (key, e / so.U)
    # without dout_all: nothing is written where it would be, everything else is the same
    out = _Out(B, T, N)
    _loss(states, out_all, B, T, N, mean, stdv, out, partial, ticket, dout=False)
    torch.cuda.synchronize(DEV)
    assert np.all(so.bits(out.flat["dout_all"]) == SENT) and out.gaps_intact() and int(ticket) == 0
    for key, value in out.host().items():
        assert key == "dout_all" or np.array_equal(so.bits(value), so.bits(one[key])), key
    # sur_latent_deltas on the same rollout: the rows of outdeltas, and row T-1 from the oracle
    dflat, d_all = so.guarded(T * B * N, DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _ok(_lib().sur_latent_deltas(_stream(), p(states), states.stride(0), p(out_all), T, B, N, DELTA, mean, stdv, p(d_all)))
    torch.cuda.synchronize(DEV)
    got = _host(d_all).reshape(T, B, N)
    assert np.all(so.bits(dflat[:so.GAP]) == SENT) and np.all(so.bits(dflat[-so.GAP:]) == SENT)
    assert np.array_equal(so.bits(got[:T - 1].transpose(1, 0, 2)), so.bits(one["outdeltas"].reshape(B, T - 1, N)))
    assert np.array_equal(so.bits(got), so.bits(do.latent_deltas_oracle(s_np[:, 0], o_np, DELTA, mean, stdv)))
