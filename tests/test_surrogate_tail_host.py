"""The tail of the surrogate's training step without a GPU: the oracles of tests/_sur_tail_oracle.py against independent
spellings, the kernels' Adam expression in plain fp32 numpy (with fp32 and with cancellation-free bias corrections) judged
in the units of tests/_sac_models.py, the synthetic pack builder, and every refusal of the reduction, fold, Adam and delta
loss entry points through the loaded library -- each is turned away on the host before any launch."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import _sur_tail_oracle as so
from _sac_models import HYPERS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "model-based-pde-control_amd", "lib", "libsurrogate_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libsurrogate_hip.so not built")


# ----------------------------------------------------------------------------------------------------------------------
# the oracles
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mean,stdv", [(0.0, 1.0), (0.01, math.sqrt(0.5))])
@pytest.mark.parametrize("B,T,N", [(1, 2, 64), (10, 5, 100), (5, 7, 205)])
def test_loss_oracle_is_the_torch_op_spelling_in_fp64(B, T, N, mean, stdv):
    """training.py's loss section (diff / delta through the undscaling, MSELoss(reduction="none"), the means and
    Tensor.std()) in fp64 from the oracle's fp32 deltas and errors: the fp64 half of the oracle is that spelling."""
    states, d_all = so.loss_inputs(B, T, N, 3)
    delta = 0.25
    ref = so.delta_loss_oracle(states, d_all, delta, mean, stdv)
    # the fp32 half against torch's fp32 ops, bit for bit
    s = torch.from_numpy(np.ascontiguousarray(states)).unsqueeze(2)                    # [B, T, 1, N]
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    deltas = (torch.diff(s, dim=1) / f32(delta) - f32(mean)) / f32(stdv)
    assert np.array_equal(so.bits(deltas[:, :, 0]), so.bits(ref["deltas"]))
    outdeltas = torch.from_numpy(d_all).unsqueeze(2).transpose(0, 1)[:, :-1]           # [B, T-1, 1, N]
    err32 = outdeltas - deltas
    sq = (err32 * err32).double()
    assert np.array_equal(so.bits((torch.tensor(2.0 / sq.numel(), dtype=torch.float32) * err32)[:, :, 0].transpose(0, 1)),
                          so.bits(ref["dd_all"][:T - 1]))
    assert not ref["dd_all"][T - 1].any()
    np.testing.assert_allclose(float(sq.mean()), ref["loss"], rtol=1e-13)
    np.testing.assert_allclose(sq.mean(dim=(0, 2, 3)).numpy(), ref["hsteploss"], rtol=1e-13)
    od, dl = outdeltas.double(), deltas.double()
    want = [float(od.mean()), float(od.std()), float(dl.mean()), float(dl.std())]
    np.testing.assert_allclose(ref["stats"], want, rtol=1e-11)
    # the second summation order stays within one fp32 rounding, and the inputs keep |mean| <= std
    alt = so.delta_loss_oracle(states, d_all, delta, mean, stdv, order=1)
    for key in ("loss", "hsteploss", "stats"):
        assert so.rel_err(np.asarray(alt[key]).astype(np.float32), ref[key]) <= so.U, key
    assert abs(ref["stats"][0]) <= ref["stats"][1] and abs(ref["stats"][2]) <= ref["stats"][3]


def test_reduce_and_fold_oracles_are_numpy_sums():
    rs = np.random.RandomState(5)
    p = so.mixed_rows(rs, 40, 19)
    s, a = so.reduce_rows(p, 33)
    np.testing.assert_allclose(s, np.sum(p[:33].astype(np.float64), axis=0), rtol=0, atol=1e-12 * a.max())
    np.testing.assert_allclose(a, np.sum(np.abs(p[:33].astype(np.float64)), axis=0), rtol=1e-14)
    folded, mag = so.fold_rows(p, 3, 20, 30)
    want = p.astype(np.float64)
    want[30] += np.sum(want[3:23], axis=0)
    want[3:23] = 0.0
    np.testing.assert_allclose(folded, want, rtol=0, atol=1e-12 * mag.max())
    assert np.array_equal(folded[:3], p[:3]) and np.array_equal(folded[23:30], p[23:30]) and np.array_equal(folded[31:], p[31:])
    assert so.depth_bound(769, 1.0) == (25 + 32) * so.U and so.depth_bound(1, 1.0) == 33 * so.U


# ----------------------------------------------------------------------------------------------------------------------
# the kernels' Adam expression in plain fp32
# ----------------------------------------------------------------------------------------------------------------------
def adam_fp32(p, m, v, g, t, lr, beta1, beta2, eps, double_bc):
    """flush_grads_body's / adam_apply_body's update in fp32 numpy, one rounding per operation.  ``double_bc``: the bias
    corrections 1 - beta^t from fp64 (rounded to fp32 once), else 1 - powf(beta, t) in fp32 with a correctly rounded powf."""
    f = np.float32
    lr, b1, b2, eps = f(lr), f(beta1), f(beta2), f(eps)
    if double_bc:
        bc1, bc2 = f(1.0 - float(b1) ** t), f(1.0 - float(b2) ** t)
    else:
        bc1, bc2 = f(1) - f(float(b1) ** t), f(1) - f(float(b2) ** t)
    m1 = b1 * m + (f(1) - b1) * g
    v1 = b2 * v + (f(1) - b2) * g * g
    denom = np.sqrt(v1) / np.sqrt(bc2) + eps
    p1 = p - (lr / bc1) * (m1 / denom)
    assert p1.dtype == m1.dtype == v1.dtype == np.float32
    return p1, m1, v1


ADAM_STEPS = tuple(range(1, 31)) + (100, 1000, 10000)


def test_adam_expression_in_fp32_needs_cancellation_free_bias_corrections():
    """The kernels' expression with double bias corrections stays within UNIT_BOUND units of the fp64 replay at every step
    count.  With fp32 bias corrections (1 - powf, the power correctly rounded) the step multiplier sqrt(bc2) / bc1 alone is off
    by up to 57 u = 3.6 units at t = 2 ... 4, which leaves the other roundings no room under the bound; the worst units of
    that form per step go to the observed file (p' on its own, and the worst of m', v', p').  Moments at step t: those of a constant-magnitude gradient history, rounded to fp32."""
    rs = np.random.RandomState(17)
    n = 400
    worst = {"double": {}, "fp32": {}, "double_p": {}, "fp32_p": {}}
    for name, h in HYPERS.items():
        hyper = (h["lr"], h["betas"][0], h["betas"][1], h["eps"])
        for t in ADAM_STEPS:
            g = so.gradient_classes(rs, n)
            # next to a small parameter the history has the gradient's sign: m' = beta1 m + (1 - beta1) g does not cancel,
            # so its own roundings stay small against the step they are judged by
            g_hist = so.gradient_classes(rs, n, np.where(so.small_parameter(n), np.sign(g), rs.choice([-1.0, 1.0], n))).astype(np.float64)
            m = (g_hist * (1.0 - hyper[1] ** (t - 1))).astype(np.float32)
            v = (g_hist ** 2 * (1.0 - hyper[2] ** (t - 1))).astype(np.float32)
            p = so.parameter_classes(rs, n)
            ref = so.adam_replay(p, m, v, g, t, *hyper, fp32_hyper=True)
            for form, flag in (("double", True), ("fp32", False)):
                units = so.adam_units(p, m, v, g, *adam_fp32(p, m, v, g, t, *hyper, double_bc=flag), ref)
                worst[form][t] = max(worst[form].get(t, 0.0), max(units.values()))
                worst[form + "_p"][t] = max(worst[form + "_p"].get(t, 0.0), units["p"])
    so.record(case="adam-expression-fp32-numpy", bound=so.UNIT_BOUND, double_bc=worst["double"], fp32_bc=worst["fp32"],
           double_bc_p=worst["double_p"], fp32_bc_p=worst["fp32_p"])
    assert max(worst["double"].values()) <= so.UNIT_BOUND, worst["double"]
    assert worst["fp32"][1] <= so.UNIT_BOUND           # 1 - beta is exact (Sterbenz): the first update is not affected


# ----------------------------------------------------------------------------------------------------------------------
# the builder
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["enc", "chunk"])
@pytest.mark.parametrize("name", so.LAYOUTS)
def test_builder_places_the_tensors_where_the_layout_says(name, kind):
    sizes = so.layout(name, kind)
    pack = so.synthetic_pack(kind, sizes, 5, 7, "cpu")
    assert pack.psize == sum(sizes) == sum(pack.c.size[i] for i in range(so.nparam(kind)))
    off = so.GAP
    for i, s in enumerate(sizes):
        assert pack.c.w[i] == pack.wflat.data_ptr() + 4 * off and pack.c.g[i] == pack.gflat.data_ptr() + 4 * off
        off += s + so.GAP
    assert off == pack.wflat.numel() == pack.gflat.numel()
    assert pack.c.partial == pack.partial_flat.data_ptr() + 4 * so.GAP and pack.c.rows == 5
    assert pack.partial.shape == (7, pack.psize) and int(pack.gap_mask.sum()) == so.GAP * (len(sizes) + 1)
    assert pack.gaps_intact()
    pack.put(pack.wflat, np.arange(pack.psize))
    assert np.array_equal(pack.get(pack.wflat).numpy(), np.arange(pack.psize, dtype=np.float32)) and pack.gaps_intact()
    assert float(pack.wflat[pack.offs[1]]) == 1.0 and float(pack.wflat[pack.offs[-1] + sizes[-1] - 1]) == pack.psize - 1
    pack.wflat[pack.offs[3] - 1] = 0.0
    assert not pack.gaps_intact()
    # what the layouts promise
    ends = np.cumsum(sizes)
    starts = ends - np.asarray(sizes)
    assert 1 in sizes
    if name == "tiny":
        assert pack.psize < so.FLUSH_COLS
    else:
        assert any(e % so.FLUSH_COLS == 0 for e in ends[:-1]), "a tensor ends on a block edge"
        assert any(s // so.FLUSH_COLS != (e - 1) // so.FLUSH_COLS for s, e in zip(starts, ends)), "a tensor straddles one"
    assert (pack.psize % so.FLUSH_COLS == 0) == (name == "even")
    if name == "wide":
        assert so.ADAM_TPB < pack.psize < 2 * so.ADAM_TPB
        assert any(s < so.ADAM_TPB < e for s, e in zip(starts, ends)), "a tensor crosses the Adam block edge"


def test_layouts_of_an_all_call_have_three_different_block_counts():
    blocks = {name: so.flush_blocks(sum(so.layout(name, "enc"))) for name in so.LAYOUTS}
    assert blocks == {name: so.flush_blocks(sum(so.layout(name, "chunk"))) for name in so.LAYOUTS}
    assert len(set(blocks.values())) == len(blocks)


# ----------------------------------------------------------------------------------------------------------------------
# refusals: through the loaded library, on the host, no launch
# ----------------------------------------------------------------------------------------------------------------------
P = ctypes.c_void_p(16)            # a non-NULL address nothing dereferences on the host


def _lib():
    from pdecontrol.surrogates import hipops
    return hipops.load(), hipops


def _fake_pack(kind, rows=8, partial=True, null_g=None, null_w=None):
    _, hipops = _lib()
    c = (hipops.EncoderParams if kind == "enc" else hipops.ChunkParams)()
    for i, s in enumerate(so.layout("odd", kind)):
        c.size[i], c.w[i], c.g[i] = s, 16, 16
    if null_g is not None:
        c.g[null_g] = None
    if null_w is not None:
        c.w[null_w] = None
    c.partial, c.rows = (16 if partial else None), rows
    return c


def _fake_adam(**null):
    _, hipops = _lib()
    fields = dict(m=16, v=16, step=16, ticket=16, lr=16)
    fields.update({k: None for k in null})
    return hipops.AdamParams(fields["m"], fields["v"], fields["step"], fields["ticket"], fields["lr"], 0.9, 0.999, 1e-8)


def _refused(rc, prefix):
    lib, _ = _lib()
    message = lib.sur_last_error().decode()
    assert rc == -1 and message.startswith(prefix), (rc, message)


FOLD_REFUSALS = [("dst inside the folded range", (2, 4, 3)), ("dst at the range's first row", (2, 4, 2)),
                 ("dst at its last row", (2, 4, 5)), ("range past rows", (5, 4, 0)), ("count 0", (2, 0, 0)),
                 ("negative count", (2, -1, 0)), ("negative base", (-1, 3, 5)), ("dst past rows", (0, 2, 8)),
                 ("negative dst", (0, 2, -1))]


@needs_lib
@pytest.mark.parametrize("what,bad", FOLD_REFUSALS, ids=[r[0] for r in FOLD_REFUSALS])
@pytest.mark.parametrize("j", [0, 1, 2])
def test_fold_rows_refuses_before_any_launch(what, bad, j):
    lib, _ = _lib()
    packs = [_fake_pack("enc"), _fake_pack("enc"), _fake_pack("chunk")]
    good = [(0, 4, 7), (1, 7, 0), (4, 4, 3)]
    good[j] = bad
    arr = lambda k: (ctypes.c_int * 3)(*[g[k] for g in good])
    rc = lib.sur_fold_rows(None, ctypes.byref(packs[0]), ctypes.byref(packs[1]), ctypes.byref(packs[2]), arr(0), arr(1), arr(2))
    _refused(rc, f"sur_fold_rows: pack {j}:")


@needs_lib
def test_fold_rows_refuses_null_arguments():
    lib, _ = _lib()
    packs = [_fake_pack("enc"), _fake_pack("enc"), _fake_pack("chunk")]
    refs = [ctypes.byref(p) for p in packs]
    a = (ctypes.c_int * 3)(0, 0, 0)
    n = (ctypes.c_int * 3)(2, 2, 2)
    d = (ctypes.c_int * 3)(5, 5, 5)
    for k in range(3):
        args = list(refs)
        args[k] = None
        _refused(lib.sur_fold_rows(None, *args, a, n, d), "sur_fold_rows:")
    for k in range(3):
        arrays = [a, n, d]
        arrays[k] = None
        _refused(lib.sur_fold_rows(None, *refs, *arrays), "sur_fold_rows:")
    packs[1] = _fake_pack("enc", partial=False)
    _refused(lib.sur_fold_rows(None, refs[0], ctypes.byref(packs[1]), refs[2], a, n, d), "sur_fold_rows: pack 1:")


ADAM_FIELDS = ("m", "v", "step", "ticket", "lr")


@needs_lib
@pytest.mark.parametrize("field", ADAM_FIELDS)
def test_flush_and_adam_refuse_an_incomplete_descriptor(field):
    lib, _ = _lib()
    e0, e1, c2 = _fake_pack("enc"), _fake_pack("enc"), _fake_pack("chunk")
    good, bad = _fake_adam(), _fake_adam(**{field: True})
    _refused(lib.sur_flush_encoder_grads(None, ctypes.byref(e0), ctypes.byref(bad), 0), "flush: incomplete Adam descriptor")
    _refused(lib.sur_flush_chunk_grads(None, ctypes.byref(c2), ctypes.byref(bad), 0), "flush: incomplete Adam descriptor")
    for j in range(3):
        ads = [ctypes.byref(good)] * 3
        ads[j] = ctypes.byref(bad)
        _refused(lib.sur_flush_all_grads(None, ctypes.byref(e0), ads[0], ctypes.byref(e1), ads[1], ctypes.byref(c2), ads[2], 0),
                 f"sur_flush_all_grads: incomplete Adam descriptor {j}")
        _refused(lib.sur_adam_apply(None, ctypes.byref(e0), ads[0], ctypes.byref(e1), ads[1], ctypes.byref(c2), ads[2]),
                 f"sur_adam_apply: incomplete Adam descriptor {j}")


@needs_lib
def test_flush_and_adam_refuse_missing_packs_and_tensors():
    lib, _ = _lib()
    e0, e1, c2 = _fake_pack("enc"), _fake_pack("enc"), _fake_pack("chunk")
    ad = ctypes.byref(_fake_adam())
    r = ctypes.byref
    # a descriptor without its pack
    _refused(lib.sur_adam_apply(None, None, ad, r(e1), ad, r(c2), ad), "sur_adam_apply: descriptor without its parameter pack")
    _refused(lib.sur_adam_apply(None, r(e0), ad, None, ad, r(c2), ad), "sur_adam_apply: descriptor without its parameter pack")
    _refused(lib.sur_adam_apply(None, r(e0), ad, r(e1), ad, None, ad), "sur_adam_apply: descriptor without its parameter pack")
    assert lib.sur_adam_apply(None, None, None, None, None, None, None) == 0          # nothing to do, no launch
    # NULL gradient or weight tensors: first / middle / last slot of either pack kind, every position of the three-pack
    # calls.  A flush updates weights only with an Adam descriptor, so its NULL-weight cases carry one (without one the
    # weights are not read and the call is valid).
    for i in (0, 13, so.ENC_NPARAM - 1):
        for field, null in (("gradient", dict(null_g=i)), ("weight", dict(null_w=i))):
            bad = _fake_pack("enc", **null)
            for j in (0, 1):
                packs = [r(e0), r(e1), r(c2)]
                packs[j] = r(bad)
                _refused(lib.sur_adam_apply(None, packs[0], ad, packs[1], ad, packs[2], ad), f"sur_adam_apply: encoder {j} tensor {i}")
                _refused(lib.sur_flush_all_grads(None, packs[0], ad, packs[1], ad, packs[2], ad, 0),
                         f"sur_flush_all_grads: encoder {field} tensor {i}")
            _refused(lib.sur_flush_encoder_grads(None, r(bad), ad, 0), f"sur_flush_encoder_grads: {field} tensor {i}")
        for j in (0, 1):                                          # a NULL gradient is refused without a descriptor too
            packs = [r(e0), r(e1), r(c2)]
            packs[j] = r(_fake_pack("enc", null_g=i))
            _refused(lib.sur_flush_all_grads(None, packs[0], None, packs[1], None, packs[2], None, 0),
                     f"sur_flush_all_grads: encoder gradient tensor {i}")
        _refused(lib.sur_flush_encoder_grads(None, r(_fake_pack("enc", null_g=i)), None, 0), f"sur_flush_encoder_grads: gradient tensor {i}")
    for i in (0, 13, so.ST_NPARAM - 1):
        for field, null in (("gradient", dict(null_g=i)), ("weight", dict(null_w=i))):
            bad = _fake_pack("chunk", **null)
            _refused(lib.sur_adam_apply(None, r(e0), ad, r(e1), ad, r(bad), ad), f"sur_adam_apply: chunk tensor {i}")
            _refused(lib.sur_flush_all_grads(None, r(e0), ad, r(e1), ad, r(bad), ad, 0), f"sur_flush_all_grads: chunk {field} tensor {i}")
            _refused(lib.sur_flush_chunk_grads(None, r(bad), ad, 0), f"sur_flush_chunk_grads: {field} tensor {i}")
        _refused(lib.sur_flush_all_grads(None, r(e0), None, r(e1), None, r(_fake_pack("chunk", null_g=i)), None, 0),
                 f"sur_flush_all_grads: chunk gradient tensor {i}")
        _refused(lib.sur_flush_chunk_grads(None, r(_fake_pack("chunk", null_g=i)), None, 0), f"sur_flush_chunk_grads: gradient tensor {i}")
    # no pack, no partial buffer
    _refused(lib.sur_flush_encoder_grads(None, None, None, 0), "sur_flush_encoder_grads:")
    _refused(lib.sur_flush_chunk_grads(None, None, None, 0), "sur_flush_chunk_grads:")
    _refused(lib.sur_flush_encoder_grads(None, r(_fake_pack("enc", partial=False)), None, 0), "sur_flush_encoder_grads:")
    _refused(lib.sur_flush_chunk_grads(None, r(_fake_pack("chunk", partial=False)), None, 0), "sur_flush_chunk_grads:")
    for k in range(3):
        packs = [r(e0), r(e1), r(c2)]
        packs[k] = None
        _refused(lib.sur_flush_all_grads(None, packs[0], None, packs[1], None, packs[2], None, 0), "sur_flush_all_grads:")
        packs = [e0, e1, c2]
        packs[k] = _fake_pack("chunk" if k == 2 else "enc", partial=False)
        _refused(lib.sur_flush_all_grads(None, r(packs[0]), None, r(packs[1]), None, r(packs[2]), None, 0), "sur_flush_all_grads:")


LOSS_GOOD = dict(states=P, sb=6 * 64, st=64, d_all=P, b=3, t=6, n=64, delta=0.25, mean=0.0, stdv=1.0, deltas=P, dd_all=None,
                 hstep=P, loss=P, stats=P, partial=P, ticket=P, t_begin=1, t_end=4)
LOSS_REFUSALS = [dict(t=1, t_begin=0, t_end=1), dict(t=0), dict(b=0), dict(n=0), dict(sb=63), dict(st=63), dict(st=8),
                 dict(stdv=0.0), dict(stdv=-1.0), dict(stdv=float("nan")), dict(delta=0.0),
                 dict(states=None), dict(d_all=None), dict(deltas=None), dict(hstep=None), dict(loss=None), dict(stats=None),
                 dict(partial=None), dict(ticket=None)]
RANGE_REFUSALS = [dict(t_begin=3, t_end=3), dict(t_begin=4, t_end=2), dict(t_begin=-1, t_end=2), dict(t_begin=2, t_end=7),
                  dict(t_begin=6, t_end=7)]


def _loss_call(name, a):
    lib, _ = _lib()
    head = (None, a["states"], a["sb"], a["st"], a["d_all"], a["b"], a["t"], a["n"], a["delta"], a["mean"], a["stdv"], a["deltas"],
            a["dd_all"], a["hstep"], a["loss"], a["stats"], a["partial"], a["ticket"])
    if name == "sur_tbptt_delta_loss":
        return lib.sur_tbptt_delta_loss(*head)
    return getattr(lib, name)(*head, a["t_begin"], a["t_end"])


@needs_lib
@pytest.mark.parametrize("name", ["sur_tbptt_delta_loss", "sur_tbptt_delta_loss_range", "sur_tbptt_delta_loss_rows"])
def test_delta_loss_entry_points_refuse_before_any_launch(name):
    ranged = name != "sur_tbptt_delta_loss"
    for change in LOSS_REFUSALS + (RANGE_REFUSALS if ranged else []):
        _refused(_loss_call(name, dict(LOSS_GOOD, **change)), name + ":")


@needs_lib
def test_delta_loss_finalize_refuses_before_any_launch():
    lib, _ = _lib()
    good = dict(b=3, t=6, n=64, hstep=P, loss=P, stats=P, partial=P, ticket=P)
    for change in (dict(t=1), dict(b=0), dict(n=0), dict(hstep=None), dict(loss=None), dict(stats=None), dict(partial=None),
                   dict(ticket=None)):
        a = dict(good, **change)
        rc = lib.sur_tbptt_delta_loss_finalize(None, a["b"], a["t"], a["n"], a["hstep"], a["loss"], a["stats"], a["partial"], a["ticket"])
        _refused(rc, "sur_tbptt_delta_loss_finalize:")
