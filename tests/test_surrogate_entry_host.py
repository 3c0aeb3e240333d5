"""The encoder and chunk entry points of libsurrogate_hip.so without a GPU: every refusal through the loaded library, with its
exact return code and the start of its message.  Each case changes ONE field of an argument set that is otherwise valid, so
the one refusal it names is the only one the call can meet, whatever the order of the checks; no case reaches a launch (where
there is no GPU a case that slipped past validation would show as the launch-failure code -2, never as -1 or -4).  The valid
set itself is never called: its pointers are fake."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "model-based-pde-control_amd", "lib", "libsurrogate_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libsurrogate_hip.so not built")

A = 16                             # a non-NULL address nothing dereferences on the host
P = ctypes.c_void_p(A)
ENC_ENTRIES = ("sur_encoder_forward", "sur_encoder_backward", "sur_encoder_forward_multi", "sur_encoder_backward_multi split",
               "sur_encoder_backward_multi unsplit")
BWD_MULTI_FORMS = ("split", "unsplit")


def _lib():
    from pdecontrol.surrogates import hipops
    return hipops.load(), hipops


def _refused(rc, code, prefix):
    lib, _ = _lib()
    message = lib.sur_last_error().decode()
    assert rc == code and message.startswith(prefix), (rc, message)


def _enc(**change):
    """The N = 64 state encoder (channels 1, 8, 16, 16, strides 2, 2, 1) over fake pointers, 8 partial rows."""
    _, hipops = _lib()
    p = hipops.EncoderParams()
    for i in range(3 * hipops.RB_NPARAM):
        p.size[i], p.w[i], p.g[i] = 5, A, A
    p.c[:], p.stride[:], p.n, p.partial, p.rows = (1, 8, 16, 16), (2, 2, 1), 64, A, 8
    for key, value in change.items():
        setattr(p, key, value)
    return p


def _chunk(**change):
    """The N = 64 cell and decoder (4 action and 16 state channels on 16 latent positions) over fake pointers."""
    _, hipops = _lib()
    p = hipops.ChunkParams()
    for i in range(hipops.ST_NPARAM):
        p.size[i], p.w[i], p.g[i] = 5, A, A
    p.ca, p.cs, p.hq, p.c_mid, p.delta, p.mul, p.add, p.partial, p.rows = 4, 16, 16, 8, 0.1, 1.0, 0.0, A, 64
    for key, value in change.items():
        setattr(p, key, value)
    return p


def _ptrs(n, null=None):
    return (ctypes.c_void_p * n)(*[None if k == null else A for k in range(n)])


def _ints(values):
    return (ctypes.c_int * len(values))(*values)


# ----------------------------------------------------------------------------------------------------------------------
# encoder entry points
# ----------------------------------------------------------------------------------------------------------------------
def _encoder_backward(p, x=P, dz=P, row_base=2, row_count=4, saved=None):
    lib, _ = _lib()
    return lib.sur_encoder_backward(None, ctypes.byref(p), x, dz, 6, None, row_base, row_count, saved)


def _forward_multi(packs, njobs=None, null=None):
    """``null`` = (array, job): that job's pointer in the x, z or saved array is NULL."""
    lib, hipops = _lib()
    n = len(packs)
    ps = (ctypes.POINTER(hipops.EncoderParams) * n)(*[ctypes.pointer(p) for p in packs])
    arrays = {name: _ptrs(n, null[1] if null and null[0] == name else None) for name in ("x", "z", "saved")}
    return lib.sur_encoder_forward_multi(None, n if njobs is None else njobs, ps, arrays["x"], _ints([6] * n), arrays["z"],
                                         arrays["saved"], 4)


def _backward_multi(packs, form, njobs=None, null=None, row_bases=None, row_counts=None):
    """The split form carries a saved buffer and a workspace for every job, the unsplit form no workspace array."""
    lib, hipops = _lib()
    n = len(packs)
    ps = (ctypes.POINTER(hipops.EncoderParams) * n)(*[ctypes.pointer(p) for p in packs])
    arrays = {name: _ptrs(n, null[1] if null and null[0] == name else None) for name in ("x", "dz")}
    return lib.sur_encoder_backward_multi(None, n if njobs is None else njobs, ps, arrays["x"], arrays["dz"], _ints([6] * n),
                                          _ints(row_bases or [2] * n), _ints(row_counts or [4] * n), _ptrs(n),
                                          _ptrs(n) if form == "split" else None)


#: (partial, row_base, row_count) against a buffer of 8 rows; the valid set is (A, 2, 4)
ROW_REFUSALS = [("partial NULL", (None, 2, 4)), ("row_count 0", (A, 2, 0)), ("row_base -1", (A, -1, 4)),
                ("one row past the buffer", (A, 5, 4))]
ROW_IDS = [r[0] for r in ROW_REFUSALS]


@needs_lib
@pytest.mark.parametrize("what,bad", ROW_REFUSALS, ids=ROW_IDS)
def test_encoder_backward_refuses_partial_rows_outside_the_buffer(what, bad):
    partial, base, count = bad
    assert base + count <= 8 + 1
    _refused(_encoder_backward(_enc(partial=partial), row_base=base, row_count=count), -1, "sur_encoder_backward: partial rows [")


@needs_lib
@pytest.mark.parametrize("what,bad", ROW_REFUSALS, ids=ROW_IDS)
@pytest.mark.parametrize("j", [0, 1, 2])
@pytest.mark.parametrize("form", BWD_MULTI_FORMS)
def test_encoder_backward_multi_refuses_partial_rows_outside_the_buffer(form, j, what, bad):
    partial, base, count = bad
    packs = [_enc(), _enc(), _enc()]
    packs[j] = _enc(partial=partial)
    bases, counts = [2, 2, 2], [4, 4, 4]
    bases[j], counts[j] = base, count
    _refused(_backward_multi(packs, form, row_bases=bases, row_counts=counts), -1,
             f"sur_encoder_backward_multi: job {j}: partial rows [")


@needs_lib
def test_encoder_multi_calls_refuse_a_job_count_outside_their_range():
    packs = [_enc() for _ in range(4)]
    for njobs in (0, 3):
        _refused(_forward_multi(packs[:3], njobs=njobs), -1, "sur_encoder_forward_multi: bad argument (1 or 2 jobs)")
    for form in BWD_MULTI_FORMS:
        for njobs in (0, 4):
            _refused(_backward_multi(packs, form, njobs=njobs), -1, "sur_encoder_backward_multi: bad argument (1 to 3 jobs)")


@needs_lib
def test_encoder_calls_refuse_null_tensors():
    lib, _ = _lib()
    p = _enc()
    for x, z in ((None, P), (P, None)):
        _refused(lib.sur_encoder_forward(None, ctypes.byref(p), x, 6, z, P), -1, "sur_encoder_forward: bad argument")
        _refused(_encoder_backward(p, x=x, dz=z), -1, "sur_encoder_backward: bad argument")
    for j in (0, 1):                                          # job 0 and the last job
        for name in ("x", "z", "saved"):
            _refused(_forward_multi([_enc(), _enc()], null=(name, j)), -1, f"sur_encoder_forward_multi: job {j}: bad argument")
    for form in BWD_MULTI_FORMS:
        for j in (0, 2):
            for name in ("x", "dz"):                          # a NULL saved buffer is valid here: it selects the unsplit form
                _refused(_backward_multi([_enc(), _enc(), _enc()], form, null=(name, j)), -1,
                         f"sur_encoder_backward_multi: job {j}: bad argument")
            packs = [ctypes.pointer(_enc()) for _ in range(3)]
            packs[j] = None
            _, hipops = _lib()
            ps = (ctypes.POINTER(hipops.EncoderParams) * 3)(*packs)
            rc = lib.sur_encoder_backward_multi(None, 3, ps, _ptrs(3), _ptrs(3), _ints([6] * 3), _ints([2] * 3), _ints([4] * 3),
                                                _ptrs(3), _ptrs(3) if form == "split" else None)
            _refused(rc, -1, f"sur_encoder_backward_multi: job {j}: no parameters")


def _encoder_call(entry, bad, j):
    """``entry`` on valid arguments except that the pack (of job ``j`` in a multi call) is ``bad``; every call has a saved buffer."""
    lib, _ = _lib()
    if entry == "sur_encoder_forward":
        return lib.sur_encoder_forward(None, ctypes.byref(bad), P, 6, P, P)
    if entry == "sur_encoder_backward":
        return _encoder_backward(bad, saved=P)
    packs = [_enc() for _ in range(2 if entry == "sur_encoder_forward_multi" else 3)]
    packs[j if j == 0 else -1] = bad
    if entry == "sur_encoder_forward_multi":
        return _forward_multi(packs)
    return _backward_multi(packs, entry.split()[1])


GEOMETRY_REFUSALS = [("stride 3 does not divide 32", dict(stride=(ctypes.c_int * 3)(2, 3, 1)), "width 32 is not a multiple of stride 3 (block 1)"),
                     ("LayerNorm row of 48", dict(n=96), "N = 96 gives a LayerNorm row of 48 in block 0"),
                     ("LayerNorm row of 8", dict(n=32), "N = 32 gives a LayerNorm row of 8 in block 1"),
                     ("LayerNorm row of 320", dict(n=640), "N = 640 gives a LayerNorm row of 320 in block 0")]


@needs_lib
@pytest.mark.parametrize("what,change,text", GEOMETRY_REFUSALS, ids=[r[0] for r in GEOMETRY_REFUSALS])
@pytest.mark.parametrize("j", [0, 1], ids=["job 0", "last job"])
@pytest.mark.parametrize("entry", ENC_ENTRIES)
def test_encoder_calls_refuse_an_unsupported_geometry(entry, j, what, change, text):
    _refused(_encoder_call(entry, _enc(**change), j), -4, f"{entry.split()[0]}: {text}")


@needs_lib
@pytest.mark.parametrize("j", [0, 1], ids=["job 0", "last job"])
@pytest.mark.parametrize("entry", ENC_ENTRIES)
def test_encoder_calls_refuse_a_saved_buffer_the_geometry_has_no_record_for(entry, j):
    """No channels behind the input: enc_geometry looks at widths only, sur_encoder_saved_floats is 0.  (With a workspace array
    the multi backward takes such a job for its unsplit form, which refuses the saved buffer.)"""
    lib, _ = _lib()
    empty = _enc(c=(ctypes.c_int * 4)(1, 0, 0, 0))
    assert lib.sur_encoder_saved_floats(ctypes.byref(empty)) == 0 and lib.sur_encoder_saved_floats(ctypes.byref(_enc())) > 0
    last = j if j == 0 else (1 if entry == "sur_encoder_forward_multi" else 2)
    text = {"sur_encoder_forward": "sur_encoder_forward: this geometry has no saved-activation path",
            "sur_encoder_backward": "sur_encoder_backward: this geometry has no saved-activation path",
            "sur_encoder_forward_multi": f"sur_encoder_forward_multi: job {last}: geometry not float4-granular"}.get(
                entry, f"sur_encoder_backward_multi: job {last}: this geometry has no saved-activation path")
    _refused(_encoder_call(entry, empty, j), -4, text)


# ----------------------------------------------------------------------------------------------------------------------
# chunk entry points
# ----------------------------------------------------------------------------------------------------------------------
CHUNK_GOOD = dict(k=3, s=2, b=4, hc_bstride=256)


def _chunk_forward(name, p, saved=None, **change):
    lib, _ = _lib()
    a = dict(CHUNK_GOOD, **change)
    if name == "sur_chunk_forward":
        return lib.sur_chunk_forward(None, ctypes.byref(p), P, P, P, P, P, a["hc_bstride"], a["k"], a["s"], a["b"], P, P, P, P, saved)
    return lib.sur_latent_chunk_forward(None, ctypes.byref(p), P, P, P, P, a["hc_bstride"], a["k"], a["s"], a["b"], P, P, P, P, saved)


@needs_lib
@pytest.mark.parametrize("name", ["sur_chunk_forward", "sur_latent_chunk_forward"])
def test_chunk_forward_calls_refuse_before_any_launch(name):
    for change in (dict(k=0), dict(b=0), dict(s=0), dict(hc_bstride=-1)):
        _refused(_chunk_forward(name, _chunk(), **change), -1, f"{name}: bad argument (need K > 0, B > 0, S >= 1)")
    _refused(_chunk_forward(name, _chunk(hq=8)), -4, f"{name}: latent width N/4 = 8 must be a multiple of 16")
    _refused(_chunk_forward(name, _chunk(hq=24)), -4, f"{name}: N = 96 gives LayerNorm rows of 48 and 96 in the decoder")


def _span(k0, k1, s):
    _, hipops = _lib()
    return hipops.ChunkSpan(k0, k1, s, A, A, A, 256, None)


def _chunk_backward(name, p, row_base=3, row_count=None, saved=P, workspace=P, spans=None, nspans=None, k=6, b=4):
    """sur_chunks_backward covers [0, k) with ``spans`` (two spans of three steps when None); the others are one chunk."""
    lib, hipops = _lib()
    if name == "sur_chunks_backward":
        spans = [_span(0, 3, 2), _span(3, 6, 3)] if spans is None else spans
        arr = (hipops.ChunkSpan * max(len(spans), 1))(*spans)
        n = len(spans) if nspans is None else nspans
        count = 2 * b if row_count is None else row_count
        return lib.sur_chunks_backward(None, ctypes.byref(p), n, arr, P, P, P, P, k, b, P, row_base, count, saved, workspace)
    count = b if row_count is None else row_count
    head = (None, ctypes.byref(p), P, P, P, P, 256, P, P)
    tail = (None, None, k, 2, b, P, P, None, None, row_base, count, saved, workspace)
    if name == "sur_chunk_backward":
        return lib.sur_chunk_backward(*head, P, None, *tail)             # dd_all, no dout_all
    return lib.sur_latent_chunk_backward(*head, P, None, *tail)          # dout_all, no dz_all


CHUNK_BACKWARDS = {"sur_chunk_backward": 1, "sur_latent_chunk_backward": 1, "sur_chunks_backward": 2}    # spans of the valid set


@needs_lib
@pytest.mark.parametrize("name", CHUNK_BACKWARDS)
def test_chunk_backward_calls_refuse_before_any_launch(name):
    need = CHUNK_BACKWARDS[name] * 4                       # one row per span and sample, B = 4
    _refused(_chunk_backward(name, _chunk(), saved=None), -1, f"{name}: needs the `saved` buffer")
    _refused(_chunk_backward(name, _chunk(), workspace=None), -1, f"{name}: needs the `saved` buffer")
    _refused(_chunk_backward(name, _chunk(), row_count=need - 1), -1,
             f"{name}: partial gradient buffer has 64 rows, need [3, {3 + need - 1}) with at least {need} of them")
    _refused(_chunk_backward(name, _chunk(rows=3 + need - 1)), -1,
             f"{name}: partial gradient buffer has {3 + need - 1} rows, need [3, {3 + need}) with at least {need} of them")
    _refused(_chunk_backward(name, _chunk(partial=None)), -1, f"{name}: partial gradient buffer has")
    _refused(_chunk_backward(name, _chunk(), row_base=-1), -1, f"{name}: partial gradient buffer has")
    _refused(_chunk_backward(name, _chunk(hq=24)), -4, f"{name}: N = 96 gives LayerNorm rows of 48 and 96 in the decoder")
    _refused(_chunk_backward(name, _chunk(hq=8)), -4, f"{name}: hq = 8, ca = 4, cs = 16: geometry not supported")


SPAN_REFUSALS = [("no span", dict(spans=[], nspans=0), "bad argument (1 to 4 chunks)"),
                 ("one span too many", dict(spans=[(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1), (4, 6, 1)]), "bad argument (1 to 4 chunks)"),
                 ("a gap between spans", dict(spans=[(0, 2, 2), (3, 6, 3)]), "chunk 1: spans must tile [0, K) in order"),
                 ("an overlap", dict(spans=[(0, 4, 2), (3, 6, 3)]), "chunk 1: spans must tile [0, K) in order"),
                 ("a first span that starts late", dict(spans=[(1, 3, 2), (3, 6, 3)]), "chunk 0: spans must tile [0, K) in order"),
                 ("s = 0", dict(spans=[(0, 3, 0), (3, 6, 3)]), "chunk 0: spans must tile [0, K) in order"),
                 ("s > k1 - k0", dict(spans=[(0, 3, 2), (3, 6, 4)]), "chunk 1: spans must tile [0, K) in order"),
                 ("an empty span", dict(spans=[(0, 3, 2), (3, 3, 1)]), "chunk 1: spans must tile [0, K) in order"),
                 ("spans covering [0, K - 1)", dict(spans=[(0, 3, 2), (3, 5, 2)]), "the chunks cover [0, 5), not [0, 6)")]


@needs_lib
@pytest.mark.parametrize("what,change,text", SPAN_REFUSALS, ids=[r[0] for r in SPAN_REFUSALS])
def test_chunks_backward_refuses_spans_that_do_not_tile_the_time_axis(what, change, text):
    change = dict(change, spans=[_span(*s) for s in change["spans"]])
    _refused(_chunk_backward("sur_chunks_backward", _chunk(), **change), -1, f"sur_chunks_backward: {text}")
