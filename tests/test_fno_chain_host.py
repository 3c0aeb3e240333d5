"""``fno_forward_chain`` and the FNO family of the surrogate-update phase without a GPU: include/spectral/forward_chain.h,
the binding's ``CHAIN_SYMBOLS`` and the built library name the same function and the same arguments, every refusal of the
entry point is made on the host before any HIP call (the device pointers of these calls are never read), the kernel tier's
reasons for refusing an FNO, and the controller's default factories refusing the Burgers id without ``cuda``."""
import ctypes
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_capi_symbols import LIBDIR, ROOT, declared_functions  # noqa: E402

from pdecontrol.surrogates import fno_hip  # noqa: E402

HEADER = os.path.join("spectral", "forward_chain.h")
LIB = os.path.join(LIBDIR, "libspectral_hip.so")
C_TYPES = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float}


def _ctype(decl):
    """The ctypes type of a C declarator's type: any pointer is a ``c_void_p`` (``fno_weights*`` its own pointer type)."""
    decl = decl.replace("const", "").strip()
    if "*" in decl:
        base = decl.replace("*", "").strip()
        return {"fno_weights": ctypes.POINTER(fno_hip.FnoWeights), "fno_chain_args": ctypes.POINTER(fno_hip.FnoChainArgs)}.get(
            base, ctypes.c_void_p)
    return C_TYPES[decl]


def test_the_chain_header_its_table_and_the_library_agree():
    declared = declared_functions(HEADER, "fno")
    assert declared == ["fno_forward_chain"] == sorted(name for name, _, _ in fno_hip.CHAIN_SYMBOLS)
    # the pinned header, the select header and their tables keep their own lists
    assert not set(declared) & set(declared_functions("spectral_hip.h", "fno|spec"))
    assert not set(declared) & set(declared_functions(os.path.join("spectral", "forward_select.h"), "fno"))
    assert not set(declared) & {name for name, _, _ in fno_hip.SYMBOLS + fno_hip.SELECT_SYMBOLS}
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "../spectral_hip.h"' in text
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    assert re.findall(r"typedef struct (\w+)", text) == ["fno_chain_args"]
    # the struct, field for field: name and type ("float cscale, cshift;" declares two)
    body = re.search(r"typedef struct fno_chain_args \{(.*?)\}", text, flags=re.S).group(1)
    fields = []
    for statement in filter(None, (s.strip() for s in body.split(";"))):
        kind, names = re.match(r"(.*?[\s*])(\w+(?:\s*,\s*\w+)*)$", statement, flags=re.S).groups()
        fields += [(name.strip(), _ctype(kind)) for name in names.split(",")]
    assert [name for name, _ in fields] == [name for name, _ in fno_hip.FnoChainArgs._fields_]
    for (name, want), (_, got) in zip(fields, fno_hip.FnoChainArgs._fields_):
        assert got is want or (want is ctypes.c_void_p and got is ctypes.c_void_p), (name, want, got)
    # the function, argument for argument
    proto = re.search(r"int fno_forward_chain\((.*?)\);", text, flags=re.S).group(1)
    args = [_ctype(re.match(r"(.*?[\s*])\w+$", a.strip(), flags=re.S).group(1)) for a in proto.split(",")]
    (name, restype, argtypes), = fno_hip.CHAIN_SYMBOLS
    assert restype is ctypes.c_int and [str(a) for a in argtypes] == [str(a) for a in args]
    assert os.path.exists(LIB), "libspectral_hip.so not built (run __graft_entry__.build())"
    lib = fno_hip.load()
    for name, restype, argtypes in fno_hip.SYMBOLS + fno_hip.SELECT_SYMBOLS + fno_hip.CHAIN_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


FAKE = 1 << 20     # stands in for every device pointer: a refusal that read it would fault
N, NB, STEPS = 64, 5, 3
WHOLE = 4 * STEPS * NB * N        # bytes of delta / out


def _weights(hole=None):
    w = fno_hip.FnoWeights()
    for name, ctype in fno_hip.FnoWeights._fields_:
        if ctype is ctypes.c_void_p:
            setattr(w, name, FAKE)
        else:
            for layer in range(4):
                getattr(w, name)[layer] = FAKE
    if hole is not None:
        name, layer = hole
        if layer is None:
            setattr(w, name, None)
        else:
            getattr(w, name)[layer] = None
    return w


def _call(lib, geometry=None, null_args=False, hole=None, **change):
    g = dict(width=32, modes=16, layers=4, n=N, nb=NB)
    g.update(geometry or {})
    w = _weights(hole)
    # four separate buffers, far apart: u0 [nb][n], act [steps][nb][n] time major, delta, out
    n = g["n"]
    fields = dict(w=ctypes.pointer(w), cscale=0.05, cshift=0.0, u0=FAKE, u0_stride_b=n, act=2 * FAKE, a_stride_t=NB * n, a_stride_b=n,
                  delta=3 * FAKE, out=4 * FAKE, steps=STEPS)
    fields.update(change)
    a = fno_hip.FnoChainArgs(**fields)
    rc = lib.fno_forward_chain(None, g["width"], g["modes"], g["layers"], g["n"], g["nb"], None if null_args else ctypes.byref(a))
    return rc, lib.fno_last_error().decode()


def test_fno_forward_chain_refuses_on_the_host():
    if not os.path.exists(LIB):
        pytest.skip("libspectral_hip.so not built (run __graft_entry__.build())")
    lib = fno_hip.load()
    row = 4 * N
    cases = {
        "NULL a": (-1, dict(null_args=True)), "NULL w": (-1, dict(w=None)), "NULL u0": (-1, dict(u0=None)),
        "NULL act": (-1, dict(act=None)), "NULL delta": (-1, dict(delta=None)), "NULL out": (-1, dict(out=None)),
        "incomplete lift": (-1, dict(hole=("lift_w", None))), "incomplete layer": (-1, dict(hole=("spec_wi", 3))),
        "incomplete project": (-1, dict(hole=("p2_b", None))),
        "steps = 0": (-1, dict(steps=0)), "steps < 0": (-1, dict(steps=-2)),
        "nb = 0": (-1, dict(geometry=dict(nb=0))), "nb < 0": (-1, dict(geometry=dict(nb=-1))),
        "u0 stride": (-1, dict(u0_stride_b=N - 1)), "act row stride": (-1, dict(a_stride_b=N - 1)),
        "act step stride": (-1, dict(a_stride_t=N - 1)), "negative stride": (-1, dict(a_stride_t=-NB * N)),
        # out or delta sharing bytes with u0, act or each other: the first byte, the last byte, the same buffer
        "out == u0": (-1, dict(out=FAKE)), "out ends inside u0": (-1, dict(out=FAKE - WHOLE + 4)),
        "out starts at u0's last float": (-1, dict(out=FAKE + NB * row - 4)),
        "out inside act": (-1, dict(out=2 * FAKE + row)), "delta == u0": (-1, dict(delta=FAKE)),
        "delta inside act": (-1, dict(delta=2 * FAKE + WHOLE - 4)), "delta == out": (-1, dict(delta=4 * FAKE)),
        "delta overlaps out": (-1, dict(delta=4 * FAKE + row)),
        "width": (-4, dict(geometry=dict(width=16))), "modes": (-4, dict(geometry=dict(modes=8))),
        "layers": (-4, dict(geometry=dict(layers=2))), "n = 32": (-4, dict(geometry=dict(n=32))),
        "n = 1024": (-4, dict(geometry=dict(n=1024))), "n = 96": (-4, dict(geometry=dict(n=96))),
    }
    texts = {}
    for what, (code, kwargs) in cases.items():
        rc, message = _call(lib, **kwargs)
        assert rc == code, (what, rc, message)
        assert message.startswith("fno_forward_chain:"), (what, message)
        texts[what] = message
    assert "weights" in texts["incomplete layer"] and "steps" in texts["steps = 0"] and "overlap" in texts["out == u0"]
    assert "stride" in texts["u0 stride"] and "batch" in texts["nb = 0"]
    distinct = ("NULL a", "incomplete lift", "steps = 0", "nb = 0", "u0 stride", "out == u0", "width", "n = 32")
    assert len({texts[k] for k in distinct}) == len(distinct)
    # the geometry refusals carry fno_forward's codes and, after the name, its text
    z = ctypes.c_void_p(FAKE)
    w = _weights()
    for what, g in (("width", dict(width=16)), ("n = 96", dict(n=96))):
        geo = dict(width=32, modes=16, layers=4, n=N)
        geo.update(g)
        rc = lib.fno_forward(None, ctypes.byref(w), geo["width"], geo["modes"], geo["layers"], geo["n"], NB, NB, z, 0, N, z, 0, N,
                             1.0, 0.0, z, z, None, None, 0, 0)
        assert rc == cases[what][0]
        assert lib.fno_last_error().decode().split(":", 1)[1] == texts[what].split(":", 1)[1]
    # the binding raises with the same text
    a = fno_hip.FnoChainArgs(w=ctypes.pointer(w), u0=FAKE, u0_stride_b=N, act=2 * FAKE, a_stride_t=NB * N, a_stride_b=N, delta=3 * FAKE,
                             out=4 * FAKE, steps=0)
    with pytest.raises(fno_hip.FnoHipError, match="0 steps"):
        fno_hip.forward_chain(None, N, NB, a)


def test_what_the_rollout_passes_is_not_a_refusal_by_overlap():
    """``_forward_launches`` hands over the last teacher-forced prediction as ``u0``: the row block just before ``out`` in
    the same buffer.  The geometry is checked last, so a call that gets past every other check with a width the kernels do
    not take is refused with -4 and no device is touched: adjacency passes, one shared float does not; strides of an axis
    that is not walked (one sample, one step) are not looked at."""
    if not os.path.exists(LIB):
        pytest.skip("libspectral_hip.so not built (run __graft_entry__.build())")
    lib = fno_hip.load()
    n, base = 32, 4 * FAKE
    small = dict(geometry=dict(n=n))
    rc, message = _call(lib, u0=base - 4 * NB * n, out=base, **small)
    assert rc == -4 and "power of two" in message, message
    rc, message = _call(lib, u0=base - 4 * NB * n + 4, out=base, **small)
    assert rc == -1 and "overlap" in message, message
    rc, message = _call(lib, **dict(small, geometry=dict(n=n, nb=1), u0_stride_b=0, a_stride_b=-7, a_stride_t=n))
    assert rc == -4, message
    rc, message = _call(lib, **dict(small, a_stride_t=0, steps=1))
    assert rc == -4, message


def test_chain_enabled_reads_the_switch(monkeypatch):
    """Off unless asked for: the measured gain is inside the spread of the rounds (profiles/fno_chain_bench.json)."""
    monkeypatch.delenv("PDECONTROL_FNO_CHAIN", raising=False)
    assert not fno_hip.chain_enabled()
    monkeypatch.setenv("PDECONTROL_FNO_CHAIN", "0")
    assert not fno_hip.chain_enabled()
    monkeypatch.setenv("PDECONTROL_FNO_CHAIN", "1")
    assert fno_hip.chain_enabled()


def test_the_kernel_tier_says_why_it_refuses_an_fno():
    import torch
    from pdecontrol.architectures.fno import BurgersFNO
    from pdecontrol.mbrl import surrogate_phase as sp
    f = BurgersFNO()
    sur = f.surrogate(delta=0.05, dscaling=None, **f.model())
    assert sp._fno_refusal(sur, 64, 64) is None and sp._fno_refusal(sur, 512, 512) is None
    narrow = sp._fno_refusal(sur, 64, 4)
    assert narrow == "an action row of 4 columns beside a state row of 64: the FNO reads the action field at every grid point"
    for other, n in ((f.surrogate(delta=0.05, dscaling=None, **f.model(width=16)), 64), (sur, 96), (sur, 1024)):
        reason = sp._fno_refusal(other, n, n)
        assert reason.startswith(f"an FNO the whole-network kernels do not take at a state row of {n} points"), reason
        assert reason != narrow
    sur.dscaling = torch.tanh                      # not an affine map
    assert "affine dscaling" in sp._fno_refusal(sur, 64, 64)


def test_the_default_factories_refuse_the_burgers_id_without_cuda(tmp_path):
    import _controller_scenario as cs
    from pdecontrol import architectures
    from pdecontrol.mbrl.mbrl import PDEModelBasedController, RunLog
    from pdegym import burgers
    args, config = cs.toy_args(cuda=False, env_id=burgers.ENV_ID), cs.toy_config()
    config.factory = "BurgersFNO"
    factory = architectures.BurgersFNO()
    with pytest.raises(ValueError, match=f"^{burgers.ENV_ID}: a controller without args.cuda is refused"):
        PDEModelBasedController(burgers.ENV_ID, factory, config, args, log=RunLog(str(tmp_path)), env_config=dict(N=64))
    # either factory on its own, by name
    bare = PDEModelBasedController.__new__(PDEModelBasedController)
    bare.env_id, bare.env_config = burgers.ENV_ID, dict(N=64)
    import torch
    bare.device = torch.device("cpu")
    for make in (bare._default_env, lambda: bare._default_envs(3)):
        with pytest.raises(ValueError, match="Burgers stepper runs on a GPU only"):
            make()
