"""``fno_forward_select`` without a GPU: include/spectral/forward_select.h, the binding's ``SELECT_SYMBOLS`` and the built
library name the same functions, ``spectral_hip.h`` keeps its own list, and every refusal of the entry point is made on the
host before any HIP call (the device pointers of these calls are never read)."""
import ctypes
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_capi_symbols import LIBDIR, ROOT, declared_functions  # noqa: E402

from pdecontrol.surrogates import fno_hip  # noqa: E402

HEADER = os.path.join("spectral", "forward_select.h")
LIB = os.path.join(LIBDIR, "libspectral_hip.so")


def test_the_select_header_its_table_and_the_library_agree():
    declared = declared_functions(HEADER, "fno")
    assert declared == ["fno_forward_select"] == sorted(name for name, _, _ in fno_hip.SELECT_SYMBOLS)
    # the pinned header and its table keep their own list
    assert not set(declared) & set(declared_functions("spectral_hip.h", "fno|spec"))
    assert not set(declared) & {name for name, _, _ in fno_hip.SYMBOLS}
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "../spectral_hip.h"' in text
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    assert re.findall(r"typedef struct (\w+)", text) == ["fno_select_args"]
    fields = re.search(r"typedef struct fno_select_args \{(.*?)\}", text, flags=re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [name for name, _ in fno_hip.FnoSelectArgs._fields_]
    assert int(re.search(r"#define FNO_MAX_MEMBERS (\d+)", text).group(1)) == fno_hip.MAX_MEMBERS == 8
    assert os.path.exists(LIB), "libspectral_hip.so not built (run __graft_entry__.build())"
    lib = fno_hip.load()
    for name, restype, argtypes in fno_hip.SYMBOLS + fno_hip.SELECT_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


FAKE = 4096        # stands in for every device pointer: a refusal that read it would fault


def _weights(members, hole=None):
    """A host array of ``members`` structs with every pointer set; ``hole`` = (member, field, layer or None) is NULL."""
    ws = (fno_hip.FnoWeights * max(members, 1))()
    for m in range(max(members, 1)):
        for name, ctype in fno_hip.FnoWeights._fields_:
            if ctype is ctypes.c_void_p:
                setattr(ws[m], name, FAKE)
            else:
                for layer in range(4):
                    getattr(ws[m], name)[layer] = FAKE
    if hole is not None:
        m, name, layer = hole
        if layer is None:
            setattr(ws[m], name, None)
        else:
            getattr(ws[m], name)[layer] = None
    return ws


def _call(lib, geometry=None, null_args=False, **change):
    g = dict(width=32, modes=16, layers=4, n=64, nb=5)
    g.update(geometry or {})
    members = change.get("members", 3)
    fields = dict(w=_weights(members, change.pop("hole", None)), cscale=(ctypes.c_float * 8)(), cshift=(ctypes.c_float * 8)(),
                  members=members, chosen=FAKE, step=FAKE, T=3, u=FAKE, act=FAKE, out=2 * FAKE)
    fields.update(change)
    a = fno_hip.FnoSelectArgs(**fields)
    rc = lib.fno_forward_select(None, g["width"], g["modes"], g["layers"], g["n"], g["nb"], None if null_args else ctypes.byref(a))
    return rc, lib.fno_last_error().decode()


def test_fno_forward_select_refuses_on_the_host():
    if not os.path.exists(LIB):
        pytest.skip("libspectral_hip.so not built (run __graft_entry__.build())")
    lib = fno_hip.load()
    cases = {
        "NULL a": (-1, dict(null_args=True)), "NULL w": (-1, dict(w=None)), "NULL cscale": (-1, dict(cscale=None)),
        "NULL cshift": (-1, dict(cshift=None)), "NULL u": (-1, dict(u=None)), "NULL act": (-1, dict(act=None)),
        "NULL out": (-1, dict(out=None)),
        "incomplete first": (-1, dict(hole=(0, "lift_w", None))), "incomplete last": (-1, dict(hole=(2, "spec_wi", 3))),
        "incomplete middle": (-1, dict(hole=(1, "p2_b", None))),
        "no member": (-1, dict(members=0)), "nine members": (-1, dict(members=9)),
        "members without chosen": (-1, dict(chosen=None)),
        "T = 0": (-1, dict(T=0)), "aliased": (-1, dict(out=FAKE)),
        "width": (-4, dict(geometry=dict(width=16))), "modes": (-4, dict(geometry=dict(modes=8))),
        "layers": (-4, dict(geometry=dict(layers=2))), "n = 32": (-4, dict(geometry=dict(n=32))),
        "n = 1024": (-4, dict(geometry=dict(n=1024))), "n = 96": (-4, dict(geometry=dict(n=96))),
        "no env": (-1, dict(geometry=dict(nb=0))),
    }
    texts = {}
    for what, (code, kwargs) in cases.items():
        rc, message = _call(lib, **kwargs)
        assert rc == code, (what, rc, message)
        assert message.startswith("fno_forward_select:"), (what, message)
        texts[what] = message
    # a hole beyond the first `members` structs is not looked at: members = 2 with member 2 incomplete passes this check
    # and is refused for the next reason in the list
    rc, message = _call(lib, members=2, w=_weights(3, (2, "lift_w", None)), T=0)
    assert rc == -1 and message == texts["T = 0"]
    assert "member 2" in texts["incomplete last"] and "member 0" in texts["incomplete first"]
    assert "9" in texts["nine members"] and "chosen" in texts["members without chosen"] and "alias" in texts["aliased"]
    distinct = ("NULL a", "incomplete first", "no member", "members without chosen", "T = 0", "aliased", "width", "n = 32", "no env")
    assert len({texts[k] for k in distinct}) == len(distinct)
    # the binding raises with the same text
    a = fno_hip.FnoSelectArgs(w=_weights(1), cscale=(ctypes.c_float * 1)(), cshift=(ctypes.c_float * 1)(), members=1, T=1,
                              u=FAKE, act=FAKE, out=FAKE)
    with pytest.raises(fno_hip.FnoHipError, match="must not alias"):
        fno_hip.forward_select(None, 64, 5, a)


def test_world_supported_names_the_fno_family():
    """An FNO surrogate of the kernels' geometry with an affine ``dscaling``, at a width the kernels take."""
    import torch
    from pdecontrol.architectures.fno import BurgersFNO
    f = BurgersFNO()
    sur = f.surrogate(delta=0.05, dscaling=None, **f.model())
    assert fno_hip.world_supported(sur, 64) and fno_hip.world_supported(sur, 512)
    assert not fno_hip.world_supported(sur, 96) and not fno_hip.world_supported(sur, 1024)
    assert not fno_hip.world_supported(f.surrogate(delta=0.05, dscaling=None, **f.model(width=16)), 64)
    assert not fno_hip.world_supported(torch.nn.Linear(2, 2), 64)
    sur.dscaling = torch.tanh                      # not an affine map
    assert not fno_hip.world_supported(sur, 64)
