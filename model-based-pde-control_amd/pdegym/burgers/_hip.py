"""ctypes binding of libburgers_hip.so (C ABI: include/burgers_hip.h).  No fallback: a missing library raises."""
import ctypes
import os

import hipbind

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.abspath(os.path.join(_HERE, "..", "..", "lib", "libburgers_hip.so"))

_p, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
Slabs = hipbind.Slabs     # ``bg_slabs`` of include/burgers_hip.h

SYMBOLS = (
    ("bg_step", _i, [_p, _p, _p, _p, _i, _i, _i, _f, _f, _f, ctypes.c_long, _p, _p, _p]),
    ("bg_step_span", _i, [_p, _p, _p, _p, _i, _i, _i, _i, _f, _f, _f, ctypes.c_long, _p, _p, _p]),
    ("bg_record", _i, [_p, _p, _p, _i, _i, _i, _p, _p, _i, ctypes.c_long, _p, _p, ctypes.POINTER(Slabs)]),
    ("bg_residual", _i, [_p, _p, _p, _i, _i, _f, _f, _p]),
    ("bg_phyloss_forward", _i, [_p, _p, _i, _i, _i, _f, _f, _f, _i, _p, _p, _p, ctypes.c_long]),
    ("bg_phyloss_backward", _i, [_p, _p, _p, _p, _p, ctypes.c_long, _i, _i, _i, _f, _f, _f, _i, _p]),
    ("bg_last_error", ctypes.c_char_p, []),
)
_lib = None


class BurgersHipError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is None:
        _lib = hipbind.open_library(LIB_PATH, SYMBOLS, BurgersHipError, "The Burgers stepper has no CPU fallback.")
    return _lib


check = hipbind.checker(BurgersHipError, "libburgers_hip", "bg_last_error", lambda: load())
