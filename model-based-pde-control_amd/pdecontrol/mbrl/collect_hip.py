"""ctypes binding of libcollect_hip.so (C ABI: include/collect_hip.h ``co_*``; kernels: csrc/collect.hip): the
action side and the observation side of the device-resident collection step.  ``co_supported``, ``co_workspace_floats``
and ``co_last_error`` are pure host functions and work without a GPU.  A missing library raises: the kernel tier of
pdecontrol/mbrl/collection_phase.py has no silent fallback.
"""
import ctypes
import os

import hipbind

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.abspath(os.path.join(_HERE, "..", "..", "lib", "libcollect_hip.so"))

MIN_STATE_DIM, MAX_STATE_DIM, MAX_ACT_DIM = 16, 1024, 16
SPAN_MAX_PARTS = 1024            # CO_SPAN_MAX_PARTS of include/collect/span.h
_p, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


class Geometry(ctypes.Structure):
    """``co_geometry`` of include/collect_hip.h"""
    _fields_ = [("E", _i), ("T", _i), ("N", _i), ("A", _i), ("obs_start", _i), ("obs_stride", _i)]


class ActArgs(ctypes.Structure):
    """``co_act_args``"""
    _fields_ = [("action", _p), ("coef", _p), ("env_action", _p), ("actions", _p), ("record_raw", _i)]


class ObserveArgs(ctypes.Structure):
    """``co_observe_args``"""
    _fields_ = [("traj", _p), ("policy_obs", _p), ("bounds", _p), ("lower", _f), ("upper", _f), ("update", _i),
                ("workspace", _p)]


class ActSpanArgs(ctypes.Structure):
    """``co_act_span_args`` of include/collect/span.h"""
    _fields_ = [("table", _p), ("coef", _p), ("env_actions", _p), ("actions", _p), ("record_raw", _i)]


_geo = ctypes.POINTER(Geometry)
SYMBOLS = (
    ("co_supported", _i, [_geo]),
    ("co_workspace_floats", ctypes.c_long, [_geo]),
    ("co_act", _i, [_p, _geo, ctypes.POINTER(ActArgs), _i]),
    ("co_observe", _i, [_p, _geo, ctypes.POINTER(ObserveArgs), _i]),
    ("co_last_error", ctypes.c_char_p, []),
)
# include/collect/span.h, the same library (tests/test_collect_span_host.py holds that header, this table and the library
# to each other as tests/test_capi_symbols.py does for SYMBOLS)
SPAN_SYMBOLS = (
    ("co_span_workspace_floats", ctypes.c_long, [_geo]),
    ("co_act_span", _i, [_p, _geo, ctypes.POINTER(ActSpanArgs)]),
    ("co_observe_span", _i, [_p, _geo, ctypes.POINTER(ObserveArgs)]),
)
_lib = None


class CollectHipError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is None:
        _lib = hipbind.open_library(LIB_PATH, SYMBOLS + SPAN_SYMBOLS, CollectHipError, "The device-resident collection step has no fallback.")
    return _lib


def last_error():
    return load().co_last_error().decode(errors="replace")


_check = hipbind.checker(CollectHipError, "libcollect_hip", "co_last_error", lambda: load())
stream = hipbind.stream          # raw handle of torch's current stream (after ``load()``)


def supported(geometry):
    """None when the kernels run ``geometry``, else the refusal's message."""
    return None if load().co_supported(ctypes.byref(geometry)) == 0 else last_error()


def workspace_floats(geometry):
    """Floats of scratch ``observe`` needs with ``update = 1``; raises for a geometry ``supported`` refuses."""
    n = load().co_workspace_floats(ctypes.byref(geometry))
    if n < 0:
        raise CollectHipError(f"libcollect_hip error {n}: {last_error()}")
    return int(n)


def _ptr(t):
    return None if t is None else t.data_ptr()


def act_args(action, coef, env_action, actions, record_raw=False):
    """``co_act_args`` from device tensors (``coef`` may be None)."""
    return ActArgs(_ptr(action), _ptr(coef), _ptr(env_action), _ptr(actions), int(bool(record_raw)))


def observe_args(traj, policy_obs, bounds=None, lower=-1.0, upper=1.0, update=False, workspace=None):
    """``co_observe_args`` from device tensors (``bounds`` None: no scaling; ``workspace`` needed with ``update``)."""
    return ObserveArgs(_ptr(traj), _ptr(policy_obs), _ptr(bounds), float(lower), float(upper), int(bool(update)),
                       _ptr(workspace))


def act(stream, geometry, args, t):
    """One launch on ``stream`` (a raw hipStream_t)."""
    _check(load().co_act(stream, ctypes.byref(geometry), ctypes.byref(args), int(t)))


def observe(stream, geometry, args, t):
    """Two launches with an updating scaling, else one."""
    _check(load().co_observe(stream, ctypes.byref(geometry), ctypes.byref(args), int(t)))


def span_workspace_floats(geometry):
    """Floats of scratch ``observe_span`` needs with ``update = 1``; raises for a geometry ``supported`` refuses."""
    n = load().co_span_workspace_floats(ctypes.byref(geometry))
    if n < 0:
        raise CollectHipError(f"libcollect_hip error {n}: {last_error()}")
    return int(n)


def act_span_args(table, coef, env_actions, actions, record_raw=False):
    """``co_act_span_args`` from device tensors of ``[T, E, A]`` (``coef`` may be None)."""
    return ActSpanArgs(_ptr(table), _ptr(coef), _ptr(env_actions), _ptr(actions), int(bool(record_raw)))


def act_span(stream, geometry, args):
    """One launch for all ``geometry.T`` steps of a segment."""
    _check(load().co_act_span(stream, ctypes.byref(geometry), ctypes.byref(args)))


def observe_span(stream, geometry, args):
    """The observation side of a whole segment (``args``: ``observe_args``; reads bounds cell 0, writes cell 1): two
    launches with an updating scaling, else one."""
    _check(load().co_observe_span(stream, ctypes.byref(geometry), ctypes.byref(args)))
