"""ctypes binding of libreplay_hip.so (C ABI: include/replay_hip.h ``rp_*``; kernel: csrc/replay.hip): the fused batch
gather of the policy-update phase.  ``rp_supported`` and ``rp_last_error`` are pure host functions and work without a GPU.
A missing library raises: the kernel tier of pdecontrol/mbrl/policy_phase.py has no silent fallback.
"""
import ctypes
import os

import hipbind

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.abspath(os.path.join(_HERE, "..", "..", "lib", "libreplay_hip.so"))

MAX_SOURCES, MAX_OBS_DIM, MAX_ACT_DIM = 8, 1024, 16
_p, _i, _l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long


class Source(ctypes.Structure):
    """``rp_source`` of include/replay_hip.h"""
    _fields_ = [("obs", _p), ("actions", _p), ("nxtobs", _p), ("rewards", _p), ("terminated", _p), ("rows", _l),
                ("obs_width", _i), ("act_width", _i), ("sensor_start", _i), ("sensor_stride", _i),
                ("obs_coef", _p), ("act_coef", _p)]


_src = ctypes.POINTER(Source)
SYMBOLS = (
    ("rp_supported", _i, [_i, _src, _i]),
    ("rp_gather", _i, [_p, _i, _src, _i, _p, _p, _p, _p, _p, _p]),
    ("rp_last_error", ctypes.c_char_p, []),
)
_lib = None


class ReplayHipError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is None:
        _lib = hipbind.open_library(LIB_PATH, SYMBOLS, ReplayHipError, "The fused batch gather has no fallback.")
    return _lib


def last_error():
    return load().rp_last_error().decode(errors="replace")


def sources(entries):
    """A host array of ``rp_source`` from Source objects."""
    return (Source * len(entries))(*entries)


def supported(srcs, B):
    """None when ``rp_gather`` runs these sources at batch size ``B``, else the refusal's message."""
    return None if load().rp_supported(len(srcs), srcs, int(B)) == 0 else last_error()


def gather(stream, srcs, B, rows_ptr, obs, actions, nxtobs, rewards, terminated):
    """One launch on ``stream`` (a raw hipStream_t): ``rows_ptr`` is the device address of B int64 rows, the outputs are
    fp32 device tensors [B, obs_dim], [B, act_dim], [B, obs_dim], [B], [B]."""
    rc = load().rp_gather(stream, len(srcs), srcs, int(B), rows_ptr, obs.data_ptr(), actions.data_ptr(), nxtobs.data_ptr(),
                          rewards.data_ptr(), terminated.data_ptr())
    if rc != 0:
        raise ReplayHipError(f"libreplay_hip error {rc}: {last_error()}")
