"""ctypes binding of libreplay_hip.so (C ABI: include/replay_hip.h ``rp_*``; kernel: csrc/replay.hip): the fused batch
gather of the policy-update phase, and the append and episode returns of the device-resident replay
(pdecontrol/mbrl/device_replay.py).  ``rp_supported`` and ``rp_last_error`` are pure host functions and work without a GPU.
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


Slab = hipbind.Slabs     # ``rp_slab`` of include/replay_hip.h

_src = ctypes.POINTER(Source)
SYMBOLS = (
    ("rp_supported", _i, [_i, _src, _i]),
    ("rp_gather", _i, [_p, _i, _src, _i, _p, _p, _p, _p, _p, _p]),
    ("rp_append", _i, [_p, _p, _i, _i, _i, _i, _i, _p, _p, ctypes.POINTER(Slab)]),
    ("rp_episode_returns", _i, [_p, _p, _l, _p, _l, _p, _i, _p]),
    ("rp_last_error", ctypes.c_char_p, []),
)
# the ``rpd_*`` half of the library (the delta statistics, pdecontrol/mbrl/delta_phase.py): a table of its own, as the
# ``fno_*`` half of libspectral_hip has; its refusals are read through ``rp_last_error`` too
DELTA_SYMBOLS = (
    ("rpd_moments", _i, [_p, _p, _p, _l, _i, _i, _i, _p, _p, _l, ctypes.c_float, _i, _p, _p, _p]),
    ("rpd_workspace_doubles", _l, [_i, _l, _i]),
)
MAX_DELTA_GROUPS = 2048
DELTA_LAUNCH_FAILURE = -80
# the ``rpn_*`` entries (include/replay/fit.h: the scaling fits of the offline evaluation,
# pdecontrol/surrogates/evaluation/evaluate.py), a third table; refusals through ``rp_last_error`` as well
FIT_SYMBOLS = (
    ("rpn_moments", _i, [_p, _p, _p, _l, _i, _i, _p, _p, _l, _i, _p, _p, _p]),
    ("rpn_workspace_doubles", _l, [_i, _i, _i, _l, _i]),
)
FIT_LAUNCH_FAILURE = -100
_lib = None


class ReplayHipError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is None:
        _lib = hipbind.open_library(LIB_PATH, SYMBOLS + DELTA_SYMBOLS + FIT_SYMBOLS, ReplayHipError, "The fused batch gather has no fallback.")
    return _lib


def last_error():
    return load().rp_last_error().decode(errors="replace")


_check = hipbind.checker(ReplayHipError, "libreplay_hip", "rp_last_error", lambda: load())


def sources(entries):
    """A host array of ``rp_source`` from Source objects."""
    return (Source * len(entries))(*entries)


def supported(srcs, B):
    """None when ``rp_gather`` runs these sources at batch size ``B``, else the refusal's message."""
    return None if load().rp_supported(len(srcs), srcs, int(B)) == 0 else last_error()


def gather(stream, srcs, B, rows_ptr, obs, actions, nxtobs, rewards, terminated):
    """One launch on ``stream`` (a raw hipStream_t): ``rows_ptr`` is the device address of B int64 rows, the outputs are
    fp32 device tensors [B, obs_dim], [B, act_dim], [B, obs_dim], [B], [B]."""
    _check(load().rp_gather(stream, len(srcs), srcs, int(B), rows_ptr, obs.data_ptr(), actions.data_ptr(), nxtobs.data_ptr(),
                            rewards.data_ptr(), terminated.data_ptr()))


def slab(tensors):
    """``rp_slab`` of the seven slab tensors (``DeviceSubSeqStore.tensors`` order)."""
    obs, actions, nxtobs, rewards, terminated, truncated, steps = tensors
    return Slab(obs.data_ptr(), actions.data_ptr(), nxtobs.data_ptr(), rewards.data_ptr(), terminated.data_ptr(),
                truncated.data_ptr(), steps.data_ptr(), int(obs.shape[0]))


def append(stream, block_ptr, T, T_cap, B, N, A, dst_ptr, dst_host, slab_struct):
    """One ``rp_append`` launch on ``stream``: the first ``T`` steps of the round block at device address ``block_ptr``
    go to the rows ``dst_ptr`` (device int64 [T][B]) names; ``dst_host`` is the contiguous int64 numpy array it was
    uploaded from, validated against the slab before the launch."""
    assert dst_host.dtype.kind == "i" and dst_host.dtype.itemsize == 8 and dst_host.flags.c_contiguous and dst_host.size == T * B
    _check(load().rp_append(stream, block_ptr, int(T), int(T_cap), int(B), int(N), int(A), dst_ptr, dst_host.ctypes.data,
                            ctypes.byref(slab_struct)))


def delta_workspace_doubles(obs_dim, n, groups=0):
    """fp64 elements of the workspace ``delta_moments`` needs; 0 where it would refuse the arguments."""
    return int(load().rpd_workspace_doubles(int(obs_dim), int(n), int(groups)))


def delta_moments(stream, obs, nxtobs, start, stride, coef, rows, n, delta, groups, workspace, sums, stats):
    """``rpd_moments`` on ``stream``, two or three launches: ``obs`` and ``nxtobs`` are contiguous fp32 device tensors
    [slab rows, (1,) obs_width], ``coef`` fp32 [4, obs_dim] or None, ``rows`` int64 [n] or None (rows 0 ... n - 1);
    ``workspace`` fp64 of ``delta_workspace_doubles`` elements, ``sums`` fp64 and ``stats`` fp32 [2, obs_dim + 1].
    A refusal raises ``ReplayHipError`` with the status as its ``code``; nothing was enqueued then unless the code is
    ``DELTA_LAUNCH_FAILURE``."""
    rc = load().rpd_moments(stream, obs.data_ptr(), nxtobs.data_ptr(), int(obs.shape[0]), int(obs.shape[-1]), int(start),
                                 int(stride), hipbind.ptr(coef), hipbind.ptr(rows), int(n), float(delta), int(groups),
                                 workspace.data_ptr(), sums.data_ptr(), stats.data_ptr())
    if rc != 0:
        error = ReplayHipError(f"libreplay_hip error {rc}: {last_error()}")
        error.code = rc
        raise error


def fit_layout(N, A, forced):
    """(offsets of the three fields, ld) of ``rpn_moments``' outputs: each field's columns, then its total."""
    N, A = int(N), int(A)
    return (0, N + 1, N + A + 2), (2 * N + A + 3 if forced else N + A + 2)


def fit_workspace_doubles(N, A, forced, n, groups=0):
    """fp64 elements of the workspace ``fit_moments`` needs; 0 where it would refuse the arguments."""
    return int(load().rpn_workspace_doubles(int(N), int(A), int(bool(forced)), int(n), int(groups)))


def fit_moments(stream, obs, actions, forcing, rows, n, groups, workspace, sums, stats):
    """``rpn_moments`` on ``stream``, two or three launches: ``obs`` and ``actions`` are contiguous fp32 device tensors
    [slab rows, (1,) N] and [slab rows, (1,) A], ``forcing`` fp32 [A, N] or None, ``rows`` int64 [n] or None (rows
    0 ... n - 1); ``workspace`` fp64 of ``fit_workspace_doubles`` elements, ``sums`` fp64 and ``stats`` fp32 [2, ld] of
    ``fit_layout``.  A refusal raises ``ReplayHipError`` with the status as its ``code``; nothing was enqueued then unless
    the code is ``FIT_LAUNCH_FAILURE``."""
    rc = load().rpn_moments(stream, obs.data_ptr(), actions.data_ptr(), int(obs.shape[0]), int(obs.shape[-1]),
                            int(actions.shape[-1]), hipbind.ptr(forcing), hipbind.ptr(rows), int(n), int(groups),
                            workspace.data_ptr(), sums.data_ptr(), stats.data_ptr())
    if rc != 0:
        error = ReplayHipError(f"libreplay_hip error {rc}: {last_error()}")
        error.code = rc
        raise error


def episode_returns(stream, rewards, rows, offsets, returns):
    """One ``rp_episode_returns`` launch on ``stream``: ``rewards`` the slab's fp32 [slab rows], ``rows`` int64 [n] and
    ``offsets`` int64 [E + 1] device tensors, ``returns`` fp32 [E]."""
    _check(load().rp_episode_returns(stream, rewards.data_ptr(), int(rewards.numel()), rows.data_ptr(), int(rows.numel()),
                                     offsets.data_ptr(), int(offsets.numel()) - 1, returns.data_ptr()))
