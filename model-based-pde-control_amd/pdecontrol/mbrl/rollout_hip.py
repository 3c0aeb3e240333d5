"""ctypes binding of librollout_hip.so (C ABI: include/rollout_hip.h ``ro_*`` and, for the dissipation objective,
include/rollout/settle_dissipation.h and include/rollout/settle_burgers_dissipation.h; kernels: csrc/rollout.hip): the action chain and the settle kernels (one per reward
objective) of the captured imagined step.  ``ro_supported`` and ``ro_last_error`` are pure host functions and work
without a GPU.  A missing library raises: the kernel tier of pdecontrol/mbrl/imagination_phase.py has
no silent fallback.
"""
import ctypes
import os

import hipbind

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.abspath(os.path.join(_HERE, "..", "..", "lib", "librollout_hip.so"))

MAX_MEMBERS, MIN_STATE_DIM, MAX_STATE_DIM, MAX_ACT_DIM = 8, 16, 1024, 16
_p, _i = ctypes.c_void_p, ctypes.c_int


class Geometry(ctypes.Structure):
    """``ro_geometry`` of include/rollout_hip.h"""
    _fields_ = [("B", _i), ("T", _i), ("N", _i), ("A", _i), ("L", _i), ("act_start", _i), ("act_stride", _i),
                ("obs_start", _i), ("obs_stride", _i), ("members", _i)]


class ActArgs(ctypes.Structure):
    """``ro_act_args``"""
    _fields_ = [("action", _p), ("actions", _p), ("in_coef", _p), ("forcing", _p), ("out_coef", _p), ("world_action", _p),
                ("step", _p)]


class SettleArgs(ctypes.Structure):
    """``ro_settle_args``"""
    _fields_ = [("member", _p * MAX_MEMBERS), ("chosen", _p), ("state", _p), ("traj", _p), ("policy_obs", _p), ("steps0", _p),
                ("steps", _p), ("rewards", _p), ("reward_coef", _p), ("step", _p)]


class DissipationArgs(ctypes.Structure):
    """``ro_dissipation_args`` of include/rollout/settle_dissipation.h"""
    _fields_ = [("actions", _p), ("in_coef", _p), ("forcing", _p), ("dx", ctypes.c_double)]


class BurgersDissipationArgs(ctypes.Structure):
    """``ro_burgers_dissipation_args`` of include/rollout/settle_burgers_dissipation.h"""
    _fields_ = [("d", DissipationArgs), ("nu", ctypes.c_double)]


_geo = ctypes.POINTER(Geometry)
SYMBOLS = (
    ("ro_supported", _i, [_geo]),
    ("ro_act_chain", _i, [_p, _geo, ctypes.POINTER(ActArgs)]),
    ("ro_settle", _i, [_p, _geo, ctypes.POINTER(SettleArgs)]),
    ("ro_last_error", ctypes.c_char_p, []),
)
# include/rollout/settle_dissipation.h, the same library (tests/test_imagination_dissipation_host.py holds that header,
# this table and the library to each other as tests/test_capi_symbols.py does for SYMBOLS)
DISSIPATION_SYMBOLS = (
    ("ro_settle_dissipation", _i, [_p, _geo, ctypes.POINTER(SettleArgs), ctypes.POINTER(DissipationArgs)]),
)
# include/rollout/settle_burgers_dissipation.h, the same library again (tests/test_burgers_objective_host.py)
BURGERS_DISSIPATION_SYMBOLS = (
    ("ro_settle_burgers_dissipation", _i, [_p, _geo, ctypes.POINTER(SettleArgs), ctypes.POINTER(BurgersDissipationArgs)]),
)
_lib = None


class RolloutHipError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is None:
        _lib = hipbind.open_library(LIB_PATH, SYMBOLS + DISSIPATION_SYMBOLS + BURGERS_DISSIPATION_SYMBOLS, RolloutHipError, "The fused imagined-rollout step has no fallback.")
    return _lib


def last_error():
    return load().ro_last_error().decode(errors="replace")


_check = hipbind.checker(RolloutHipError, "librollout_hip", "ro_last_error", lambda: load())
stream = hipbind.stream          # raw handle of torch's current stream (after ``load()``)


def supported(geometry):
    """None when both kernels run ``geometry``, else the refusal's message."""
    return None if load().ro_supported(ctypes.byref(geometry)) == 0 else last_error()


def act_args(action, actions, in_coef, forcing, out_coef, world_action, step):
    """``ro_act_args`` from device tensors (``in_coef`` / ``out_coef`` may be None)."""
    return ActArgs(*(None if t is None else t.data_ptr() for t in (action, actions, in_coef, forcing, out_coef, world_action,
                                                                   step)))


def settle_args(members, chosen, state, traj, policy_obs, steps0, steps, rewards, reward_coef, step):
    """``ro_settle_args`` from device tensors (``chosen`` may be None with one member, ``reward_coef`` may be None)."""
    assert 1 <= len(members) <= MAX_MEMBERS
    a = SettleArgs()
    for m, t in enumerate(members):
        a.member[m] = t.data_ptr()
    for name, t in (("chosen", chosen), ("state", state), ("traj", traj), ("policy_obs", policy_obs), ("steps0", steps0),
                    ("steps", steps), ("rewards", rewards), ("reward_coef", reward_coef), ("step", step)):
        setattr(a, name, None if t is None else t.data_ptr())
    return a


def dissipation_args(actions, in_coef, forcing, dx):
    """``ro_dissipation_args`` from device tensors: the raw-action record ``ro_act_chain`` writes, its ``in_coef`` (may be
    None) and its forcing, which must span the whole state row; ``dx`` is the grid spacing."""
    return DissipationArgs(actions.data_ptr(), None if in_coef is None else in_coef.data_ptr(), forcing.data_ptr(), float(dx))


def act_chain(stream, geometry, args):
    """One launch on ``stream`` (a raw hipStream_t)."""
    _check(load().ro_act_chain(stream, ctypes.byref(geometry), ctypes.byref(args)))


def settle(stream, geometry, args):
    _check(load().ro_settle(stream, ctypes.byref(geometry), ctypes.byref(args)))


def settle_dissipation(stream, geometry, args, dissipation):
    """``settle`` with the dissipation reward (``dissipation``: ``dissipation_args``)."""
    _check(load().ro_settle_dissipation(stream, ctypes.byref(geometry), ctypes.byref(args), ctypes.byref(dissipation)))


def burgers_dissipation_args(actions, in_coef, forcing, dx, nu):
    """``ro_burgers_dissipation_args``: ``dissipation_args`` and the viscosity."""
    return BurgersDissipationArgs(dissipation_args(actions, in_coef, forcing, dx), float(nu))


def settle_burgers_dissipation(stream, geometry, args, dissipation):
    """``settle`` with the Burgers env's dissipation reward (``dissipation``: ``burgers_dissipation_args``)."""
    _check(load().ro_settle_burgers_dissipation(stream, ctypes.byref(geometry), ctypes.byref(args), ctypes.byref(dissipation)))
