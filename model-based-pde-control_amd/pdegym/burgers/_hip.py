"""ctypes binding of libburgers_hip.so (C ABI: include/burgers_hip.h, include/burgers/eval.h for the test-phase
entries and include/burgers/objective.h for the objective entries).  No fallback: a missing library raises."""
import ctypes
import os

import hipbind

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.abspath(os.path.join(_HERE, "..", "..", "lib", "libburgers_hip.so"))

_p, _i, _f, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double
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


class EvalBatch(ctypes.Structure):
    """``bg_eval_batch`` of include/burgers/eval.h: truth and prediction rows through element strides, the inverse
    observation map and the optional inverse-scaled outputs of ``bg_eval_rows``."""
    _fields_ = [("truth", _p), ("truth_bstride", ctypes.c_long), ("truth_tstride", ctypes.c_long),
                ("pred", _p), ("pred_bstride", ctypes.c_long), ("pred_tstride", ctypes.c_long),
                ("pred_shift", _i), ("inv_kind", _i), ("inv_coef", _p), ("truth_out", _p), ("pred_out", _p)]


EVAL_ROW_STATS = 14      # BG_EVAL_ROW_STATS
EVAL_TABLES = 20         # BG_EVAL_TABLES
# the names of the per-step tables of bg_eval_fold, in its order: the keys of the dict test_step returns on a Burgers env
EVAL_TABLE_NAMES = (("l1_loss", "l2_loss", "l1_loss_scaled", "l2_loss_scaled", "nrmse")
                    + ("l1_loss_rews", "l2_loss_rews", "l1_loss_scaled_rews", "l2_loss_scaled_rews", "nrmse_rews")
                    + tuple(f"{name}-derivative-{d}" for name in ("l1_loss_derivs", "l2_loss_derivs", "l1_loss_scaled_derivs",
                                                                  "l2_loss_scaled_derivs", "nrms_derivs") for d in range(2)))

# include/burgers/eval.h: a second table over the same library (burgers_hip.h's list is pinned to SYMBOLS)
EVAL_SYMBOLS = (
    ("bg_eval_rows", _i, [_p, ctypes.POINTER(EvalBatch), _i, _i, _i, _d, _p]),
    ("bg_eval_fold", _i, [_p, _p, _i, _i, _i, _p, _p]),
    ("bg_derivatives", _i, [_p, _p, _i, _i, _d, _p, _p]),
    ("bg_eval_rows_host", _i, [ctypes.POINTER(EvalBatch), _i, _i, _i, _d, _p]),
    ("bg_eval_fold_host", _i, [_p, _i, _i, _i, _p, _p]),
    ("bg_derivatives_host", _i, [_p, _i, _i, _d, _p, _p]),
    ("bg_eval_last_error", ctypes.c_char_p, []),
)
# include/burgers/objective.h: a third table over the same library; the *_host entries make no HIP call
OBJECTIVES = {"l2control": 0, "dissipation": 1}      # BG_OBJECTIVE_*
OBJECTIVE_SYMBOLS = (
    ("bg_step_objective", _i, [_p, _p, _p, _p, _i, _i, _i, _f, _f, _f, ctypes.c_long, _p, _p, _p, _i]),
    ("bg_step_span_objective", _i, [_p, _p, _p, _p, _i, _i, _i, _i, _f, _f, _f, ctypes.c_long, _p, _p, _p, _i]),
    ("bg_reward_rows", _i, [_p, _p, _p, _p, _p, _i, _i, _i, _d, _d, _p]),
    ("bg_step_objective_host", _i, [_p, _p, _p, _i, _i, _i, _f, _f, _f, ctypes.c_long, _p, _p, _p, _i]),
    ("bg_reward_rows_host", _i, [_p, _p, _p, _p, _i, _i, _i, _d, _d, _p]),
    ("bg_objective_last_error", ctypes.c_char_p, []),
)
_lib = None


class BurgersHipError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is None:
        _lib = hipbind.open_library(LIB_PATH, SYMBOLS + EVAL_SYMBOLS + OBJECTIVE_SYMBOLS, BurgersHipError,
                                    "The Burgers stepper has no CPU fallback.")
    return _lib


check = hipbind.checker(BurgersHipError, "libburgers_hip", "bg_last_error", lambda: load())
# the test-phase entries report through a message buffer of their own
check_eval = hipbind.checker(BurgersHipError, "libburgers_hip (eval)", "bg_eval_last_error", lambda: load())
# and so do the objective entries
check_objective = hipbind.checker(BurgersHipError, "libburgers_hip (objective)", "bg_objective_last_error", lambda: load())
