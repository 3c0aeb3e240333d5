"""How the ``bg_eval_*`` tests call include/burgers/eval.h: one context per memory -- ``Mem("host")`` runs the ``*_host``
entries on numpy arrays, ``Mem("cuda")`` the launches on torch tensors of device 0 (torch's current stream) -- and the same
three calls on both."""
import ctypes

import numpy as np

import _bg_eval_oracle as mo
from pdegym.burgers import _hip


def batch_major(B, T, N):
    return (T * N, N)


def time_major(B, T, N):
    return (N, B * N)


class Mem:
    def __init__(self, where):
        assert where in ("host", "cuda")
        self.where, self.lib = where, _hip.load()
        if where == "cuda":
            import torch
            self.torch, self.device = torch, torch.device("cuda", 0)

    def up(self, a):
        a = np.array(a, order="C", copy=True)           # the shared cases are read-only
        return a if self.where == "host" else self.torch.from_numpy(a).to(self.device)

    def ptr(self, a):
        if a is None:
            return None
        return ctypes.c_void_p(a.ctypes.data if self.where == "host" else a.data_ptr())

    def down(self, a):
        return a if self.where == "host" else a.cpu().numpy()

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def rows(self, truth, pred, tstrides, pstrides, B, T, N, dx, *, shift=0, kind=0, coef=None, outs=False):
        """``bg_eval_rows`` (or its host twin) on host arrays put into this memory: ``truth`` / ``pred`` are the storage,
        ``tstrides`` / ``pstrides`` their (batch, time) element strides.  Returns (rowstats, truth_out, pred_out)."""
        mem = [self.up(np.asarray(v, dtype=np.float32)) if v is not None else None for v in (truth, pred, coef)]
        t_out = self.up(np.zeros((B, T, N), dtype=np.float32)) if outs else None
        p_out = self.up(np.zeros((B, T, N), dtype=np.float32)) if outs else None
        stats = self.up(np.zeros((B, T, mo.ROW_STATS)))
        batch = _hip.EvalBatch(self.ptr(mem[0]), tstrides[0], tstrides[1], self.ptr(mem[1]), pstrides[0], pstrides[1], shift,
                               kind, self.ptr(mem[2]), self.ptr(t_out), self.ptr(p_out))
        if self.where == "host":
            rc = self.lib.bg_eval_rows_host(ctypes.byref(batch), B, T, N, dx, self.ptr(stats))
        else:
            rc = self.lib.bg_eval_rows(self._stream(), ctypes.byref(batch), B, T, N, dx, self.ptr(stats))
        assert rc == 0, (rc, self.lib.bg_eval_last_error())
        return self.down(stats), (self.down(t_out) if outs else None), (self.down(p_out) if outs else None)

    def fold(self, stats, B, T, N, accum=None):
        """``bg_eval_fold`` (or its host twin) on rowstats (host array); ``accum`` is a memory object of this context."""
        mem, tables = self.up(stats), self.up(np.zeros(1 + mo.TABLES * T))
        if self.where == "host":
            rc = self.lib.bg_eval_fold_host(self.ptr(mem), B, T, N, self.ptr(tables), self.ptr(accum))
        else:
            rc = self.lib.bg_eval_fold(self._stream(), self.ptr(mem), B, T, N, self.ptr(tables), self.ptr(accum))
        assert rc == 0, (rc, self.lib.bg_eval_last_error())
        return self.down(tables)

    def derivatives(self, u, dx):
        """``bg_derivatives`` (or its host twin) on fp32 rows [M, N]: (ux, uxx) fp64 [M, N]."""
        u = np.ascontiguousarray(u, dtype=np.float32)
        mem, ux, uxx = self.up(u), self.up(np.zeros(u.shape)), self.up(np.zeros(u.shape))
        if self.where == "host":
            rc = self.lib.bg_derivatives_host(self.ptr(mem), u.shape[0], u.shape[1], dx, self.ptr(ux), self.ptr(uxx))
        else:
            rc = self.lib.bg_derivatives(self._stream(), self.ptr(mem), u.shape[0], u.shape[1], dx, self.ptr(ux), self.ptr(uxx))
        assert rc == 0, (rc, self.lib.bg_eval_last_error())
        return self.down(ux), self.down(uxx)

    def case_rows(self, c, outs=True):
        """The shared case ``c`` (``_bg_eval_oracle.case``) through its kind-1 map and the shifted time-major prediction."""
        n, b, t = c["n"], c["b"], c["t"]
        return self.rows(c["truth"], c["pred_tm"], batch_major(b, t, n), time_major(b, t, n), b, t, n, c["dx"], shift=1,
                         kind=1, coef=c["coef"], outs=outs)
