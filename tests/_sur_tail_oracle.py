"""Shared pieces of tests/test_surrogate_tail_host.py and tests/test_surrogate_tail_gpu.py: synthetic parameter packs for the
entry points of the surrogate step's tail (gradient reduction, row fold, Adam, delta loss; include/surrogate_hip.h) and
their fp64 oracles.  Nothing in here needs a GPU.

The reduction, fold and Adam entry points read only ``w``, ``g``, ``size``, ``partial`` and ``rows`` of a pack, so the packs
built here carry ANY size list (the geometry fields stay zero) and the code's own boundaries -- FLUSH_COLS = 32 columns per
block, FLUSH_RG = 32 row groups x 8 loads per round, TPB = 256 elements per Adam block -- are placed on purpose."""
import ctypes
import json
import os

import numpy as np
import torch

from _sac_models import U, UNIT_BOUND, adam_replay, adam_units  # noqa: F401  (one spelling of the Adam oracle)

from conftest import GRAD_LOG

OBSERVED = os.path.join(os.path.dirname(GRAD_LOG), "sur_tail_parity_observed.jsonl")
ENC_NPARAM, ST_NPARAM = 27, 26
FLUSH_COLS, FLUSH_RG, ADAM_TPB = 32, 32, 256
GAP = 3                       # guard floats between two tensors and at both ends (odd: no tensor is 8- or 16-byte aligned)
SENTINEL = np.float32(-12345.678)
#: rows of the reduction tests: fewer rows than row groups, both sides of one full round of 32 x 8 rows, the pipelined
#: layout's 768 + 1
ROWS = (1, 31, 32, 33, 255, 256, 257, 769)


def nparam(kind):
    return {"enc": ENC_NPARAM, "chunk": ST_NPARAM}[kind]


def flush_blocks(psize):
    return (psize + FLUSH_COLS - 1) // FLUSH_COLS


def layout(name, kind):
    """Size list of a pack of ``kind``.  Every layout holds size-1 tensors; all but "tiny" (which fits no edge) hold a
    tensor that ends exactly on a 32-column block edge ([1, 31]: columns 1..31) and tensors that straddle one.
      odd   psize = 70 + (NP - 5) = 92 / 91      psize % 32 != 0, 3 blocks; the 30-wide tensor covers columns 40..69
      even  psize = 128                          psize % 32 == 0, 4 blocks; the 40-wide tensor covers 33..72, the last
                                                 one (33 / 34 wide) 95 / 94 .. 127, across column 96
      tiny  psize = NP < 32                      1 block, only size-1 tensors
      wide  psize = 273 + (NP - 5) = 295 / 294   10 blocks, 2 Adam blocks; the 200-wide tensor covers 73..272 (crosses 256)"""
    n = nparam(kind)
    if name == "odd":
        sizes = [1, 31, 7, 1, 30] + [1] * (n - 5)
    elif name == "even":
        sizes = [1, 31, 1, 40] + [1] * (n - 5)
        sizes.append(128 - sum(sizes))
    elif name == "tiny":
        sizes = [1] * n
    elif name == "wide":
        sizes = [1, 31, 1, 40, 200] + [1] * (n - 5)
    else:
        raise KeyError(name)
    assert len(sizes) == n and min(sizes) >= 1
    return sizes


LAYOUTS = ("odd", "even", "tiny", "wide")


def guarded(n, device, dtype=torch.float32, fill=None):
    """(flat, view): ``view`` = n elements of ``flat`` with GAP sentinel elements on either side."""
    flat = torch.full((n + 2 * GAP,), float(SENTINEL), dtype=dtype, device=device)
    view = flat[GAP:GAP + n]
    if fill is not None:
        view.fill_(fill)
    return flat, view


def bits(t):
    """The int32 bit patterns of an fp32 tensor / array, on the host."""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.int32 if a.dtype.itemsize == 4 else np.int64).copy()


class Pack:
    """One synthetic parameter pack.  ``wflat`` / ``gflat``: GAP sentinel floats, tensor 0, GAP, tensor 1, ..., GAP;
    ``offs[i]`` the position of tensor i in either.  ``partial`` = the [alloc_rows][psize] view of ``partial_flat`` (GAP
    sentinels on both sides); rows [rows, alloc_rows) hold the sentinel."""

    def __init__(self, kind, sizes, rows, alloc_rows, device):
        from pdecontrol.surrogates import hipops
        assert alloc_rows > rows >= 1 and len(sizes) == nparam(kind)
        self.kind, self.sizes, self.rows, self.alloc_rows = kind, list(sizes), rows, alloc_rows
        self.psize = int(sum(sizes))
        self.offs, off = [], GAP
        for s in sizes:
            self.offs.append(off)
            off += s + GAP
        self.flat_len = off
        self.wflat = torch.full((off,), float(SENTINEL), dtype=torch.float32, device=device)
        self.gflat = torch.full((off,), float(SENTINEL), dtype=torch.float32, device=device)
        self.partial_flat, view = guarded(alloc_rows * self.psize, device)
        self.partial = view.view(alloc_rows, self.psize)
        self.c = (hipops.EncoderParams if kind == "enc" else hipops.ChunkParams)()
        for i, (s, o) in enumerate(zip(sizes, self.offs)):
            self.c.size[i] = s
            self.c.w[i] = self.wflat.data_ptr() + 4 * o
            self.c.g[i] = self.gflat.data_ptr() + 4 * o
        self.c.partial, self.c.rows = self.partial.data_ptr(), rows
        self.index = torch.cat([torch.arange(o, o + s) for s, o in zip(sizes, self.offs)]).to(device)
        self.gap_mask = torch.ones(off, dtype=torch.bool, device=device)
        self.gap_mask[self.index] = False

    def ref(self):
        return ctypes.byref(self.c)

    def get(self, flat):
        """The packed [psize] values of ``wflat`` / ``gflat`` (a copy)."""
        return flat[self.index].clone()

    def put(self, flat, values):
        flat[self.index] = torch.as_tensor(values, dtype=torch.float32).to(flat.device)

    def gaps_intact(self):
        """Guard gaps of w, g and around the partial buffer, and the surplus partial rows, still hold the sentinel bits."""
        want = bits(np.float32(SENTINEL).reshape(1))[0]
        return all(bool(np.all(bits(x) == want)) for x in (self.wflat[self.gap_mask], self.gflat[self.gap_mask],
                                                             self.partial_flat[:GAP], self.partial_flat[-GAP:],
                                                             self.partial[self.rows:]))


def synthetic_pack(kind, sizes, rows, alloc_rows, device):
    """A filled ``hipops.EncoderParams`` (kind "enc") or ``hipops.ChunkParams`` ("chunk") with its backing tensors."""
    return Pack(kind, sizes, rows, alloc_rows, device)


def mixed_rows(rs, rows, psize):
    """[rows][psize] fp32: mixed signs, magnitudes log-uniform over six decades (1e-3 .. 1e3)."""
    mag = 10.0 ** rs.uniform(-3.0, 3.0, (rows, psize))
    return (mag * rs.choice([-1.0, 1.0], (rows, psize))).astype(np.float32)


class AdamState:
    """Moments, step counter, ticket and device learning rate of one pack, each between guard sentinels, and the descriptor
    that points at them."""

    def __init__(self, pack, lr, beta1, beta2, eps, device):
        from pdecontrol.surrogates import hipops
        self.hyper = dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps)
        self.mflat, self.m = guarded(pack.psize, device, fill=0.0)
        self.vflat, self.v = guarded(pack.psize, device, fill=0.0)
        self.iflat, ints = guarded(2, device, dtype=torch.int32, fill=0)     # [step, ticket]
        self.step, self.ticket = ints[0:1], ints[1:2]
        self.lrflat, self.lr = guarded(1, device, fill=lr)
        self.desc = hipops.AdamParams(self.m.data_ptr(), self.v.data_ptr(), self.step.data_ptr(), self.ticket.data_ptr(),
                                      self.lr.data_ptr(), beta1, beta2, eps)

    def ref(self):
        return ctypes.byref(self.desc)

    def gaps_intact(self):
        f = bits(np.float32(SENTINEL).reshape(1))[0]
        i = int(np.int32(float(SENTINEL)))
        return (all(bool(np.all(bits(x[:GAP]) == f) and np.all(bits(x[-GAP:]) == f)) for x in (self.mflat, self.vflat, self.lrflat))
                and bool(np.all(self.iflat[:GAP].cpu().numpy() == i) and np.all(self.iflat[-GAP:].cpu().numpy() == i)))


# ----------------------------------------------------------------------------------------------------------------------
# fp64 oracles
# ----------------------------------------------------------------------------------------------------------------------
def reduce_rows(partial, rows):
    """(sum, sum of magnitudes) over rows [0, rows) of an fp32 [*, psize] array, both fp64, accumulated row by row."""
    p = np.asarray(partial, dtype=np.float64)
    s, a = np.zeros(p.shape[1]), np.zeros(p.shape[1])
    for r in range(rows):
        s += p[r]
        a += np.abs(p[r])
    return s, a


def fold_rows(partial, base, count, dst):
    """The buffer after folding rows [base, base + count) into row dst (fp64 [*, psize]) and the magnitude sum that went
    into dst (its prior content included)."""
    p = np.array(partial, dtype=np.float64)
    s, a = np.zeros(p.shape[1]), np.abs(p[dst]).copy()
    for r in range(base, base + count):
        s += p[r]
        a += np.abs(p[r])
    p[dst] += s
    p[base:base + count] = 0.0
    return p, a


def depth_bound(nrows, abs_sum):
    """Worst error of the kernels' two summation chains (ceil(nrows / 32) adds per row group, then 32 row groups):
    (ceil(nrows / 32) + 32) u sum |x|."""
    return (-(-nrows // FLUSH_RG) + FLUSH_RG) * U * abs_sum


def delta_loss_oracle(states, d_all, delta, mean, stdv, order=0):
    """The delta loss of training.py:100-121 as include/surrogate_hip.h states it.  states [B, T, N] fp32 (any strides),
    d_all [T, B, N] fp32.  fp32, one rounding per operation: ``deltas`` [B, T-1, N], the error, its square and ``dd_all``
    [T, B, N] (row T-1 zero).  fp64: every sum, and from the sums ``loss``, ``hsteploss`` [T-1] and ``stats`` = (mean,
    unbiased std) of d_all[:T-1], then of the deltas.  ``order`` 1 sums the same terms in another order (reversed, pairwise)."""
    s, od = np.asarray(states), np.asarray(d_all)
    assert s.dtype == np.float32 and od.dtype == np.float32
    B, T, N = s.shape
    f = np.float32
    dl = ((s[:, 1:] - s[:, :-1]) / f(delta) - f(mean)) / f(stdv)          # [B, T-1, N]
    assert dl.dtype == np.float32
    odt = od[:T - 1].transpose(1, 0, 2)                                      # [B, T-1, N]
    err = odt - dl
    sq = err * err
    count = float(B * N * (T - 1))
    dd = np.zeros((T, B, N), dtype=np.float32)
    dd[:T - 1] = (f(2.0 / count) * err).transpose(1, 0, 2)
    assert err.dtype == sq.dtype == np.float32

    def total(x, axis=None):
        x = x.astype(np.float64)
        if order == 0:
            return np.add.reduce(x.transpose(1, 0, 2).reshape(T - 1, -1), axis=1) if axis == "t" else float(np.sum(x))
        x = x[::-1, :, ::-1]
        return np.array([np.sum(x[:, t].ravel()) for t in range(T - 1)]) if axis == "t" else float(np.sum(np.sum(x, axis=2)))

    def mean_std(x):
        x64 = x.astype(np.float64)
        s1, s2 = total(x), total(x64 * x64 if order == 0 else x * x.astype(np.float64))
        m = s1 / count
        return m, float(np.sqrt(max(s2 - count * m * m, 0.0) / (count - 1.0)))

    m_od, s_od = mean_std(odt)
    m_dl, s_dl = mean_std(dl)
    return dict(deltas=dl, dd_all=dd, loss=total(sq) / count, hsteploss=total(sq, "t") / float(B * N),
                stats=np.array([m_od, s_od, m_dl, s_dl]))


def rel_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.abs(ref))) if got.size else 0.0


# ----------------------------------------------------------------------------------------------------------------------
# inputs and the observation log
# ----------------------------------------------------------------------------------------------------------------------
_stamp = []


def library_stamp():
    """First 16 hex digits of the SHA-256 of the libsurrogate_hip.so the tests load: which build a record belongs to."""
    if not _stamp:
        import hashlib
        from pdecontrol.surrogates import hipops
        try:
            _stamp.append(hashlib.sha256(open(hipops.LIB_PATH, "rb").read()).hexdigest()[:16])
        except OSError:
            _stamp.append("not built")
    return _stamp[0]


def record(**rec):
    """Append one observation to OBSERVED, stamped with the library build it was made on: the log is append-only across
    runs, and tools/sur_tail_parity_report.py keeps the records of the log's latest build only."""
    rec["lib"] = library_stamp()
    print("sur tail parity", json.dumps(rec))
    try:
        os.makedirs(os.path.dirname(OBSERVED), exist_ok=True)
        with open(OBSERVED, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


def loss_inputs(B, T, N, seed, storage="batch"):
    """states [B, T, N] (a view of the storage asked for) and d_all [T, B, N], fp32, such that |mean| <= std for the
    predicted and the true deltas under both scalings the tests use."""
    rs = np.random.RandomState(seed)
    if storage == "batch":
        states = rs.uniform(-1, 1, (B, T, N)).astype(np.float32)
    elif storage == "time":
        states = rs.uniform(-1, 1, (T, B, N)).astype(np.float32).transpose(1, 0, 2)
    else:                                                              # padded strides
        states = rs.uniform(-1, 1, (B, T + 2, N + 5)).astype(np.float32)[:, 1:T + 1, 2:N + 2]
    d_all = (rs.standard_normal((T, B, N)) * 3.0 + 0.25).astype(np.float32)
    return states, d_all


def gradient_classes(rs, n, signs=None):
    """n fp32 gradients, by position i % 5: exactly 0, |g| near 1e-12 (eps dominates; g^2 a normal fp32 number), near
    1e-3, near 1, near 1e3; signs mixed (drawn, or the ones given)."""
    base = np.array([0.0, 1e-12, 1e-3, 1.0, 1e3])[np.arange(n) % 5]
    signs = rs.choice([-1.0, 1.0], n) if signs is None else signs
    return (base * rs.uniform(0.5, 2.0, n) * signs).astype(np.float32)


def parameter_classes(rs, n):
    """n fp32 parameters, by position (i // 5) % 3: of order 0.1, of order 1e-7, exactly 0.  Next to a small parameter the
    unit of p' (u |p| + 16 u |step|) is the step's own, so an error of the step multiplier is not hidden behind |p|."""
    scale = np.array([0.1, 1e-7, 0.0])[(np.arange(n) // 5) % 3]
    return (rs.standard_normal(n) * scale).astype(np.float32)


def small_parameter(n):
    return (np.arange(n) // 5) % 3 != 0
