"""The cases of ``ks_eval_rows_device`` / ``ks_eval_fold_device`` that the host suite runs on the library's CPU twin
(tests/test_eval_rows_host.py) and the GPU suite on device 0 (tests/test_eval_rows_gpu.py): one body per case, the memory
behind a small context.  Yardsticks: tests/golden/evalstep_golden.npz (recorded from the reference's own ``test_step``),
the fp64 numpy restatement of tests/_eval_metrics_oracle.py, and torch's host transforms for the inverse maps.

The largest deviation from the fixture is appended to test_phase_parity_observed.jsonl next to conftest's gradient parity
log (tools/test_phase_bench.py --parity folds it into profiles/test_phase_parity_observed.json)."""
import json
import os

import numpy as np
import torch

import _eval_metrics_oracle as mo
from conftest import GOLDEN, GRAD_LOG, KS_CONFIGS

OBSERVED = os.path.join(os.path.dirname(GRAD_LOG), "test_phase_parity_observed.jsonl")
DT = 1e-3


class Ctx:
    """A ``kspde.KSStepper`` of one N on ``device`` (-1: the twin on numpy arrays; >= 0: torch tensors on that GPU, the
    handle bound to torch's current stream) and the three memory operations the cases need."""

    def __init__(self, device, N, L):
        import kspde
        self.kspde, self.device, self.N, self.L = kspde, device, N, L
        self.h = kspde.KSStepper(1, N, L, DT, device=device)
        if device >= 0:
            self.h.set_stream(torch.cuda.current_stream(torch.device("cuda", device)).cuda_stream)

    def up(self, a):
        a = np.ascontiguousarray(a)
        return a.copy() if self.device < 0 else torch.from_numpy(a).to(torch.device("cuda", self.device))

    def ptr(self, a):
        return 0 if a is None else (a.ctypes.data if self.device < 0 else a.data_ptr())

    def down(self, a):
        return a if self.device < 0 else a.cpu().numpy()

    def rows(self, truth, pred, tstrides, pstrides, B, T, *, shift=0, phi=None, kind=0, coef=None, objective="l2control",
             outs=False):
        """Runs ks_eval_rows_device on host arrays put into this context's memory: ``truth`` / ``pred`` are the storage,
        ``tstrides`` / ``pstrides`` their (batch, time) element strides.  Returns (rowstats, truth_out, pred_out)."""
        N = self.N
        mem = [self.up(np.asarray(v, dtype=np.float32)) if v is not None else None for v in (truth, pred, phi, coef)]
        t_out = self.up(np.zeros((B, T, N), dtype=np.float32)) if outs else None
        p_out = self.up(np.zeros((B, T, N), dtype=np.float32)) if outs else None
        stats = self.up(np.zeros((B, T, mo.ROW_STATS)))
        vp = lambda a: self.ptr(a) or None
        batch = self.kspde.ks_eval_batch(vp(mem[0]), tstrides[0], tstrides[1], vp(mem[1]), pstrides[0], pstrides[1], shift,
                                         vp(mem[2]), kind, vp(mem[3]), vp(t_out), vp(p_out))
        self.h.eval_rows_device(objective, batch, B, T, self.ptr(stats))
        self.stats_mem = stats
        return self.down(stats), (self.down(t_out) if outs else None), (self.down(p_out) if outs else None)

    def fold(self, stats, B, T, accum=None):
        """Runs ks_eval_fold_device on rowstats (host array); ``accum`` is a memory object of this context or None."""
        mem, tables = self.up(stats), self.up(np.zeros(1 + mo.TABLES * T))
        self.h.eval_fold_device(self.ptr(mem), B, T, self.ptr(tables), self.ptr(accum))
        return self.down(tables)


def batch_major(B, T, N):
    return (T * N, N)


def fixture():
    return np.load(os.path.join(GOLDEN, "evalstep_golden.npz"))


def random_rows(seed, B, T, N, scale=1.5):
    """A smooth-ish truth and a prediction a few per cent off, fp32 [B, T, N]."""
    rs = np.random.RandomState(seed)
    x = np.arange(N) * (2 * np.pi / N)
    truth = sum(rs.uniform(-scale, scale, (B, T, 1)) * np.sin((k + 1) * x + rs.uniform(0, 6, (B, T, 1))) for k in range(3))
    pred = truth + 0.05 * rs.standard_normal((B, T, N))
    return truth.astype(np.float32), pred.astype(np.float32)


# ---- case 1: the recorded fixture ----------------------------------------------------------------------------------------
def check_fixture_case(device, label):
    g = fixture()
    L, N = KS_CONFIGS["n64"]
    truth, pred = g["test_states"][:, :, 0], g["test_outputs"][:, :, 0]
    B, T, _ = truth.shape
    ctx = Ctx(device, N, L)
    stats, _, _ = ctx.rows(truth, pred, batch_major(B, T, N), batch_major(B, T, N), B, T)
    got = mo.named(ctx.fold(stats, B, T), T)
    worst = {}
    for name, value in got.items():
        ref = g["test_" + name].astype(np.float64)
        top = float(np.abs(ref).max())
        worst[name] = float(np.abs(value - ref).max() / top) if top > 0 else float(np.abs(value).max())
    rec = {"label": label, "largest_deviation_over_largest_reference_entry": worst, "rtol": 2e-5, "atol_over_largest": 2e-5}
    print("test phase parity", json.dumps(rec))
    try:
        os.makedirs(os.path.dirname(OBSERVED), exist_ok=True)
        with open(OBSERVED, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass
    for name, value in got.items():
        ref = g["test_" + name].astype(np.float64)
        # the reference sums fp32 over N = 64 (<= N 2^-24 ~ 4e-6 relative), the kernels in fp64: that is the whole difference
        np.testing.assert_allclose(value, ref, rtol=2e-5, atol=2e-5 * float(np.abs(ref).max()), err_msg=name)
    # the fixture's step 0 is the initial condition on both sides: its error tables are exactly 0
    for name, value in got.items():
        if name != "MSE":
            assert value[0] == 0.0, (name, value[0])


# ---- case 2: inverse maps and prediction layouts -----------------------------------------------------------------------
def _normalize_like_eval_module(columns):
    from pdegym.common import transforms as T
    g = fixture()
    norm = T.Normalize(aggregate=not columns, batched=not columns)
    norm.update(g["raw_states"])
    return norm, g


def check_normalize_inverse(device, columns):
    """Kind 2 with the Normalize of build_eval_module (scalar statistics) or a per-column one: truth_out has the bits of
    stransf.otransf.Inverse(states) computed by torch on the host."""
    from pdecontrol.mbrl.recognition import inverse_map
    from pdegym.common import transforms as T
    norm, g = _normalize_like_eval_module(columns)
    L, N = KS_CONFIGS["n64"]
    stransf = T.SampleTransform(norm, None)
    states = stransf.otransf(torch.from_numpy(g["raw_states"])).reshape(3, 9, 1, N)
    kind, coef = inverse_map(stransf.otransf.Inverse, N)
    assert kind == 2 and tuple(coef.shape) == (2, N)
    want = stransf.otransf.Inverse(states).numpy()[:, :, 0]
    B, T = 3, 9
    rows = states.numpy()[:, :, 0]
    ctx = Ctx(device, N, L)
    _, t_out, p_out = ctx.rows(rows, rows[:, ::-1].copy(), batch_major(B, T, N), batch_major(B, T, N), B, T, kind=kind,
                               coef=coef.numpy(), outs=True)
    np.testing.assert_array_equal(t_out, want)
    np.testing.assert_array_equal(p_out, want[:, ::-1])


def check_scale_inverse(device):
    """Kind 1 against a per-column ScaleTransform's inverse on the host."""
    from pdecontrol.mbrl.recognition import inverse_map
    from pdegym.common import transforms as T
    g = fixture()
    L, N = KS_CONFIGS["n64"]
    scale = T.ScaleTransform(scale=(-1.0, 1.0))
    scale.update(torch.from_numpy(g["raw_states"]))
    chain = T.Operation([T.BatchTransform(scale)])
    states = chain(torch.from_numpy(g["raw_states"])).reshape(3, 9, 1, N)
    kind, coef = inverse_map(chain.Inverse, N)
    assert kind == 1 and tuple(coef.shape) == (4, N)
    want = chain.Inverse(states.reshape(27, 1, N)).numpy().reshape(3, 9, N)
    rows = states.numpy()[:, :, 0]
    ctx = Ctx(device, N, L)
    _, t_out, _ = ctx.rows(rows, rows, batch_major(3, 9, N), batch_major(3, 9, N), 3, 9, kind=kind, coef=coef.numpy(), outs=True)
    np.testing.assert_array_equal(t_out, want)
    np.testing.assert_array_equal(t_out, mo.affine_inverse(rows, coef.numpy()))


def check_shift_over_time_major(device):
    """pred_shift = 1 over time-major prediction storage gives the tables of the explicitly concatenated batch-major
    layout, bit for bit, and exact zeros at step 0."""
    B, T, N, L = 5, 6, 64, 22.0
    truth, rollout = random_rows(3, B, T, N)          # rollout[b, t] predicts truth[b, t + 1]
    norm, _ = _normalize_like_eval_module(False)
    from pdecontrol.mbrl.recognition import inverse_map
    kind, coef = inverse_map(norm.Inverse, N)
    ctx = Ctx(device, N, L)
    time_major = np.ascontiguousarray(rollout.transpose(1, 0, 2))        # [T, B, N]: what the fused chunk kernels write
    s1, t1, p1 = ctx.rows(truth, time_major, batch_major(B, T, N), (N, B * N), B, T, shift=1, kind=kind, coef=coef.numpy(),
                          outs=True)
    s2, t2, p2 = ctx.rows(truth, mo.shifted(truth, rollout), batch_major(B, T, N), batch_major(B, T, N), B, T, shift=0,
                          kind=kind, coef=coef.numpy(), outs=True)
    np.testing.assert_array_equal(s1, s2)
    np.testing.assert_array_equal(p1, p2)
    np.testing.assert_array_equal(t1, t2)
    np.testing.assert_array_equal(ctx.fold(s1, B, T), ctx.fold(s2, B, T))
    for j in (0, 1, 6, 7, 10, 11, 14, 15):
        assert np.all(s1[:, 0, j] == 0.0), j
    assert np.array_equal(s1[:, 0, 4], s1[:, 0, 5])


# ---- case 3: dissipation -----------------------------------------------------------------------------------------------
def check_dissipation_rewards(device, N=64, L=22.0, B=3, T=7):
    """Rows 4 and 5 under dissipation have the bits of ks_reward_rows_device on the same rows and phi; the whole row agrees
    with the numpy restatement."""
    truth, pred = random_rows(5, B, T, N)
    phi = (0.3 * np.random.RandomState(6).standard_normal((B, T, N))).astype(np.float32)
    ctx = Ctx(device, N, L)
    stats, _, _ = ctx.rows(truth, pred, batch_major(B, T, N), batch_major(B, T, N), B, T, phi=phi, objective="dissipation")
    for column, rows in ((4, truth), (5, pred)):
        obs, p, out = ctx.up(rows.reshape(B * T, N)), ctx.up(phi.reshape(B * T, N)), ctx.up(np.zeros(B * T))
        ctx.h.reward_rows_device("dissipation", ctx.ptr(obs), ctx.ptr(p), B * T, ctx.ptr(out))
        np.testing.assert_array_equal(stats[..., column].reshape(-1), ctx.down(out))
    np.testing.assert_allclose(stats, mo.row_stats(truth, pred, L / N, "dissipation", phi), rtol=1e-12, atol=0)
    # phi = NULL is phi = 0
    stats0, _, _ = ctx.rows(truth, pred, batch_major(B, T, N), batch_major(B, T, N), B, T, objective="dissipation")
    np.testing.assert_allclose(stats0, mo.row_stats(truth, pred, L / N, "dissipation", None), rtol=1e-12, atol=0)


# ---- case 4: the fold --------------------------------------------------------------------------------------------------
def check_fold(device):
    N, L = 64, 22.0
    ctx = Ctx(device, N, L)
    for B, T in ((1, 4), (3, 7)):
        truth, pred = random_rows(7 + B, B, T, N)
        stats = mo.row_stats(truth, pred, L / N)
        want = mo.fold(stats, N)
        got = ctx.fold(stats, B, T)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
        accum = ctx.up(np.zeros(1 + mo.TABLES * T))
        first = ctx.fold(stats, B, T, accum)
        second = ctx.fold(stats, B, T, accum)
        np.testing.assert_array_equal(first, got)
        np.testing.assert_array_equal(second, got)
        np.testing.assert_array_equal(ctx.down(accum), 2 * B * got)
    # a zero truth row: 0 / 0 and x / 0 as IEEE (and the reference) give them
    B, T = 2, 3
    truth, pred = random_rows(11, B, T, N)
    truth[1, 2] = 0.0                      # x / 0
    truth[0, 0] = pred[0, 0] = 0.0         # 0 / 0
    stats = mo.row_stats(truth, pred, L / N)
    want, got = mo.fold(stats, N), ctx.fold(stats, B, T)
    assert np.isinf(want).any() and np.isnan(want).any() and not np.isfinite(want[1 + 2 * T + 2])
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(np.isinf(got), np.isinf(want))
    ok = np.isfinite(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=1e-12, atol=0)


# ---- shapes (the lane-group widths of the launcher, a ragged N, a ragged last workgroup) -------------------------------
SHAPES = [(64, 22.0, 3, 7), (100, 34.375, 3, 7), (256, 88.0, 2, 5), (1024, 352.0, 2, 3), (48, 16.5, 17, 1)]


def check_shape(device, N, L, B, T):
    """rowstats against the numpy restatement at rtol 1e-12 (fp64 sums of <= 1024 terms), both objectives' l2control
    rows included, through a non-trivial inverse map and a shifted time-major prediction."""
    truth, rollout = random_rows(N + B, B, T, N)
    rs = np.random.RandomState(N)
    coef = np.stack([rs.uniform(0.5, 2.0, N), rs.uniform(-0.5, 0.5, N)]).astype(np.float32)      # kind 2: v * s + m
    ctx = Ctx(device, N, L)
    time_major = np.ascontiguousarray(rollout.transpose(1, 0, 2))
    stats, t_out, p_out = ctx.rows(truth, time_major, batch_major(B, T, N), (N, B * N), B, T, shift=1, kind=2, coef=coef,
                                   outs=True)
    s = (truth * coef[0]).astype(np.float32) + coef[1]
    o = (mo.shifted(truth, rollout) * coef[0]).astype(np.float32) + coef[1]
    np.testing.assert_array_equal(t_out, s)
    np.testing.assert_array_equal(p_out, o)
    np.testing.assert_allclose(stats, mo.row_stats(s, o, L / N), rtol=1e-12, atol=0)
    return stats


# ---- case 5: bad arguments ---------------------------------------------------------------------------------------------
def check_bad_arguments(device):
    import ctypes
    import kspde
    N, L, B, T = 64, 22.0, 2, 3
    ctx = Ctx(device, N, L)
    lib, h = kspde.load(), ctx.h._h
    keep = [ctx.up(np.zeros((B, T, N), dtype=np.float32)), ctx.up(np.zeros((4, N), dtype=np.float32)),
            ctx.up(np.zeros((B, T, mo.ROW_STATS))), ctx.up(np.zeros(1 + mo.TABLES * T))]
    rows, coef, stats, tables = (ctypes.c_void_p(ctx.ptr(m)) for m in keep)

    def batch(**change):
        fields = dict(truth=rows.value, truth_bstride=T * N, truth_tstride=N, pred=rows.value, pred_bstride=T * N,
                      pred_tstride=N, pred_shift=0, phi=None, inv_kind=0, inv_coef=None, truth_out=None, pred_out=None)
        fields.update(change)
        return ctypes.byref(kspde.ks_eval_batch(**fields))

    def refused(rc, name):
        assert rc < 0, rc
        assert lib.ks_last_error().startswith(name.encode()), lib.ks_last_error()

    R, F = "ks_eval_rows_device", "ks_eval_fold_device"
    assert lib.ks_eval_rows_device(h, 0, batch(), B, T, stats) == 0
    refused(lib.ks_eval_rows_device(None, 0, batch(), B, T, stats), R)
    refused(lib.ks_eval_rows_device(h, 0, None, B, T, stats), R)
    refused(lib.ks_eval_rows_device(h, 0, batch(), B, T, None), R)
    refused(lib.ks_eval_rows_device(h, 0, batch(truth=None), B, T, stats), R)
    refused(lib.ks_eval_rows_device(h, 0, batch(pred=None), B, T, stats), R)
    refused(lib.ks_eval_rows_device(h, 0, batch(), 0, T, stats), R)
    refused(lib.ks_eval_rows_device(h, 0, batch(), B, 0, stats), R)
    refused(lib.ks_eval_rows_device(h, 2, batch(), B, T, stats), R)
    refused(lib.ks_eval_rows_device(h, 0, batch(inv_kind=3), B, T, stats), R)
    refused(lib.ks_eval_rows_device(h, 0, batch(inv_kind=-1), B, T, stats), R)
    refused(lib.ks_eval_rows_device(h, 0, batch(inv_kind=1), B, T, stats), R)
    refused(lib.ks_eval_rows_device(h, 0, batch(inv_kind=2), B, T, stats), R)
    assert lib.ks_eval_rows_device(h, 0, batch(inv_kind=0, inv_coef=coef.value), B, T, stats) == 0
    refused(lib.ks_eval_rows_device(h, 0, batch(pred_shift=2), B, T, stats), R)
    for name in ("truth_bstride", "truth_tstride", "pred_bstride", "pred_tstride"):
        refused(lib.ks_eval_rows_device(h, 0, batch(**{name: N - 1}), B, T, stats), R)
        refused(lib.ks_eval_rows_device(h, 0, batch(**{name: 0}), B, T, stats), R)
    assert lib.ks_eval_fold_device(h, stats, B, T, tables, None) == 0
    refused(lib.ks_eval_fold_device(None, stats, B, T, tables, None), F)
    refused(lib.ks_eval_fold_device(h, None, B, T, tables, None), F)
    refused(lib.ks_eval_fold_device(h, stats, B, T, None, None), F)
    refused(lib.ks_eval_fold_device(h, stats, 0, T, tables, None), F)
    refused(lib.ks_eval_fold_device(h, stats, B, -1, tables, None), F)
    ctx.h.sync()


# ---- case 6: test_surrogate --------------------------------------------------------------------------------------------
def two_batch_loader(g, device="cpu"):
    s, a = torch.from_numpy(g["states"]).to(device), torch.from_numpy(g["actions"]).to(device)
    return [(s[:2], a[:2]), (s[2:], a[2:])]


ROW_MEAN_KEYS = [name for name in mo.TABLE_NAMES if not name.endswith("_rews")]


def reward_tables_of_two_batches(g):
    """What EvalLogCallback's weighted mean makes of the reward tables for batches [0, 1] and [2]: restated in numpy from
    the fixture's own rows (l2control rewards in fp32, as the reference forms them)."""
    N = g["test_states"].shape[-1]
    # kuramoto.py:64-65 of the reference, row by row in fp32 torch (its norm's summation order is part of the record)
    rew = lambda v: np.array([[float((-1.0) * (1 / N) * torch.norm(torch.from_numpy(row)) ** 2) for row in seq] for seq in v],
                             dtype=np.float32)
    r, p = rew(g["test_states"]), rew(g["test_outputs"])
    out = {name: 0.0 for name in mo.TABLE_NAMES if name.endswith("_rews")}
    for rows in (slice(0, 2), slice(2, 3)):
        rb, d = r[rows].astype(np.float64), (r[rows] - p[rows]).astype(np.float64)
        n = rb.shape[0]
        e1, e2, r1, r2 = np.abs(d).sum(0), np.sqrt((d * d).sum(0)), np.abs(rb).sum(0), np.sqrt((rb * rb).sum(0))
        for name, value in (("l1_loss_rews", e1), ("l2_loss_rews", e2), ("l1_loss_scaled_rews", e1 / r1),
                            ("l2_loss_scaled_rews", e2 / r2), ("nrmse_rews", e2 ** 2 / r2 ** 2)):
            out[name] = out[name] + n * value / 3.0
    return out
