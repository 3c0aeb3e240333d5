"""The metric section of the reference's ``PDETrainingModule.test_step`` (pdecontrol/surrogates/training.py:195-243) restated
in fp64 numpy: the yardstick of the ``ks_eval_rows_device`` / ``ks_eval_fold_device`` tests for shapes the recorded fixture
lacks.  Derivatives come from the oracle's KS rhs (oracle/ks_oracle.c, which shares nothing with csrc/); nothing here is
ever compared with the code under test's own output.

``row_stats`` takes the rows as the metrics read them (inverse-scaled, the prediction aligned with the truth) and returns
the 18 sums per row of include/kspde.h; ``fold`` turns them into the MSE and the 25 per-step tables in the order of the
dict ``test_step`` returns.  Sums are fp64 throughout; the error is the fp32 difference the reference forms; an l2control
reward is rounded to fp32, the precision the reference's reward has there."""
import numpy as np

from oracle import ks_oracle as ko

ROW_STATS, TABLES = 18, 25
TABLE_NAMES = (["l1_loss", "l2_loss", "l1_loss_scaled", "l2_loss_scaled", "nrmse"]
               + ["l1_loss_rews", "l2_loss_rews", "l1_loss_scaled_rews", "l2_loss_scaled_rews", "nrmse_rews"]
               + [f"{name}-derivative-{d}" for name in ("l1_loss_derivs", "l2_loss_derivs", "l1_loss_scaled_derivs",
                                                        "l2_loss_scaled_derivs", "nrms_derivs") for d in range(3)])


def affine_inverse(values, coef):
    """``ScaleTransform._affine`` with coef [4][N] = (a, b - a, d - c, c), four separately rounded fp32 steps."""
    a, ba, dc, c = (np.asarray(coef[i], dtype=np.float32) for i in range(4))
    return (((np.asarray(values, dtype=np.float32) - a) / ba) * dc + c).astype(np.float32)


def shifted(truth, pred):
    """The IC-augmented prediction: step 0 is the truth's step 0, step t >= 1 the prediction's step t - 1."""
    return np.concatenate((truth[:, :1], pred[:, :-1]), axis=1)


def _derivatives(rows, dx):
    """u_x, u_xx, u_xxxx of fp32 rows [B, T, N], cast to fp64, as [3, B, T, N]."""
    b, t, n = rows.shape
    u = rows.astype(np.float64).reshape(b * t, n)
    _, ux, uxx, uxxxx = ko.rhs(u, np.zeros((b * t, n), dtype=np.float32), dx)
    return np.stack([ux, uxx, uxxxx]).reshape(3, b, t, n)


def row_stats(truth, pred, dx, objective="l2control", phi=None):
    """truth, pred fp32 [B, T, N] (already aligned), phi fp32 [B, T, N] or None -> fp64 [B, T, 18]."""
    s32, o32 = np.asarray(truth, dtype=np.float32), np.asarray(pred, dtype=np.float32)
    b, t, n = s32.shape
    e = (o32 - s32).astype(np.float64)                 # the fp32 difference, then widened
    s, o = s32.astype(np.float64), o32.astype(np.float64)
    out = np.empty((b, t, ROW_STATS))
    out[..., 0], out[..., 1] = np.abs(e).sum(-1), (e * e).sum(-1)
    out[..., 2], out[..., 3] = np.abs(s).sum(-1), (s * s).sum(-1)
    ds, dp = _derivatives(s32, dx), _derivatives(o32, dx)
    for side, (u, d) in enumerate(((s, ds), (o, dp))):
        if objective == "dissipation":
            p = np.zeros_like(u) if phi is None else np.asarray(phi, dtype=np.float32).astype(np.float64)
            out[..., 4 + side] = -1.0 * (((d[1] * d[1]).sum(-1) / n + (d[0] * d[0]).sum(-1) / n) + (u * p).sum(-1) / n)
        else:
            out[..., 4 + side] = ((-1.0) * (1.0 / n) * (u * u).sum(-1)).astype(np.float32).astype(np.float64)
    for k in range(3):
        diff = ds[k] - dp[k]
        out[..., 6 + 4 * k] = np.abs(diff).sum(-1)
        out[..., 7 + 4 * k] = (diff * diff).sum(-1)
        out[..., 8 + 4 * k] = np.abs(ds[k]).sum(-1)
        out[..., 9 + 4 * k] = (ds[k] * ds[k]).sum(-1)
    return out


def _row_mean_tables(st):
    """The five row-mean tables of sums (sum|e|, sum e^2, sum|s|, sum s^2) [B, T, 4] -> [5, T]."""
    e1, e2, r1, r2 = (st[..., j] for j in range(4))
    return np.stack([e1.mean(0), np.sqrt(e2).mean(0), (e1 / r1).mean(0), (np.sqrt(e2) / np.sqrt(r2)).mean(0),
                     (e2 / r2).mean(0)])


def fold(stats, n):
    """fp64 [B, T, 18] -> fp64 [1 + 25 T]: the MSE, then the tables of TABLE_NAMES, [T] each."""
    b, t, _ = stats.shape
    with np.errstate(divide="ignore", invalid="ignore"):
        state = _row_mean_tables(stats[..., 0:4])
        r, d = stats[..., 4], stats[..., 4] - stats[..., 5]
        e1, e2, r1, r2 = np.abs(d).sum(0), (d * d).sum(0), np.abs(r).sum(0), (r * r).sum(0)
        rews = np.stack([e1, np.sqrt(e2), e1 / r1, np.sqrt(e2) / np.sqrt(r2), e2 / r2])
        derivs = np.stack([_row_mean_tables(stats[..., 6 + 4 * k:10 + 4 * k]) for k in range(3)], axis=1)   # [5, 3, T]
    mse = stats[..., 1].sum() / (b * t * n)
    return np.concatenate([[mse], state.reshape(-1), rews.reshape(-1), derivs.reshape(-1)])


def named(values, t):
    out = {"MSE": values[0]}
    for k, name in enumerate(TABLE_NAMES):
        out[name] = values[1 + k * t:1 + (k + 1) * t]
    return out
