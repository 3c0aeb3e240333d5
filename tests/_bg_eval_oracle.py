"""The metric section of ``PDETrainingModule.test_step`` on a Burgers env restated in fp64 numpy: the yardstick of the
``bg_eval_rows`` / ``bg_eval_fold`` / ``bg_derivatives`` tests.  Derivatives come from ``oracle.burgers_oracle.grad`` /
``laplace`` with ``dtype=np.float64`` (which shares nothing with csrc/); nothing here is ever compared with its own output.

``row_stats`` takes the rows as the metrics read them (inverse-scaled, the prediction aligned with the truth) and returns
the 14 sums per row of include/burgers/eval.h; ``fold`` turns them into the MSE and the 20 per-step tables in the order
of the dict ``test_step`` returns.  Sums are fp64 throughout; the error is the fp32 difference the host lines form; the
l2control reward is rounded to fp32, the precision the env's ``reward_func`` has there.

``cases`` builds the inputs the tests share: white-noise truth rows (a wrong or shifted tap is visible and the stencils
do not cancel) and predictions 3 % off."""
import numpy as np

from oracle import burgers_oracle as bo

ROW_STATS, TABLES = 14, 20
TABLE_NAMES = (["l1_loss", "l2_loss", "l1_loss_scaled", "l2_loss_scaled", "nrmse"]
               + ["l1_loss_rews", "l2_loss_rews", "l1_loss_scaled_rews", "l2_loss_scaled_rews", "nrmse_rews"]
               + [f"{name}-derivative-{d}" for name in ("l1_loss_derivs", "l2_loss_derivs", "l1_loss_scaled_derivs",
                                                        "l2_loss_scaled_derivs", "nrms_derivs") for d in range(2)])
# (N, B, T): each lane-group width (16 up to N = 64, 32 up to 512, 64 above), an N that is no multiple of its width, last
# workgroups that are not full (21 and 17 rows) and the smallest N
SHAPES = [(64, 3, 7), (100, 3, 7), (256, 2, 5), (1024, 2, 3), (48, 17, 1), (5, 2, 2)]
L = 2 * np.pi


def affine_inverse(values, coef):
    """``ScaleTransform._affine`` with coef [4][N] = (a, b - a, d - c, c), four separately rounded fp32 steps."""
    a, ba, dc, c = (np.asarray(coef[i], dtype=np.float32) for i in range(4))
    return (((np.asarray(values, dtype=np.float32) - a) / ba) * dc + c).astype(np.float32)


def normalize_inverse(values, coef):
    """``Normalize._inv`` with coef [2][N] = (s, m), two separately rounded fp32 steps."""
    s, m = (np.asarray(coef[i], dtype=np.float32) for i in range(2))
    return (np.asarray(values, dtype=np.float32) * s + m).astype(np.float32)


def shifted(truth, pred):
    """The IC-augmented prediction: step 0 is the truth's step 0, step t >= 1 the prediction's step t - 1."""
    return np.concatenate((truth[:, :1], pred[:, :-1]), axis=1)


def derivatives(rows, dx):
    """u_x, u_xx of fp32 rows [..., N], taken in fp64 from the widened values, as [2, ..., N]."""
    u = np.asarray(rows, dtype=np.float32).astype(np.float64)
    return np.stack([bo.grad(u, dx, dtype=np.float64), bo.laplace(u, dx, dtype=np.float64)])


def row_stats(truth, pred, dx):
    """truth, pred fp32 [B, T, N] (already aligned and inverse-scaled) -> fp64 [B, T, 14]."""
    s32, o32 = np.asarray(truth, dtype=np.float32), np.asarray(pred, dtype=np.float32)
    b, t, n = s32.shape
    e = (o32 - s32).astype(np.float64)                 # the fp32 difference, then widened
    s, o = s32.astype(np.float64), o32.astype(np.float64)
    out = np.empty((b, t, ROW_STATS))
    out[..., 0], out[..., 1] = np.abs(e).sum(-1), (e * e).sum(-1)
    out[..., 2], out[..., 3] = np.abs(s).sum(-1), (s * s).sum(-1)
    for side, u in enumerate((s, o)):
        out[..., 4 + side] = ((-1.0) * (1.0 / n) * (u * u).sum(-1)).astype(np.float32).astype(np.float64)
    ds, dp = derivatives(s32, dx), derivatives(o32, dx)
    for k in range(2):
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
    """fp64 [B, T, 14] -> fp64 [1 + 20 T]: the MSE, then the tables of TABLE_NAMES, [T] each."""
    b, t, _ = stats.shape
    with np.errstate(divide="ignore", invalid="ignore"):
        state = _row_mean_tables(stats[..., 0:4])
        r, d = stats[..., 4], stats[..., 4] - stats[..., 5]
        e1, e2, r1, r2 = np.abs(d).sum(0), (d * d).sum(0), np.abs(r).sum(0), (r * r).sum(0)
        rews = np.stack([e1, np.sqrt(e2), e1 / r1, np.sqrt(e2) / np.sqrt(r2), e2 / r2])
        derivs = np.stack([_row_mean_tables(stats[..., 6 + 4 * k:10 + 4 * k]) for k in range(2)], axis=1)   # [5, 2, T]
    mse = stats[..., 1].sum() / (b * t * n)
    return np.concatenate([[mse], state.reshape(-1), rews.reshape(-1), derivs.reshape(-1)])


def named(values, t):
    out = {"MSE": values[0]}
    for k, name in enumerate(TABLE_NAMES):
        out[name] = values[1 + k * t:1 + (k + 1) * t]
    return out


def noise_rows(n, b, t, seed=0):
    """(truth, pred) fp32 [B, T, N]: seeded white noise in (-1, 1) and truth * (1 + 0.03 g) + 0.01 g'."""
    rs = np.random.RandomState(seed + 7 * n + b)
    truth = rs.uniform(-1.0, 1.0, (b, t, n)).astype(np.float32)
    pred = (truth * (1.0 + 0.03 * rs.standard_normal((b, t, n))) + 0.01 * rs.standard_normal((b, t, n))).astype(np.float32)
    return truth, pred


def affine_coef(n, seed=1):
    """A non-trivial kind-1 map, coef [4][N] = (a, b - a, d - c, c), different in every column."""
    rs = np.random.RandomState(seed + n)
    a, b = rs.uniform(-1.5, -1.0, n), rs.uniform(1.0, 1.5, n)
    c, d = rs.uniform(-3.0, -2.0, n), rs.uniform(2.0, 3.0, n)
    return np.stack([a, b - a, d - c, c]).astype(np.float32)


def normalize_coef(n, seed=2):
    """A kind-2 map, coef [2][N] = (s, m)."""
    rs = np.random.RandomState(seed + n)
    return np.stack([rs.uniform(0.5, 2.0, n), rs.uniform(-0.5, 0.5, n)]).astype(np.float32)


_CASES = {}


def case(shape):
    """The shared case of one (N, B, T): scaled truth and prediction rows, the kind-1 coefficients, the prediction in
    time-major storage to be read with ``pred_shift``, and the yardstick's row stats and fold.  Built once, never written."""
    if shape not in _CASES:
        n, b, t = shape
        truth, pred = noise_rows(n, b, t)
        coef = affine_coef(n)
        dx = L / n
        s, o = affine_inverse(truth, coef), affine_inverse(shifted(truth, pred), coef)
        stats = row_stats(s, o, dx)
        c = dict(n=n, b=b, t=t, dx=dx, truth=truth, pred=pred, coef=coef, pred_tm=np.ascontiguousarray(pred.transpose(1, 0, 2)),
                 s=s, o=o, stats=stats, tables=fold(stats, n))
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CASES[shape] = c
    return _CASES[shape]
