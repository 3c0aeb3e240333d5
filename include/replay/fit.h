/*
 * replay/fit.h -- the scaling fits of the offline surrogate evaluation, an entry of libreplay_hip.so (kernels:
 * csrc/replay.hip; binding: pdecontrol/mbrl/replay_hip.py, FIT_SYMBOLS; caller: pdecontrol/surrogates/evaluation/
 * evaluate.py: fit_scalings).  An extension of ../replay_hip.h, whose limits, conventions and rp_last_error() it uses
 * unchanged.
 *
 * A fold of the evaluation fits three Normalize transforms on its training rows: one on the observations, one on the
 * actions and one on the forced actions (the Gaussian forcing of the action, what the KS stepper adds to its right-hand
 * side).  rpn_moments reads the rows in place and reduces all three fields in ONE pass, by the launch scheme of
 * rpd_moments: partials per workgroup, above 32 workgroups a middle launch that adds each 32 consecutive partial rows in
 * index order, and a closing launch of one workgroup.  No floating-point atomics: at a given group count the result is the
 * same bit for bit from run to run.
 *
 * Row i is physical row rows[i] of `obs` ([slab_rows][N] fp32) and `actions` ([slab_rows][A] fp32); rows: DEVICE int64
 * [n], NULL for rows 0 ... n - 1.  Per listed row and column the kernel adds v and v * v in fp64 (the square of an fp32
 * value is exact there) of
 *   field 0  obs[row][j],                                   j < N
 *   field 1  actions[row][m],                               m < A
 *   field 2  forced[row][j] = sum over m of actions[row][m] * F[m][j], j < N, only with F ([A][N] fp32, NULL: no field 2):
 *            one rounded fp32 product and then one fmaf per further actuator in index order, row_ops.h's forcing_col,
 *            the chain the stepper, ro_act_chain and the window gather share.
 *
 * One wave per row, four rows of a wave in flight, four waves per workgroup, lanes along the columns: float4 loads where
 * N is above 192 and a multiple of four and obs and F are 16-byte aligned; narrower rows keep a lane per column.  The A
 * action columns sit in the first lanes of the first column tile.  Workgroup g of G takes the rows 16 g ... 16 g + 15,
 * 16 (g + G) ...; G = `groups` (at most RP_MAX_DELTA_GROUPS, above which it is clamped), or for groups = 0 the default
 * min(ceil(n / 16), RP_MAX_DELTA_GROUPS).
 *
 * Output layout, LD = N + A + 2 without F and 2 N + A + 3 with it: every field's columns are followed by its total over
 * the columns, added in column order:
 *   [0 ... N - 1] field 0, [N] its total, [N + 1 ... N + A] field 1, [N + A + 1] its total,
 *   [N + A + 2 ... 2 N + A + 1] field 2, [2 N + A + 2] its total.
 * sums:  fp64 [2][LD]: sum v and sum v * v.
 * stats: fp32 [2][LD]: mean = S / m and unbiased variance = (Q - S * S / m) / (m - 1), evaluated in fp64 and rounded
 *        once; m = n per column and n * width for a field's total; m < 2 gives a NaN variance.
 * A rows entry outside [0, slab_rows) reads nothing and makes every statistic NaN.
 *
 * Refusals, decided on the host before any HIP call: -90 NULL obs, actions, workspace, sums or stats, -91 n < 1, -92 a
 * slab without rows, -93 N outside 1 ... RP_MAX_OBS_DIM, -94 A outside 1 ... RP_MAX_ACT_DIM, -95 a negative group
 * count.  -100 launch failure.
 */
#ifndef REPLAY_FIT_H
#define REPLAY_FIT_H

#include "../replay_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int rpn_moments(void* stream, const float* obs, const float* actions, long slab_rows, int N, int A, const float* F,
                const long* rows, long n, int groups, double* workspace, double* sums, float* stats);

/* Doubles of the workspace rpn_moments needs for these arguments (forced: non-zero with F); 0 where it would refuse. */
long rpn_workspace_doubles(int N, int A, int forced, long n, int groups);

#ifdef __cplusplus
}
#endif

#endif
