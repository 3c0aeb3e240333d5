/*
 * replay_hip.h -- C ABI of libreplay_hip.so: the batch gather of the controller's policy-update phase on gfx950
 * (pdecontrol/mbrl/policy_phase.py: update_policy; kernel: csrc/replay.hip), and the append and the episode returns of
 * the device-resident replay of imagined experience (pdecontrol/mbrl/device_replay.py): `rp_append` places a rollout
 * round into the replay's slabs, `rp_episode_returns` sums the rewards of episodes for statistics().
 *
 * The controller samples its SAC batches from several replays at once (imagined and real transitions), each with its own
 * connector transform.  `rp_gather` assembles one batch in ONE launch: for each of B rows of the concatenated row space it
 * finds the source replay, reads that row of the source's packed tensors (DeviceSubSeqStore.tensors: obs, nxtobs
 * [rows][obs_width], actions [rows][act_width], rewards [rows] fp32, terminated [rows] bytes), applies the source's
 * sensor (output column j reads input column sensor_start + j * sensor_stride) and per-column affine maps, and writes the
 * flat fp32 buffers `sac_update` reads.
 *
 * The affine map of output column j with coefficients coef[0..3][j] = (a, b - a, d - c, c) is ScaleTransform._affine's
 *   out = ((v - a) / (b - a)) * (d - c) + c
 * as four separately rounded fp32 operations (round to nearest even, correctly rounded division, nothing contracted), so
 * the result equals the host transform's bit for bit.  A NULL coefficient pointer is the identity.
 *
 * One wave per sample, four per workgroup, lanes along the columns; float4 loads and stores where sensor_stride is 1 and
 * every row is 16-byte aligned.  A row outside [0, total rows) reads nothing and writes NaN to that sample.
 *
 * `rp_source` entries are HOST structs, read during the call and passed to the kernel by value; every pointer in them is
 * a DEVICE pointer.  In every entry the arguments are validated on the host before any device call and everything is
 * enqueued on `stream`: no host synchronisation, no device allocation.  Return 0 on success, negative on error
 * (rp_last_error()).  Plain vector stores, no scratch, no atomics; LDS only in rpd_moments and in rpn_moments
 * (replay/fit.h: the scaling fits of the offline evaluation), where the four waves of a workgroup add up their partial sums.
 */
#ifndef REPLAY_HIP_H
#define REPLAY_HIP_H

#include "replay/slabs.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RP_MAX_SOURCES 8
#define RP_MAX_OBS_DIM 1024
#define RP_MAX_ACT_DIM 16

typedef struct rp_source {
    const float* obs;                /* [rows][obs_width] */
    const float* actions;            /* [rows][act_width] */
    const float* nxtobs;             /* [rows][obs_width] */
    const float* rewards;            /* [rows] */
    const unsigned char* terminated; /* [rows], non-zero: terminated */
    long rows;
    int obs_width, act_width;        /* row widths of the packed tensors */
    int sensor_start, sensor_stride; /* observation columns: obs_dim = ceil((obs_width - sensor_start) / sensor_stride) */
    const float* obs_coef;           /* [4][obs_dim]: a, b - a, d - c, c per OUTPUT column; NULL: identity */
    const float* act_coef;           /* [4][act_width]; NULL: identity */
} rp_source;

/* Refusals: -1 no sources / too many, -2 NULL source array or NULL field pointer, -3 B < 1, -4 sensor stride < 1,
 * -5 sensor start outside the row, -6 action width outside 1 ... RP_MAX_ACT_DIM, -7 observation width outside
 * 1 ... RP_MAX_OBS_DIM columns, -8 sources that disagree on obs_dim or act_width, -9 a source without rows.
 * 0 when rp_gather runs these sources. */
int rp_supported(int nsrc, const rp_source* srcs, int B);

/* rows: DEVICE int64 [B], rows of the concatenation of the sources in `srcs` order.
 * obs, nxtobs [B][obs_dim]; actions [B][act_width]; rewards, terminated [B] (terminated as 0.0f / 1.0f). */
int rp_gather(void* stream, int nsrc, const rp_source* srcs, int B, const long* rows, float* obs, float* actions,
              float* nxtobs, float* rewards, float* terminated);

/* The slabs of a DeviceExperienceReplay (replay/slabs.h): a HOST struct of DEVICE pointers, read during the call. */
typedef replay_slabs rp_slab;

/* Places one rollout round into the slabs in ONE launch.  `block` is the round block of the imagined-rollout phase as it
 * lies in HBM, laid out for T_cap steps: traj [T_cap + 1][B][N] | actions [T_cap][B][A] | rewards [T_cap][B] | steps
 * [T_cap][B] (int32); the first T steps of it are placed.  Transition (t, b) writes row dst[t][b] of the slabs:
 * obs = traj[t][b], nxtobs = traj[t + 1][b], the action, reward and steps of (t, b), terminated = 0,
 * truncated = (t == T - 1).  A negative dst entry writes nothing.
 * dst: DEVICE int64 [T][B]; dst_host: the HOST copy it was uploaded from, validated before the launch: every entry is
 * below slab->rows and no row appears twice.  One wave per transition, four per workgroup, lanes along the columns; float4
 * where the width is a multiple of four and every base is 16-byte aligned.
 * Refusals: -30 NULL block, dst, dst_host, slab or slab field, -31 T < 1 or T > T_cap, -32 B < 1, -33 N outside
 * 1 ... RP_MAX_OBS_DIM, -34 A outside 1 ... RP_MAX_ACT_DIM, -35 a slab without rows, -36 a dst entry beyond the slab,
 * -37 a row named twice, -40 launch failure. */
int rp_append(void* stream, const float* block, int T, int T_cap, int B, int N, int A, const long* dst, const long* dst_host,
              const rp_slab* slab);

/* returns[e] = the fp32 sum of rewards[rows[offsets[e]]], ..., rewards[rows[offsets[e + 1] - 1]] in that order, starting
 * from 0.0f: a sequential chain of correctly rounded fp32 additions, one lane per episode, which is Python's sum() over
 * the fp32 reward array bit for bit.  rewards: the slab's [slab_rows]; rows: DEVICE int64 [nrows]; offsets: DEVICE int64
 * [E + 1], ascending from 0 to nrows.  A row outside the slab or an offset outside rows makes that return NaN.
 * Refusals: -50 NULL pointer, -51 E < 1, -52 nrows < 1 or slab_rows < 1, -60 launch failure. */
int rp_episode_returns(void* stream, const float* rewards, long slab_rows, const long* rows, long nrows, const long* offsets,
                       int E, float* returns);

/* The moments of the scaled state changes of `n` transitions, read from the slabs in place (the controller's
 * update_delta_transform, pdecontrol/mbrl/delta_phase.py).  Row i is physical row rows[i] of `obs` and `nxtobs`
 * ([slab_rows][obs_width] fp32); rows: DEVICE int64 [n], NULL for rows 0 ... n - 1.  Output column j of obs_dim =
 * ceil((obs_width - sensor_start) / sensor_stride) reads input column sensor_start + j * sensor_stride:
 *   d[i][j] = (affine_j(nxtobs) - affine_j(obs)) / delta
 * with the affine map of rp_gather (obs_coef [4][obs_dim], NULL: identity) and then one correctly rounded fp32
 * subtraction and one correctly rounded fp32 DIVISION by `delta` (not a multiplication by its reciprocal).
 *
 * Sum d and sum d * d are accumulated per column in fp64.  One wave per row, four rows of a wave in flight, four waves per
 * workgroup, lanes along the columns: float4 loads where there are more than 192 columns, sensor_stride is 1, obs_width
 * and sensor_start are multiples of four and obs, nxtobs and obs_coef are 16-byte aligned; narrower rows keep a lane per
 * column.  Workgroup g of G takes the rows 16 g ... 16 g + 15, 16 (g + G) ..., and writes its partial pair to row g of
 * `workspace`.  Above 32 workgroups a middle launch adds each 32 consecutive partial rows in index order; a closing
 * launch of one workgroup adds what is left in index order.  No floating-point atomics: at a given G the result is the
 * same bit for bit from run to run.  G = `groups` (at most RP_MAX_DELTA_GROUPS, above which it is clamped), or for
 * groups = 0 the default min(ceil(n / 16), RP_MAX_DELTA_GROUPS).
 *
 * sums:  fp64 [2][obs_dim + 1]: sum d and sum d * d per column; entry obs_dim is the total over the columns, added in
 *        column order.
 * stats: fp32 [2][obs_dim + 1]: mean = S / m and unbiased variance = (Q - S * S / m) / (m - 1), evaluated in fp64 and
 *        rounded once; m = n per column and n * obs_dim for the aggregate; m < 2 gives a NaN variance.
 * A rows entry outside [0, slab_rows) reads nothing and makes every statistic NaN.
 * Refusals: -70 NULL obs, nxtobs, workspace, sums or stats, -71 n < 1, -72 a slab without rows, -73 sensor stride < 1,
 * -74 sensor start outside the row, -75 more than RP_MAX_OBS_DIM output columns, -76 delta zero or not finite,
 * -77 a negative group count, -80 launch failure.
 *
 * The two entries carry the prefix rpd_: they are bound by a table of their own (replay_hip.DELTA_SYMBOLS), beside the
 * rp_ entries above and their table, and report through rp_last_error(). */
#define RP_MAX_DELTA_GROUPS 2048
int rpd_moments(void* stream, const float* obs, const float* nxtobs, long slab_rows, int obs_width, int sensor_start,
                int sensor_stride, const float* obs_coef, const long* rows, long n, float delta, int groups,
                double* workspace, double* sums, float* stats);

/* Doubles of the workspace rpd_moments needs for these arguments; 0 where it would refuse them. */
long rpd_workspace_doubles(int obs_dim, long n, int groups);

const char* rp_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
