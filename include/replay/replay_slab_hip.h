/*
 * replay_slab_hip.h -- the second half of the C ABI of libreplay_hip.so (first half: include/replay_hip.h): what the
 * device-resident replay of imagined experience (pdecontrol/mbrl/device_replay.py) runs on gfx950.  `rp_append` places a
 * rollout round into the replay's slabs, `rp_episode_returns` sums the rewards of episodes for statistics().
 * Kernels: csrc/replay.hip; binding: pdecontrol/mbrl/replay_hip.py (SLAB_SYMBOLS).
 *
 * As for rp_gather: arguments are validated on the host before any device call, everything is enqueued on `stream`, no
 * host synchronisation, no device allocation; 0 on success, negative on error (rp_last_error()).  Plain vector stores,
 * no LDS, no scratch, no atomics.
 */
#ifndef REPLAY_SLAB_HIP_H
#define REPLAY_SLAB_HIP_H

#include "../replay_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The slabs of a DeviceExperienceReplay: one tensor per field in DeviceSubSeqStore.tensors dtypes, `rows` rows each.
 * A HOST struct of DEVICE pointers, read during the call. */
typedef struct rp_slab {
    float* obs;                      /* [rows][N] */
    float* actions;                  /* [rows][A] */
    float* nxtobs;                   /* [rows][N] */
    float* rewards;                  /* [rows] */
    unsigned char* terminated;       /* [rows] */
    unsigned char* truncated;        /* [rows] */
    int* steps;                      /* [rows] */
    long rows;
} rp_slab;

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

#ifdef __cplusplus
}
#endif

#endif
