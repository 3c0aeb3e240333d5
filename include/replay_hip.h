/*
 * replay_hip.h -- C ABI of libreplay_hip.so: the batch gather of the controller's policy-update phase on gfx950
 * (pdecontrol/mbrl/policy_phase.py: update_policy; kernel: csrc/replay.hip).  The same library exports the append and
 * the episode returns of the device-resident replay: include/replay/replay_slab_hip.h.
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
 * a DEVICE pointer.  Everything is enqueued on `stream`: no host synchronisation, no device allocation.  Return 0 on
 * success, negative on error (rp_last_error()).
 */
#ifndef REPLAY_HIP_H
#define REPLAY_HIP_H

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

const char* rp_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
