/*
 * kspde.h -- C ABI of libkspde.so: the MI355X (gfx950) batched Kuramoto-Sivashinsky stepper.
 *
 * This is the drop-in boundary for the reference's KS hot path.  The reference
 * (stwerner97/model-based-pde-control) is pure Python and has no FFI of its own; each entry
 * point below names the reference interface it replaces (paths relative to the reference
 * root).  The Python side (model-based-pde-control_amd/kspde, ctypes) binds exactly these
 * symbols; INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C linkage, plain pointers and sizes; no C++/torch types cross this boundary
 *   - every function returns KS_OK (0) or a negative ks_status code; the message of the last
 *     failure on the calling thread is available from ks_last_error()
 *   - a handle owns its device buffers and (unless ks_set_stream was called) its HIP stream;
 *     a handle is not re-entrant; distinct handles (e.g. one per GPU) may be driven from
 *     distinct host threads
 *   - "host" pointers are ordinary host memory owned by the caller; the *_device variants
 *     take device pointers, enqueue on the handle's stream and do NOT synchronise
 *   - device >= 0 names a HIP device; nothing ever falls back to the CPU.  device = -1 is an EXPLICIT request for
 *     the CPU twin (csrc/ks_cpu.cpp: the same arithmetic on host memory, same entry points; BASELINE configs[0],
 *     SURVEY 8(b) b4 / 8(d) baseline (B)); on such a handle the *_device entries take host pointers and run
 *     synchronously, ks_set_stream / a non-auto ks_set_variant return KS_ERR_UNSUPPORTED
 *
 * State layout in HBM: u is fp64, row-major [num_envs, N] (one env = one contiguous row of
 * N doubles); phi / obs are fp32 [num_envs, N]; actions fp32 [num_envs, n_act];
 * forcing matrix F fp32 [n_act, N].
 */
#ifndef KSPDE_H
#define KSPDE_H

#include "replay/slabs.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ks_handle ks_handle;

typedef enum ks_status {
    KS_OK = 0,
    KS_ERR_INVALID = -1,     /* bad argument (NULL handle, N unsupported, ...)       */
    KS_ERR_HIP = -2,         /* a HIP runtime call failed (message has the detail)   */
    KS_ERR_NO_DEVICE = -3,   /* no such HIP device                                   */
    KS_ERR_UNSUPPORTED = -4, /* feature not available for this N / layout            */
    KS_ERR_SELFTEST = -5     /* ks_selftest found a mismatching primitive            */
} ks_status;

/* Arithmetic mode of the fused stepper.
 *   KS_MODE_FAST  : merged 9-point linear stencil, FMA everywhere, reward reduced once per
 *                   call.  Differs from the reference by rounding only (<= 1e-12 per sub-step;
 *                   the contract is L_inf < 1e-9 per sub-step).
 *   KS_MODE_EXACT : the reference's operation order (scipy correlate1d summation order,
 *                   true divisions, no FMA contraction).  State is bit-identical to the
 *                   reference CPU stepper.  ~3-4x slower; used as the parity anchor. */
typedef enum ks_mode { KS_MODE_FAST = 0, KS_MODE_EXACT = 1 } ks_mode;

/* Reward objective of the step entries (kuramoto.py:64-73): what the per-env accumulator ssq_sum collects.
 *   KS_OBJECTIVE_L2CONTROL   : sum_i u_i^2                                   (reward -(1/N) ||u||^2)
 *   KS_OBJECTIVE_DISSIPATION : sum_i (u_xx,i^2 + u_x,i^2 + u_i * phi_i)      (reward -(mean(u_xx^2) + mean(u_x^2)
 *                              + mean(u * phi))), u_x the upwind derivative of u^2 that rhs forms (ks_rhs's ux),
 *                              u_xx the 7-point second derivative, phi the fp32 forcing widened to fp64.
 * Either way the reward of a step is -(1/N) * ssq_sum / cfg_steps, every term taken at the pre-update state of each
 * sub-step.  The reference selects dissipation only for a falsy objective string. */
typedef enum ks_objective { KS_OBJECTIVE_L2CONTROL = 0, KS_OBJECTIVE_DISSIPATION = 1 } ks_objective;

/* Kernel layout / halo-exchange variant.  KS_VARIANT_AUTO picks per (N, num_envs). */
typedef enum ks_variant {
    KS_VARIANT_AUTO = 0,
    KS_VARIANT_ROW16_DPP = 1,  /* env = 16 lanes x N/16 points, halo by DPP row_ror          */
    KS_VARIANT_ROW16_BPERM = 2,/* same layout, halo by ds_bpermute                            */
    KS_VARIANT_WAVE64_DPP = 3, /* env = 64 lanes x N/64 points, halo by DPP wave_ror/rol:1    */
    KS_VARIANT_WAVE64_BPERM = 4,/* same layout, halo by ds_bpermute                           */
    KS_VARIANT_HALF32_BPERM = 5,/* env = 32 lanes x N/32 points, halo by ds_bpermute          */
    KS_VARIANT_LDS = 6,        /* one workgroup per env, state staged in LDS; any 9 <= N <= 2048 */
    KS_VARIANT_WAVE64_HYBRID = 7, /* N = 64: env = one wavefront, halo +-1, +-2 by DPP wave_ror/rol, +-3, +-4 by ds_bpermute */
    KS_VARIANT_WAVE64_HYBRID1 = 8 /* N = 64: halo +-1..+-3 by the DPP chain, +-4 by ds_bpermute */
} ks_variant;

/* ---- lifetime -------------------------------------------------------------------------- */

/* Replaces: KuramotoSivashinskyEnv.__init__ (pdegym/kuramoto/kuramoto.py:29-57) for a batch of
 * num_envs independent environments: grid size N, domain length L (dx = L/N), RK4 step dt.
 * device: HIP device ordinal, or -1 for the CPU twin. */
int ks_create(int device, int num_envs, int N, double L, double dt, ks_handle** out);
int ks_destroy(ks_handle* h);

/* Run on a caller-provided hipStream_t (e.g. torch's current stream) instead of the handle's own. */
int ks_set_stream(ks_handle* h, void* hip_stream);
int ks_set_mode(ks_handle* h, int mode /* ks_mode */);
/* Handle state like the mode: applies to every step entry (ks_step, _actions, _rows, _begin/_end, _device).  Default
 * KS_OBJECTIVE_L2CONTROL.  A step that is given no reward buffer runs the l2control kernels whatever the objective.
 * KS_VARIANT_WAVE64_HYBRID / HYBRID1 have no dissipation form: a step with a reward buffer returns KS_ERR_UNSUPPORTED. */
int ks_set_objective(ks_handle* h, int objective /* ks_objective */);
int ks_set_variant(ks_handle* h, int variant /* ks_variant */);
/* Threads per workgroup of the fused kernels (64, 128 or 256; 0 = default). */
int ks_set_block_size(ks_handle* h, int threads);
/* Reports the layout the next ks_step will use. */
int ks_get_layout(ks_handle* h, int* variant, int* lanes_per_env, int* points_per_lane,
                  int* block_threads, int* grid_blocks);

/* ---- forcing ----------------------------------------------------------------------------- */

/* Replaces: GaussianForcing.forcing, the fp32 [n_act, N] matrix built in
 * pdegym/common/transforms.py:256-260.  The host computes it once (same torch ops as the
 * reference) and uploads it; ks_step_actions then evaluates phi = actions @ F on the device as
 * the fp32 FMA chain a0*F0 (+) a1*F1 (+) ... that torch's CPU matmul uses (transforms.py:262-265). */
int ks_set_forcing(ks_handle* h, const float* F_host, int n_act);

/* ---- state ------------------------------------------------------------------------------- */

/* Replaces: assignment to KuramotoSivashinskyEnv.u (kuramoto.py:106) / reading it (:94). */
int ks_set_state(ks_handle* h, const double* u_host /* [num_envs, N] */);
int ks_get_state(ks_handle* h, double* u_host /* [num_envs, N] */);
/* Scatter n rows: row i of u_host goes to env env_ids[i] (masked reset of finished episodes). */
int ks_set_state_rows(ks_handle* h, const int* env_ids_host, int n, const double* u_host /* [n, N] */);
/* Device pointer of the [num_envs, N] fp64 state (for zero-copy consumers). */
int ks_state_device_ptr(ks_handle* h, double** d_u);

/* ---- the hot path ------------------------------------------------------------------------ */

/* Replaces: the loop body of KuramotoSivashinskyEnv.step (kuramoto.py:83-90) run n_substeps
 * times for every env: reward term, then one classical RK4 update of u' = rhs(u, phi).
 *   phi_host   fp32 [num_envs, N] forcing field, or NULL for phi = 0 (reset burn-in, :108-109)
 *   obs_f32    out, fp32 [num_envs, N] copy of the new state (gym observation dtype), or NULL
 *   ssq_sum    out, fp64 [num_envs]: the reward accumulator, summed over the n_substeps and taken
 *              BEFORE each update -- sum_i u_i^2 under KS_OBJECTIVE_L2CONTROL, sum_i (u_xx,i^2 +
 *              u_x,i^2 + u_i phi_i) under KS_OBJECTIVE_DISSIPATION (ks_objective); the reward of
 *              kuramoto.py:64-73,84,96 is -(1/N) * ssq_sum / cfg_steps either way.  May be NULL.
 *   status     out, int [num_envs]: 1 if the env's state is non-finite after the call (the
 *              reference raises FloatingPointError via np.seterr(over="raise"), kuramoto.py:12).
 * Synchronous: results are in the host buffers on return. */
int ks_step(ks_handle* h, const float* phi_host, long n_substeps, float* obs_f32, double* ssq_sum,
            int* status);

/* Same, with phi computed on the device from actions [num_envs, n_act] and the uploaded forcing
 * matrix.  Replaces kuramoto.py:79-80 + :83-90. */
int ks_step_actions(ks_handle* h, const float* actions_host, long n_substeps, float* obs_f32,
                    double* ssq_sum, int* status);

/* Step only the n envs listed in env_ids_host with phi = 0 (burn-in of freshly reset envs,
 * kuramoto.py:103-109: Tsteps * cfg_steps sub-steps).  Outputs are indexed by position i. */
int ks_step_rows(ks_handle* h, const int* env_ids_host, int n, long n_substeps, float* obs_f32,
                 double* ssq_sum, int* status);

/* Split form of the host-boundary step, for ONE host thread driving several handles (one per GPU; replaces the
 * reference's one-subprocess-per-env AsyncVectorEnv.step_async / step_wait, pdecontrol/mbrl/mbrl.py:81-86):
 * ks_step_begin stages its inputs through pinned memory, enqueues the launch and the copy of the outputs into the
 * handle's pinned mirror, and returns WITHOUT waiting; ks_step_end waits for that step and hands the results over.
 * Call begin on every handle first, then end on every handle: all devices run concurrently.
 *   actions_host  fp32 [num_envs, n_act] or NULL (phi = 0)
 *   env_ids_host  int [n_rows] subset (outputs then in list order, as ks_step_rows) or NULL = all envs
 *   want_obs      0: ks_step_end may only be given obs_f32 = NULL
 * Between begin and end the handle accepts no other call that touches the stream (KS_ERR_INVALID). */
int ks_step_begin(ks_handle* h, const float* actions_host, const int* env_ids_host, int n_rows, long n_substeps,
                  int want_obs);
int ks_step_end(ks_handle* h, float* obs_f32, double* ssq_sum, int* status);

/* Asynchronous, device-resident form: every pointer is a DEVICE pointer (or NULL), the launch is
 * enqueued on the handle's stream and the call returns immediately.  Exactly one of d_phi /
 * d_actions may be non-NULL (both NULL: phi = 0).  d_env_ids (int [n_rows]) selects a subset of
 * envs, NULL = all num_envs (then n_rows is ignored); outputs are indexed by env id. */
int ks_step_device(ks_handle* h, const float* d_phi, const float* d_actions, const int* d_env_ids,
                   int n_rows, long n_substeps, float* d_obs_f32, double* d_ssq_sum, int* d_status);
int ks_sync(ks_handle* h);

/* Replaces: reward_func evaluated sample by sample over a batch of observations (pdecontrol/mbrl/world/world.py:170,
 * kuramoto.py:64-70) -- the world model's per-row reward.  d_obs fp32 [n_rows, N], d_phi fp32 [n_rows, N] (NULL = 0),
 * d_reward fp64 [n_rows] out: -(mean(u_xx^2) + mean(u_x^2) + mean(u * phi)) per row for KS_OBJECTIVE_DISSIPATION, in
 * fp64 with the reference's stencil order; -(1/N) sum u^2 for KS_OBJECTIVE_L2CONTROL.  Uses the handle's N and dx,
 * not its state.  Enqueued on the handle's stream; on the CPU twin host pointers, synchronous. */
int ks_reward_rows_device(ks_handle* h, int objective, const float* d_obs, const float* d_phi, int n_rows,
                          double* d_reward);

/* Replaces: KSBatchedVecEnv._finish_step + Sample.split + ExperienceReplay.add (pdecontrol/mbrl/types.py,
 * pdecontrol/mbrl/replay.py) for the T * num_envs transitions of T consecutive steps without a truncation, read where
 * ks_step_device left its outputs and written as rows of a device-resident replay.  ks_record is a HOST struct of DEVICE
 * pointers, the seven slabs: obs / nxtobs fp32 [rows, N], actions fp32 [rows, A], rewards fp32 [rows], terminated /
 * truncated bytes [rows], steps int [rows].  Transition (t, e) writes row d_dst[t][e] (a negative entry writes nothing):
 * obs = traj[t][e], nxtobs = traj[t + 1][e], the action and steps of (t, e), terminated = truncated = 0 and
 * rewards = (float)((c * ssq[t][e]) / (double)n_substeps), c = -1.0 * (1.0 / (double)N): numpy's
 * (-1.0) * (1 / N) * ssq / cfg_steps cast to fp32, bit for bit.  dst_host is d_dst on the host: every refusal (NULL
 * pointers, T < 1, A outside 1 ... 16, n_substeps < 1, slabs without rows, an entry >= rows, a row named twice) is made
 * from it before any HIP call.  Enqueued on the handle's stream; it does not synchronise and does not allocate device
 * memory.  On the CPU twin host pointers, synchronous. */
typedef replay_slabs ks_record;                 /* replay/slabs.h */

int ks_record_device(ks_handle* h, const float* d_traj /* [T+1][E][N] */, const float* d_actions /* [T][E][A] */, int A,
                     const double* d_ssq /* [T][E] */, const int* d_steps /* [T][E] */, int T, long n_substeps,
                     const long* d_dst /* [T][E] */, const long* dst_host, const ks_record* out);

/* ---- surrogate test phase -------------------------------------------------------------------- */

/* Replaces: the metric section of PDETrainingModule.test_step (pdecontrol/surrogates/training.py:195-243) for a batch of
 * B sequences of T steps -- 2 * B * T reward_func calls, 2 * B * T env.rhs calls and some forty torch reductions -- by
 * two launches.  Both follow ks_reward_rows_device: the handle's N and dx, not its state; enqueued on the handle's
 * stream; on the CPU twin host pointers, synchronous, plain C++.  Every argument error is refused on the host before
 * any HIP call, with a message that starts with the function's name. */
#define KS_EVAL_ROW_STATS 18
#define KS_EVAL_TABLES    25          /* per-time-step tables; + 1 scalar (MSE) */

typedef struct ks_eval_batch {
    const float* truth;  long truth_bstride, truth_tstride;   /* [B][T][N] through element strides            */
    const float* pred;   long pred_bstride,  pred_tstride;    /* prediction rows, batch- or time-major         */
    int pred_shift;      /* 1: predicted row of (b, 0) is truth (b, 0), of (b, t >= 1) is pred (b, t-1)       */
    const float* phi;    /* [B][T][N] contiguous fp32 forcing field, or NULL (read under dissipation only)    */
    int inv_kind;        /* 0 identity; 1 four-step affine, coef [4][N] = (a, b-a, d-c, c); 2 mul-add [2][N]  */
    const float* inv_coef;
    float* truth_out;    /* [B][T][N] contiguous: the inverse-scaled rows as the metrics read them, or NULL   */
    float* pred_out;
} ks_eval_batch;

/* Per (b, t) row, with s the truth row and o the predicted row after stransf.otransf.Inverse (inv_kind, in separately
 * rounded fp32 steps: kind 1 ScaleTransform._affine, kind 2 Normalize._inv with coef = (sqrt(var + epsilon), mean)) and
 * e_i = (float)(o_i - s_i), 18 fp64 values (sums in fp64):
 *   0-3    sum|e|, sum e^2, sum|s|, sum s^2
 *   4, 5   the reward of s and of o as ks_reward_rows_device forms it (phi enters both under KS_OBJECTIVE_DISSIPATION and
 *          is not read under KS_OBJECTIVE_L2CONTROL, where the reward is rounded to fp32, the reference's precision there)
 *   6-17   for u_x, u_xx, u_xxxx of the fp64-cast rows (reference operation order, ds of s, do of o):
 *          sum|ds - do|, sum (ds - do)^2, sum|ds|, sum ds^2
 * With pred_shift = 1 both sides of step 0 read the same value through the same map: its error sums are exactly 0. */
int ks_eval_rows_device(ks_handle* h, int objective, const ks_eval_batch* in, int B, int T, double* rowstats /* [B][T][18] */);

/* tables[0] = MSE = sum_{b,t} sum e^2 / (B T N); tables[1 + k T + t] = table k at step t, k in the order of the dict
 * test_step returns: l1_loss, l2_loss, l1_loss_scaled, l2_loss_scaled, nrmse (means over b of sum|e|, sqrt(sum e^2),
 * sum|e| / sum|s|, sqrt(sum e^2) / sqrt(sum s^2), sum e^2 / sum s^2); the five *_rews (norms over the batch: sum_b|r - r^|,
 * sqrt(sum_b (r - r^)^2), their ratios to sum_b|r| and sqrt(sum_b r^2), sum_b (r - r^)^2 / sum_b r^2); then the five
 * row-mean tables of each derivative as l1_loss_derivs-derivative-0, -1, -2, l2_loss_derivs-..., l1_loss_scaled_derivs-...,
 * l2_loss_scaled_derivs-..., nrms_derivs-....  One thread per value, b in index order, fp64; a zero norm divides to
 * IEEE inf / NaN as in the reference.  accum (same shape, or NULL): accum[i] += B * tables[i] by the same thread, so the
 * batches of an epoch on one stream sum deterministically. */
int ks_eval_fold_device(ks_handle* h, const double* rowstats, int B, int T,
                        double* tables /* [1 + 25*T] */, double* accum /* same shape: += B * value; or NULL */);

/* ---- test hooks -------------------------------------------------------------------------- */

/* Replaces: KuramotoSivashinskyEnv.rhs (kuramoto.py:118-129) on a batch, in the reference's
 * operation order.  All buffers host, [n_rows, N]; any of ux/uxx/uxxxx may be NULL.
 * Does not touch the handle's state. */
int ks_rhs(ks_handle* h, const double* u_host, const float* phi_host, int n_rows, double* rhs,
           double* ux, double* uxx, double* uxxxx);

/* Runs every cross-lane primitive the fused kernels rely on (DPP row_ror, wave_ror/rol,
 * ds_bpermute) on lane ids and checks the result against the definition.  failed_mask gets one
 * bit per ks_variant value whose primitive misbehaved. */
int ks_selftest(ks_handle* h, unsigned* failed_mask);

const char* ks_last_error(void);
const char* ks_version(void);

#ifdef __cplusplus
}
#endif
#endif /* KSPDE_H */
