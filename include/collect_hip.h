/*
 * collect_hip.h -- C ABI of libcollect_hip.so: the kernels that keep the real-env collection loop of the controller in
 * HBM on gfx950 (pdecontrol/mbrl/collection_phase.py: collect; kernels: csrc/collect.hip).
 *
 * One collected step is the eager chain  sac_policy_forward -> co_act -> ks_step_device -> co_observe.  The KS stepper
 * writes its observations straight into the trajectory slot traj[t + 1]; the two entries here replace what the wrapper
 * stack does on the host around the stepper:
 *
 *   co_act       the action side.  Reads the policy's action [E][A], maps it per column through an optional affine map
 *                (the frozen TransformActionWrapper), writes the result to the stepper's action buffer [E][A] and records
 *                in actions[t][e][:] what the stack's action store holds: the env-side action when the store sits below
 *                the scaling (the controller's real stack), the raw action (record_raw = 1) when it sits on top.
 *   co_observe   the observation side.  Copies nothing: traj[t + 1] is read only.  With update = 1 it first takes the
 *                minimum and maximum over the whole [E][N] block and joins them with the running bounds (ScaleTransform
 *                .update with scalar vmin / vmax: an unset bound, -inf or +inf, gives way to the block's extremum; a NaN
 *                propagates as torch.minimum's does), then writes
 *                    policy_obs[e][j] = affine(traj[t + 1][e][obs_start + j * obs_stride])
 *                with the UPDATED bounds and the target range (lower, upper).  With update = 0 (a frozen scaling) the
 *                bounds are read and not written.  With bounds = NULL it is the sensor copy alone.
 *
 * Affine maps are ScaleTransform._affine's  out = ((v - a) / (b - a)) * (d - c) + c  as four separately rounded fp32
 * operations.  co_act takes coef[0..3][j] = (a, b - a, d - c, c) per action column (replay_hip.h); NULL is the identity.
 * co_observe forms (a, b - a, d - c, c) = (vmin, vmax - vmin, upper - lower, lower) itself, each difference one fp32
 * subtraction.
 *
 * The grid-wide dependency of co_observe (every output needs the extrema of the whole block) is two launches: the first
 * reduces the rows of each workgroup to one (min, max) partial in `workspace` (lanes along the columns, xor shuffles in
 * the wave, LDS across the workgroup's four waves); in the second every wave folds all partials itself and scales its
 * row.  No workgroup waits for another, there is no grid barrier and no atomic, and the result does not depend on the
 * launch shape (minimum and maximum are exact and associative).
 *
 * The running bounds.  `bounds` points at FOUR device floats, two cells of (vmin, vmax).  Step t reads cell t & 1; with
 * update = 1 it writes the joined bounds to cell (t + 1) & 1.  No workgroup reads a cell that another workgroup of the
 * same launch writes (the step[2] rule of rollout_hip.h).  The host sets cell 0 before step 0 of an updating
 * scaling and both cells of a frozen one.
 *
 * One wave per env row, four per workgroup; plain vector stores; float4 accesses where N % 4 == 0, the sensor is
 * (start % 4 == 0, stride 1) and the bases are 16-byte aligned (decided on the host per launch).  The structs are HOST
 * structs read during the call and passed to the kernels by value; every pointer in them is a DEVICE pointer.  `t` is
 * passed by value.  Everything is enqueued on `stream`: no host synchronisation, no device allocation.  Arguments are
 * validated on the host before any HIP call.  Return 0 on success, negative on error (co_last_error()).
 */
#ifndef COLLECT_HIP_H
#define COLLECT_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define CO_MIN_STATE_DIM 16
#define CO_MAX_STATE_DIM 1024
#define CO_MAX_ACT_DIM 16

typedef struct co_geometry {
    int E;                           /* envs */
    int T;                           /* trajectory slots: steps 0 ... T-1 */
    int N;                           /* state width: the stepper's observation rows and the trajectory rows */
    int A;                           /* action width */
    int obs_start, obs_stride;       /* agent sensor over the state columns */
} co_geometry;

typedef struct co_act_args {
    const float* action;             /* [E][A] the policy's output */
    const float* coef;               /* [4][A] affine map of the action columns; NULL: identity */
    float* env_action;               /* [E][A] the stepper's action buffer */
    float* actions;                  /* [T][E][A] trajectory record; only slot t is written */
    int record_raw;                  /* 0: record the env-side action, 1: the raw action */
} co_act_args;

typedef struct co_observe_args {
    const float* traj;               /* [T + 1][E][N]; slot t + 1 holds the stepper's observations of step t */
    float* policy_obs;               /* [E][O], O = ceil((N - obs_start) / obs_stride) */
    float* bounds;                   /* float[2][2]: two cells of (vmin, vmax), see above; NULL: no scaling */
    float lower, upper;              /* target range of the scaling */
    int update;                      /* 1: join the block's extrema with the running bounds first */
    float* workspace;                /* co_workspace_floats(g) floats; needed with update = 1 */
} co_observe_args;

/* Refusals: -1 NULL geometry, -2 E < 1, -3 T < 1, -4 N outside CO_MIN_STATE_DIM ... CO_MAX_STATE_DIM, -5 A outside
 * 1 ... CO_MAX_ACT_DIM, -6 an agent sensor with stride < 1 or a start outside the state row.  0 when the kernels run
 * this geometry. */
int co_supported(const co_geometry* g);

/* Floats of scratch co_observe needs with update = 1 (one (min, max) pair per workgroup of four rows); the refusal's
 * negative code for a geometry co_supported refuses.  Pure host function. */
long co_workspace_floats(const co_geometry* g);

/* -10 a NULL pointer the kernel needs; -11 t outside 0 ... T-1; -12 update = 1 without a workspace; -20 launch failure */
int co_act(void* stream, const co_geometry* g, const co_act_args* a, int t);
int co_observe(void* stream, const co_geometry* g, const co_observe_args* a, int t);

const char* co_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
