/*
 * rollout_hip.h -- C ABI of librollout_hip.so: the kernels that close the imagined-rollout loop of the controller on
 * gfx950 (pdecontrol/mbrl/imagination_phase.py: imagine; kernels: csrc/rollout.hip).
 *
 * One imagined step is a captured chain  sac_policy_forward -> ro_act_chain -> every ensemble member's fused one-step
 * rollout -> ro_settle.  The two kernels here replace what the wrapper stack does on the host between those launches:
 *
 *   ro_act_chain   the action side.  Reads the agent's action [B][A], records it unchanged in the trajectory
 *                  (actions[t][b][:], the raw action the outermost store keeps), maps it per action column through an
 *                  optional affine map, forms the forcing field as the fp32 chain
 *                      acc = a[0] * F[0][i];  acc = fmaf(a[k], F[k][i], acc), k = 1 ... A-1
 *                  (the chain of the KS stepper's action path; it equals the host's `actions @ forcing`), maps that
 *                  through an optional per-column affine map and writes the columns the sensor keeps to the world's
 *                  action buffer: output column j is forcing column sensor_start + j * sensor_stride.
 *   ro_settle      the observation side.  Takes row b of member chosen[t][b]'s output as env b's new state, writes it
 *                  to the world state in place, to the trajectory slot traj[t + 1][b][:] and, through the agent's sensor,
 *                  to the policy's observation buffer; writes steps[t][b] = steps0[b] + t + 1 and the l2control reward
 *                      reward[t][b] = (float)((-1.0) * (1.0 / N) * sum_i (double)w_i * (double)w_i)
 *                  of the row rescaled by the optional per-column affine map w_i = affine_i(v_i) (fp64 sum over strided
 *                  lanes and xor shuffles, as the KS reward-row kernel).
 *                  (The same kernel with the KS env's dissipation reward is declared in a header of its own,
 *                  rollout/settle_dissipation.h, which includes this one.)
 *
 * Affine maps are ScaleTransform._affine's  out = ((v - a) / (b - a)) * (d - c) + c  with coef[0..3][j] = (a, b - a,
 * d - c, c) per OUTPUT column, as four separately rounded fp32 operations; NULL is the identity (replay_hip.h).
 *
 * The step counter.  `step` points at TWO device int32: step[1] is the step the next ro_act_chain works on, step[0] the
 * step the current chain works on.  ro_act_chain reads step[1] and publishes it in step[0]; ro_settle reads step[0] and
 * publishes step[0] + 1 in step[1].  No kernel reads the cell it writes, so a captured chain replays correctly without
 * an atomic; the host zeroes both cells at the start of a round.  A step outside [0, T) writes nothing.
 *
 * One wave per env, four per workgroup, lanes along the columns; no LDS, no atomics, plain vector stores; float4 accesses
 * where the widths and alignments allow (decided on the host per launch).  The structs are HOST structs read during the
 * call and passed to the kernel by value; every pointer in them is a DEVICE pointer.  Everything is enqueued on `stream`:
 * no host synchronisation, no device allocation.  Return 0 on success, negative on error (ro_last_error()).
 */
#ifndef ROLLOUT_HIP_H
#define ROLLOUT_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define RO_MAX_MEMBERS 8
#define RO_MIN_STATE_DIM 16
#define RO_MAX_STATE_DIM 1024
#define RO_MAX_ACT_DIM 16

typedef struct ro_geometry {
    int B;                           /* envs */
    int T;                           /* trajectory slots: steps 0 ... T-1 */
    int N;                           /* state width: world state, member outputs and trajectory rows */
    int A;                           /* agent action width */
    int L;                           /* forcing width: forcing is [A][L] */
    int act_start, act_stride;       /* action-side sensor over the forcing columns */
    int obs_start, obs_stride;       /* agent sensor over the state columns */
    int members;                     /* ensemble members */
} ro_geometry;

typedef struct ro_act_args {
    const float* action;             /* [B][A] the policy's output */
    float* actions;                  /* [T][B][A] trajectory record of the raw actions */
    const float* in_coef;            /* [4][A] affine map of the action columns; NULL: identity */
    const float* forcing;            /* [A][L] */
    const float* out_coef;           /* [4][W] affine map per OUTPUT column, W = ceil((L - act_start) / act_stride); NULL */
    float* world_action;             /* [B][W] */
    int* step;                       /* int32[2], see above */
} ro_act_args;

typedef struct ro_settle_args {
    const float* member[RO_MAX_MEMBERS]; /* [B][N] each: the members' one-step outputs */
    const int* chosen;               /* [T][B] member of each env at each step; NULL with one member */
    float* state;                    /* [B][N] the world state, written in place */
    float* traj;                     /* [T + 1][B][N]; slot 0 is the reset's */
    float* policy_obs;               /* [B][O], O = ceil((N - obs_start) / obs_stride) */
    const int* steps0;               /* [B] env step counters after the reset */
    int* steps;                      /* [T][B] */
    float* rewards;                  /* [T][B] */
    const float* reward_coef;        /* [4][N] rescaling of the state before the reward; NULL: identity */
    int* step;                       /* int32[2], see above */
} ro_settle_args;

/* Refusals: -1 NULL geometry, -2 B < 1, -3 T < 1, -4 N outside RO_MIN_STATE_DIM ... RO_MAX_STATE_DIM, -5 A outside
 * 1 ... RO_MAX_ACT_DIM, -6 forcing width < 1, -7 an action sensor with stride < 1 or a start outside the forcing row,
 * -8 an agent sensor with stride < 1 or a start outside the state row, -9 members outside 1 ... RO_MAX_MEMBERS.
 * 0 when the kernels run this geometry. */
int ro_supported(const ro_geometry* g);

/* -10 a NULL pointer the kernel needs; -20 launch failure */
int ro_act_chain(void* stream, const ro_geometry* g, const ro_act_args* a);
int ro_settle(void* stream, const ro_geometry* g, const ro_settle_args* a);

const char* ro_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
