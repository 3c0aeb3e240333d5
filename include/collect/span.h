/*
 * collect/span.h -- the whole-segment entry points of libcollect_hip.so (kernels: csrc/collect.hip; binding:
 * pdecontrol/mbrl/collect_hip.py, SPAN_SYMBOLS).  An extension of ../collect_hip.h, whose geometry, argument structs,
 * affine maps and conventions it uses unchanged.
 *
 * An agent whose actions do not depend on the observation (the controller's warm-up RandomAgent, the ActionRepeatAgent of
 * its surrogate evaluation) needs neither co_act nor co_observe once per step: all g->T actions of a segment are known
 * before its first launch, and the policy's observation is needed only after its last step.  A segment is then
 *
 *     co_act_span -> T x ks_step_device (d_actions = env_actions + t * E * A, d_obs = traj[t + 1]) -> co_observe_span
 *
 *   co_act_span      co_act for every step at once, one launch.  For every (t, e) it reads table[t][e][:] (the agent's
 *                    actions, on the agent's side of the wrapper stack), maps each column through coef, writes
 *                    env_actions[t][e][:] (the stepper reads row t at step t) and records in actions[t][e][:] the
 *                    env-side action, or the raw one with record_raw = 1.  One wave per (t, e) row, four per workgroup,
 *                    lanes along A.
 *   co_observe_span  co_observe for every step at once.  With update = 1 it takes the minimum and maximum over
 *                    traj[1 ... T] (slot 0 is the observation the segment started from and is NOT part of the update),
 *                    joins them with the running bounds by co_observe's rule (an unset bound gives way, a NaN
 *                    propagates), writes the joined bounds and
 *                        policy_obs[e][j] = affine(traj[T][e][obs_start + j * obs_stride])
 *                    with the joined bounds.  That equals T successive co_observe calls: minimum and maximum are exact
 *                    and associative, an unset bound stays unset until the first block, a NaN anywhere ends in NaN
 *                    either way.  With update = 0 it is the sensor and affine copy of slot T alone, with
 *                    bounds = NULL the sensor copy alone.
 *
 * Bounds cells.  co_observe_span takes co_observe_args (its `t` is g->T).  It READS cell 0 of `bounds` and, with
 * update = 1, WRITES cell 1: no launch reads a cell it writes.
 *
 * Launches.  co_act_span: one.  co_observe_span: two with update = 1, else one.  The first reduces the T * E rows to
 * min(ceil(T * E / 4), CO_SPAN_MAX_PARTS) partials of (min, max): that many workgroups of four waves
 * walk the rows with a grid stride.  In the second, ceil(E / 4) workgroups, every wave folds all partials itself and
 * scales its row of slot T.  The result does not depend on the launch shape.  `workspace` holds
 *     co_span_workspace_floats(g) = 2 * min(ceil(T * E / 4), CO_SPAN_MAX_PARTS)
 * floats.  float4 accesses under co_observe's host-decided conditions.
 */
#ifndef COLLECT_SPAN_H
#define COLLECT_SPAN_H

#include "../collect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CO_SPAN_MAX_PARTS 1024

typedef struct co_act_span_args {
    const float* table;              /* [T][E][A] the agent's actions of the whole segment */
    const float* coef;               /* [4][A] affine map of the action columns; NULL: identity */
    float* env_actions;              /* [T][E][A] the stepper's actions: row t is step t's d_actions */
    float* actions;                  /* [T][E][A] trajectory record */
    int record_raw;                  /* 0: record the env-side action, 1: the raw action */
} co_act_span_args;

/* 2 * min(ceil(T * E / 4), CO_SPAN_MAX_PARTS); the refusal's negative code for a geometry co_supported refuses.  Pure
 * host function. */
long co_span_workspace_floats(const co_geometry* g);

/* co_supported's refusals, and: -10 a NULL pointer the kernel needs; -12 update = 1 without a workspace; -20 launch
 * failure.  All but -20 are decided before any HIP call. */
int co_act_span(void* stream, const co_geometry* g, const co_act_span_args* a);
int co_observe_span(void* stream, const co_geometry* g, const co_observe_args* a);

#ifdef __cplusplus
}
#endif

#endif
