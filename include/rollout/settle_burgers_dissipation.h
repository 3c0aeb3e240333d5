/*
 * rollout/settle_burgers_dissipation.h -- the entry point of librollout_hip.so for a world whose reward is the Burgers
 * env's dissipation objective (kernels: csrc/rollout.hip; binding: pdecontrol/mbrl/rollout_hip.py,
 * BURGERS_DISSIPATION_SYMBOLS).  An extension of ../rollout_hip.h and of settle_dissipation.h, whose geometry, argument
 * structs, step-counter rule and conventions it uses unchanged.
 *
 *   ro_settle_burgers_dissipation   everything ro_settle does, with the same values (elite pick, world state in place,
 *                  trajectory slot t + 1, agent sensor, steps, the step-counter hand-over, the NaN row for a member index
 *                  outside the ensemble, nothing for a step outside [0, T)), and in place of the l2control reward the row
 *                  reward of include/burgers/objective.h,
 *                      reward[t][b] = (float)((-1.0) * (nu_d * (sum_i ux_i^2 / N) + sum_i u_i * phi_i / N))
 *                  with u_i = (double)w_i of the rescaled row, ux = (u[+1] - u[-1]) / (2 dx) in fp64 over the periodic
 *                  row, nu_d = (double)(float)nu, and phi the fp32 forcing field of the scaled action, recomputed from
 *                  the raw actions ro_act_chain recorded for this step exactly as ro_settle_dissipation recomputes it.
 *                  The two sums are taken per lane over its columns and reduced by xor shuffles.
 *
 * It is declared here and not in rollout_hip.h because that header's list of functions is pinned, name by name, as the
 * ABI of the l2control step; tests/test_burgers_objective_host.py holds this header, its binding table and the library to
 * each other.
 */
#ifndef ROLLOUT_SETTLE_BURGERS_DISSIPATION_H
#define ROLLOUT_SETTLE_BURGERS_DISSIPATION_H

#include "settle_dissipation.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ro_burgers_dissipation_args {
    ro_dissipation_args d;           /* recorded actions, their affine map, the full-width forcing, the grid spacing */
    double nu;                       /* viscosity */
} ro_burgers_dissipation_args;

/* ro_settle's refusals, and those of ro_settle_dissipation: -10 also for d, d->d.actions or d->d.forcing NULL; -11
 * g->L != g->N; -12 dx not finite or <= 0; and -13 nu negative or not finite.  All are decided before any HIP call. */
int ro_settle_burgers_dissipation(void* stream, const ro_geometry* g, const ro_settle_args* a,
                                  const ro_burgers_dissipation_args* d);

#ifdef __cplusplus
}
#endif

#endif
