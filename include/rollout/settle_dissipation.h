/*
 * rollout/settle_dissipation.h -- the dissipation-objective entry point of librollout_hip.so (kernels: csrc/rollout.hip;
 * binding: pdecontrol/mbrl/rollout_hip.py, DISSIPATION_SYMBOLS).  An extension of ../rollout_hip.h, whose geometry,
 * argument structs, step-counter rule and conventions it uses unchanged.
 *
 *   ro_settle_dissipation   ro_settle for a world whose reward is the KS env's dissipation objective: everything
 *                  ro_settle does, with the same values (elite pick, world state in place, trajectory slot t + 1, agent
 *                  sensor, steps, the step-counter hand-over, the NaN row for a member index outside the ensemble,
 *                  nothing for a step outside [0, T)), and in place of the l2control reward
 *                      reward[t][b] = (float)((-1.0) * ((sum_i uxx_i^2 / N + sum_i ux_i^2 / N) + sum_i u_i * phi_i / N))
 *                  with u_i = (double)w_i of the rescaled row, ux (the upwind derivative of u^2) and uxx in the
 *                  reference's operation order over the periodic row (the expression and the stencil of the KS
 *                  reward-row kernel, grid spacing dx), and phi the fp32 forcing field of the scaled action, recomputed
 *                  from the raw actions ro_act_chain recorded for this step: that kernel's chain before its output map,
 *                  over the full forcing width.
 *
 * It is declared here and not in rollout_hip.h because that header's list of functions is pinned, name by name, as the
 * ABI of the l2control step; tests/test_imagination_dissipation_host.py holds this header, its binding table and the
 * library to each other.
 */
#ifndef ROLLOUT_SETTLE_DISSIPATION_H
#define ROLLOUT_SETTLE_DISSIPATION_H

#include "../rollout_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ro_dissipation_args {
    const float* actions;            /* [T][B][A] the raw actions ro_act_chain recorded (slot t is read) */
    const float* in_coef;            /* [4][A] affine map of the action columns; NULL: identity */
    const float* forcing;            /* [A][N] full-width forcing (the forcing width must equal N) */
    double dx;                       /* grid spacing of the periodic row */
} ro_dissipation_args;

/* ro_settle's refusals, and: -10 also for d, d->actions or d->forcing NULL; -11 g->L != g->N; -12 dx not finite or <= 0.
 * All are decided before any HIP call. */
int ro_settle_dissipation(void* stream, const ro_geometry* g, const ro_settle_args* a, const ro_dissipation_args* d);

#ifdef __cplusplus
}
#endif

#endif
