/*
 * burgers/objective.h -- the objective entries of libburgers_hip.so (kernels: csrc/bg_objective.hip; arithmetic:
 * csrc/bg_objective.h; binding: pdegym/burgers/_hip.py, OBJECTIVE_SYMBOLS).  An extension of ../burgers_hip.h: the
 * stepper with the reward sum of either objective, and the row reward of the dissipation objective.
 *
 * Objectives: BG_OBJECTIVE_L2CONTROL (0), the reward -(1/N)|u|^2 of bg_step, and BG_OBJECTIVE_DISSIPATION (1), the energy
 * budget of the forced equation, d/dt 1/2 <u^2> = -nu <u_x^2> + <u phi>:  r = -(nu <u_x^2> + <u phi>).
 *
 * bg_step_objective       bg_step with `objective`: the same layout (one env per wave, P = N / 64 points per lane, the
 * bg_step_span_objective  halo by DPP, tail waves redoing the last env), the same state arithmetic, so u, obs and status
 *                         are the same bytes under either objective, and under objective 0 every byte is bg_step's /
 *                         bg_step_span's.  The span equals T step launches byte for byte.  Under objective 1 the fp64
 *                         sum (ssq_sum [E] / ssq [T][E]) holds
 *                             S = sum over sub-steps, sum over lanes of ((double)qd * nu_d + (double)qp)
 *                         taken at the state before each sub-step's update: per lane, over its P points in index order,
 *                         qd = fmaf(g_j, g_j, qd) and qp = fmaf(u_j, phi_j, qp), g_j = (w[+1] - w[-1]) * (0.5f / dx) the
 *                         fp32 gradient of the stage-1 residual itself, nu_d = (double)nu; each lane adds its sub-steps'
 *                         terms in order, the lanes are reduced by the xor butterfly (a balanced tree).  With
 *                         c = -(1/N) / max(n_substeps, 1) the reward is S * c, as under l2control.  actions == NULL is
 *                         legal for bg_step_objective under either objective (phi = 0).
 * bg_reward_rows          reward [M] fp64, before the caller's cast to fp32:
 *                             (-1.0) * (nu_d * (sum_i ux_i^2 / N) + sum_i u_i * phi_i / N)
 *                         u_i = (double) of the fp32 row, ux = (u[+1] - u[-1]) / (2 dx) in fp64, periodic, phi the fp32
 *                         field widened: row `phi` [M][N], or the chain actions [M][A] @ F [A][N] (one rounded product,
 *                         one fmaf per further actuator), or zero when both are NULL; nu_d = (double)(float)nu.  One
 *                         group of 16 (N <= 64), 32 (N <= 512) or 64 lanes per row, lane gl takes the points gl, gl + G,
 *                         ..., the two sums are reduced by xor shuffles and lane 0 writes.  Any N >= 3.
 * No atomics: the same bits on every run.  The launches are asynchronous on the given hipStream_t, take DEVICE pointers,
 * do not synchronise and do not allocate.
 *
 * The *_host entries run the same arithmetic serially on HOST memory and make no HIP call.  bg_step_objective_host
 * reproduces the kernel's bits, the lane partition and the butterfly of the sum included; bg_reward_rows_host sums a row
 * in index order (the kernel's sums are in its groups' order).  They are test twins, not env backends.
 *
 * Return 0, -1 for a refusal, -4 for a width the stepper does not have, -2 when the launch failed;
 * bg_objective_last_error() holds the text.  Every refusal is made on the host before any HIP call, with a message that
 * starts with the entry's name.  Steppers: NULL u (span: NULL u, actions, F or traj); actions without F; n_act outside
 * 1 ... 16 with actions; T < 1; n_envs < 1; n_substeps < 0; dx, dt not positive or nu negative; an objective other than
 * 0 and 1; N not a multiple of 64 or not one of 64, 128, 256, 512, 1024 (-4).  bg_reward_rows: NULL u or reward; phi and
 * actions both given; actions without F or A outside 1 ... 16; M < 1 or above 2^30; N < 3; dx not positive and finite;
 * nu negative or not finite.
 *
 * It is declared here and not in burgers_hip.h because that header's list of functions is pinned, name by name;
 * tests/test_burgers_objective_host.py holds this header, its binding table and the library to each other.
 */
#ifndef BURGERS_OBJECTIVE_H
#define BURGERS_OBJECTIVE_H

#include "../burgers_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BG_OBJECTIVE_L2CONTROL   0
#define BG_OBJECTIVE_DISSIPATION 1

int bg_step_objective(void* stream, float* u, const float* actions, const float* F, int n_act, int n_envs, int N, float dx,
                      float dt, float nu, long n_substeps, float* obs, double* ssq_sum, int* status, int objective);
int bg_step_span_objective(void* stream, float* u, const float* actions, const float* F, int n_act, int n_envs, int N, int T,
                           float dx, float dt, float nu, long n_substeps, float* traj, double* ssq, int* status, int objective);
int bg_reward_rows(void* stream, const float* u, const float* phi, const float* actions, const float* F, int M, int N, int A,
                   double dx, double nu, double* reward);
int bg_step_objective_host(float* u, const float* actions, const float* F, int n_act, int n_envs, int N, float dx, float dt,
                           float nu, long n_substeps, float* obs, double* ssq_sum, int* status, int objective);
int bg_reward_rows_host(const float* u, const float* phi, const float* actions, const float* F, int M, int N, int A, double dx,
                        double nu, double* reward);

const char* bg_objective_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
