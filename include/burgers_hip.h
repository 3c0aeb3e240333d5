/*
 * burgers_hip.h -- C ABI of libburgers_hip.so: batched viscous-Burgers stepper for gfx950 (SURVEY.md 8(f) row f4,
 * BASELINE.json configs[4]: "Burgers-1D env, 512 grid pts ... fp32").
 *
 * The reference ships NO Burgers environment (pdegym/__init__.py:2 imports a module that does not exist).  The
 * discretisation is the one its BurgersPhyPDELoss defines (pdecontrol/surrogates/phyloss/phyloss.py:36-86):
 *
 *   residual(u) = nu * laplace(u) - u * grad(u) (+ phi)        grad    = [-1/2, 0, 1/2] / dx            (circular)
 *                                                              laplace = [-1/12, 4/3, -5/2, 4/3, -1/12] / dx^2
 *   one sub-step: u <- u + dt * residual(u + dt/2 * residual(u))            ("improved Euler", :83-86)
 *
 * and these entry points replace what a pdegym/burgers env's step()/reset() would loop over in Python, in the same
 * way libkspde.so replaces pdegym/kuramoto/kuramoto.py:78-129: ONE launch advances every env by all n_substeps with
 * the fp32 state in registers (one env = one 64-lane wavefront x N/64 points per lane, +-2 halo by DPP wave
 * rotations = the periodic boundary), the forcing phi = actions @ F evaluated in-kernel, the l2 reward term
 * accumulated per sub-step (before the update, like the KS env) and reduced once.
 *
 * All pointers are DEVICE pointers; launches are asynchronous on the given hipStream_t.  Return 0 on success,
 * negative on error (bg_last_error()).  Supported grid sizes: N = 64 * P with P in {1, 2, 4, 8, 16}.
 */
#ifndef BURGERS_HIP_H
#define BURGERS_HIP_H

#include "replay/slabs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* u [E,N] fp32 in/out; actions [E,n_act] fp32 with F [n_act,N] fp32 (phi = actions @ F, fp32 FMA chain), or
 * actions == NULL for phi = 0; obs [E,N] fp32 or NULL; ssq_sum [E] fp64 (sum over sub-steps of sum_i u_i^2) or NULL;
 * status [E] int (1 = non-finite state) or NULL. */
int bg_step(void* stream, float* u, const float* actions, const float* F, int n_act, int n_envs, int N, float dx, float dt,
            float nu, long n_substeps, float* obs, double* ssq_sum, int* status);

/* T successive bg_step launches in one: step t takes row t of actions [T,E,n_act] (never NULL here), advances u by
 * n_substeps sub-steps and stores the state to traj[t+1] (traj [T+1,E,N]; slot 0 is not touched), ssq[t] and status[t]
 * (ssq fp64 [T,E], status int [T,E]; either may be NULL).  The state stays in registers between the steps and u is stored
 * once, after the last.  Every output byte equals what
 *   for t: bg_step(stream, u, actions + t*E*n_act, F, ..., obs = traj + (t+1)*E*N, ssq + t*E, status + t*E)
 * leaves: the same operations in the same order, the same reduction.  Refused on the host before any HIP call, with a
 * message that starts with "bg_step_span:": NULL u / actions / F / traj, T < 1, n_envs < 1, n_act outside 1 ... 16, an N
 * bg_step refuses, n_substeps < 0, dx or dt not positive, nu negative. */
int bg_step_span(void* stream, float* u, const float* actions, const float* F, int n_act, int n_envs, int N, int T, float dx,
                 float dt, float nu, long n_substeps, float* traj, double* ssq, int* status);

/* The T * E transitions of T consecutive steps without a truncation, read where bg_step / bg_step_span left them and
 * written as rows of a device-resident replay: the counterpart of ks_record_device (include/kspde.h) without a handle.
 * bg_slabs is a HOST struct of DEVICE pointers, the one struct ks_record is: obs / nxtobs fp32 [rows,N], actions fp32
 * [rows,A], rewards fp32 [rows], terminated / truncated bytes [rows], steps int [rows].  Transition (t, e) writes row
 * d_dst[t][e] (a negative entry writes nothing): obs = traj[t][e], nxtobs = traj[t+1][e], the action and steps of (t, e),
 * terminated = truncated = 0 and rewards = (float)(ssq[t][e] * c), c = -(1.0 / (double)N) / (double)max(n_substeps, 1):
 * BurgersBatchedVecEnv.step_torch's reward, one fp64 product, cast to fp32.  dst_host is d_dst on the host: every refusal
 * (NULL pointers, T < 1, n_envs < 1, N < 1, A outside 1 ... 16, n_substeps < 0, slabs without rows, an entry >= rows, a row
 * named twice) is made from it before any HIP call, with a message that starts with "bg_record:".  One launch; it does not
 * synchronise and does not allocate device memory. */
typedef replay_slabs bg_slabs;                  /* replay/slabs.h */

int bg_record(void* stream, const float* d_traj /* [T+1][E][N] */, const float* d_actions /* [T][E][A] */, int n_envs, int N,
              int A, const double* d_ssq /* [T][E] */, const int* d_steps /* [T][E] */, int T, long n_substeps,
              const long* d_dst /* [T][E] */, const long* dst_host, const bg_slabs* out);

/* test hook: out [n_rows,N] = nu * laplace(u) - u * grad(u) + phi (phi may be NULL) */
int bg_residual(void* stream, const float* u, const float* phi, int n_rows, int N, float dx, float nu, float* out);

/* Physics-informed loss of the reference's BurgersPhyPDELoss (phyloss.py:17-25, 62-86) on augmented [B,T,N] fp32:
 *   target[:,0] = augmented[:,T-1] (the LAST slice, as the reference has it), target[:,t] = Phi(augmented[:,t-1]) with
 *   Phi = `substeps` explicit-midpoint steps of the residual above (no forcing), loss = (augmented - target)^2.
 * One launch each, one (b,t) row per wavefront as in the stepper; no atomics, results bit-identical run to run.
 *
 * forward:  loss [B,T,N] out.  diff [B,T,N] out (augmented - target) or NULL when no gradient will be asked for.  With diff
 *           and substeps > 1, states must hold B*(T-1)*(substeps-1)*N floats (states_len = its capacity in floats): the
 *           state before sub-steps 1 .. substeps-1 of every row t <= T-2, read back by the adjoint.  NULL otherwise.
 * backward: g_loss [B,T,N] = d L / d loss; diff and states as the forward wrote them; grad [B,T,N] out = d L / d augmented
 *           = e_t - [t <= T-2] DPhi(a_t)^T e_(t+1) - [t = T-1] e_0 with e = 2 diff g_loss; the midpoint sub-steps are
 *           walked in reverse with J(v)^T p = nu laplace(p) - grad(v) p + grad(v p). */
int bg_phyloss_forward(void* stream, const float* augmented, int B, int T, int N, float dx, float dt, float nu, int substeps,
                       float* loss, float* diff, float* states, long states_len);
int bg_phyloss_backward(void* stream, const float* augmented, const float* diff, const float* g_loss, const float* states,
                        long states_len, int B, int T, int N, float dx, float dt, float nu, int substeps, float* grad);

const char* bg_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
