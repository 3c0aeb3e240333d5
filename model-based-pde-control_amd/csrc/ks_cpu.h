// ks_cpu.h -- the CPU twin of the fused stepper (device = -1 behind the C ABI of include/kspde.h).
//
// Plain C++17, no HIP: the arithmetic of ks_internal.h -- the same source text as the kernels of ks_kernels.hip, built by
// a second compiler (both modes, same operation order) -- on host memory, envs spread over host threads.  It serves
// BASELINE configs[0] (one env on a GPU-less host), SURVEY 8(d) baseline (B) and the sanitizer build (make -C csrc asan).
// Sharing its source with the kernels, it is no independent check of them: that is oracle/ks_oracle.c alone (test
// infrastructure, which shares nothing with csrc/); the twin is compared with it by tests/test_cpu_twin.py through the
// golden vectors.
#pragma once
#include <cstddef>

#include "ks_eval.h"
#include "ks_internal.h"

namespace kscpu {

using ks::Consts;   // the step constants of one (dx, dt): ks::make_consts

// Advance the n_rows envs listed in env_ids (nullptr = rows 0..n_rows-1) by n_substeps RK4 sub-steps.
//   u        [E,N] fp64 in/out            phi      [E,N] fp32 or nullptr
//   actions  [E,n_act] fp32 or nullptr    F        [n_act,N] fp32 (needed iff actions)
//   obs / ssq_sum / status  outputs indexed by env id, any may be nullptr
// mode: 0 = fast (merged stencil, FMA), 1 = exact (reference operation order, true divisions, no contraction).
// objective: 0 = l2control (ssq_sum collects sum u^2), 1 = dissipation (sum u_xx^2 + u_x^2 + u*phi); see kspde.h.
void step(int N, const Consts& c, int mode, int objective, double* u, const float* phi, const float* actions, const float* F,
          int n_act, const int* env_ids, int n_rows, long n_substeps, float* obs, double* ssq_sum, int* status, int n_threads);

// rhs test hook in the reference's operation order; u, phi and outputs [n_rows, N]; ux / uxx / uxxxx may be nullptr.
void rhs(int N, const Consts& c, const double* u, const float* phi, int n_rows, double* out, double* ux, double* uxx,
         double* uxxxx);

// Per-row reward of fp32 obs [n_rows, N] with fp32 phi (nullptr = 0) -> out [n_rows] (ks_reward_rows_device).
void reward_rows(int N, const Consts& c, int objective, const float* obs, const float* phi, int n_rows, double* out);

// ks_record_device on host memory: transition w = t * E + e of [T][E] goes to row dst[w] of the seven slabs (a negative
// dst writes nothing); reward (float)((scale * ssq[w]) / substeps).
void record(int E, int N, int A, long n, const float* traj, const float* actions, const double* ssq, const int* steps,
            const long* dst, double scale, double substeps, float* obs, float* act, float* nxtobs, float* rewards,
            unsigned char* terminated, unsigned char* truncated, int* out_steps);

// ks_eval_rows_device / ks_eval_fold_device on host memory: the arithmetic of ks_eval.h (eval_row_share,
// eval_row_finish, eval_fold_value) row by row and value by value, with the true division.
void eval_rows(int objective, const ks::EvalArgs& a);
void eval_fold(const double* rowstats, int B, int T, int N, double* tables, double* accum);

// Host threads the twin uses by default: the affinity mask, capped by KSPDE_CPU_THREADS.
int default_threads();

}  // namespace kscpu
