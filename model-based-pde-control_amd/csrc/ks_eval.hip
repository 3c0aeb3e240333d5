// ks_eval.hip -- ks_eval_rows_device / ks_eval_fold_device (include/kspde.h): the metric section of
// PDETrainingModule.test_step (pdecontrol/surrogates/training.py:195-243 of the reference) as two launches.
//
// Rows: one group of G lanes per (b, t) row, lane gl takes the points gl, gl + G, ... (the partition of
// ks_reward_rows_kernel, so the rewards have its bits); the 22 partial sums are reduced by xor shuffles inside the
// group and lane 0 writes the row's 18 values.  Fold: one thread per output value walks the batch in index order and
// adds B times its value to the epoch accumulator: no atomics, no ticket, no grid barrier, so successive batches on one
// stream give an epoch's sums the same bits every time.  The arithmetic is ks_eval.h's (eval_row_share,
// eval_row_finish, eval_fold_value), the text the twin runs; the derivatives divide by DivMarkstein here.
#include <hip/hip_runtime.h>

#include "../../include/kspde.h"
#include "ks_eval.h"

namespace ks {

template <int G, bool DISS>
__global__ void __launch_bounds__(256) ks_eval_rows_kernel(const EvalArgs a) {
    const int gl = threadIdx.x & (G - 1);
    const long row = ((long)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const bool active = row < (long)a.B * a.T;     // inactive groups still take part in the shuffles
    EvalSums sums;
#pragma unroll
    for (int j = 0; j < EvalSums::COUNT; ++j) sums.v[j] = 0.0;
    if (active) eval_row_share<DivMarkstein, DISS>(a, row, gl, G, sums);
#pragma unroll
    for (int m = 1; m < G; m <<= 1) {
#pragma unroll
        for (int j = 0; j < EvalSums::COUNT; ++j) sums.v[j] += __shfl_xor(sums.v[j], m, 64);
    }
    if (active && gl == 0) eval_row_finish<DISS>(sums, a.N, a.rowstats + row * EVAL_ROW_STATS);
}

__global__ void __launch_bounds__(64) ks_eval_fold_kernel(const double* __restrict__ rowstats, int B, int T, int N,
                                                          double* __restrict__ tables, double* __restrict__ accum) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 1 + EVAL_TABLES * T) return;
    const double v = eval_fold_value(rowstats, B, T, N, i);
    tables[i] = v;
    if (accum) accum[i] += (double)B * v;
}

template <int G>
static hipError_t launch_eval_rows_g(bool diss, const EvalArgs& a, hipStream_t st) {
    const int block = 256, rows_per_block = block / G;
    const long rows = (long)a.B * a.T;
    const unsigned grid = (unsigned)((rows + rows_per_block - 1) / rows_per_block);
    return with_flags(true, diss, [&](auto, auto dissipation) {
        hipLaunchKernelGGL((ks_eval_rows_kernel<G, decltype(dissipation)::value>), dim3(grid), dim3(block), 0, st, a);
        return hipGetLastError();
    });
}

hipError_t launch_eval_rows(int objective, const EvalArgs& a, hipStream_t st) {
    const bool diss = objective == KS_OBJECTIVE_DISSIPATION;
    // the partition of launch_reward_rows
    if (a.N <= 64) return launch_eval_rows_g<16>(diss, a, st);
    if (a.N <= 512) return launch_eval_rows_g<32>(diss, a, st);
    return launch_eval_rows_g<64>(diss, a, st);
}

hipError_t launch_eval_fold(const double* rowstats, int B, int T, int N, double* tables, double* accum, hipStream_t st) {
    const int block = 64, n = 1 + EVAL_TABLES * T;
    hipLaunchKernelGGL(ks_eval_fold_kernel, dim3((unsigned)((n + block - 1) / block)), dim3(block), 0, st, rowstats, B, T,
                       N, tables, accum);
    return hipGetLastError();
}

}  // namespace ks
