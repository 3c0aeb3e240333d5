// bg_eval.hip -- bg_eval_rows / bg_eval_fold / bg_derivatives and their *_host twins (include/burgers/eval.h): the metric
// section of PDETrainingModule.test_step for a Burgers env as two launches, and the derivatives behind env.rhs.
//
// Rows: one group of G lanes per (b, t) row, lane gl takes the points gl, gl + G, ... (the partition of ks_eval.hip's
// launch_eval_rows); the 14 partial sums are reduced by xor shuffles inside the group and lane 0 writes the row's 14
// values.  Fold: one thread per output value walks the batch in index order and adds B times its value to the epoch
// accumulator: no atomics, no ticket, no grid barrier, so successive batches on one stream give an epoch's sums the same
// bits every time.  Derivatives: one thread per point.  The arithmetic is bg_eval.h's, the text the *_host entries run
// serially on host memory; this translation unit is built with -ffp-contract=off and linked beside burgers.hip, whose
// kernels it does not touch.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/burgers/eval.h"
#include "bg_eval.h"
#include "capi_error.h"

namespace {

using namespace bg;

template <int G>
__global__ void __launch_bounds__(256) bg_eval_rows_kernel(const EvalArgs a) {
    const int gl = threadIdx.x & (G - 1);
    const long row = ((long)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const bool active = row < (long)a.B * a.T;     // inactive groups still take part in the shuffles
    EvalSums sums;
#pragma unroll
    for (int j = 0; j < EvalSums::COUNT; ++j) sums.v[j] = 0.0;
    if (active) eval_row_share(a, row, gl, G, sums);
#pragma unroll
    for (int m = 1; m < G; m <<= 1) {
#pragma unroll
        for (int j = 0; j < EvalSums::COUNT; ++j) sums.v[j] += __shfl_xor(sums.v[j], m, 64);
    }
    if (active && gl == 0) eval_row_finish(sums, a.N, a.rowstats + row * EVAL_ROW_STATS);
}

__global__ void __launch_bounds__(64) bg_eval_fold_kernel(const double* __restrict__ rowstats, int B, int T, int N,
                                                          double* __restrict__ tables, double* __restrict__ accum) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 1 + EVAL_TABLES * T) return;
    const double v = eval_fold_value(rowstats, B, T, N, i);
    tables[i] = v;
    if (accum) accum[i] += (double)B * v;
}

__global__ void __launch_bounds__(256) bg_derivatives_kernel(const float* __restrict__ u, long total, int N, double two_dx,
                                                             double twelve_dx2, double* __restrict__ ux,
                                                             double* __restrict__ uxx) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int i = (int)(gid % N);
    double w[5];
    window(u + (gid - i), N, i, w);
    derivatives(w, two_dx, twelve_dx2, ux[gid], uxx[gid]);
}

template <int G>
void launch_rows(const EvalArgs& a, hipStream_t st) {
    const int block = 256, rows_per_block = block / G;
    const long rows = (long)a.B * a.T;
    const unsigned grid = (unsigned)((rows + rows_per_block - 1) / rows_per_block);
    hipLaunchKernelGGL(bg_eval_rows_kernel<G>, dim3(grid), dim3(block), 0, st, a);
}

constexpr long MAX_ROWS = 1L << 30;

bool good_dx(double dx) { return dx > 0.0 && std::isfinite(dx); }

// the refusals of bg_eval_rows and bg_eval_rows_host, and the launch arguments when there is none
int rows_args(const char* who, const bg_eval_batch* in, int B, int T, int N, double dx, double* rowstats, EvalArgs& a) {
    if (!in) return fail(-1, "%s: NULL batch", who);
    if (!in->truth || !in->pred || !rowstats) return fail(-1, "%s: NULL truth, pred or rowstats", who);
    if (B < 1 || T < 1) return fail(-1, "%s: a batch of %d x %d rows (at least 1 x 1)", who, B, T);
    if (N < 5) return fail(-1, "%s: rows of %d points (the stencils need at least 5)", who, N);
    if ((long)B * T > MAX_ROWS) return fail(-1, "%s: B * T = %ld rows is too many", who, (long)B * T);
    if (!good_dx(dx)) return fail(-1, "%s: dx = %g is not positive and finite", who, dx);
    if (in->inv_kind < 0 || in->inv_kind > 2) return fail(-1, "%s: inverse kind %d (0, 1 and 2 are known)", who, in->inv_kind);
    if (in->inv_kind != 0 && !in->inv_coef) return fail(-1, "%s: inverse kind %d without coefficients", who, in->inv_kind);
    if (in->pred_shift != 0 && in->pred_shift != 1) return fail(-1, "%s: pred_shift = %d (0 or 1)", who, in->pred_shift);
    if (in->truth_bstride < N || in->truth_tstride < N || in->pred_bstride < N || in->pred_tstride < N)
        return fail(-1, "%s: strides (%ld, %ld) and (%ld, %ld) below the row width %d", who, in->truth_bstride,
                    in->truth_tstride, in->pred_bstride, in->pred_tstride, N);
    for (const float* out : {(const float*)in->truth_out, (const float*)in->pred_out})
        if (out && (out == in->truth || out == in->pred)) return fail(-1, "%s: an output must not alias truth or pred", who);
    if (in->truth_out && in->truth_out == in->pred_out) return fail(-1, "%s: truth_out and pred_out must not alias", who);
    a.truth = in->truth; a.truth_bs = in->truth_bstride; a.truth_ts = in->truth_tstride;
    a.pred = in->pred; a.pred_bs = in->pred_bstride; a.pred_ts = in->pred_tstride;
    a.pred_shift = in->pred_shift; a.inv_kind = in->inv_kind; a.inv_coef = in->inv_coef;
    a.truth_out = in->truth_out; a.pred_out = in->pred_out;
    a.B = B; a.T = T; a.N = N;
    a.two_dx = 2.0 * dx; a.twelve_dx2 = 12.0 * (dx * dx);
    a.rowstats = rowstats;
    return 0;
}

int fold_args(const char* who, const double* rowstats, int B, int T, int N, const double* tables) {
    if (!rowstats || !tables) return fail(-1, "%s: NULL rowstats or tables", who);
    if (B < 1 || T < 1) return fail(-1, "%s: a batch of %d x %d rows (at least 1 x 1)", who, B, T);
    if (N < 5) return fail(-1, "%s: rows of %d points (at least 5)", who, N);
    if ((long)B * T > MAX_ROWS) return fail(-1, "%s: B * T = %ld rows is too many", who, (long)B * T);
    return 0;
}

int derivatives_args(const char* who, const float* u, int n_rows, int N, double dx, const double* ux, const double* uxx) {
    if (!u || !ux || !uxx) return fail(-1, "%s: NULL u, ux or uxx", who);
    if (n_rows < 1) return fail(-1, "%s: %d rows (at least 1)", who, n_rows);
    if (N < 5) return fail(-1, "%s: rows of %d points (the stencils need at least 5)", who, N);
    if ((long)n_rows * N > (1L << 38)) return fail(-1, "%s: %ld points are too many", who, (long)n_rows * N);
    if (!good_dx(dx)) return fail(-1, "%s: dx = %g is not positive and finite", who, dx);
    if (ux == uxx) return fail(-1, "%s: ux and uxx must not alias", who);
    return 0;
}

}  // namespace

extern "C" {

const char* bg_eval_last_error(void) { return g_err; }

int bg_eval_rows(void* stream, const bg_eval_batch* in, int B, int T, int N, double dx, double* rowstats) {
    EvalArgs a{};
    if (const int rc = rows_args("bg_eval_rows", in, B, T, N, dx, rowstats, a)) return rc;
    // the partition of ks_eval.hip's launch_eval_rows
    if (N <= 64) launch_rows<16>(a, (hipStream_t)stream);
    else if (N <= 512) launch_rows<32>(a, (hipStream_t)stream);
    else launch_rows<64>(a, (hipStream_t)stream);
    return launch_status(-2, "bg_eval_rows");
}

int bg_eval_fold(void* stream, const double* rowstats, int B, int T, int N, double* tables, double* accum) {
    if (const int rc = fold_args("bg_eval_fold", rowstats, B, T, N, tables)) return rc;
    const int block = 64, n = 1 + EVAL_TABLES * T;
    hipLaunchKernelGGL(bg_eval_fold_kernel, dim3((unsigned)((n + block - 1) / block)), dim3(block), 0, (hipStream_t)stream,
                       rowstats, B, T, N, tables, accum);
    return launch_status(-2, "bg_eval_fold");
}

int bg_derivatives(void* stream, const float* u, int n_rows, int N, double dx, double* ux, double* uxx) {
    if (const int rc = derivatives_args("bg_derivatives", u, n_rows, N, dx, ux, uxx)) return rc;
    const long total = (long)n_rows * N;
    hipLaunchKernelGGL(bg_derivatives_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, u,
                       total, N, 2.0 * dx, 12.0 * (dx * dx), ux, uxx);
    return launch_status(-2, "bg_derivatives");
}

int bg_eval_rows_host(const bg_eval_batch* in, int B, int T, int N, double dx, double* rowstats) {
    EvalArgs a{};
    if (const int rc = rows_args("bg_eval_rows_host", in, B, T, N, dx, rowstats, a)) return rc;
    for (long row = 0; row < (long)B * T; ++row) {
        EvalSums sums;
        for (int j = 0; j < EvalSums::COUNT; ++j) sums.v[j] = 0.0;
        eval_row_share(a, row, 0, 1, sums);
        eval_row_finish(sums, N, rowstats + row * EVAL_ROW_STATS);
    }
    return 0;
}

int bg_eval_fold_host(const double* rowstats, int B, int T, int N, double* tables, double* accum) {
    if (const int rc = fold_args("bg_eval_fold_host", rowstats, B, T, N, tables)) return rc;
    for (int i = 0; i < 1 + EVAL_TABLES * T; ++i) {
        const double v = eval_fold_value(rowstats, B, T, N, i);
        tables[i] = v;
        if (accum) accum[i] += (double)B * v;
    }
    return 0;
}

int bg_derivatives_host(const float* u, int n_rows, int N, double dx, double* ux, double* uxx) {
    if (const int rc = derivatives_args("bg_derivatives_host", u, n_rows, N, dx, ux, uxx)) return rc;
    const double two_dx = 2.0 * dx, twelve_dx2 = 12.0 * (dx * dx);
    for (long gid = 0; gid < (long)n_rows * N; ++gid) {
        const int i = (int)(gid % N);
        double w[5];
        window(u + (gid - i), N, i, w);
        derivatives(w, two_dx, twelve_dx2, ux[gid], uxx[gid]);
    }
    return 0;
}

}  // extern "C"
