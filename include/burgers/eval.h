/*
 * burgers/eval.h -- the test-phase entries of libburgers_hip.so (kernels: csrc/bg_eval.hip; arithmetic: csrc/bg_eval.h;
 * binding: pdegym/burgers/_hip.py, EVAL_SYMBOLS).  An extension of ../burgers_hip.h: the metric section of
 * PDETrainingModule.test_step for a Burgers env as two launches, and the derivatives behind env.rhs.  The counterpart of
 * ks_eval_rows_device / ks_eval_fold_device (../kspde.h) without a handle.
 *
 * For a row (b, t): s is the inverse-scaled truth, o the inverse-scaled prediction aligned with it (with pred_shift,
 * step 0 is the truth row itself and step t >= 1 is prediction row t - 1).  Both are fp32 through one of three inverse
 * kinds: 0 identity; 1 ScaleTransform._affine with inv_coef [4][N] = (a, b - a, d - c, c), four separately rounded steps
 * ((v - a) / (b - a)) * (d - c) + c; 2 Normalize._inv with inv_coef [2][N] = (s, m), two steps v * s + m.
 *
 * rowstats [B][T][BG_EVAL_ROW_STATS] fp64:
 *    0 ..  3   sum|e|, sum e^2, sum|s|, sum s^2 with e = (double)(o - s) of the fp32 difference and s widened to fp64
 *    4,    5   the l2control reward of s and of o: (double)(float)(-1.0 * (1.0 / N) * sum u^2)
 *    6 ..  9   for u_x:  sum|ds - do|, sum (ds - do)^2, sum|ds|, sum ds^2
 *   10 .. 13   the same four for u_xx
 * The derivatives are taken in fp64 from the widened fp32 values, periodic, with the stencils of ../burgers_hip.h:
 *   u_x = (u[+1] - u[-1]) / (2 dx),   u_xx = (-u[-2] + 16 u[-1] - 30 u[0] + 16 u[+1] - u[+2]) / (12 dx^2).
 *
 * tables [1 + BG_EVAL_TABLES * T] fp64: the MSE, then [T] each, in the order of the dict test_step returns:
 *   l1_loss, l2_loss, l1_loss_scaled, l2_loss_scaled, nrmse (means over the batch of the row norms),
 *   l1_loss_rews, l2_loss_rews, l1_loss_scaled_rews, l2_loss_scaled_rews, nrmse_rews (norms over the batch),
 *   then for l1_loss_derivs, l2_loss_derivs, l1_loss_scaled_derivs, l2_loss_scaled_derivs, nrms_derivs:
 *   -derivative-0 (u_x), -derivative-1 (u_xx).   A zero norm divides as IEEE does.
 *
 * bg_eval_rows      one group of 16 (N <= 64), 32 (N <= 512) or 64 lanes per row; lane gl takes the points gl, gl + G, ...;
 *                   the partial sums are reduced by xor shuffles inside the group and lane 0 writes.  Any N >= 5.
 * bg_eval_fold      one thread per output value walks the batch in index order; accum (or NULL) [1 + 20 T] += B * value.
 * bg_derivatives    u [n_rows][N] fp32 -> ux, uxx [n_rows][N] fp64, one thread per point.
 * No atomics, no ticket, no grid barrier: the same bits on every run.  The launches are asynchronous on the given
 * hipStream_t, take DEVICE pointers, do not synchronise and do not allocate.
 *
 * The *_host entries run the same arithmetic serially on HOST memory (every pointer of the struct a host pointer) and
 * make no HIP call; bg_eval_fold and bg_derivatives have their bits, bg_eval_rows their sums in another order.
 *
 * Return 0, -1 for a refusal, -2 when the launch failed; bg_eval_last_error() holds the text.  Every refusal is made on
 * the host before any HIP call, with a message that starts with the entry's name: NULL in / truth / pred / rowstats /
 * tables / u / ux / uxx; B < 1, T < 1, N < 5; dx not positive and finite; inv_kind outside 0 ... 2 or non-zero with a NULL
 * inv_coef; pred_shift outside 0 / 1; a batch or time stride below N; truth_out or pred_out equal to truth, pred or each
 * other; more than 2^30 rows.
 *
 * It is declared here and not in burgers_hip.h because that header's list of functions is pinned, name by name;
 * tests/test_bg_eval_host.py holds this header, its binding table and the library to each other.
 */
#ifndef BURGERS_EVAL_H
#define BURGERS_EVAL_H

#include "../burgers_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BG_EVAL_ROW_STATS 14
#define BG_EVAL_TABLES    20

typedef struct bg_eval_batch {            /* host struct of device (or, for *_host, host) pointers */
    const float* truth; long truth_bstride, truth_tstride;   /* row (b, t) at truth + b * bstride + t * tstride */
    const float* pred;  long pred_bstride,  pred_tstride;
    int pred_shift;
    int inv_kind; const float* inv_coef;   /* 0 / 1: [4][N] / 2: [2][N] */
    float* truth_out; float* pred_out;     /* [B][T][N] inverse-scaled rows, or NULL */
} bg_eval_batch;

int bg_eval_rows(void* stream, const bg_eval_batch* in, int B, int T, int N, double dx, double* rowstats);
int bg_eval_fold(void* stream, const double* rowstats, int B, int T, int N, double* tables, double* accum);
int bg_derivatives(void* stream, const float* u, int n_rows, int N, double dx, double* ux, double* uxx);
int bg_eval_rows_host(const bg_eval_batch* in, int B, int T, int N, double dx, double* rowstats);
int bg_eval_fold_host(const double* rowstats, int B, int T, int N, double* tables, double* accum);
int bg_derivatives_host(const float* u, int n_rows, int N, double dx, double* ux, double* uxx);

const char* bg_eval_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
