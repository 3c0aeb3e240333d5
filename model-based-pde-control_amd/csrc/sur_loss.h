// sur_loss.h -- the loss kernels: the TBPTT delta-mode loss (delta_loss_kernel, delta_loss_finish, delta_loss_finalize_kernel)
// and the validation loss (val_loss_kernel).  Needs sur_common.h and sur_loss_sums.h (the end of a loss workgroup).
#ifndef SUR_LOSS_H
#define SUR_LOSS_H

#include "sur_common.h"
#include "sur_loss_sums.h"

namespace {

// ---------------------------------------------------------------------------------------------
// TBPTT delta-mode loss: one launch for what the reference spells as ~30 tiny torch ops
// (pdecontrol/surrogates/training.py:100-121): true deltas from the state sequence, the undscaling
// forward, the element-wise MSE, its time-resolved and overall means, the four logged statistics and
// the gradient of the mean loss wrt the predicted deltas.
//   grid = T x nsplit workgroups: row t < T-1 handles time step t of all samples, row T-1 only zeroes the
//   (unused) last step's gradient.  Partial sums are fp64 and reduced in a fixed order by the
//   workgroup that arrives last (ticket counter), so the result does not depend on scheduling.
// ---------------------------------------------------------------------------------------------
constexpr int LOSS_NSUM = 5;  // squared error, sum / sum of squares of predicted deltas, same of true deltas
constexpr int LOSS_UNROLL = 4;
constexpr int LOSS_MAX_SPLIT = 8;

// wave_sum and loss_block_sums -- the end of a loss workgroup -- are sur_loss_sums.h's (shared with sur_decoded.hip)
static_assert(TPB == LOSS_TPB, "the loss kernels run sur_loss_sums.h's workgroup size");

__device__ void delta_loss_finish(int B, int T, int N, int nsplit, float* __restrict__ hsteploss, float* __restrict__ loss,
                                  float* __restrict__ stats, double* __restrict__ partial, unsigned int* __restrict__ ticket);

__global__ void __launch_bounds__(TPB)
delta_loss_kernel(const float* __restrict__ states, long sb, long st, const float* __restrict__ d_all, int B, int T, int N, float delta,
                  float mean, float stdv, float* __restrict__ deltas, float* __restrict__ dd_all,
                  float* __restrict__ hsteploss, float* __restrict__ loss, float* __restrict__ stats,
                  double* __restrict__ partial, unsigned int* __restrict__ ticket, int t0, int take_ticket) {
    // blockIdx.x = time step, blockIdx.y = slice of the B*N elements of that step; LOSS_UNROLL elements per
    // thread per round with every load of the round issued before the first use
    // a launch covers the time steps [t0, t0 + gridDim.x) of the T rows; the ticket counts the workgroups of ALL T rows, so
    // the launches of one loss (one per TBPTT chunk, in any order, on any streams) share the final reduction
    const int t = t0 + blockIdx.x, per_t = B * N, nsplit = gridDim.y;
    const double count = (double)per_t * (T - 1);
    double acc[LOSS_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const int stride = nsplit * TPB;
    if (t < T - 1) {
        const float gscale = (float)(2.0 / count);
        for (int e0 = blockIdx.y * TPB + threadIdx.x; e0 < per_t; e0 += LOSS_UNROLL * stride) {
            float s0[LOSS_UNROLL], s1[LOSS_UNROLL], od[LOSS_UNROLL];
#pragma unroll
            for (int u = 0; u < LOSS_UNROLL; ++u) {
                const int e = e0 + u * stride, ec = e < per_t ? e : e0;
                const int b = ec / N, i = ec - b * N;
                const size_t sidx = (size_t)b * sb + (size_t)t * st + i;   // states[b, t] (any batch / time strides)
                s0[u] = states[sidx];
                s1[u] = states[sidx + st];
                od[u] = d_all[((size_t)t * B + b) * N + i];
            }
#pragma unroll
            for (int u = 0; u < LOSS_UNROLL; ++u) {
                const int e = e0 + u * stride;
                if (e >= per_t) continue;
                const int b = e / N, i = e - b * N;
                const float dl = ((s1[u] - s0[u]) / delta - mean) / stdv;
                deltas[((size_t)b * (T - 1) + t) * N + i] = dl;
                const float err = od[u] - dl;
                if (dd_all) dd_all[((size_t)t * B + b) * N + i] = gscale * err;
                acc[0] += (double)(err * err);
                acc[1] += od[u];
                acc[2] += (double)od[u] * od[u];
                acc[3] += dl;
                acc[4] += (double)dl * dl;
            }
        }
    } else if (dd_all) {
        for (int e = blockIdx.y * TPB + threadIdx.x; e < per_t; e += stride) dd_all[(size_t)t * per_t + e] = 0.0f;
    }
    // without a ticket the caller finishes the loss with delta_loss_finalize_kernel, off its critical path
    if (!loss_block_sums(acc, partial + ((size_t)t * nsplit + blockIdx.y) * LOSS_NSUM, ticket, T * nsplit, take_ticket != 0)) return;
    __threadfence();
    delta_loss_finish(B, T, N, nsplit, hsteploss, loss, stats, partial, ticket);
}

// fixed-order reduction of the (T-1) x nsplit partial sums: by the workgroup that arrived last, or by a launch of its own
__device__ void delta_loss_finish(int B, int T, int N, int nsplit, float* __restrict__ hsteploss, float* __restrict__ loss,
                                  float* __restrict__ stats, double* __restrict__ partial, unsigned int* __restrict__ ticket) {
    const int per_t = B * N;
    const double count = (double)per_t * (T - 1);
    // fixed-order reduction of the (T-1) x nsplit partial sums by the workgroup that arrived last.  The partials are
    // fetched with relaxed device-scope atomic loads, one partial per thread, so the loads overlap (a serial loop
    // of volatile loads cost ~20 us here).
    auto peek = [&](size_t i) { return __hip_atomic_load(partial + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    __shared__ double tsum[LOSS_NSUM];
    __shared__ double stage[LOSS_NSUM][TPB];
    for (int tt = threadIdx.x; tt < T - 1; tt += blockDim.x) {
        double se = 0.0;
        for (int y = 0; y < nsplit; ++y) se += peek(((size_t)tt * nsplit + y) * LOSS_NSUM);
        hsteploss[tt] = (float)(se / per_t);
    }
    const int nq = (T - 1) * nsplit;
    double tot = 0.0;
    for (int q0 = 0; q0 < nq; q0 += TPB) {
        const int q = q0 + threadIdx.x;
#pragma unroll
        for (int j = 0; j < LOSS_NSUM; ++j) stage[j][threadIdx.x] = q < nq ? peek((size_t)q * LOSS_NSUM + j) : 0.0;
        __syncthreads();
        if (threadIdx.x < LOSS_NSUM) {
            const int lim = nq - q0 < TPB ? nq - q0 : TPB;
            for (int i = 0; i < lim; ++i) tot += stage[threadIdx.x][i];
        }
        __syncthreads();
    }
    if (threadIdx.x < LOSS_NSUM) tsum[threadIdx.x] = tot;
    __syncthreads();
    if (threadIdx.x == 0) {
        *loss = (float)(tsum[0] / count);
        const double m_od = tsum[1] / count, m_dl = tsum[3] / count;
        stats[0] = (float)m_od;
        stats[1] = (float)sqrt(fmax(tsum[2] - count * m_od * m_od, 0.0) / (count - 1.0));  // unbiased, like Tensor.std()
        stats[2] = (float)m_dl;
        stats[3] = (float)sqrt(fmax(tsum[4] - count * m_dl * m_dl, 0.0) / (count - 1.0));
        *ticket = 0u;  // ready for the next launch (graph replay)
    }
}

__global__ void __launch_bounds__(TPB)
delta_loss_finalize_kernel(int B, int T, int N, int nsplit, float* __restrict__ hsteploss, float* __restrict__ loss,
                           float* __restrict__ stats, double* __restrict__ partial, unsigned int* __restrict__ ticket) {
    delta_loss_finish(B, T, N, nsplit, hsteploss, loss, stats, partial, ticket);
}

// ---------------------------------------------------------------------------------------------
// The loss section of validation_step as one launch (reference: pdecontrol/surrogates/training.py:132-174; ~15 torch
// ops per batch): the IC-augmented prediction decoded[t] = states[0] (t = 0) / out_all[t-1], the true deltas through the
// undscaling forward, the delta loss, the scaled loss, the inverse observation scaling of both sides (the affine map in
// its four separately rounded steps: val_affine below) and the unscaled loss with its per-step means.
//   grid = T x nsplit workgroups, row t = time step t of all samples; three fp64 partial sums per workgroup, reduced in a
//   fixed order by the workgroup that arrives last (ticket counter), which is also the single writer of the caller's
//   epoch accumulator: accum[0..2] += the batch's (unscaled, scaled, delta) error sums, accum[3 + t] += step t's.
// ---------------------------------------------------------------------------------------------
constexpr int VAL_NSUM = 3;   // squared errors: unscaled, scaled, delta

// ScaleTransform._affine's  ((v - a) / (b - a)) * (d - c) + c  in four separately rounded fp32 steps.  This file is built
// with the compiler's default contraction, under which the _rn intrinsics (plain operators of the compiler's own headers)
// fuse once inlined; the operators below are written out under a contract(off) of their own, so the multiply and the add
// stay two roundings and `decoded` has the bits of the host transform.
__device__ __forceinline__ float val_affine(const float* __restrict__ coef, int n, int i, float v) {
#pragma clang fp contract(off)
    if (!coef) return v;
    const float q = (v - coef[i]) / coef[n + i];
    const float m = q * coef[2 * n + i];
    return m + coef[3 * n + i];
}

__global__ void __launch_bounds__(TPB)
val_loss_kernel(const float* __restrict__ states, long sb, long st, const float* __restrict__ out_all,
                const float* __restrict__ d_all, int B, int T, int N, float delta, float mean, float stdv,
                const float* __restrict__ inv_coef, float* __restrict__ deltas, float* __restrict__ decoded,
                float* __restrict__ hsteploss, float* __restrict__ loss, float* __restrict__ scalars,
                double* __restrict__ accum, double* __restrict__ partial, unsigned int* __restrict__ ticket) {
    const int t = blockIdx.x, per_t = B * N, nsplit = gridDim.y;
    double acc[VAL_NSUM] = {0.0, 0.0, 0.0};
    for (int e = blockIdx.y * TPB + threadIdx.x; e < per_t; e += nsplit * TPB) {
        const int b = e / N, i = e - b * N;
        const size_t sidx = (size_t)b * sb + (size_t)t * st + i;           // states[b, t] (any batch / time strides)
        const float s0 = states[sidx];
        const float dec = t == 0 ? s0 : out_all[((size_t)(t - 1) * B + b) * N + i];
        const float es = __fsub_rn(dec, s0);
        const float ud = val_affine(inv_coef, N, i, dec);
        const float eu = __fsub_rn(ud, val_affine(inv_coef, N, i, s0));
        if (decoded) decoded[((size_t)b * T + t) * N + i] = ud;
        acc[0] += (double)__fmul_rn(eu, eu);
        acc[1] += (double)__fmul_rn(es, es);
        if (t < T - 1) {
            const float dl = __fdiv_rn(__fsub_rn(__fdiv_rn(__fsub_rn(states[sidx + st], s0), delta), mean), stdv);
            if (deltas) deltas[((size_t)b * (T - 1) + t) * N + i] = dl;
            const float ed = __fsub_rn(d_all[((size_t)t * B + b) * N + i], dl);
            acc[2] += (double)__fmul_rn(ed, ed);
        }
    }
    if (!loss_block_sums(acc, partial + ((size_t)t * nsplit + blockIdx.y) * VAL_NSUM, ticket, T * nsplit)) return;
    __threadfence();

    // the last workgroup: per-step sums by one thread per step (fixed order over the slices), then the three totals by
    // threads 0..2 in step order.  The partials are fetched with relaxed device-scope atomic loads (see delta_loss_finish).
    auto peek = [&](size_t i) { return __hip_atomic_load(partial + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    __shared__ double stage[VAL_NSUM][TPB];
    double tot = 0.0;
    for (int t0 = 0; t0 < T; t0 += TPB) {
        const int tt = t0 + threadIdx.x;
        double sums[VAL_NSUM] = {0.0, 0.0, 0.0};
        if (tt < T) {
            for (int y = 0; y < nsplit; ++y)
#pragma unroll
                for (int j = 0; j < VAL_NSUM; ++j) sums[j] += peek(((size_t)tt * nsplit + y) * VAL_NSUM + j);
            hsteploss[tt] = (float)(sums[0] / per_t);
            if (accum) accum[VAL_NSUM + tt] += sums[0];
        }
#pragma unroll
        for (int j = 0; j < VAL_NSUM; ++j) stage[j][threadIdx.x] = sums[j];
        __syncthreads();
        if (threadIdx.x < VAL_NSUM) {
            const int lim = T - t0 < TPB ? T - t0 : TPB;
            for (int i = 0; i < lim; ++i) tot += stage[threadIdx.x][i];
        }
        __syncthreads();
    }
    if (threadIdx.x < VAL_NSUM) {
        const double count = (double)per_t * (threadIdx.x == 2 ? T - 1 : T);
        if (threadIdx.x == 0) *loss = (float)(tot / count);
        else scalars[threadIdx.x - 1] = (float)(tot / count);
        if (accum) accum[threadIdx.x] += tot;
    }
    if (threadIdx.x == 0) *ticket = 0u;   // ready for the next launch
}

}  // namespace

#endif  // SUR_LOSS_H
