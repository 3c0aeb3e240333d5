// sur_decoded.hip -- the decoded-mode TBPTT loss of the latent surrogate (LatentAutoRegPDESurrogate, the
// KSLatentConvolutionalLSTM ablation) and the deltas of its rollout: sur_tbptt_decoded_loss and sur_latent_deltas of
// include/surrogate_hip.h (binding: pdecontrol/surrogates/hipops.py).
//
// Reference: pdecontrol/surrogates/training.py:100-121 with training_mode == "decoded" -- the MSE of the IC-augmented
// prediction against the states, its mean per time step, the predicted deltas as the chunk loop's
// dscaling.Inverse(diff(cat(states[:, :1], outputs)) / delta) yields them, the true deltas and the four logged statistics:
// ~25 torch ops per step.  Here one launch, laid out as the delta loss of sur_kernels.hip: grid = T x nsplit workgroups,
// row t = time step t of all samples, LOSS_NSUM fp64 partial sums per workgroup, reduced in a fixed order by the workgroup
// that takes the last ticket (sur_loss_sums.h).
//
// Every elementwise value is fp32 with one rounding per operation.  The gradient scale times the error is the only
// multiply next to an add or a subtraction; the Makefile compiles this translation unit with EXACT (-ffp-contract=off) and
// the pragma below says the same for this file's own expressions, so no two operations fuse.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>

#include "../../include/surrogate_hip.h"
#include "capi_error.h"
#include "sur_loss_sums.h"

namespace {

constexpr int TPB = LOSS_TPB;
constexpr int NSUM = 5;        // squared error; sum / sum of squares of the predicted deltas; the same of the true deltas
constexpr int UNROLL = 4;      // elements per thread per round, every load of the round issued before the first use
constexpr int MAX_SPLIT = 8;   // workgroups per time step: `partial` holds NSUM * MAX_SPLIT = 40 doubles per step

__device__ __forceinline__ float scaled_delta(float next, float prev, float delta, float mean, float stdv) {
    return ((next - prev) / delta - mean) / stdv;
}

__global__ void __launch_bounds__(TPB)
decoded_loss_kernel(const float* __restrict__ states, long sb, long st, const float* __restrict__ out_all, int B, int T, int N,
                    float delta, float mean, float stdv, float* __restrict__ outdeltas, float* __restrict__ deltas,
                    float* __restrict__ dout_all, float* __restrict__ hsteploss, float* __restrict__ loss,
                    float* __restrict__ stats, double* __restrict__ partial, unsigned int* __restrict__ ticket) {
    // blockIdx.x = time step t, blockIdx.y = slice of the B*N elements of that step.  Row t owns: the squared error of step
    // t (prev[t] - states[t]), and for t < T-1 the two deltas of the transition t -> t+1 and row t of dout_all, which is the
    // gradient of step t+1's error (out_all[t] is prev[t+1]).
    const int t = blockIdx.x, per_t = B * N, nsplit = gridDim.y;
    const double count = (double)per_t * T;
    const float gscale = (float)(2.0 / count);
    const bool inner = t < T - 1;
    double acc[NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const int stride = nsplit * TPB;
    for (int e0 = blockIdx.y * TPB + threadIdx.x; e0 < per_t; e0 += UNROLL * stride) {
        float s0[UNROLL], s1[UNROLL], pv[UNROLL], ot[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int e = e0 + u * stride, ec = e < per_t ? e : e0;
            const int b = ec / N, i = ec - b * N;
            const size_t sidx = (size_t)b * sb + (size_t)t * st + i;            // states[b, t] (any batch / time strides)
            s0[u] = states[sidx];
            s1[u] = inner ? states[sidx + st] : 0.0f;
            pv[u] = t == 0 ? s0[u] : out_all[((size_t)(t - 1) * B + b) * N + i];  // prev[b, t]
            ot[u] = inner ? out_all[((size_t)t * B + b) * N + i] : 0.0f;         // row T-1 of out_all is not read
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int e = e0 + u * stride;
            if (e >= per_t) continue;
            const int b = e / N, i = e - b * N;
            const float err = pv[u] - s0[u];                                     // step 0: the same value twice, exactly 0
            acc[0] += (double)(err * err);
            const size_t tidx = ((size_t)t * B + b) * N + i;
            if (!inner) {
                if (dout_all) dout_all[tidx] = 0.0f;
                continue;
            }
            const float od = scaled_delta(ot[u], pv[u], delta, mean, stdv);
            const float dl = scaled_delta(s1[u], s0[u], delta, mean, stdv);
            const size_t didx = ((size_t)b * (T - 1) + t) * N + i;
            outdeltas[didx] = od;
            deltas[didx] = dl;
            if (dout_all) dout_all[tidx] = gscale * (ot[u] - s1[u]);
            acc[1] += od;
            acc[2] += (double)od * od;
            acc[3] += dl;
            acc[4] += (double)dl * dl;
        }
    }
    if (!loss_block_sums(acc, partial + ((size_t)t * nsplit + blockIdx.y) * NSUM, ticket, T * nsplit)) return;
    __threadfence();

    // The workgroup that arrived last: fixed-order reduction of the T x nsplit partial sums.  The partials are fetched with
    // relaxed device-scope atomic loads, one per thread, so the loads overlap and none is served from this CU's L1.
    auto peek = [&](size_t i) { return __hip_atomic_load(partial + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    __shared__ double tsum[NSUM];
    __shared__ double stage[NSUM][TPB];
    for (int tt = threadIdx.x; tt < T; tt += TPB) {
        double se = 0.0;
        for (int y = 0; y < nsplit; ++y) se += peek(((size_t)tt * nsplit + y) * NSUM);
        hsteploss[tt] = (float)(se / per_t);
    }
    const int nq = T * nsplit;      // row T-1 carries zeros in the four delta sums
    double tot = 0.0;
    for (int q0 = 0; q0 < nq; q0 += TPB) {
        const int q = q0 + threadIdx.x;
#pragma unroll
        for (int j = 0; j < NSUM; ++j) stage[j][threadIdx.x] = q < nq ? peek((size_t)q * NSUM + j) : 0.0;
        __syncthreads();
        if (threadIdx.x < NSUM) {
            const int lim = nq - q0 < TPB ? nq - q0 : TPB;
            for (int i = 0; i < lim; ++i) tot += stage[threadIdx.x][i];
        }
        __syncthreads();
    }
    if (threadIdx.x < NSUM) tsum[threadIdx.x] = tot;
    __syncthreads();
    if (threadIdx.x == 0) {
        *loss = (float)(tsum[0] / count);
        const double dcount = (double)per_t * (T - 1);
        const double m_od = tsum[1] / dcount, m_dl = tsum[3] / dcount;
        stats[0] = (float)m_od;
        stats[1] = (float)sqrt(fmax(tsum[2] - dcount * m_od * m_od, 0.0) / (dcount - 1.0));   // unbiased, like Tensor.std()
        stats[2] = (float)m_dl;
        stats[3] = (float)sqrt(fmax(tsum[4] - dcount * m_dl * m_dl, 0.0) / (dcount - 1.0));
        *ticket = 0u;   // ready for the next launch (graph replay)
    }
}

// d_all[k, b] = ((out_all[k, b] - prev) / delta - mean) / stdv with prev = state0[b] for k = 0 and out_all[k-1, b] after it
__global__ void __launch_bounds__(TPB)
latent_deltas_kernel(const float* __restrict__ state0, long sb, const float* __restrict__ out_all, int K, int B, int N, float delta,
                     float mean, float stdv, float* __restrict__ d_all) {
    const int per_k = B * N;
    const size_t total = (size_t)K * per_k;
    for (size_t e = (size_t)blockIdx.x * TPB + threadIdx.x; e < total; e += (size_t)gridDim.x * TPB) {
        const int k = (int)(e / per_k), r = (int)(e - (size_t)k * per_k);
        const int b = r / N, i = r - b * N;
        const float prev = k == 0 ? state0[(size_t)b * sb + i] : out_all[e - per_k];
        d_all[e] = scaled_delta(out_all[e], prev, delta, mean, stdv);
    }
}

// capi_error.h's fail(), written into the buffer sur_last_error() hands out (sur_kernels.hip owns that one; the header gives
// every translation unit a thread-local g_err of its own, all of sizeof(g_err) bytes)
__attribute__((format(printf, 2, 3))) int dec_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(const_cast<char*>(sur_last_error()), sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int dec_launch_status(const char* who) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : dec_fail(-2, "%s launch failed: %s", who, hipGetErrorString(e));
}

}  // namespace

extern "C" {

int sur_tbptt_decoded_loss(void* stream, const float* states, long states_bstride, long states_tstride, const float* out_all, int b,
                           int t, int n, float delta, float mean, float stdv, float* outdeltas, float* deltas, float* dout_all,
                           float* hsteploss, float* loss, float* stats, double* partial, unsigned int* ticket) {
    if (!states || !out_all || !outdeltas || !deltas || !hsteploss || !loss || !stats || !partial || !ticket)
        return dec_fail(-1, "sur_tbptt_decoded_loss: a required pointer is NULL (only dout_all may be)");
    if (b <= 0 || t < 2 || n <= 0) return dec_fail(-1, "sur_tbptt_decoded_loss: B = %d, T = %d, N = %d (need B > 0, T >= 2, N > 0)", b, t, n);
    if ((long)b * n > 0x7fffffffL / 2) return dec_fail(-1, "sur_tbptt_decoded_loss: B * N = %ld elements per step is too many", (long)b * n);
    if (states_bstride < n || states_tstride < n) return dec_fail(-1, "sur_tbptt_decoded_loss: state strides must be at least N");
    if (!(delta < 0.0f || delta > 0.0f) || !(stdv > 0.0f)) return dec_fail(-1, "sur_tbptt_decoded_loss: delta must be non-zero and std positive");
    int nsplit = (b * n + UNROLL * TPB - 1) / (UNROLL * TPB);
    nsplit = nsplit < 1 ? 1 : (nsplit > MAX_SPLIT ? MAX_SPLIT : nsplit);
    hipLaunchKernelGGL(decoded_loss_kernel, dim3(t, nsplit), dim3(TPB), 0, (hipStream_t)stream, states, states_bstride, states_tstride,
                       out_all, b, t, n, delta, mean, stdv, outdeltas, deltas, dout_all, hsteploss, loss, stats, partial, ticket);
    return dec_launch_status("sur_tbptt_decoded_loss");
}

int sur_latent_deltas(void* stream, const float* state0, long state_bstride, const float* out_all, int k, int b, int n, float delta,
                      float mean, float stdv, float* d_all) {
    if (!state0 || !out_all || !d_all) return dec_fail(-1, "sur_latent_deltas: a NULL pointer");
    if (k <= 0 || b <= 0 || n <= 0) return dec_fail(-1, "sur_latent_deltas: K = %d, B = %d, N = %d must be positive", k, b, n);
    if ((long)b * n > 0x7fffffffL / 2) return dec_fail(-1, "sur_latent_deltas: B * N = %ld elements per step is too many", (long)b * n);
    if (state_bstride < n) return dec_fail(-1, "sur_latent_deltas: the state stride must be at least N");
    if (!(delta < 0.0f || delta > 0.0f) || !(stdv > 0.0f)) return dec_fail(-1, "sur_latent_deltas: delta must be non-zero and std positive");
    const size_t total = (size_t)k * b * n;
    const size_t want = (total + TPB - 1) / TPB;
    const unsigned grid = (unsigned)(want > 2048 ? 2048 : want);
    hipLaunchKernelGGL(latent_deltas_kernel, dim3(grid), dim3(TPB), 0, (hipStream_t)stream, state0, state_bstride, out_all, k, b, n,
                       delta, mean, stdv, d_all);
    return dec_launch_status("sur_latent_deltas");
}

}  // extern "C"
