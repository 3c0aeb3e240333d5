// sur_params.h -- parameter staging: a module's weights copied into LDS once per workgroup (ParamViews, stage_weights), its
// gradient accumulators (setup_grads), their way into the workgroup's partial row (add_to_row) and psize_of.
// Needs sur_common.h.
#ifndef SUR_PARAMS_H
#define SUR_PARAMS_H

#include "sur_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// parameter staging: weights of a module are copied into LDS once per workgroup; gradient
// accumulators live either in LDS (flushed into the workgroup's partial row at the end) or, when LDS
// is too small, directly in the partial row (owner-exclusive read-modify-write, no atomics).
// ---------------------------------------------------------------------------------------------
template <int NP>
struct ParamViews {
    const float* w[NP];  // LDS copies of the weights
    float* g[NP];        // gradient accumulators (LDS or partial row); unset in forward kernels
};

template <int NP>
__device__ void stage_weights(const float* const* gw, const int* size, float* lds_w, ParamViews<NP>& v) {
    int off = 0;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        v.w[i] = lds_w + off;
        off += size[i];
    }
    // first TPB elements of every parameter (all of it for the small ones): NP independent loads in flight at once
    float head[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) head[i] = (int)threadIdx.x < size[i] ? gw[i][threadIdx.x] : 0.0f;
#pragma unroll
    for (int i = 0; i < NP; ++i)
        if ((int)threadIdx.x < size[i]) const_cast<float*>(v.w[i])[threadIdx.x] = head[i];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        float* dst = const_cast<float*>(v.w[i]);
        for (int j = threadIdx.x + TPB; j < size[i]; j += 4 * TPB) {   // the tails of the large ones, four loads per round
            float t[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) t[u] = j + u * TPB < size[i] ? gw[i][j + u * TPB] : 0.0f;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (j + u * TPB < size[i]) dst[j + u * TPB] = t[u];
        }
    }
    __syncthreads();
}

template <int NP>
__device__ void setup_grads(const int* size, float* base, bool zero, ParamViews<NP>& v) {
    int off = 0;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        v.g[i] = base + off;
        off += size[i];
    }
    if (zero)
        for (int j = threadIdx.x; j < off; j += blockDim.x) base[j] = 0.0f;
    __syncthreads();
}

// row[j] += acc[j] for the workgroup's partial-gradient row.  The global loads of a batch are all issued before
// the first add/store: as a plain loop this read-modify-write paid one HBM round trip per iteration (20-30 of them).
__device__ __forceinline__ void add_to_row(float* __restrict__ row, const float* acc, int psize) {
    constexpr int U = 8;
    for (int j0 = threadIdx.x; j0 < psize; j0 += U * TPB) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * TPB;
            v[u] = j < psize ? row[j] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * TPB;
            if (j < psize) row[j] = v[u] + acc[j];
        }
    }
}

template <int NP>
__host__ __device__ inline int psize_of(const int* size) {
    int t = 0;
    for (int i = 0; i < NP; ++i) t += size[i];
    return t;
}

}  // namespace

#endif  // SUR_PARAMS_H
