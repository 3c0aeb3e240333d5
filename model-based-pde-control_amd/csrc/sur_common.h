// sur_common.h -- what every stage of the surrogate kernels uses: the STAMP macro and its buffers, TPB, LN_EPS, the DPP / swap
// lane reductions (group_sum2, group_sum1), sigmoid_ / tanh_, wrapi, and the global <-> LDS movers (lds_load, lds_dma_v4, lds_store,
// lds_load_v4).  Needs no other sur_*.h.
#ifndef SUR_COMMON_H
#define SUR_COMMON_H

#include <hip/hip_runtime.h>

#include <cmath>

// Diagnostic build only (-DSUR_STAMP): shader-clock stamps per phase for workgroup 0 of each launch,
// accumulated in a __device__ buffer nothing else reads (guide section 7, In-kernel stamps).
#ifdef SUR_STAMP
__device__ long long sur_stamp_buf[128];
__device__ long long sur_stamp_last;
#define STAMP(id)                                                                 \
    do {                                                                          \
        __syncthreads();                                                          \
        if (threadIdx.x == 0 && blockIdx.x == 0) {                                \
            const long long now_ = (long long)__builtin_amdgcn_s_memtime();       \
            sur_stamp_buf[id] += now_ - sur_stamp_last;                           \
            sur_stamp_last = now_;                                                \
        }                                                                         \
    } while (0)
#else
#define STAMP(id) do { } while (0)
#endif

namespace {

constexpr int TPB = 256;
constexpr float LN_EPS = 1e-5f;

template <int CTRL>
__device__ __forceinline__ float dpp_rot(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xf, 0xf, false));
}

// v + (v of lane ^ 16) / (v of lane ^ 32): the swap instructions exchange the odd rows of 16 (the upper 32 lanes) of their first
// operand with the even rows (the lower 32 lanes) of the second; on two copies of v that leaves [r0 r0 r2 r2] and [r1 r1 r3 r3]
typedef unsigned swap_u2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float swap_add16(float v) {
    const swap_u2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float swap_add32(float v) {
    const swap_u2 r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// sums of a and b over aligned groups of `lpc` lanes (16, 32 or 64); every lane gets both totals
__device__ __forceinline__ void group_sum2(float& a, float& b, int lpc) {
    a += dpp_rot<0x128>(a);  // row_ror:8
    b += dpp_rot<0x128>(b);
    a += dpp_rot<0x124>(a);  // row_ror:4
    b += dpp_rot<0x124>(b);
    a += dpp_rot<0x122>(a);  // row_ror:2
    b += dpp_rot<0x122>(b);
    a += dpp_rot<0x121>(a);  // row_ror:1
    b += dpp_rot<0x121>(b);
    if (lpc >= 32) {   // lane ^ 16: v_permlane16_swap of a value with itself (gfx950) -- same operands as a ds_bpermute exchange,
        a = swap_add16(a);   // without the trip through the LDS crossbar
        b = swap_add16(b);
    }
    if (lpc >= 64) {   // lane ^ 32
        a = swap_add32(a);
        b = swap_add32(b);
    }
}

// the same for one value: a reduction that has to wait for the result of another (the two-pass variance of sur_layernorm.h)
__device__ __forceinline__ void group_sum1(float& a, int lpc) {
    a += dpp_rot<0x128>(a);
    a += dpp_rot<0x124>(a);
    a += dpp_rot<0x122>(a);
    a += dpp_rot<0x121>(a);
    if (lpc >= 32) a = swap_add16(a);
    if (lpc >= 64) a = swap_add32(a);
}

// sigmoid / tanh on the hardware transcendentals (v_exp_f32, v_rcp_f32: ~1 ulp each) instead of libm's expf / tanhf and an
// IEEE division: 5 / 8 VALU instructions instead of ~25 / ~35.  These kernels are VALU-issue bound,
// SiLU / gate non-linearities are a third of their VALU work; parity against the golden tensors is unchanged
// (loss <= 1e-5 relative, gradients <= 2e-4 of the tensor scale: tests/test_surrogate_gpu.py).
#ifndef SUR_LIBM_ACTIVATIONS
__device__ __forceinline__ float sigmoid_(float x) { return __frcp_rn(1.0f + __expf(-x)); }
__device__ __forceinline__ float tanh_(float x) {
    const float t = __expf(-2.0f * fabsf(x));          // in (0, 1]: no overflow for any x
    return copysignf((1.0f - t) * __frcp_rn(1.0f + t), x);
}
#else
__device__ __forceinline__ float sigmoid_(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float tanh_(float x) { return tanhf(x); }
#endif
__device__ __forceinline__ int wrapi(int j, int n) { return j < 0 ? j + n : (j >= n ? j - n : j); }

// ---------------------------------------------------------------------------------------------
// block-cooperative copies between global memory and LDS
// ---------------------------------------------------------------------------------------------
__device__ void lds_load(float* dst, const float* __restrict__ src, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
}
// n4 float4 global -> LDS by LDS-DMA (global_load_lds_dwordx4: one wave instruction moves 64 x 16 B, no VGPRs in between), NOT
// waited for: any number of these may be in flight; lds_dma_wait() -- or any barrier behind an s_waitcnt vmcnt(0) -- completes
// them.  dst and src 16-byte aligned.
__device__ __forceinline__ void lds_dma_v4(float* dst, const float* __restrict__ src, int n4) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int j = wave; j * 64 < n4; j += nw) {
        const int i4 = j * 64 + lane;
        if (i4 < n4)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + 4 * i4),
                                             (__attribute__((address_space(3))) void*)(dst + 4 * i4), 16, 0, 0);
    }
}
__device__ __forceinline__ void lds_dma_wait() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}
__device__ void lds_store(float* __restrict__ dst, const float* src, int n) {
    if (dst)
        for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
}
// n4 float4 from global to LDS with all of a thread's loads of a round in flight before the first store
__device__ __forceinline__ void lds_load_v4(float* dst, const float* __restrict__ src, int n4) {
    constexpr int U = 4;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (int i0 = threadIdx.x; i0 < n4; i0 += U * TPB) {
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = s4[i0 + u * TPB < n4 ? i0 + u * TPB : i0];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (i0 + u * TPB < n4) d4[i0 + u * TPB] = v[u];
    }
    __syncthreads();
}

}  // namespace

#endif  // SUR_COMMON_H
