// row_ops.h -- the arithmetic of the wrapper stack that replay.hip, rollout.hip and collect.hip share: inline device and
// host helpers only, no kernels, no C ABI.  In all three a wave owns a row and lanes run along its columns.
//
// The affine map is ScaleTransform._affine's  out = ((v - a) / (b - a)) * (d - c) + c  as four separately rounded fp32
// operations (__fsub_rn, __fdiv_rn, __fmul_rn, __fadd_rn), so a kernel's result equals the host transform's bit for bit.
// Every file that includes this header must be built with the Makefile's EXACT (-ffp-contract=off): the intrinsics pin
// the map itself, the flag keeps the expressions around it from being contracted.
#ifndef ROW_OPS_H
#define ROW_OPS_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int WAVE = 64;
constexpr int WAVES = 4;               // rows per workgroup
constexpr int NT = WAVE * WAVES;

__device__ __forceinline__ float affine(float v, float a, float ba, float dc, float c)
{
    return __fadd_rn(__fmul_rn(__fdiv_rn(__fsub_rn(v, a), ba), dc), c);
}

// column j of n: coef is [4][n] = (a, b - a, d - c, c) per column, or NULL for the identity
__device__ __forceinline__ float affine_col(const float* __restrict__ coef, int n, int j, float v)
{
    return coef ? affine(v, coef[j], coef[n + j], coef[2 * n + j], coef[3 * n + j]) : v;
}

// columns j ... j + 3: j and n multiples of 4, coef 16-byte aligned
__device__ __forceinline__ f4 affine_col4(const float* __restrict__ coef, int n, int j, f4 v)
{
    if (!coef) return v;
    const f4 a = *reinterpret_cast<const f4*>(coef + j);
    const f4 ba = *reinterpret_cast<const f4*>(coef + n + j);
    const f4 dc = *reinterpret_cast<const f4*>(coef + 2 * n + j);
    const f4 c = *reinterpret_cast<const f4*>(coef + 3 * n + j);
    v.x = affine(v.x, a.x, ba.x, dc.x, c.x);
    v.y = affine(v.y, a.y, ba.y, dc.y, c.y);
    v.z = affine(v.z, a.z, ba.z, dc.z, c.z);
    v.w = affine(v.w, a.w, ba.w, dc.w, c.w);
    return v;
}

// a NULL pointer counts as aligned
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// columns a sensor (start, stride) keeps of a row of n
inline int width_of(int n, int start, int stride) { return (n - start + stride - 1) / stride; }

}  // namespace

#endif
