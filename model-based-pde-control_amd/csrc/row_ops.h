// row_ops.h -- the arithmetic of the wrapper stack that the controller-loop kernels share: inline device and host helpers
// only, no kernels, no C ABI.  Includers: replay.hip (affine map, row copy), rollout.hip (affine map, forcing chain),
// collect.hip (affine map), sur_windows.hip (affine map, row copy, forcing chain); place_rows.h (the row placement of
// replay.hip, ks_record.hip and burgers.hip) takes f4, the wave / workgroup constants and, for its includers' launches,
// aligned16.  In all of them a wave owns a row and lanes run along its columns.
//
// The affine map is ScaleTransform._affine's  out = ((v - a) / (b - a)) * (d - c) + c  as four separately rounded fp32
// operations (__fsub_rn, __fdiv_rn, __fmul_rn, __fadd_rn), so a kernel's result equals the host transform's bit for bit.
// The forcing chain is GaussianForcing's  sum over m of affine(act[m]) * f[m][column]  as one rounded product and then one
// fmaf per further actuator in index order: the one spelling ro_act_chain, the dissipation settle kernel and the window
// gather must share with each other and with the host.  The row copy is the sensor followed by the affine map.
// Every file that uses the arithmetic of this header must be built with the Makefile's EXACT (-ffp-contract=off): the
// intrinsics pin the operations themselves, the flag keeps the expressions around them from being contracted.
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

// the Gaussian forcing of the scaled action at the one column f[0]: f is [A][ld], in_coef [4][A] or NULL
__device__ __forceinline__ float forcing_col(const float* __restrict__ in_coef, int A, const float* __restrict__ act,
                                             const float* __restrict__ f, int ld)
{
    float acc = __fmul_rn(affine_col(in_coef, A, 0, act[0]), f[0]);
    for (int m = 1; m < A; ++m) acc = __fmaf_rn(affine_col(in_coef, A, m, act[m]), f[(long)m * ld], acc);
    return acc;
}

// the same at the four columns f[0 ... 3]: f 16-byte aligned, ld a multiple of 4
__device__ __forceinline__ f4 forcing_col4(const float* __restrict__ in_coef, int A, const float* __restrict__ act,
                                           const float* __restrict__ f, int ld)
{
    const float a0 = affine_col(in_coef, A, 0, act[0]);
    const f4 f0 = *reinterpret_cast<const f4*>(f);
    f4 acc;
    acc.x = __fmul_rn(a0, f0.x);
    acc.y = __fmul_rn(a0, f0.y);
    acc.z = __fmul_rn(a0, f0.z);
    acc.w = __fmul_rn(a0, f0.w);
    for (int m = 1; m < A; ++m) {
        const float am = affine_col(in_coef, A, m, act[m]);
        const f4 fm = *reinterpret_cast<const f4*>(f + (long)m * ld);
        acc.x = __fmaf_rn(am, fm.x, acc.x);
        acc.y = __fmaf_rn(am, fm.y, acc.y);
        acc.z = __fmaf_rn(am, fm.z, acc.z);
        acc.w = __fmaf_rn(am, fm.w, acc.w);
    }
    return acc;
}

// n output columns of one row: out[j] = affine(in[start + j * stride]); coef is [4][n] or NULL
__device__ __forceinline__ void copy_row(const float* __restrict__ in, const float* __restrict__ coef, float* __restrict__ out,
                                         int n, int start, int stride, int lane)
{
    for (int j = lane; j < n; j += WAVE) out[j] = affine_col(coef, n, j, in[start + (long)j * stride]);
}

// the same for stride 1 with every address a multiple of 16 bytes and n a multiple of 4
__device__ __forceinline__ void copy_row4(const float* __restrict__ in, const float* __restrict__ coef, float* __restrict__ out,
                                          int n, int start, int lane)
{
    for (int j = 4 * lane; j < n; j += 4 * WAVE)
        *reinterpret_cast<f4*>(out + j) = affine_col4(coef, n, j, *reinterpret_cast<const f4*>(in + start + j));
}

// a NULL pointer counts as aligned
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// columns a sensor (start, stride) keeps of a row of n
inline int width_of(int n, int start, int stride) { return (n - start + stride - 1) / stride; }

}  // namespace

#endif
