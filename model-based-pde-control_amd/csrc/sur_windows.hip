// sur_windows.hip -- the fused window gather of the surrogate-update phase (C entry and host validation:
// sur_gather_windows in sur_kernels.hip; binding: pdecontrol/surrogates/hipops.py; caller:
// pdecontrol/mbrl/surrogate_phase.py).
//
// One launch assembles the `states` and `actions` of one TBPTT batch from the packed replay: a wave owns one
// (window, step) row, lanes run along the columns.  The observation row goes through the sensor and the observation
// coefficients; the action row through the action scaling, the Gaussian forcing chain (row_ops.h's forcing_col, which
// ro_act_chain calls too: the chain of the KS stepper's action path), the sensor and the forcing scaling.  float4 where the host found the geometry and every
// base and stride 16-byte aligned, the scalar path otherwise.  No LDS, no atomics; every store is a plain vector store.
//
// The affine map, the row copy and the forcing chain are row_ops.h's, so a batch equals the host loader's connector
// bit for bit.  row_ops.h demands an uncontracted includer and the rest of the library is built with the compiler's
// default contraction: hence this translation unit of its own, which the Makefile compiles with EXACT (-ffp-contract=off).
// The pragma below covers this file's own expressions only: the _rn intrinsics are plain operators in headers the
// compiler includes ahead of it, and without the flag their multiplies, adds and subtractions fuse once inlined.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>

#include "row_ops.h"
#include "sur_windows.h"

namespace {

__device__ __forceinline__ void poison_row(float* __restrict__ out, int n, int lane)
{
    for (int j = lane; j < n; j += WAVE) out[j] = NAN;
}

__global__ __launch_bounds__(NT) void sur_gather_windows_kernel(const SurWindowsArgs k)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const long w = (long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (w >= (long)k.B * k.L) return;
    const int b = (int)(w / k.L), t = (int)(w % k.L);
    float* __restrict__ st = k.states + b * k.s_bstride + t * k.s_tstride;
    float* __restrict__ ac = k.actions_out + b * k.a_bstride + t * k.a_tstride;

    long row = k.first[b] + t;
    bool ok = row >= 0 && row < k.total;
    if (ok && k.rowmap) {
        row = k.rowmap[row];
        ok = row >= 0 && row < k.rows;
    }
    if (!ok) {                                   // not a row of the replay: read nothing, poison the row
        poison_row(st, k.No, lane);
        poison_row(ac, k.Na, lane);
        return;
    }

    const float* __restrict__ obs = k.obs + row * k.obs_width + k.obs_start;     // from the sensor's first column on
    if (k.vec_obs)
        copy_row4(obs, k.obs_coef, st, k.No, 0, lane);
    else
        copy_row(obs, k.obs_coef, st, k.No, 0, k.obs_stride, lane);

    const float* __restrict__ act = k.actions + row * k.A;
    if (!k.forcing) {                            // no forcing: sensor and output scaling over the action row itself
        copy_row(act, k.act_out_coef, ac, k.Na, k.act_start, k.act_stride, lane);
        return;
    }
    if (k.vec_act) {                             // stride 1; start, Lf and Na multiples of 4; aligned
        for (int j = 4 * lane; j < k.Na; j += 4 * WAVE)
            *reinterpret_cast<f4*>(ac + j) =
                affine_col4(k.act_out_coef, k.Na, j, forcing_col4(k.act_in_coef, k.A, act, k.forcing + k.act_start + j, k.Lf));
        return;
    }
    for (int j = lane; j < k.Na; j += WAVE)
        ac[j] = affine_col(k.act_out_coef, k.Na, j,
                           forcing_col(k.act_in_coef, k.A, act, k.forcing + k.act_start + (long)j * k.act_stride, k.Lf));
}

}  // namespace

int sur_windows_launch(void* stream, const SurWindowsArgs& k)
{
    const long n = (long)k.B * k.L;
    hipLaunchKernelGGL(sur_gather_windows_kernel, dim3((unsigned)((n + WAVES - 1) / WAVES)), dim3(NT), 0,
                       static_cast<hipStream_t>(stream), k);
    return (int)hipGetLastError();
}
