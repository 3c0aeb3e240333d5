// collect.hip -- the kernels that keep the real-env collection loop in HBM (C ABI: include/collect_hip.h;
// binding: pdecontrol/mbrl/collect_hip.py; caller: pdecontrol/mbrl/collection_phase.py).
//
// co_act is the wrapper stack's action side (frozen action scaling, action-store record), co_observe its observation
// side (running min / max of the observation scaling, the affine map, the agent sensor).  A wave owns an env row, lanes
// run along the columns, four waves per workgroup.  co_observe's grid-wide dependency is two launches: per-workgroup
// (min, max) partials, then every wave folds the partials itself.  No atomics, no spin-wait; every store is a plain
// vector store.
//
// The affine maps are row_ops.h's, so the results equal the host wrappers' bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/collect_hip.h"
#include "capi_error.h"
#include "row_ops.h"

namespace {

// torch.minimum / torch.maximum and numpy's min / max: a NaN on either side gives NaN
__device__ __forceinline__ float min_nan(float a, float b) { return (a != a || b != b) ? NAN : fminf(a, b); }
__device__ __forceinline__ float max_nan(float a, float b) { return (a != a || b != b) ? NAN : fmaxf(a, b); }

__device__ __forceinline__ void wave_minmax(float& lo, float& hi)
{
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) {
        lo = min_nan(lo, __shfl_xor(lo, m, WAVE));
        hi = max_nan(hi, __shfl_xor(hi, m, WAVE));
    }
}

struct ActKernelArgs {
    co_act_args a;
    int E, A, t;
};

__global__ __launch_bounds__(NT) void co_act_kernel(const ActKernelArgs k)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int e = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (e >= k.E || lane >= k.A) return;
    const long at = (long)e * k.A + lane;
    const float raw = k.a.action[at];
    const float env = affine_col(k.a.coef, k.A, lane, raw);
    k.a.env_action[at] = env;
    k.a.actions[(long)k.t * k.E * k.A + at] = k.a.record_raw ? raw : env;
}

struct ObserveKernelArgs {
    co_observe_args a;
    int E, N, O, start, stride, t, parts, vec;
};

// launch one: partial[block] = (min, max) over the rows of this workgroup
__global__ __launch_bounds__(NT) void co_extrema_kernel(const ObserveKernelArgs k)
{
    __shared__ float s_lo[WAVES], s_hi[WAVES];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x >> 6;
    const int e = blockIdx.x * WAVES + wave;
    float lo = INFINITY, hi = -INFINITY;
    if (e < k.E) {                                                   // rows past the end keep the identities
        const float* __restrict__ row = k.a.traj + ((long)(k.t + 1) * k.E + e) * k.N;
        if (k.vec & 1) {                                             // N a multiple of 4, the block 16-byte aligned
            for (int i = 4 * lane; i < k.N; i += 4 * WAVE) {
                const f4 v = *reinterpret_cast<const f4*>(row + i);
                lo = min_nan(min_nan(min_nan(lo, v.x), min_nan(v.y, v.z)), v.w);
                hi = max_nan(max_nan(max_nan(hi, v.x), max_nan(v.y, v.z)), v.w);
            }
        } else {
            for (int i = lane; i < k.N; i += WAVE) {
                const float v = row[i];
                lo = min_nan(lo, v);
                hi = max_nan(hi, v);
            }
        }
    }
    wave_minmax(lo, hi);
    if (lane == 0) {
        s_lo[wave] = lo;
        s_hi[wave] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
            lo = min_nan(lo, s_lo[w]);
            hi = max_nan(hi, s_hi[w]);
        }
        k.a.workspace[2 * blockIdx.x] = lo;
        k.a.workspace[2 * blockIdx.x + 1] = hi;
    }
}

// launch two: every wave folds the partials itself, joins them with the running bounds and scales its row
__global__ __launch_bounds__(NT) void co_scale_kernel(const ObserveKernelArgs k)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int e = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (e >= k.E) return;                                            // whole waves leave: the shuffles below stay complete
    float vmin = 0.0f, vmax = 0.0f;
    const bool scaled = k.a.bounds != nullptr;
    if (scaled) {
        const float* __restrict__ cell = k.a.bounds + 2 * (k.t & 1);
        vmin = cell[0];
        vmax = cell[1];
        if (k.a.update) {
            float lo = INFINITY, hi = -INFINITY;
            for (int p = lane; p < k.parts; p += WAVE) {
                lo = min_nan(lo, k.a.workspace[2 * p]);
                hi = max_nan(hi, k.a.workspace[2 * p + 1]);
            }
            wave_minmax(lo, hi);
            // an unset bound gives way to the block's extremum
            vmin = (vmin == -INFINITY) ? lo : min_nan(lo, vmin);
            vmax = (vmax == INFINITY) ? hi : max_nan(hi, vmax);
            if (e == 0 && lane == 0) {                               // the other cell: nobody in this launch reads it
                float* __restrict__ out = k.a.bounds + 2 * ((k.t + 1) & 1);
                out[0] = vmin;
                out[1] = vmax;
            }
        }
    }
    const float ba = __fsub_rn(vmax, vmin), dc = __fsub_rn(k.a.upper, k.a.lower), c = k.a.lower;
    const float* __restrict__ row = k.a.traj + ((long)(k.t + 1) * k.E + e) * k.N + k.start;
    float* __restrict__ pol = k.a.policy_obs + (long)e * k.O;
    if (k.vec & 2) {                                                 // stride 1, start and O multiples of 4, aligned
        for (int j = 4 * lane; j < k.O; j += 4 * WAVE) {
            f4 v = *reinterpret_cast<const f4*>(row + j);
            if (scaled) {
                v.x = affine(v.x, vmin, ba, dc, c);
                v.y = affine(v.y, vmin, ba, dc, c);
                v.z = affine(v.z, vmin, ba, dc, c);
                v.w = affine(v.w, vmin, ba, dc, c);
            }
            *reinterpret_cast<f4*>(pol + j) = v;
        }
        return;
    }
    for (int j = lane; j < k.O; j += WAVE) {
        const float v = row[(long)j * k.stride];
        pol[j] = scaled ? affine(v, vmin, ba, dc, c) : v;
    }
}

int blocks_of(int E) { return (E + WAVES - 1) / WAVES; }

}  // namespace

extern "C" {

int co_supported(const co_geometry* g)
{
    if (!g) return fail(-1, "collect: NULL geometry");
    if (g->E < 1) return fail(-2, "collect: %d envs (at least 1)", g->E);
    if (g->T < 1) return fail(-3, "collect: %d trajectory slots (at least 1)", g->T);
    if (g->N < CO_MIN_STATE_DIM || g->N > CO_MAX_STATE_DIM)
        return fail(-4, "collect: state width %d (%d ... %d are supported)", g->N, CO_MIN_STATE_DIM, CO_MAX_STATE_DIM);
    if (g->A < 1 || g->A > CO_MAX_ACT_DIM)
        return fail(-5, "collect: action width %d (1 ... %d are supported)", g->A, CO_MAX_ACT_DIM);
    if (g->obs_stride < 1 || g->obs_start < 0 || g->obs_start >= g->N)
        return fail(-6, "collect: agent sensor (start %d, stride %d) over %d state columns", g->obs_start, g->obs_stride, g->N);
    return 0;
}

long co_workspace_floats(const co_geometry* g)
{
    const int rc = co_supported(g);
    if (rc != 0) return rc;
    return 2L * blocks_of(g->E);
}

int co_act(void* stream, const co_geometry* g, const co_act_args* a, int t)
{
    const int rc = co_supported(g);
    if (rc != 0) return rc;
    if (!a || !a->action || !a->env_action || !a->actions)
        return fail(-10, "co_act: NULL argument, action, stepper action or trajectory pointer");
    if (t < 0 || t >= g->T) return fail(-11, "co_act: step %d outside 0 ... %d", t, g->T - 1);
    ActKernelArgs k = {};
    k.a = *a;
    k.E = g->E; k.A = g->A; k.t = t;
    hipLaunchKernelGGL(co_act_kernel, dim3(blocks_of(g->E)), dim3(NT), 0, static_cast<hipStream_t>(stream), k);
    return launch_status(-20, "co_act");
}

int co_observe(void* stream, const co_geometry* g, const co_observe_args* a, int t)
{
    const int rc = co_supported(g);
    if (rc != 0) return rc;
    if (!a || !a->traj || !a->policy_obs) return fail(-10, "co_observe: NULL argument, trajectory or observation pointer");
    if (t < 0 || t >= g->T) return fail(-11, "co_observe: step %d outside 0 ... %d", t, g->T - 1);
    const bool update = a->bounds && a->update;
    if (update && !a->workspace) return fail(-12, "co_observe: an updating scaling without a workspace");
    ObserveKernelArgs k = {};
    k.a = *a;
    k.a.update = update ? 1 : 0;
    k.E = g->E; k.N = g->N; k.t = t;
    k.start = g->obs_start; k.stride = g->obs_stride;
    k.O = width_of(g->N, g->obs_start, g->obs_stride);
    k.parts = blocks_of(g->E);
    const bool rows4 = g->N % 4 == 0 && aligned16(a->traj);          // every slot and row then starts 16-byte aligned
    k.vec = (rows4 ? 1 : 0) |
            ((rows4 && g->obs_stride == 1 && g->obs_start % 4 == 0 && aligned16(a->policy_obs)) ? 2 : 0);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (update) {
        hipLaunchKernelGGL(co_extrema_kernel, dim3(k.parts), dim3(NT), 0, s, k);
        const int rc1 = launch_status(-20, "co_observe (extrema)");
        if (rc1 != 0) return rc1;
    }
    hipLaunchKernelGGL(co_scale_kernel, dim3(k.parts), dim3(NT), 0, s, k);
    return launch_status(-20, "co_observe");
}

const char* co_last_error(void) { return g_err; }

}  // extern "C"
