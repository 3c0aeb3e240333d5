// collect.hip -- the kernels that keep the real-env collection loop in HBM (C ABI: include/collect_hip.h;
// binding: pdecontrol/mbrl/collect_hip.py; caller: pdecontrol/mbrl/collection_phase.py).
//
// co_act is the wrapper stack's action side (frozen action scaling, action-store record), co_observe its observation
// side (running min / max of the observation scaling, the affine map, the agent sensor).  A wave owns an env row, lanes
// run along the columns, four waves per workgroup.  co_observe's grid-wide dependency is two launches: per-workgroup
// (min, max) partials, then every wave folds the partials itself.  No atomics, no spin-wait; every store is a plain
// vector store.
//
// The span entries (include/collect/span.h) do a whole segment at once for agents whose actions are known beforehand:
// co_act_span_kernel owns one wave per (t, e) row; co_span_extrema_kernel reduces the rows of slots 1 ... T to at most
// CO_SPAN_MAX_PARTS partials with a grid stride, and co_scale_kernel folds them as it folds a step's.  A step is a span
// of one: co_act and co_observe launch the same two kernels over the E rows of their step.
//
// The affine maps are row_ops.h's, so the results equal the host wrappers' bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/collect/span.h"
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

struct ActSpanKernelArgs {
    co_act_span_args a;
    long rows;                                                       // T * E
    int A;
};

__global__ __launch_bounds__(NT) void co_act_span_kernel(const ActSpanKernelArgs k)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const long r = (long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (r >= k.rows || lane >= k.A) return;
    const long at = r * k.A + lane;
    const float raw = k.a.table[at];
    const float env = affine_col(k.a.coef, k.A, lane, raw);
    k.a.env_actions[at] = env;
    k.a.actions[at] = k.a.record_raw ? raw : env;
}

// slot: the trajectory slot scaled; cell_in / cell_out: the bounds cells read and (with update) written
struct ObserveKernelArgs {
    co_observe_args a;
    int E, N, O, start, stride, slot, cell_in, cell_out, parts, vec;
    long first, rows;                                                // the rows of [T + 1][E] the extrema are taken over
};

__device__ __forceinline__ void row_minmax(const float* __restrict__ row, int N, int vec, int lane, float& lo, float& hi)
{
    if (vec & 1) {                                                   // N a multiple of 4, the block 16-byte aligned
        for (int i = 4 * lane; i < N; i += 4 * WAVE) {
            const f4 v = *reinterpret_cast<const f4*>(row + i);
            lo = min_nan(min_nan(min_nan(lo, v.x), min_nan(v.y, v.z)), v.w);
            hi = max_nan(max_nan(max_nan(hi, v.x), max_nan(v.y, v.z)), v.w);
        }
    } else {
        for (int i = lane; i < N; i += WAVE) {
            const float v = row[i];
            lo = min_nan(lo, v);
            hi = max_nan(hi, v);
        }
    }
}

// the workgroup's four wave results into partial[block]
__device__ __forceinline__ void store_partial(float* __restrict__ workspace, float lo, float hi)
{
    __shared__ float s_lo[WAVES], s_hi[WAVES];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x >> 6;
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
        workspace[2 * blockIdx.x] = lo;
        workspace[2 * blockIdx.x + 1] = hi;
    }
}

// launch one: partial[block] = (min, max) over the rows block * 4 + wave, + 4 * gridDim.x, ... of the span (the rows of
// [T + 1][E][N] are contiguous: row r of the span is row first + r of the block).  A step is the span of the E rows of
// slot t + 1 on ceil(E / 4) workgroups, one row per wave; a segment the T * E rows of slots 1 ... T.  Rows past the end
// keep the identities.
__global__ __launch_bounds__(NT) void co_span_extrema_kernel(const ObserveKernelArgs k)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const long step = (long)gridDim.x * WAVES;
    float lo = INFINITY, hi = -INFINITY;
    for (long r = k.first + (long)blockIdx.x * WAVES + (threadIdx.x >> 6); r < k.first + k.rows; r += step)
        row_minmax(k.a.traj + r * k.N, k.N, k.vec, lane, lo, hi);
    store_partial(k.a.workspace, lo, hi);
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
        const float* __restrict__ cell = k.a.bounds + 2 * k.cell_in;
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
                float* __restrict__ out = k.a.bounds + 2 * k.cell_out;
                out[0] = vmin;
                out[1] = vmax;
            }
        }
    }
    const float ba = __fsub_rn(vmax, vmin), dc = __fsub_rn(k.a.upper, k.a.lower), c = k.a.lower;
    const float* __restrict__ row = k.a.traj + ((long)k.slot * k.E + e) * k.N + k.start;
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

// partials of a span's first launch
long span_parts(const co_geometry* g)
{
    const long groups = ((long)g->T * g->E + WAVES - 1) / WAVES;
    return groups < CO_SPAN_MAX_PARTS ? groups : CO_SPAN_MAX_PARTS;
}

// what both observation entries decide on the host: widths, the sensor and the float4 conditions
void observe_shape(ObserveKernelArgs& k, const co_geometry* g, const co_observe_args* a)
{
    const bool update = a->bounds && a->update;
    k.a = *a;
    k.a.update = update ? 1 : 0;
    k.E = g->E; k.N = g->N;
    k.start = g->obs_start; k.stride = g->obs_stride;
    k.O = width_of(g->N, g->obs_start, g->obs_stride);
    const bool rows4 = g->N % 4 == 0 && aligned16(a->traj);          // every slot and row then starts 16-byte aligned
    k.vec = (rows4 ? 1 : 0) |
            ((rows4 && g->obs_stride == 1 && g->obs_start % 4 == 0 && aligned16(a->policy_obs)) ? 2 : 0);
}

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
    ActSpanKernelArgs k = {};                                        // a step is a span of E rows, recorded at step t
    k.a.table = a->action; k.a.coef = a->coef; k.a.env_actions = a->env_action;
    k.a.actions = a->actions + (long)t * g->E * g->A;
    k.a.record_raw = a->record_raw;
    k.rows = g->E; k.A = g->A;
    hipLaunchKernelGGL(co_act_span_kernel, dim3(blocks_of(g->E)), dim3(NT), 0, static_cast<hipStream_t>(stream), k);
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
    observe_shape(k, g, a);
    k.slot = t + 1; k.cell_in = t & 1; k.cell_out = (t + 1) & 1;
    k.first = (long)(t + 1) * g->E; k.rows = g->E;                   // a step is the span of slot t + 1, a row per wave
    k.parts = blocks_of(g->E);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (update) {
        hipLaunchKernelGGL(co_span_extrema_kernel, dim3(k.parts), dim3(NT), 0, s, k);
        const int rc1 = launch_status(-20, "co_observe (extrema)");
        if (rc1 != 0) return rc1;
    }
    hipLaunchKernelGGL(co_scale_kernel, dim3(k.parts), dim3(NT), 0, s, k);
    return launch_status(-20, "co_observe");
}

long co_span_workspace_floats(const co_geometry* g)
{
    const int rc = co_supported(g);
    if (rc != 0) return rc;
    return 2L * span_parts(g);
}

int co_act_span(void* stream, const co_geometry* g, const co_act_span_args* a)
{
    const int rc = co_supported(g);
    if (rc != 0) return rc;
    if (!a || !a->table || !a->env_actions || !a->actions)
        return fail(-10, "co_act_span: NULL argument, table, stepper action or trajectory pointer");
    ActSpanKernelArgs k = {};
    k.a = *a;
    k.rows = (long)g->T * g->E; k.A = g->A;
    const long groups = (k.rows + WAVES - 1) / WAVES;
    if (groups > 0x7fffffffL) return fail(-3, "collect: %d steps of %d envs are more rows than one launch covers", g->T, g->E);
    hipLaunchKernelGGL(co_act_span_kernel, dim3((unsigned)groups), dim3(NT), 0, static_cast<hipStream_t>(stream), k);
    return launch_status(-20, "co_act_span");
}

int co_observe_span(void* stream, const co_geometry* g, const co_observe_args* a)
{
    const int rc = co_supported(g);
    if (rc != 0) return rc;
    if (!a || !a->traj || !a->policy_obs) return fail(-10, "co_observe_span: NULL argument, trajectory or observation pointer");
    const bool update = a->bounds && a->update;
    if (update && !a->workspace) return fail(-12, "co_observe_span: an updating scaling without a workspace");
    ObserveKernelArgs k = {};
    observe_shape(k, g, a);
    k.slot = g->T; k.cell_in = 0; k.cell_out = 1;
    k.first = g->E; k.rows = (long)g->T * g->E;                      // slots 1 ... T
    k.parts = (int)span_parts(g);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (update) {
        hipLaunchKernelGGL(co_span_extrema_kernel, dim3(k.parts), dim3(NT), 0, s, k);
        const int rc1 = launch_status(-20, "co_observe_span (extrema)");
        if (rc1 != 0) return rc1;
    }
    hipLaunchKernelGGL(co_scale_kernel, dim3(blocks_of(g->E)), dim3(NT), 0, s, k);
    return launch_status(-20, "co_observe_span");
}

const char* co_last_error(void) { return g_err; }

}  // extern "C"
