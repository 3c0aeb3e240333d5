// rollout.hip -- the two kernels that close the imagined-rollout loop in HBM (C ABI: include/rollout_hip.h;
// binding: pdecontrol/mbrl/rollout_hip.py; caller: pdecontrol/mbrl/imagination_phase.py).
//
// ro_act_chain is the wrapper stack's action side (raw-action record, action scaling, Gaussian forcing, forcing scaling,
// sensor), ro_settle its observation side (per-env elite pick, world state in place, trajectory slot, agent sensor, step
// counters, l2control reward).  A wave owns an env, lanes run along the columns.  The ensemble members travel in the
// kernel arguments and are picked by wave-uniform selects over constant indices, so the argument struct is never indexed
// dynamically and nothing spills.  No LDS, no atomics; every store is a plain vector store.
//
// The affine maps are row_ops.h's and the forcing chain is explicit fmaf, so the results equal the host wrappers' bit for
// bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/rollout_hip.h"
#include "capi_error.h"
#include "row_ops.h"

namespace {

struct ActKernelArgs {
    ro_act_args a;
    int B, T, A, L, W, start, stride, vec;
};

__global__ __launch_bounds__(NT) void ro_act_chain_kernel(const ActKernelArgs k)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int b = blockIdx.x * WAVES + (threadIdx.x >> 6);
    const int t = k.a.step[1];
    if (blockIdx.x == 0 && threadIdx.x == 0) k.a.step[0] = t;      // publish: ro_settle reads step[0], nobody here does
    if (b >= k.B || t < 0 || t >= k.T) return;
    const float* __restrict__ act = k.a.action + (long)b * k.A;
    if (lane < k.A) k.a.actions[((long)t * k.B + b) * k.A + lane] = act[lane];
    float* __restrict__ out = k.a.world_action + (long)b * k.W;
    if (k.vec) {                                                     // stride 1, start, L and W multiples of 4, aligned
        for (int j = 4 * lane; j < k.W; j += 4 * WAVE) {
            const float* __restrict__ f = k.a.forcing + k.start + j;
            const float a0 = affine_col(k.a.in_coef, k.A, 0, act[0]);
            const f4 f0 = *reinterpret_cast<const f4*>(f);
            f4 acc;
            acc.x = __fmul_rn(a0, f0.x);
            acc.y = __fmul_rn(a0, f0.y);
            acc.z = __fmul_rn(a0, f0.z);
            acc.w = __fmul_rn(a0, f0.w);
            for (int m = 1; m < k.A; ++m) {
                const float am = affine_col(k.a.in_coef, k.A, m, act[m]);
                const f4 fm = *reinterpret_cast<const f4*>(f + (long)m * k.L);
                acc.x = __fmaf_rn(am, fm.x, acc.x);
                acc.y = __fmaf_rn(am, fm.y, acc.y);
                acc.z = __fmaf_rn(am, fm.z, acc.z);
                acc.w = __fmaf_rn(am, fm.w, acc.w);
            }
            *reinterpret_cast<f4*>(out + j) = affine_col4(k.a.out_coef, k.W, j, acc);
        }
        return;
    }
    for (int j = lane; j < k.W; j += WAVE) {
        const float* __restrict__ f = k.a.forcing + k.start + (long)j * k.stride;
        float acc = __fmul_rn(affine_col(k.a.in_coef, k.A, 0, act[0]), f[0]);
        for (int m = 1; m < k.A; ++m) acc = __fmaf_rn(affine_col(k.a.in_coef, k.A, m, act[m]), f[(long)m * k.L], acc);
        out[j] = affine_col(k.a.out_coef, k.W, j, acc);
    }
}

struct SettleKernelArgs {
    ro_settle_args a;
    int B, T, N, O, start, stride, members, vec;
};

// the agent sensor: state column i is policy column (i - start) / stride when that division is exact
__device__ __forceinline__ void sense(float* __restrict__ pol, int i, float v, int start, int stride, int O)
{
    const int d = i - start;
    if (d < 0) return;
    const int j = d / stride;
    if (j * stride == d && j < O) pol[j] = v;
}

__global__ __launch_bounds__(NT) void ro_settle_kernel(const SettleKernelArgs k)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int b = blockIdx.x * WAVES + (threadIdx.x >> 6);
    const int t = k.a.step[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) k.a.step[1] = t + 1;  // advance: ro_act_chain reads step[1], nobody here does
    if (b >= k.B || t < 0 || t >= k.T) return;                      // whole waves leave: the shuffles below stay complete
    const long slot = (long)t * k.B + b;

    // wave-uniform selects over constant indices: the argument struct is never indexed dynamically
    const int pick = k.a.chosen ? k.a.chosen[slot] : 0;
    const float* src = k.a.member[0];
#pragma unroll
    for (int m = 1; m < RO_MAX_MEMBERS; ++m)
        if (m < k.members && pick == m) src = k.a.member[m];
    const bool known = pick >= 0 && pick < k.members;               // an index outside the ensemble: poison, read nothing
    const float* __restrict__ row = src + (long)b * k.N;
    float* __restrict__ state = k.a.state + (long)b * k.N;
    float* __restrict__ traj = k.a.traj + (slot + k.B) * k.N;       // slot t + 1
    float* __restrict__ pol = k.a.policy_obs + (long)b * k.O;

    double sum = 0.0;
    if (k.vec) {                                                     // N a multiple of 4, every row 16-byte aligned
        for (int i = 4 * lane; i < k.N; i += 4 * WAVE) {
            f4 v = {NAN, NAN, NAN, NAN};
            if (known) v = *reinterpret_cast<const f4*>(row + i);
            *reinterpret_cast<f4*>(state + i) = v;
            *reinterpret_cast<f4*>(traj + i) = v;
            sense(pol, i, v.x, k.start, k.stride, k.O);
            sense(pol, i + 1, v.y, k.start, k.stride, k.O);
            sense(pol, i + 2, v.z, k.start, k.stride, k.O);
            sense(pol, i + 3, v.w, k.start, k.stride, k.O);
            const f4 w = affine_col4(k.a.reward_coef, k.N, i, v);
            sum += (double)w.x * (double)w.x;
            sum += (double)w.y * (double)w.y;
            sum += (double)w.z * (double)w.z;
            sum += (double)w.w * (double)w.w;
        }
    } else {
        for (int i = lane; i < k.N; i += WAVE) {
            const float v = known ? row[i] : NAN;
            state[i] = v;
            traj[i] = v;
            sense(pol, i, v, k.start, k.stride, k.O);
            const double w = (double)affine_col(k.a.reward_coef, k.N, i, v);
            sum += w * w;
        }
    }
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) sum += __shfl_xor(sum, m, WAVE);
    if (lane == 0) {
        k.a.rewards[slot] = (float)((-1.0) * (1.0 / k.N) * sum);
        k.a.steps[slot] = k.a.steps0[b] + t + 1;
    }
}

}  // namespace

extern "C" {

int ro_supported(const ro_geometry* g)
{
    if (!g) return fail(-1, "rollout: NULL geometry");
    if (g->B < 1) return fail(-2, "rollout: %d envs (at least 1)", g->B);
    if (g->T < 1) return fail(-3, "rollout: %d trajectory slots (at least 1)", g->T);
    if (g->N < RO_MIN_STATE_DIM || g->N > RO_MAX_STATE_DIM)
        return fail(-4, "rollout: state width %d (%d ... %d are supported)", g->N, RO_MIN_STATE_DIM, RO_MAX_STATE_DIM);
    if (g->A < 1 || g->A > RO_MAX_ACT_DIM)
        return fail(-5, "rollout: action width %d (1 ... %d are supported)", g->A, RO_MAX_ACT_DIM);
    if (g->L < 1) return fail(-6, "rollout: forcing width %d (at least 1)", g->L);
    if (g->act_stride < 1 || g->act_start < 0 || g->act_start >= g->L)
        return fail(-7, "rollout: action sensor (start %d, stride %d) over %d forcing columns", g->act_start, g->act_stride, g->L);
    if (g->obs_stride < 1 || g->obs_start < 0 || g->obs_start >= g->N)
        return fail(-8, "rollout: agent sensor (start %d, stride %d) over %d state columns", g->obs_start, g->obs_stride, g->N);
    if (g->members < 1 || g->members > RO_MAX_MEMBERS)
        return fail(-9, "rollout: %d ensemble members (1 ... %d are supported)", g->members, RO_MAX_MEMBERS);
    return 0;
}

int ro_act_chain(void* stream, const ro_geometry* g, const ro_act_args* a)
{
    const int rc = ro_supported(g);
    if (rc != 0) return rc;
    if (!a || !a->action || !a->actions || !a->forcing || !a->world_action || !a->step)
        return fail(-10, "ro_act_chain: NULL argument, action, trajectory, forcing, output or step pointer");
    ActKernelArgs k = {};
    k.a = *a;
    k.B = g->B; k.T = g->T; k.A = g->A; k.L = g->L;
    k.start = g->act_start; k.stride = g->act_stride;
    k.W = width_of(g->L, g->act_start, g->act_stride);
    k.vec = g->act_stride == 1 && g->act_start % 4 == 0 && g->L % 4 == 0 && k.W % 4 == 0 && aligned16(a->forcing) &&
            aligned16(a->world_action) && aligned16(a->out_coef);
    hipLaunchKernelGGL(ro_act_chain_kernel, dim3((g->B + WAVES - 1) / WAVES), dim3(NT), 0, static_cast<hipStream_t>(stream), k);
    return launch_status(-20, "ro_act_chain");
}

int ro_settle(void* stream, const ro_geometry* g, const ro_settle_args* a)
{
    const int rc = ro_supported(g);
    if (rc != 0) return rc;
    if (!a || !a->state || !a->traj || !a->policy_obs || !a->steps0 || !a->steps || !a->rewards || !a->step)
        return fail(-10, "ro_settle: NULL argument, state, trajectory, observation, steps, rewards or step pointer");
    if (g->members > 1 && !a->chosen) return fail(-10, "ro_settle: %d members without a chosen-member array", g->members);
    SettleKernelArgs k = {};
    k.a = *a;
    k.B = g->B; k.T = g->T; k.N = g->N; k.members = g->members;
    k.start = g->obs_start; k.stride = g->obs_stride;
    k.O = width_of(g->N, g->obs_start, g->obs_stride);
    k.vec = g->N % 4 == 0 && aligned16(a->state) && aligned16(a->traj) && aligned16(a->reward_coef);
    for (int m = 0; m < RO_MAX_MEMBERS; ++m) {
        if (m >= g->members) {
            k.a.member[m] = nullptr;
            continue;
        }
        if (!a->member[m]) return fail(-10, "ro_settle: member %d has a NULL output pointer", m);
        k.vec = k.vec && aligned16(a->member[m]);
    }
    hipLaunchKernelGGL(ro_settle_kernel, dim3((g->B + WAVES - 1) / WAVES), dim3(NT), 0, static_cast<hipStream_t>(stream), k);
    return launch_status(-20, "ro_settle");
}

const char* ro_last_error(void) { return g_err; }

}  // extern "C"
