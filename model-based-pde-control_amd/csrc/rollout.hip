// rollout.hip -- the kernels that close the imagined-rollout loop in HBM (C ABI: include/rollout_hip.h and, for
// ro_settle_dissipation and ro_settle_burgers_dissipation, include/rollout/settle_dissipation.h and
// include/rollout/settle_burgers_dissipation.h;
// binding: pdecontrol/mbrl/rollout_hip.py; caller: pdecontrol/mbrl/imagination_phase.py).
//
// ro_act_chain is the wrapper stack's action side (raw-action record, action scaling, Gaussian forcing, forcing scaling,
// sensor), ro_settle its observation side (per-env elite pick, world state in place, trajectory slot, agent sensor, step
// counters, l2control reward); ro_settle_dissipation is ro_settle with the KS env's dissipation reward,
// ro_settle_burgers_dissipation with the Burgers env's: the three are instantiations of one kernel template, which differ
// in the reward alone.  A wave owns an env, lanes run along the columns.  The ensemble members travel in the kernel arguments and are picked by wave-uniform selects over
// constant indices, so the argument struct is never indexed dynamically and nothing spills.  No LDS, no atomics; every
// store is a plain vector store.
//
// The affine maps and the forcing chain are row_ops.h's, so the results equal the host wrappers' bit for bit.  The
// dissipation reward's stencil is ks_internal.h's ref_terms, the one the KS reward-row kernel evaluates.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "../../include/rollout/settle_burgers_dissipation.h"
#include "../../include/rollout/settle_dissipation.h"
#include "../../include/rollout_hip.h"
#include "capi_error.h"
#include "ks_internal.h"
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
        for (int j = 4 * lane; j < k.W; j += 4 * WAVE)
            *reinterpret_cast<f4*>(out + j) =
                affine_col4(k.a.out_coef, k.W, j, forcing_col4(k.a.in_coef, k.A, act, k.a.forcing + k.start + j, k.L));
        return;
    }
    for (int j = lane; j < k.W; j += WAVE)
        out[j] = affine_col(k.a.out_coef, k.W, j,
                            forcing_col(k.a.in_coef, k.A, act, k.a.forcing + k.start + (long)j * k.stride, k.L));
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

__device__ __forceinline__ void sense4(float* __restrict__ pol, int i, f4 v, int start, int stride, int O)
{
    sense(pol, i, v.x, start, stride, O);
    sense(pol, i + 1, v.y, start, stride, O);
    sense(pol, i + 2, v.z, start, stride, O);
    sense(pol, i + 3, v.w, start, stride, O);
}

// row b of the member chosen for `slot`, by wave-uniform selects over constant indices: the argument struct is never
// indexed dynamically.  known: the index lies inside the ensemble; outside, the callers poison and read nothing
__device__ __forceinline__ const float* member_row(const SettleKernelArgs& k, long slot, int b, bool& known)
{
    const int pick = k.a.chosen ? k.a.chosen[slot] : 0;
    const float* src = k.a.member[0];
#pragma unroll
    for (int m = 1; m < RO_MAX_MEMBERS; ++m)
        if (m < k.members && pick == m) src = k.a.member[m];
    known = pick >= 0 && pick < k.members;
    return src + (long)b * k.N;
}

// what ro_settle_dissipation adds to ro_settle's arguments
struct DissKernelArgs : SettleKernelArgs {
    const float* actions;     // [T][B][A]
    const float* in_coef;     // [4][A] or NULL
    const float* forcing;     // [A][N]
    int A;
    double dx, r_dx, dx2, r_dx2;
};

// what ro_settle_burgers_dissipation adds: the recorded actions and the forcing as above, and the reward's two constants
struct BurgersDissKernelArgs : SettleKernelArgs {
    const float* actions;     // [T][B][A]
    const float* in_coef;     // [4][A] or NULL
    const float* forcing;     // [A][N]
    int A;
    double two_dx, nu_d;
};

// column i of a periodic row of n, for -n <= i < 2n.  (ks_kernels.hip's wrap_idx, respelled: that function lives in the KS
// translation unit, and bench.py quotes its counter profiles only while ks_kernels.hip and ks_internal.h are the files
// they were measured on, so neither is edited for one line)
__device__ __forceinline__ int wrap_col(int i, int n) { return i < 0 ? i + n : (i >= n ? i - n : i); }

// the three partial sums of one point: window w, its squares q, centre c, forcing phi
__device__ __forceinline__ void dissipation_point(const double* w, const double* q, int c, float phi, const DissKernelArgs& d,
                                                  double& sxx, double& sx, double& sup)
{
    const ks::RefTerms p = ks::ref_terms<ks::DivMarkstein>(w, q, c, d.dx, d.r_dx, d.dx2, d.r_dx2);
    sxx += p.d2 * p.d2;
    sx += p.d1 * p.d1;
    sup += w[c] * (double)phi;
}

// the two partial sums of one point of the Burgers dissipation reward: neighbours um, up, centre u0, forcing phi
__device__ __forceinline__ void burgers_dissipation_point(float um, float u0, float up, float phi, const BurgersDissKernelArgs& d,
                                                          double& sx, double& sup)
{
    const double ux = ((double)up - (double)um) / d.two_dx;
    sx += ux * ux;
    sup += (double)u0 * (double)phi;
}

// ro_settle (Args = SettleKernelArgs, the l2control reward), ro_settle_dissipation (Args = DissKernelArgs) and
// ro_settle_burgers_dissipation (Args = BurgersDissKernelArgs): one body, of which the reward's sums (one for l2control;
// sxx, sx and sup for the KS dissipation; sx and sup for the Burgers one) and its closing expression depend on Args.
//
// The dissipation stencil needs the rescaled row's periodic halo of 4 columns on both sides: a lane re-reads its
// neighbours from the member's output row (read-only and cache-hot: the lanes next to it have just fetched the same
// lines) and rescales them again, which costs arithmetic that this latency-bound step has to spare and keeps the kernel
// free of LDS and of any wait between a store and a load.  On the float4 path the halo of a lane's four columns is
// exactly the float4 before and the float4 after, wrapped around the row.  Its forcing is that of the scaled action, as
// ro_act_chain forms it before its output map.
template <class Args>
__global__ __launch_bounds__(NT) void ro_settle_kernel(const Args k)
{
    constexpr bool DISS = std::is_same<Args, DissKernelArgs>::value;
    constexpr bool BURGERS = std::is_same<Args, BurgersDissKernelArgs>::value;
    const int lane = threadIdx.x & (WAVE - 1);
    const int b = blockIdx.x * WAVES + (threadIdx.x >> 6);
    const int t = k.a.step[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) k.a.step[1] = t + 1;  // advance: ro_act_chain reads step[1], nobody here does
    if (b >= k.B || t < 0 || t >= k.T) return;                      // whole waves leave: the shuffles below stay complete
    const long slot = (long)t * k.B + b;
    bool known;
    const float* __restrict__ row = member_row(k, slot, b, known);
    float* __restrict__ state = k.a.state + (long)b * k.N;
    float* __restrict__ traj = k.a.traj + (slot + k.B) * k.N;       // slot t + 1
    float* __restrict__ pol = k.a.policy_obs + (long)b * k.O;
    [[maybe_unused]] const float* __restrict__ act = nullptr;       // the raw actions ro_act_chain recorded for this step
    if constexpr (DISS || BURGERS) act = k.actions + slot * k.A;
    const int N = k.N;

    double sum[DISS ? 3 : BURGERS ? 2 : 1] = {};
    if (k.vec) {                                                     // N a multiple of 4, every row 16-byte aligned
        for (int i = 4 * lane; i < N; i += 4 * WAVE) {
            // the halo is the dissipation reward's alone; its loads stay beside the row's own, under the one test of `known`
            [[maybe_unused]] const int il = wrap_col(i - 4, N), ir = wrap_col(i + 4, N);
            f4 v = {NAN, NAN, NAN, NAN};
            [[maybe_unused]] f4 vl = v, vr = v;
            if (known) {
                v = *reinterpret_cast<const f4*>(row + i);
                if constexpr (DISS || BURGERS) {
                    vl = *reinterpret_cast<const f4*>(row + il);
                    vr = *reinterpret_cast<const f4*>(row + ir);
                }
            }
            *reinterpret_cast<f4*>(state + i) = v;
            *reinterpret_cast<f4*>(traj + i) = v;
            sense4(pol, i, v, k.start, k.stride, k.O);
            const f4 u = affine_col4(k.a.reward_coef, N, i, v);
            if constexpr (DISS) {
                const f4 ul = affine_col4(k.a.reward_coef, N, il, vl);
                const f4 ur = affine_col4(k.a.reward_coef, N, ir, vr);
                const f4 phi = forcing_col4(k.in_coef, k.A, act, k.forcing + i, N);
                const double w[12] = {(double)ul.x, (double)ul.y, (double)ul.z, (double)ul.w, (double)u.x,  (double)u.y,
                                      (double)u.z,  (double)u.w,  (double)ur.x, (double)ur.y, (double)ur.z, (double)ur.w};
                double q[12];
#pragma unroll
                for (int j = 0; j < 12; ++j) q[j] = w[j] * w[j];
                dissipation_point(w, q, 4, phi.x, k, sum[0], sum[1], sum[2]);
                dissipation_point(w, q, 5, phi.y, k, sum[0], sum[1], sum[2]);
                dissipation_point(w, q, 6, phi.z, k, sum[0], sum[1], sum[2]);
                dissipation_point(w, q, 7, phi.w, k, sum[0], sum[1], sum[2]);
            } else if constexpr (BURGERS) {                          // the halo of +-1: the last column before, the first after
                const f4 ul = affine_col4(k.a.reward_coef, N, il, vl);
                const f4 ur = affine_col4(k.a.reward_coef, N, ir, vr);
                const f4 phi = forcing_col4(k.in_coef, k.A, act, k.forcing + i, N);
                burgers_dissipation_point(ul.w, u.x, u.y, phi.x, k, sum[0], sum[1]);
                burgers_dissipation_point(u.x, u.y, u.z, phi.y, k, sum[0], sum[1]);
                burgers_dissipation_point(u.y, u.z, u.w, phi.z, k, sum[0], sum[1]);
                burgers_dissipation_point(u.z, u.w, ur.x, phi.w, k, sum[0], sum[1]);
            } else {
                sum[0] += (double)u.x * (double)u.x;
                sum[0] += (double)u.y * (double)u.y;
                sum[0] += (double)u.z * (double)u.z;
                sum[0] += (double)u.w * (double)u.w;
            }
        }
    } else {
        for (int i = lane; i < N; i += WAVE) {
            const float v = known ? row[i] : NAN;
            state[i] = v;
            traj[i] = v;
            sense(pol, i, v, k.start, k.stride, k.O);
            if constexpr (DISS) {
                double w[9], q[9];
#pragma unroll
                for (int j = -4; j <= 4; ++j) {
                    const int c = wrap_col(i + j, N);
                    w[j + 4] = (double)affine_col(k.a.reward_coef, N, c, known ? row[c] : NAN);
                    q[j + 4] = w[j + 4] * w[j + 4];
                }
                dissipation_point(w, q, 4, forcing_col(k.in_coef, k.A, act, k.forcing + i, N), k, sum[0], sum[1], sum[2]);
            } else if constexpr (BURGERS) {
                const int cl = wrap_col(i - 1, N), cr = wrap_col(i + 1, N);
                burgers_dissipation_point(affine_col(k.a.reward_coef, N, cl, known ? row[cl] : NAN),
                                          affine_col(k.a.reward_coef, N, i, v),
                                          affine_col(k.a.reward_coef, N, cr, known ? row[cr] : NAN),
                                          forcing_col(k.in_coef, k.A, act, k.forcing + i, N), k, sum[0], sum[1]);
            } else {
                const double w = (double)affine_col(k.a.reward_coef, N, i, v);
                sum[0] += w * w;
            }
        }
    }
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1)
        for (double& s : sum) s += __shfl_xor(s, m, WAVE);
    if (lane == 0) {
        if constexpr (DISS)                                          // the KS reward-row kernel's expression
            k.a.rewards[slot] = (float)((-1.0) * ((sum[0] / N + sum[1] / N) + sum[2] / N));
        else if constexpr (BURGERS)                                  // the row reward of include/burgers/objective.h
            k.a.rewards[slot] = (float)((-1.0) * (k.nu_d * (sum[0] / N) + sum[1] / N));
        else
            k.a.rewards[slot] = (float)((-1.0) * (1.0 / N) * sum[0]);
        k.a.steps[slot] = k.a.steps0[b] + t + 1;
    }
}

// the argument checks and the kernel arguments ro_settle and ro_settle_dissipation share; `who` names the caller
int settle_kernel_args(const char* who, const ro_geometry* g, const ro_settle_args* a, SettleKernelArgs& k)
{
    if (!a || !a->state || !a->traj || !a->policy_obs || !a->steps0 || !a->steps || !a->rewards || !a->step)
        return fail(-10, "%s: NULL argument, state, trajectory, observation, steps, rewards or step pointer", who);
    if (g->members > 1 && !a->chosen) return fail(-10, "%s: %d members without a chosen-member array", who, g->members);
    k = {};
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
        if (!a->member[m]) return fail(-10, "%s: member %d has a NULL output pointer", who, m);
        k.vec = k.vec && aligned16(a->member[m]);
    }
    return 0;
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
    SettleKernelArgs k;
    const int bad = settle_kernel_args("ro_settle", g, a, k);
    if (bad != 0) return bad;
    hipLaunchKernelGGL(ro_settle_kernel<SettleKernelArgs>, dim3((g->B + WAVES - 1) / WAVES), dim3(NT), 0,
                       static_cast<hipStream_t>(stream), k);
    return launch_status(-20, "ro_settle");
}

int ro_settle_dissipation(void* stream, const ro_geometry* g, const ro_settle_args* a, const ro_dissipation_args* d)
{
    const int rc = ro_supported(g);
    if (rc != 0) return rc;
    DissKernelArgs k = {};
    const int bad = settle_kernel_args("ro_settle_dissipation", g, a, k);
    if (bad != 0) return bad;
    if (!d || !d->actions || !d->forcing)
        return fail(-10, "ro_settle_dissipation: NULL dissipation argument, recorded-actions or forcing pointer");
    if (g->L != g->N)
        return fail(-11, "ro_settle_dissipation: forcing width %d for a state width of %d (the reward needs the forcing at "
                         "every grid point)", g->L, g->N);
    if (!std::isfinite(d->dx) || d->dx <= 0.0)
        return fail(-12, "ro_settle_dissipation: grid spacing %g (finite and above 0)", d->dx);
    k.actions = d->actions; k.in_coef = d->in_coef; k.forcing = d->forcing;
    k.A = g->A;
    k.dx = d->dx;
    k.dx2 = d->dx * d->dx;            // as ks::make_consts and the KS reward-row launch form them
    k.r_dx = 1.0 / k.dx;
    k.r_dx2 = 1.0 / k.dx2;
    k.vec = k.vec && aligned16(d->forcing);
    hipLaunchKernelGGL(ro_settle_kernel<DissKernelArgs>, dim3((g->B + WAVES - 1) / WAVES), dim3(NT), 0,
                       static_cast<hipStream_t>(stream), k);
    return launch_status(-20, "ro_settle_dissipation");
}

int ro_settle_burgers_dissipation(void* stream, const ro_geometry* g, const ro_settle_args* a,
                                  const ro_burgers_dissipation_args* d)
{
    const int rc = ro_supported(g);
    if (rc != 0) return rc;
    BurgersDissKernelArgs k = {};
    const int bad = settle_kernel_args("ro_settle_burgers_dissipation", g, a, k);
    if (bad != 0) return bad;
    if (!d || !d->d.actions || !d->d.forcing)
        return fail(-10, "ro_settle_burgers_dissipation: NULL dissipation argument, recorded-actions or forcing pointer");
    if (g->L != g->N)
        return fail(-11, "ro_settle_burgers_dissipation: forcing width %d for a state width of %d (the reward needs the "
                         "forcing at every grid point)", g->L, g->N);
    if (!std::isfinite(d->d.dx) || d->d.dx <= 0.0)
        return fail(-12, "ro_settle_burgers_dissipation: grid spacing %g (finite and above 0)", d->d.dx);
    if (!std::isfinite(d->nu) || d->nu < 0.0)
        return fail(-13, "ro_settle_burgers_dissipation: viscosity %g (finite and not negative)", d->nu);
    k.actions = d->d.actions; k.in_coef = d->d.in_coef; k.forcing = d->d.forcing;
    k.A = g->A;
    k.two_dx = 2.0 * d->d.dx;
    k.nu_d = (double)(float)d->nu;
    k.vec = k.vec && aligned16(d->d.forcing);
    hipLaunchKernelGGL(ro_settle_kernel<BurgersDissKernelArgs>, dim3((g->B + WAVES - 1) / WAVES), dim3(NT), 0,
                       static_cast<hipStream_t>(stream), k);
    return launch_status(-20, "ro_settle_burgers_dissipation");
}

const char* ro_last_error(void) { return g_err; }

}  // extern "C"
