// burgers.hip -- gfx950 (MI355X / CDNA4) batched viscous-Burgers stepper; C ABI in include/burgers_hip.h.
//
// What is computed (the reference's only Burgers artefact, pdecontrol/surrogates/phyloss/phyloss.py:36-86):
//   residual(u) = nu * u_xx - u * u_x + phi, u_x by the 2nd-order central stencil [-1/2, 0, 1/2]/dx, u_xx by the
//   4th-order central stencil [-1/12, 4/3, -5/2, 4/3, -1/12]/dx^2, periodic; one sub-step is the explicit midpoint
//   rule u <- u + dt * residual(u + dt/2 * residual(u))   (:83-86).
//
// Design (same as the KS stepper, csrc/ks_kernels.hip): one launch = all envs x all sub-steps, the fp32 state lives in
// VGPRs; one env is one 64-lane wavefront with P = N/64 contiguous points per lane; the +-2 halo comes from the two
// neighbouring lanes by DPP wave rotations (wave_ror:1 / wave_rol:1), which ARE the periodic boundary: no LDS, no
// barrier, no index arithmetic.  HBM is touched once on entry and once on exit; the kernel is VALU-issue bound.
//
// Built with -ffp-contract=off: every device operation below is one rounded fp32 operation or one explicit fmaf, in the
// order oracle/burgers_oracle.c restates as flat loops.  tests/test_burgers_gpu.py holds bg_step (scalar, packed and
// pair-native forms), bg_phyloss_forward and bg_residual to that twin bit for bit.
//
// The collection phase's two entries (pdecontrol/mbrl/collection_phase.py): bg_step_span, T steps in one launch with the
// state held in VGPRs between them, and bg_record, a segment's transitions into the slabs of the device-resident replay.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../include/burgers_hip.h"
#include "capi_error.h"
#include "place_rows.h"
#include "row_ops.h"

namespace {

struct Args {
    float* u;
    const float* actions;
    const float* F;
    float* obs;
    double* ssq_sum;
    int* status;
    int n_act, n_envs, N;
    long n_substeps;
    float half_inv_dx;        // 1 / (2 dx)
    float l0, l1, l2;         // nu * laplace coefficients / dx^2: centre, +-1, +-2
    float dt, hdt;
};

// the stencil coefficients every kernel of this file reads, pre-divided once on the host
void set_coefficients(Args& a, float dx, float dt, float nu) {
    a.half_inv_dx = 0.5f / dx;
    const float s = nu / (dx * dx);
    a.l0 = s * (-5.0f / 2.0f); a.l1 = s * (4.0f / 3.0f); a.l2 = s * (-1.0f / 12.0f);
    a.dt = dt; a.hdt = 0.5f * dt;
}

// DPP control words (GFX9): wave_ror:1 = 0x13C (lane i receives lane i-1), wave_rol:1 = 0x134 (lane i receives lane i+1)
__device__ __forceinline__ float from_lower(float x) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x13C, 0xf, 0xf, false));
}
__device__ __forceinline__ float from_upper(float x) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x134, 0xf, 0xf, false));
}

// window w[0 .. P+3]: w[2 + j] = v[j]; w[0], w[1] the two points left of the lane's first, w[P+2], w[P+3] right of its last
template <int P>
__device__ __forceinline__ void window(const float (&v)[P], float (&w)[P + 4]) {
#pragma unroll
    for (int j = 0; j < P; ++j) w[2 + j] = v[j];
    if constexpr (P == 1) {
        w[1] = from_lower(v[0]);
        w[0] = from_lower(w[1]);
        w[3] = from_upper(v[0]);
        w[4] = from_upper(w[3]);
    } else {
        w[1] = from_lower(v[P - 1]);
        w[0] = from_lower(v[P - 2]);
        w[P + 2] = from_upper(v[0]);
        w[P + 3] = from_upper(v[1]);
    }
}

// Two points per instruction: gfx950 has packed fp32 VALU ops (v_pk_fma_f32 / v_pk_add_f32 / v_pk_mul_f32, IEEE per
// half, so the results are bit-identical to the scalar form), and this kernel is VALU-issue bound.  The stencil is
// written on <2 x float> values whose halves are neighbouring points; the compiler pairs the registers.
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int P>
__device__ __forceinline__ void residual(const float (&w)[P + 4], const float (&phi)[P], const Args& a, float (&r)[P]) {
    if constexpr (P >= 2) {
        const f32x2 hid = {a.half_inv_dx, a.half_inv_dx}, l0 = {a.l0, a.l0}, l1 = {a.l1, a.l1}, l2 = {a.l2, a.l2};
#pragma unroll
        for (int j = 0; j < P; j += 2) {
            const f32x2 wm2 = {w[j], w[j + 1]}, wm1 = {w[j + 1], w[j + 2]}, w0 = {w[j + 2], w[j + 3]},
                        wp1 = {w[j + 3], w[j + 4]}, wp2 = {w[j + 4], w[j + 5]}, ph = {phi[j], phi[j + 1]};
            const f32x2 grad = (wp1 - wm1) * hid;
            f32x2 lap = __builtin_elementwise_fma(l0, w0, ph);
            lap = __builtin_elementwise_fma(l1, wm1 + wp1, lap);
            lap = __builtin_elementwise_fma(l2, wm2 + wp2, lap);
            const f32x2 rr = __builtin_elementwise_fma(-w0, grad, lap);
            r[j] = rr[0];
            r[j + 1] = rr[1];
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const float grad = (w[j + 3] - w[j + 1]) * a.half_inv_dx;
        float lap = fmaf(a.l0, w[j + 2], phi[j]);
        lap = fmaf(a.l1, w[j + 1] + w[j + 3], lap);
        lap = fmaf(a.l2, w[j] + w[j + 4], lap);
        r[j] = fmaf(-w[j + 2], grad, lap);
    }
}

// Pair-native form of one residual evaluation for P >= 4 (P even): the state is held as P/2 <2 x float> pairs of
// neighbouring points.  E[k] are the aligned pairs of the window (E[0] / E[P/2 + 1] the halo pairs from the neighbouring
// lanes), O[k] = (E[k].hi, E[k+1].lo) the pairs at odd offsets -- ONE v_pk_mov_b32 each instead of two v_mov_b32.
template <int H>   // H = P / 2 pairs per lane
__device__ __forceinline__ void residual_pairs(const f32x2 (&U)[H], const f32x2 (&PH)[H], const Args& a, f32x2 (&R)[H]) {
    f32x2 E[H + 2], O[H + 1];
#pragma unroll
    for (int k = 0; k < H; ++k) E[k + 1] = U[k];
    E[0] = f32x2{from_lower(U[H - 1][0]), from_lower(U[H - 1][1])};
    E[H + 1] = f32x2{from_upper(U[0][0]), from_upper(U[0][1])};
#pragma unroll
    for (int k = 0; k <= H; ++k) O[k] = __builtin_shufflevector(E[k], E[k + 1], 1, 2);
    const f32x2 hid = {a.half_inv_dx, a.half_inv_dx}, l0 = {a.l0, a.l0}, l1 = {a.l1, a.l1}, l2 = {a.l2, a.l2};
#pragma unroll
    for (int k = 0; k < H; ++k) {
        // points 2k, 2k + 1: centre E[k+1], +-2 E[k] / E[k+2], -1 O[k], +1 O[k+1]
        const f32x2 grad = (O[k + 1] - O[k]) * hid;
        f32x2 lap = __builtin_elementwise_fma(l0, E[k + 1], PH[k]);
        lap = __builtin_elementwise_fma(l1, O[k] + O[k + 1], lap);
        lap = __builtin_elementwise_fma(l2, E[k] + E[k + 2], lap);
        R[k] = __builtin_elementwise_fma(-E[k + 1], grad, lap);
    }
}

template <int P>
__global__ void __launch_bounds__(256) bg_step_kernel(const Args a) {
    const int lane = threadIdx.x & 63;
    const int slot = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const bool active = slot < a.n_envs;
    const int env = active ? slot : a.n_envs - 1;   // tail waves redo the last env (their lanes must still rotate)
    const size_t off = (size_t)env * a.N + (size_t)lane * P;

    float u[P], phi[P];
#pragma unroll
    for (int j = 0; j < P; ++j) u[j] = a.u[off + j];
    if (a.actions) {
        const float* act = a.actions + (size_t)env * a.n_act;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int i = lane * P + j;
            float acc = act[0] * a.F[i];
            for (int k = 1; k < a.n_act; ++k) acc = fmaf(act[k], a.F[(size_t)k * a.N + i], acc);
            phi[j] = acc;
        }
    } else {
#pragma unroll
        for (int j = 0; j < P; ++j) phi[j] = 0.0f;
    }

    double racc = 0.0;
    if constexpr (P >= 4) {
        constexpr int H = P / 2;
        f32x2 U[H], PH[H];
#pragma unroll
        for (int k = 0; k < H; ++k) {
            U[k] = f32x2{u[2 * k], u[2 * k + 1]};
            PH[k] = f32x2{phi[2 * k], phi[2 * k + 1]};
        }
        const f32x2 hdt2 = {a.hdt, a.hdt}, dt2 = {a.dt, a.dt};
        for (long s = 0; s < a.n_substeps; ++s) {
            float q = 0.0f;
#pragma unroll
            for (int k = 0; k < H; ++k) {            // same order as the scalar form: u[0], u[1], ...
                q = fmaf(U[k][0], U[k][0], q);
                q = fmaf(U[k][1], U[k][1], q);
            }
            racc += (double)q;
            f32x2 R[H], UT[H];
            residual_pairs<H>(U, PH, a, R);
#pragma unroll
            for (int k = 0; k < H; ++k) UT[k] = __builtin_elementwise_fma(hdt2, R[k], U[k]);
            residual_pairs<H>(UT, PH, a, R);
#pragma unroll
            for (int k = 0; k < H; ++k) U[k] = __builtin_elementwise_fma(dt2, R[k], U[k]);
        }
#pragma unroll
        for (int k = 0; k < H; ++k) {
            u[2 * k] = U[k][0];
            u[2 * k + 1] = U[k][1];
        }
    } else
    for (long s = 0; s < a.n_substeps; ++s) {
        float w[P + 4], r[P], ut[P];
        float q = 0.0f;
#pragma unroll
        for (int j = 0; j < P; ++j) q = fmaf(u[j], u[j], q);
        racc += (double)q;                       // reward term of this sub-step, before the update
        window<P>(u, w);
        residual<P>(w, phi, a, r);
#pragma unroll
        for (int j = 0; j < P; ++j) ut[j] = fmaf(a.hdt, r[j], u[j]);
        window<P>(ut, w);
        residual<P>(w, phi, a, r);
#pragma unroll
        for (int j = 0; j < P; ++j) u[j] = fmaf(a.dt, r[j], u[j]);
    }

    int bad = 0;
#pragma unroll
    for (int j = 0; j < P; ++j) bad |= !__builtin_isfinite(u[j]);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        racc += __shfl_xor(racc, m, 64);
        bad |= __shfl_xor(bad, m, 64);
    }
    if (active) {
#pragma unroll
        for (int j = 0; j < P; ++j) a.u[off + j] = u[j];
        if (a.obs) {
#pragma unroll
            for (int j = 0; j < P; ++j) a.obs[off + j] = u[j];
        }
        if (lane == 0) {
            if (a.ssq_sum) a.ssq_sum[env] = racc;
            if (a.status) a.status[env] = bad;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The three parts of a step, as bg_step_span_kernel takes them.  They restate bg_step_kernel's body operation for
// operation; that kernel keeps its own inline spelling (called through these its schedule moves by a few instructions,
// and its code object is held to what it was).  tests/test_burgers_span_gpu.py holds the two to each other bit for bit.
//
// phi = act @ F at the lane's P points: one rounded product, then one fmaf per further actuator, in index order
template <int P>
__device__ __forceinline__ void forcing(const float* act, const Args& a, int lane, float (&phi)[P]) {
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int i = lane * P + j;
        float acc = act[0] * a.F[i];
        for (int k = 1; k < a.n_act; ++k) acc = fmaf(act[k], a.F[(size_t)k * a.N + i], acc);
        phi[j] = acc;
    }
}

// a.n_substeps midpoint sub-steps of the lane's P points with phi held; racc += the reward term of every sub-step
template <int P>
__device__ __forceinline__ void advance(float (&u)[P], const float (&phi)[P], const Args& a, double& racc) {
    if constexpr (P >= 4) {
        constexpr int H = P / 2;
        f32x2 U[H], PH[H];
#pragma unroll
        for (int k = 0; k < H; ++k) {
            U[k] = f32x2{u[2 * k], u[2 * k + 1]};
            PH[k] = f32x2{phi[2 * k], phi[2 * k + 1]};
        }
        const f32x2 hdt2 = {a.hdt, a.hdt}, dt2 = {a.dt, a.dt};
        for (long s = 0; s < a.n_substeps; ++s) {
            float q = 0.0f;
#pragma unroll
            for (int k = 0; k < H; ++k) {            // same order as the scalar form: u[0], u[1], ...
                q = fmaf(U[k][0], U[k][0], q);
                q = fmaf(U[k][1], U[k][1], q);
            }
            racc += (double)q;
            f32x2 R[H], UT[H];
            residual_pairs<H>(U, PH, a, R);
#pragma unroll
            for (int k = 0; k < H; ++k) UT[k] = __builtin_elementwise_fma(hdt2, R[k], U[k]);
            residual_pairs<H>(UT, PH, a, R);
#pragma unroll
            for (int k = 0; k < H; ++k) U[k] = __builtin_elementwise_fma(dt2, R[k], U[k]);
        }
#pragma unroll
        for (int k = 0; k < H; ++k) {
            u[2 * k] = U[k][0];
            u[2 * k + 1] = U[k][1];
        }
    } else
    for (long s = 0; s < a.n_substeps; ++s) {
        float w[P + 4], r[P], ut[P];
        float q = 0.0f;
#pragma unroll
        for (int j = 0; j < P; ++j) q = fmaf(u[j], u[j], q);
        racc += (double)q;                       // reward term of this sub-step, before the update
        window<P>(u, w);
        residual<P>(w, phi, a, r);
#pragma unroll
        for (int j = 0; j < P; ++j) ut[j] = fmaf(a.hdt, r[j], u[j]);
        window<P>(ut, w);
        residual<P>(w, phi, a, r);
#pragma unroll
        for (int j = 0; j < P; ++j) u[j] = fmaf(a.dt, r[j], u[j]);
    }
}

// the wave's reward sum and non-finite flag, by xor shuffles: every lane ends with both
template <int P>
__device__ __forceinline__ int settle(const float (&u)[P], double& racc) {
    int bad = 0;
#pragma unroll
    for (int j = 0; j < P; ++j) bad |= !__builtin_isfinite(u[j]);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        racc += __shfl_xor(racc, m, 64);
        bad |= __shfl_xor(bad, m, 64);
    }
    return bad;
}

// bg_step_span: T env steps of one launch.  The layout and every operation of a step are bg_step_kernel's (forcing,
// advance, settle), so a step's bytes are those of a bg_step launch; what the span saves is T - 1 launches and the
// round trip of u through HBM between them.  Step t reads row t of the action table [T][E][A], stores the
// state to traj slot t + 1 and, by lane 0, ssq[t][e] and status[t][e]; u is stored once, after the last step.  F is
// re-read per step (A x P values per lane from L2 against n_substeps sub-steps of arithmetic): held in registers it would
// not fit at A = 16, P = 16.
struct SpanArgs {
    Args s;                    // u, F, n_act, n_envs, N, n_substeps, coefficients; actions = the table; obs/ssq_sum/status unused
    float* traj;               // [T + 1][E][N], slot 0 is not touched
    double* ssq;               // [T][E] or null
    int* status;               // [T][E] or null
    int T;
};

template <int P>
__global__ void __launch_bounds__(256) bg_step_span_kernel(const SpanArgs a) {
    const Args& s = a.s;
    const int lane = threadIdx.x & 63;
    const int slot = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const bool active = slot < s.n_envs;
    const int env = active ? slot : s.n_envs - 1;   // tail waves redo the last env (their lanes must still rotate)
    const size_t off = (size_t)env * s.N + (size_t)lane * P;
    const size_t slab = (size_t)s.n_envs * s.N;

    float u[P], phi[P];
#pragma unroll
    for (int j = 0; j < P; ++j) u[j] = s.u[off + j];
    for (int t = 0; t < a.T; ++t) {
        const size_t cell = (size_t)t * s.n_envs + env;
        forcing<P>(s.actions + cell * s.n_act, s, lane, phi);
        double racc = 0.0;
        advance<P>(u, phi, s, racc);
        const int bad = settle<P>(u, racc);
        if (active) {
            float* out = a.traj + (size_t)(t + 1) * slab + off;
#pragma unroll
            for (int j = 0; j < P; ++j) out[j] = u[j];
            if (lane == 0) {
                if (a.ssq) a.ssq[cell] = racc;
                if (a.status) a.status[cell] = bad;
            }
        }
    }
    if (active) {
#pragma unroll
        for (int j = 0; j < P; ++j) s.u[off + j] = u[j];
    }
}

// bg_record: transition w = t * E + e of a segment goes to replay row dst[w].  A wave owns a transition, lanes run along
// the columns (ks_record_kernel's shape, csrc/ks_record.hip).  The reward is (float)(ssq * c) with c formed on the host:
// BurgersBatchedVecEnv.step_torch's one fp64 product, cast as the replay casts it.  Plain vector stores only.
struct RecordArgs {
    const float* traj;         // [T + 1][E][N]
    const float* actions;      // [T][E][A]
    const double* ssq;         // [T][E]
    const int* steps;          // [T][E]
    const long* dst;           // [T][E]
    bg_slabs out;
    long n;                    // T * E
    int E, N, A;
    int vec_obs, vec_act;
    double c;                  // -(1.0 / N) / max(n_substeps, 1)
};

__global__ void __launch_bounds__(NT) bg_record_kernel(const RecordArgs a) {
    const int lane = threadIdx.x & (WAVE - 1);
    const long w = (long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (w >= a.n) return;
    const long r = a.dst[w];
    if (r < 0 || r >= a.out.rows) return;            // negative: skipped by contract; beyond the slab: never written
    place_row(a.traj + w * a.N, a.out.obs + r * a.N, a.N, a.vec_obs, lane);
    place_row(a.traj + (w + a.E) * a.N, a.out.nxtobs + r * a.N, a.N, a.vec_obs, lane);
    place_row(a.actions + w * a.A, a.out.actions + r * a.A, a.A, a.vec_act, lane);
    if (lane == 0) {
        a.out.rewards[r] = __double2float_rn(__dmul_rn(a.ssq[w], a.c));
        a.out.steps[r] = a.steps[w];
        a.out.terminated[r] = 0;
        a.out.truncated[r] = 0;
    }
}

__global__ void bg_residual_kernel(const float* __restrict__ u, const float* __restrict__ phi, int n_rows, int N, float half_inv_dx,
                                   float l0, float l1, float l2, float* __restrict__ out) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (size_t)n_rows * N) return;
    const int i = (int)(gid % N);
    const float* row = u + (gid - i);
    auto at = [&](int k) { int idx = i + k; idx = idx < 0 ? idx + N : (idx >= N ? idx - N : idx); return row[idx]; };
    const float grad = (at(1) - at(-1)) * half_inv_dx;
    float lap = fmaf(l0, at(0), phi ? phi[gid] : 0.0f);
    lap = fmaf(l1, at(-1) + at(1), lap);
    lap = fmaf(l2, at(-2) + at(2), lap);
    out[gid] = fmaf(-at(0), grad, lap);
}

template <int P>
int launch(const Args& a, hipStream_t st) {
    const int waves_per_block = 4;
    const int grid = (a.n_envs + waves_per_block - 1) / waves_per_block;
    hipLaunchKernelGGL(bg_step_kernel<P>, dim3(grid), dim3(64 * waves_per_block), 0, st, a);
    return launch_status(-2, "bg_step");
}

template <int P>
int launch_span(const SpanArgs& a, hipStream_t st) {
    const int waves_per_block = 4;
    const int grid = (a.s.n_envs + waves_per_block - 1) / waves_per_block;
    hipLaunchKernelGGL(bg_step_span_kernel<P>, dim3(grid), dim3(64 * waves_per_block), 0, st, a);
    return launch_status(-2, "bg_step_span");
}

// ---------------------------------------------------------------------------------------------------------------------
// Physics-informed loss (the reference's BurgersPhyPDELoss.__call__, phyloss.py:17-25): for augmented [B, T, N]
//   target[:, 0] = a[:, T-1],  target[:, t] = Phi(a[:, t-1]) (Phi = ``substeps`` midpoint steps),  loss = (a - target)^2.
// Same layout as bg_step_kernel: one row (b, t) = one wavefront, P points per lane, the halo by ``window``.  Row (b, t)
// produces slot t + 1 (row T - 1: slot 0), so no row waits for another.  Stored for the adjoint: diff [B, T, N] and, for
// substeps > 1, the state before sub-steps 1 .. substeps-1 of every row t <= T-2 ([B, T-1, substeps-1, N]; the state
// before sub-step 0 is a_t itself).
struct PhyArgs {
    Args c;                    // coefficients only
    const float* a;            // [B, T, N]
    const float* diff_in;      // backward: [B, T, N]
    const float* g;            // backward: d L / d loss [B, T, N]
    float* loss;               // forward out [B, T, N]
    float* diff;               // forward out [B, T, N] or null
    float* states;             // forward out / backward in, or null
    float* grad;               // backward out [B, T, N]
    int B, T, N, S;
};

template <int P>
__device__ __forceinline__ void midpoint_step(float (&u)[P], const Args& c) {
    float w[P + 4], r[P], ut[P], zero[P];
#pragma unroll
    for (int j = 0; j < P; ++j) zero[j] = 0.0f;
    window<P>(u, w);
    residual<P>(w, zero, c, r);
#pragma unroll
    for (int j = 0; j < P; ++j) ut[j] = fmaf(c.hdt, r[j], u[j]);
    window<P>(ut, w);
    residual<P>(w, zero, c, r);
#pragma unroll
    for (int j = 0; j < P; ++j) u[j] = fmaf(c.dt, r[j], u[j]);
}

// out = J(v)^T p = nu Lap(p) - Grad(v) o p + Grad(v o p), from the windows of v and p (Lap is symmetric, the central Grad
// antisymmetric under the periodic boundary; the window of v o p is the product of the windows: no further rotation)
template <int P>
__device__ __forceinline__ void residual_adjoint(const float (&wv)[P + 4], const float (&wp)[P + 4], const Args& c, float (&out)[P]) {
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const float gradv = (wv[j + 3] - wv[j + 1]) * c.half_inv_dx;
        const float gradq = fmaf(wv[j + 3], wp[j + 3], -(wv[j + 1] * wp[j + 1])) * c.half_inv_dx;
        float acc = fmaf(c.l0, wp[j + 2], gradq);
        acc = fmaf(c.l1, wp[j + 1] + wp[j + 3], acc);
        acc = fmaf(c.l2, wp[j] + wp[j + 4], acc);
        out[j] = fmaf(-gradv, wp[j + 2], acc);
    }
}

// lam (d L / d u') -> d L / d u of one midpoint sub-step started at u:  w = dt J(u~)^T lam',  lam = lam' + w + dt/2 J(u)^T w
template <int P>
__device__ __forceinline__ void midpoint_step_adjoint(const float (&u)[P], float (&lam)[P], const Args& c) {
    float wu[P + 4], wt[P + 4], wl[P + 4], r[P], ut[P], w[P], zero[P];
#pragma unroll
    for (int j = 0; j < P; ++j) zero[j] = 0.0f;
    window<P>(u, wu);
    residual<P>(wu, zero, c, r);
#pragma unroll
    for (int j = 0; j < P; ++j) ut[j] = fmaf(c.hdt, r[j], u[j]);
    window<P>(ut, wt);
    window<P>(lam, wl);
    residual_adjoint<P>(wt, wl, c, w);
#pragma unroll
    for (int j = 0; j < P; ++j) w[j] *= c.dt;
    window<P>(w, wl);
    residual_adjoint<P>(wu, wl, c, r);
#pragma unroll
    for (int j = 0; j < P; ++j) lam[j] = fmaf(c.hdt, r[j], lam[j] + w[j]);
}

template <int P>
__global__ void __launch_bounds__(256) bg_phyloss_fwd_kernel(const PhyArgs a) {
    const int lane = threadIdx.x & 63;
    const int slot = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int rows = a.B * a.T;
    const bool active = slot < rows;
    const int row = active ? slot : rows - 1;       // tail waves redo the last row (their lanes must still rotate)
    const int b = row / a.T, t = row - b * a.T;
    const size_t col = (size_t)lane * P;
    const float* src = a.a + (size_t)row * a.N + col;

    float u[P], d[P];
#pragma unroll
    for (int j = 0; j < P; ++j) u[j] = src[j];
    size_t out;                                      // the slot this row produces
    if (t + 1 < a.T) {
        float* st = a.states ? a.states + ((size_t)(b * (a.T - 1) + t) * (a.S - 1)) * a.N + col : nullptr;
        for (int s = 0; s < a.S; ++s) {
            if (st && s > 0 && active) {
#pragma unroll
                for (int j = 0; j < P; ++j) st[(size_t)(s - 1) * a.N + j] = u[j];
            }
            midpoint_step<P>(u, a.c);
        }
        out = (size_t)(row + 1) * a.N + col;
#pragma unroll
        for (int j = 0; j < P; ++j) d[j] = a.a[out + j] - u[j];
    } else {                                         // slot 0 is compared with the LAST slice (the reference's choice)
        out = (size_t)(b * a.T) * a.N + col;
#pragma unroll
        for (int j = 0; j < P; ++j) d[j] = a.a[out + j] - u[j];
    }
    if (active) {
#pragma unroll
        for (int j = 0; j < P; ++j) a.loss[out + j] = d[j] * d[j];
        if (a.diff) {
#pragma unroll
            for (int j = 0; j < P; ++j) a.diff[out + j] = d[j];
        }
    }
}

// d L / d a_t = e_t - [t <= T-2] DPhi(a_t)^T e_{t+1} - [t = T-1] e_0,  e = 2 diff g.  One row per wavefront, no atomics.
template <int P>
__global__ void __launch_bounds__(256) bg_phyloss_bwd_kernel(const PhyArgs a) {
    const int lane = threadIdx.x & 63;
    const int slot = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int rows = a.B * a.T;
    const bool active = slot < rows;
    const int row = active ? slot : rows - 1;
    const int b = row / a.T, t = row - b * a.T;
    const size_t col = (size_t)lane * P;
    const size_t own = (size_t)row * a.N + col;
    const size_t other = (t + 1 < a.T ? (size_t)(row + 1) : (size_t)(b * a.T)) * a.N + col;

    float lam[P], u[P];
#pragma unroll
    for (int j = 0; j < P; ++j) lam[j] = 2.0f * a.diff_in[other + j] * a.g[other + j];
    if (t + 1 < a.T) {
        const float* st = a.S > 1 ? a.states + ((size_t)(b * (a.T - 1) + t) * (a.S - 1)) * a.N + col : nullptr;
        for (int s = a.S - 1; s >= 0; --s) {
            const float* src = s > 0 ? st + (size_t)(s - 1) * a.N : a.a + own;
#pragma unroll
            for (int j = 0; j < P; ++j) u[j] = src[j];
            midpoint_step_adjoint<P>(u, lam, a.c);
        }
    }
    if (active) {
#pragma unroll
        for (int j = 0; j < P; ++j) a.grad[own + j] = fmaf(2.0f * a.diff_in[own + j], a.g[own + j], -lam[j]);
    }
}

template <int P>
int launch_phyloss(const char* who, const PhyArgs& a, bool backward, hipStream_t st) {
    const int waves_per_block = 4;
    const int grid = (a.B * a.T + waves_per_block - 1) / waves_per_block;
    if (backward) hipLaunchKernelGGL(bg_phyloss_bwd_kernel<P>, dim3(grid), dim3(64 * waves_per_block), 0, st, a);
    else hipLaunchKernelGGL(bg_phyloss_fwd_kernel<P>, dim3(grid), dim3(64 * waves_per_block), 0, st, a);
    return launch_status(-2, who);
}

// shared host-side validation and dispatch of the two loss entry points
int phyloss_launch(const char* who, PhyArgs& a, bool backward, void* stream, long states_len, float dx, float dt, float nu) {
    if (a.B <= 0 || a.T <= 0 || a.N <= 0 || a.S < 1) return fail(-1, "%s: bad argument", who);
    if (!(dx > 0.0f) || !(dt > 0.0f) || !(nu >= 0.0f)) return fail(-1, "%s: dx, dt must be positive, nu non-negative", who);
    if (a.N % 64) return fail(-4, "%s: N = %d is not a multiple of 64", who, a.N);
    if ((long)a.B * a.T > (1L << 30)) return fail(-1, "%s: B * T = %ld rows is too many", who, (long)a.B * a.T);
    const long need = (long)a.B * (a.T - 1) * (a.S - 1) * a.N;
    if (a.states ? states_len < need : (backward && need > 0))
        return fail(-3, "%s: the sub-step state store holds %ld floats, B (T-1) (substeps-1) N = %ld are needed", who,
                    a.states ? states_len : 0L, need);
    set_coefficients(a.c, dx, dt, nu);
    switch (a.N / 64) {
        case 1: return launch_phyloss<1>(who, a, backward, (hipStream_t)stream);
        case 2: return launch_phyloss<2>(who, a, backward, (hipStream_t)stream);
        case 4: return launch_phyloss<4>(who, a, backward, (hipStream_t)stream);
        case 8: return launch_phyloss<8>(who, a, backward, (hipStream_t)stream);
        case 16: return launch_phyloss<16>(who, a, backward, (hipStream_t)stream);
        default: return fail(-4, "%s: N = %d: supported sizes are 64, 128, 256, 512, 1024", who, a.N);
    }
}

}  // namespace

extern "C" {

const char* bg_last_error(void) { return g_err; }

int bg_step(void* stream, float* u, const float* actions, const float* F, int n_act, int n_envs, int N, float dx, float dt,
            float nu, long n_substeps, float* obs, double* ssq_sum, int* status) {
    if (!u || n_envs <= 0 || N <= 0) return fail(-1, "bg_step: bad argument");
    if (n_substeps < 0) return fail(-1, "bg_step: n_substeps = %ld is negative", n_substeps);
    if (actions && (!F || n_act <= 0)) return fail(-1, "bg_step: actions need the forcing matrix F and n_act > 0");
    if (!(dx > 0.0f) || !(dt > 0.0f) || !(nu >= 0.0f)) return fail(-1, "bg_step: dx, dt must be positive, nu non-negative");
    if (N % 64) return fail(-4, "bg_step: N = %d is not a multiple of 64", N);
    Args a{};
    a.u = u; a.actions = actions; a.F = F; a.obs = obs; a.ssq_sum = ssq_sum; a.status = status;
    a.n_act = n_act; a.n_envs = n_envs; a.N = N; a.n_substeps = n_substeps;
    set_coefficients(a, dx, dt, nu);
    switch (N / 64) {
        case 1: return launch<1>(a, (hipStream_t)stream);
        case 2: return launch<2>(a, (hipStream_t)stream);
        case 4: return launch<4>(a, (hipStream_t)stream);
        case 8: return launch<8>(a, (hipStream_t)stream);
        case 16: return launch<16>(a, (hipStream_t)stream);
        default: return fail(-4, "bg_step: N = %d: supported sizes are 64, 128, 256, 512, 1024", N);
    }
}

int bg_step_span(void* stream, float* u, const float* actions, const float* F, int n_act, int n_envs, int N, int T, float dx,
                 float dt, float nu, long n_substeps, float* traj, double* ssq, int* status) {
    // everything is refused here, before any HIP call
    if (!u || !actions || !F || !traj) return fail(-1, "bg_step_span: NULL u, actions, F or traj");
    if (T < 1) return fail(-1, "bg_step_span: %d steps (at least 1)", T);
    if (n_envs < 1) return fail(-1, "bg_step_span: %d envs (at least 1)", n_envs);
    if (n_act < 1 || n_act > 16) return fail(-1, "bg_step_span: %d actuators (1 ... 16 are supported)", n_act);
    if (n_substeps < 0) return fail(-1, "bg_step_span: n_substeps = %ld is negative", n_substeps);
    if (!(dx > 0.0f) || !(dt > 0.0f) || !(nu >= 0.0f)) return fail(-1, "bg_step_span: dx, dt must be positive, nu non-negative");
    if (N <= 0 || N % 64) return fail(-4, "bg_step_span: N = %d is not a positive multiple of 64", N);
    SpanArgs a{};
    a.s.u = u; a.s.actions = actions; a.s.F = F;
    a.s.n_act = n_act; a.s.n_envs = n_envs; a.s.N = N; a.s.n_substeps = n_substeps;
    a.traj = traj; a.ssq = ssq; a.status = status; a.T = T;
    set_coefficients(a.s, dx, dt, nu);
    switch (N / 64) {
        case 1: return launch_span<1>(a, (hipStream_t)stream);
        case 2: return launch_span<2>(a, (hipStream_t)stream);
        case 4: return launch_span<4>(a, (hipStream_t)stream);
        case 8: return launch_span<8>(a, (hipStream_t)stream);
        case 16: return launch_span<16>(a, (hipStream_t)stream);
        default: return fail(-4, "bg_step_span: N = %d: supported sizes are 64, 128, 256, 512, 1024", N);
    }
}

int bg_record(void* stream, const float* d_traj, const float* d_actions, int n_envs, int N, int A, const double* d_ssq,
              const int* d_steps, int T, long n_substeps, const long* d_dst, const long* dst_host, const bg_slabs* out) {
    // everything is refused here, before any HIP call
    if (!d_traj || !d_actions || !d_ssq || !d_steps || !d_dst || !dst_host || !out)
        return fail(-1, "bg_record: NULL traj, actions, ssq, steps, dst, dst_host or out");
    const PlaceRefusals refusals = {"bg_record", true, -1, -1, -1};
    if (const int rc = check_slab_fields(refusals, out)) return rc;
    if (T < 1) return fail(-1, "bg_record: %d steps (at least 1)", T);
    if (n_envs < 1) return fail(-1, "bg_record: %d envs (at least 1)", n_envs);
    if (N < 1) return fail(-1, "bg_record: rows of %d columns (at least 1)", N);
    if (A < 1 || A > 16) return fail(-1, "bg_record: action width %d (1 ... 16 are supported)", A);
    if (n_substeps < 0) return fail(-1, "bg_record: n_substeps = %ld is negative", n_substeps);
    if (out->rows < 1) return fail(-1, "bg_record: slabs of %ld rows (at least 1)", out->rows);
    const long n = (long)T * n_envs;
    if (const int rc = check_dst_rows(refusals, dst_host, n, out->rows)) return rc;
    RecordArgs a{};
    a.traj = d_traj; a.actions = d_actions; a.ssq = d_ssq; a.steps = d_steps; a.dst = d_dst;
    a.out = *out;
    a.n = n; a.E = n_envs; a.N = N; a.A = A;
    a.vec_obs = N % 4 == 0 && aligned16(d_traj) && aligned16(out->obs) && aligned16(out->nxtobs);
    a.vec_act = A % 4 == 0 && aligned16(d_actions) && aligned16(out->actions);
    a.c = -(1.0 / (double)N) / (double)(n_substeps > 1 ? n_substeps : 1);
    hipLaunchKernelGGL(bg_record_kernel, dim3((unsigned)((n + WAVES - 1) / WAVES)), dim3(NT), 0, (hipStream_t)stream, a);
    return launch_status(-2, "bg_record");
}

int bg_residual(void* stream, const float* u, const float* phi, int n_rows, int N, float dx, float nu, float* out) {
    if (!u || !out || n_rows <= 0 || N < 5 || !(dx > 0.0f)) return fail(-1, "bg_residual: bad argument");
    const float s = nu / (dx * dx);
    const size_t total = (size_t)n_rows * N;
    hipLaunchKernelGGL(bg_residual_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, u, phi, n_rows, N,
                       0.5f / dx, s * (-5.0f / 2.0f), s * (4.0f / 3.0f), s * (-1.0f / 12.0f), out);
    return launch_status(-2, "bg_residual");
}

int bg_phyloss_forward(void* stream, const float* augmented, int B, int T, int N, float dx, float dt, float nu, int substeps,
                       float* loss, float* diff, float* states, long states_len) {
    if (!augmented || !loss) return fail(-1, "bg_phyloss_forward: bad argument");
    if (states && !diff) return fail(-1, "bg_phyloss_forward: a state store without diff");
    PhyArgs a{};
    a.a = augmented; a.loss = loss; a.diff = diff; a.states = substeps > 1 ? states : nullptr;
    a.B = B; a.T = T; a.N = N; a.S = substeps;
    if (diff && substeps > 1 && T > 1 && !states) return fail(-3, "bg_phyloss_forward: substeps > 1 with diff needs the state store");
    return phyloss_launch("bg_phyloss_forward", a, false, stream, states_len, dx, dt, nu);
}

int bg_phyloss_backward(void* stream, const float* augmented, const float* diff, const float* g_loss, const float* states,
                        long states_len, int B, int T, int N, float dx, float dt, float nu, int substeps, float* grad) {
    if (!augmented || !diff || !g_loss || !grad) return fail(-1, "bg_phyloss_backward: bad argument");
    PhyArgs a{};
    a.a = augmented; a.diff_in = diff; a.g = g_loss; a.states = const_cast<float*>(states); a.grad = grad;
    a.B = B; a.T = T; a.N = N; a.S = substeps;
    return phyloss_launch("bg_phyloss_backward", a, true, stream, states_len, dx, dt, nu);
}

}  // extern "C"
