// bg_objective.hip -- bg_step_objective / bg_step_span_objective / bg_reward_rows and the host twins
// (include/burgers/objective.h): the Burgers stepper with the reward sum of either objective, and the row reward of the
// dissipation objective.
//
// Steppers: the layout of bg_step_kernel / bg_step_span_kernel (csrc/burgers.hip): one env per 64-lane wave, P = N / 64
// contiguous points per lane in VGPRs, the +-2 halo from the two neighbouring lanes by DPP wave rotations, tail waves
// redoing the last env; HBM is touched once on entry and once on exit.  The arithmetic of a lane is bg_objective.h's,
// the text the host twin runs over the 64 lanes of a row in turn; under the dissipation objective stage 1 of a sub-step
// feeds its own gradient and u * phi into two more fmaf chains, and nothing of the state arithmetic moves.
// Rows: one group of G lanes per row as bg_eval_rows, two partial sums reduced by xor shuffles, lane 0 writes.
// No atomics, plain vector stores.  Built with -ffp-contract=off and linked beside burgers.hip and bg_eval.hip, whose
// kernels it does not touch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>
#include <vector>

#include "../../include/burgers/objective.h"
#include "bg_objective.h"
#include "capi_error.h"

namespace {

using namespace bgo;

struct Args {
    float* u;
    const float* actions;     // [E][A] (span: [T][E][A]) or null
    const float* F;
    float* obs;
    double* ssq_sum;
    int* status;
    int n_act, n_envs, N;
    long n_substeps;
    Coef c;
};

struct SpanArgs {
    Args s;                    // obs / ssq_sum / status unused
    float* traj;               // [T + 1][E][N], slot 0 is not touched
    double* ssq;               // [T][E] or null
    int* status;               // [T][E] or null
    int T;
};

// DPP control words (GFX9): wave_ror:1 = 0x13C (lane i receives lane i-1), wave_rol:1 = 0x134 (lane i receives lane i+1)
__device__ __forceinline__ float from_lower(float x) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x13C, 0xf, 0xf, false));
}
__device__ __forceinline__ float from_upper(float x) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x134, 0xf, 0xf, false));
}

// the two points on either side of the lane's P: the rotations ARE the periodic boundary
template <int P>
__device__ __forceinline__ void halo(const float (&v)[P], float (&lo)[2], float (&hi)[2]) {
    if constexpr (P == 1) {
        lo[1] = from_lower(v[0]);
        lo[0] = from_lower(lo[1]);
        hi[0] = from_upper(v[0]);
        hi[1] = from_upper(hi[0]);
    } else {
        lo[0] = from_lower(v[P - 2]);
        lo[1] = from_lower(v[P - 1]);
        hi[0] = from_upper(v[0]);
        hi[1] = from_upper(v[1]);
    }
}

template <int P>
__device__ __forceinline__ void forcing(const float* act, const Args& a, int lane, float (&phi)[P]) {
    if (act) {
#pragma unroll
        for (int j = 0; j < P; ++j) phi[j] = forcing_at(act, a.F, a.n_act, a.N, lane * P + j);
    } else {
#pragma unroll
        for (int j = 0; j < P; ++j) phi[j] = 0.0f;
    }
}

// a.n_substeps midpoint sub-steps of the lane's P points with phi held; racc += the reward term of every sub-step
template <int P, int OBJ>
__device__ __forceinline__ void advance(float (&u)[P], const float (&phi)[P], const Args& a, double& racc) {
    for (long s = 0; s < a.n_substeps; ++s) {
        float lo[2], hi[2], ut[P];
        halo<P>(u, lo, hi);
        lane_stage1<P, OBJ>(u, lo, hi, phi, a.c, ut, racc);
        halo<P>(ut, lo, hi);
        lane_stage2<P>(u, ut, lo, hi, phi, a.c);
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

template <int P, int OBJ>
__global__ void __launch_bounds__(256) bg_step_objective_kernel(const Args a) {
    const int lane = threadIdx.x & 63;
    const int slot = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const bool active = slot < a.n_envs;
    const int env = active ? slot : a.n_envs - 1;   // tail waves redo the last env (their lanes must still rotate)
    const size_t off = (size_t)env * a.N + (size_t)lane * P;

    float u[P], phi[P];
#pragma unroll
    for (int j = 0; j < P; ++j) u[j] = a.u[off + j];
    forcing<P>(a.actions ? a.actions + (size_t)env * a.n_act : nullptr, a, lane, phi);
    double racc = 0.0;
    advance<P, OBJ>(u, phi, a, racc);
    const int bad = settle<P>(u, racc);
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

// T env steps of one launch, as bg_step_span_kernel: step t reads row t of the action table, stores the state to traj
// slot t + 1 and, by lane 0, ssq[t][e] and status[t][e]; u is stored once, after the last step
// waves per SIMD of bg_step_span_kernel<P> (profiles/burgers_span_kernel_resources.txt): asked of the compiler, so that
// the two more chains of the dissipation objective do not cost the span its occupancy
constexpr int span_waves(int P) { return P <= 4 ? 8 : P == 8 ? 6 : 4; }

template <int P, int OBJ>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(span_waves(P))))
bg_step_span_objective_kernel(const SpanArgs a) {
    const Args& s = a.s;
    const int lane = threadIdx.x & 63;
    const int slot = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const bool active = slot < s.n_envs;
    const int env = active ? slot : s.n_envs - 1;
    const size_t off = (size_t)env * s.N + (size_t)lane * P;
    const size_t slab = (size_t)s.n_envs * s.N;

    float u[P], phi[P];
#pragma unroll
    for (int j = 0; j < P; ++j) u[j] = s.u[off + j];
    for (int t = 0; t < a.T; ++t) {
        const size_t cell = (size_t)t * s.n_envs + env;
        forcing<P>(s.actions + cell * s.n_act, s, lane, phi);
        double racc = 0.0;
        advance<P, OBJ>(u, phi, s, racc);
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

template <int G>
__global__ void __launch_bounds__(256) bg_reward_rows_kernel(const RewardArgs a) {
    const int gl = threadIdx.x & (G - 1);
    const long row = ((long)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const bool active = row < a.M;                  // inactive groups still take part in the shuffles
    double sd = 0.0, sp = 0.0;
    if (active) reward_row_share(a, row, gl, G, sd, sp);
#pragma unroll
    for (int m = 1; m < G; m <<= 1) {
        sd += __shfl_xor(sd, m, 64);
        sp += __shfl_xor(sp, m, 64);
    }
    if (active && gl == 0) a.reward[row] = reward_row_finish(sd, sp, a.N, a.nu_d);
}

constexpr int WAVES_PER_BLOCK = 4;

template <int P, int OBJ>
void launch_step(const Args& a, hipStream_t st) {
    const int grid = (a.n_envs + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    hipLaunchKernelGGL((bg_step_objective_kernel<P, OBJ>), dim3(grid), dim3(64 * WAVES_PER_BLOCK), 0, st, a);
}

template <int P, int OBJ>
void launch_span(const SpanArgs& a, hipStream_t st) {
    const int grid = (a.s.n_envs + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    hipLaunchKernelGGL((bg_step_span_objective_kernel<P, OBJ>), dim3(grid), dim3(64 * WAVES_PER_BLOCK), 0, st, a);
}

template <int G>
void launch_rows(const RewardArgs& a, hipStream_t st) {
    const int block = 256, rows_per_block = block / G;
    const unsigned grid = (unsigned)((a.M + rows_per_block - 1) / rows_per_block);
    hipLaunchKernelGGL(bg_reward_rows_kernel<G>, dim3(grid), dim3(block), 0, st, a);
}

// one row of the host twin: the 64 lanes of the kernel's wave in turn, stage by stage
template <int P, int OBJ>
void host_env(float* row, const float* act, const Args& a, double& sum, int& bad) {
    const int N = a.N;
    std::vector<float> phi(N, 0.0f), ut(N);
    if (act)
        for (int i = 0; i < N; ++i) phi[i] = forcing_at(act, a.F, a.n_act, N, i);
    double racc[LANES] = {};
    auto lane_of = [](float* p, int lane) -> float (&)[P] { return *reinterpret_cast<float (*)[P]>(p + lane * P); };
    auto halo_of = [N](const float* p, int lane, float (&lo)[2], float (&hi)[2]) {
        const int i = lane * P;
        lo[0] = p[wrap(i - 2, N)]; lo[1] = p[wrap(i - 1, N)];
        hi[0] = p[wrap(i + P, N)]; hi[1] = p[wrap(i + P + 1, N)];
    };
    for (long s = 0; s < a.n_substeps; ++s) {
        float lo[2], hi[2];
        for (int lane = 0; lane < LANES; ++lane) {
            halo_of(row, lane, lo, hi);
            lane_stage1<P, OBJ>(lane_of(row, lane), lo, hi, lane_of(phi.data(), lane), a.c, lane_of(ut.data(), lane), racc[lane]);
        }
        for (int lane = 0; lane < LANES; ++lane) {
            halo_of(ut.data(), lane, lo, hi);
            lane_stage2<P>(lane_of(row, lane), lane_of(ut.data(), lane), lo, hi, lane_of(phi.data(), lane), a.c);
        }
    }
    for (int m = 1; m < LANES; m <<= 1) {            // the butterfly of `settle`
        double next[LANES];
        for (int l = 0; l < LANES; ++l) next[l] = racc[l] + racc[l ^ m];
        for (int l = 0; l < LANES; ++l) racc[l] = next[l];
    }
    sum = racc[0];
    bad = 0;
    for (int i = 0; i < N; ++i) bad |= !std::isfinite(row[i]);
}

template <int P, int OBJ>
void host_step(const Args& a) {
    for (int e = 0; e < a.n_envs; ++e) {
        float* row = a.u + (size_t)e * a.N;
        double sum;
        int bad;
        host_env<P, OBJ>(row, a.actions ? a.actions + (size_t)e * a.n_act : nullptr, a, sum, bad);
        if (a.obs)
            for (int i = 0; i < a.N; ++i) a.obs[(size_t)e * a.N + i] = row[i];
        if (a.ssq_sum) a.ssq_sum[e] = sum;
        if (a.status) a.status[e] = bad;
    }
}

// f.template operator()<P, OBJ>() for the width and the objective (both already checked)
template <class Fn>
void dispatch(int N, int objective, Fn&& f) {
    auto by_objective = [&](auto p) {
        constexpr int P = decltype(p)::value;
        if (objective == DISSIPATION) f.template operator()<P, DISSIPATION>();
        else f.template operator()<P, L2CONTROL>();
    };
    switch (N / 64) {
        case 1: by_objective(std::integral_constant<int, 1>{}); break;
        case 2: by_objective(std::integral_constant<int, 2>{}); break;
        case 4: by_objective(std::integral_constant<int, 4>{}); break;
        case 8: by_objective(std::integral_constant<int, 8>{}); break;
        default: by_objective(std::integral_constant<int, 16>{}); break;
    }
}

struct StepLaunch {
    const Args& a; hipStream_t st;
    template <int P, int OBJ> void operator()() const { launch_step<P, OBJ>(a, st); }
};
struct SpanLaunch {
    const SpanArgs& a; hipStream_t st;
    template <int P, int OBJ> void operator()() const { launch_span<P, OBJ>(a, st); }
};
struct HostStep {
    const Args& a;
    template <int P, int OBJ> void operator()() const { host_step<P, OBJ>(a); }
};

// the refusals the stepper entries share, and the arguments when there is none; T and traj are read for a span only
int step_args(const char* who, bool span, float* u, const float* actions, const float* F, int n_act, int n_envs, int N, int T,
              float dx, float dt, float nu, long n_substeps, const float* traj, int objective, Args& a) {
    if (span) {
        if (!u || !actions || !F || !traj) return fail(-1, "%s: NULL u, actions, F or traj", who);
        if (T < 1) return fail(-1, "%s: %d steps (at least 1)", who, T);
    } else {
        if (!u) return fail(-1, "%s: NULL u", who);
        if (actions && !F) return fail(-1, "%s: actions need the forcing matrix F", who);
    }
    if (n_envs < 1) return fail(-1, "%s: %d envs (at least 1)", who, n_envs);
    if (actions && (n_act < 1 || n_act > 16)) return fail(-1, "%s: %d actuators (1 ... 16 are supported)", who, n_act);
    if (n_substeps < 0) return fail(-1, "%s: n_substeps = %ld is negative", who, n_substeps);
    if (!(dx > 0.0f) || !(dt > 0.0f) || !(nu >= 0.0f)) return fail(-1, "%s: dx, dt must be positive, nu non-negative", who);
    if (objective != L2CONTROL && objective != DISSIPATION)
        return fail(-1, "%s: objective %d (0 l2control and 1 dissipation are known)", who, objective);
    if (N <= 0 || N % 64) return fail(-4, "%s: N = %d is not a positive multiple of 64", who, N);
    const int P = N / 64;
    if (P != 1 && P != 2 && P != 4 && P != 8 && P != 16)
        return fail(-4, "%s: N = %d: supported sizes are 64, 128, 256, 512, 1024", who, N);
    a = {};
    a.u = u; a.actions = actions; a.F = F;
    a.n_act = n_act; a.n_envs = n_envs; a.N = N; a.n_substeps = n_substeps;
    a.c = coefficients(dx, dt, nu);
    return 0;
}

constexpr int MAX_ROWS = 1 << 30;

int reward_args(const char* who, const float* u, const float* phi, const float* actions, const float* F, int M, int N, int A,
                double dx, double nu, double* reward, RewardArgs& a) {
    if (!u || !reward) return fail(-1, "%s: NULL u or reward", who);
    if (phi && actions) return fail(-1, "%s: both a forcing field and actions", who);
    if (actions && !F) return fail(-1, "%s: actions need the forcing matrix F", who);
    if (actions && (A < 1 || A > 16)) return fail(-1, "%s: %d actuators (1 ... 16 are supported)", who, A);
    if (M < 1 || M > MAX_ROWS) return fail(-1, "%s: %d rows (1 ... 2^30)", who, M);
    if (N < 3) return fail(-1, "%s: rows of %d points (the gradient needs at least 3)", who, N);
    if (!(dx > 0.0) || !std::isfinite(dx)) return fail(-1, "%s: dx = %g is not positive and finite", who, dx);
    if (!(nu >= 0.0) || !std::isfinite(nu)) return fail(-1, "%s: nu = %g is negative or not finite", who, nu);
    a = {};
    a.u = u; a.phi = phi; a.actions = actions; a.F = F;
    a.M = M; a.N = N; a.A = A;
    a.two_dx = 2.0 * dx; a.nu_d = (double)(float)nu;
    a.reward = reward;
    return 0;
}

}  // namespace

extern "C" {

const char* bg_objective_last_error(void) { return g_err; }

int bg_step_objective(void* stream, float* u, const float* actions, const float* F, int n_act, int n_envs, int N, float dx,
                      float dt, float nu, long n_substeps, float* obs, double* ssq_sum, int* status, int objective) {
    Args a;
    if (const int rc = step_args("bg_step_objective", false, u, actions, F, n_act, n_envs, N, 0, dx, dt, nu, n_substeps,
                                 nullptr, objective, a))
        return rc;
    a.obs = obs; a.ssq_sum = ssq_sum; a.status = status;
    dispatch(N, objective, StepLaunch{a, (hipStream_t)stream});
    return launch_status(-2, "bg_step_objective");
}

int bg_step_span_objective(void* stream, float* u, const float* actions, const float* F, int n_act, int n_envs, int N, int T,
                           float dx, float dt, float nu, long n_substeps, float* traj, double* ssq, int* status, int objective) {
    SpanArgs a{};
    if (const int rc = step_args("bg_step_span_objective", true, u, actions, F, n_act, n_envs, N, T, dx, dt, nu, n_substeps,
                                 traj, objective, a.s))
        return rc;
    a.traj = traj; a.ssq = ssq; a.status = status; a.T = T;
    dispatch(N, objective, SpanLaunch{a, (hipStream_t)stream});
    return launch_status(-2, "bg_step_span_objective");
}

int bg_reward_rows(void* stream, const float* u, const float* phi, const float* actions, const float* F, int M, int N, int A,
                   double dx, double nu, double* reward) {
    RewardArgs a;
    if (const int rc = reward_args("bg_reward_rows", u, phi, actions, F, M, N, A, dx, nu, reward, a)) return rc;
    // the partition of bg_eval_rows
    if (N <= 64) launch_rows<16>(a, (hipStream_t)stream);
    else if (N <= 512) launch_rows<32>(a, (hipStream_t)stream);
    else launch_rows<64>(a, (hipStream_t)stream);
    return launch_status(-2, "bg_reward_rows");
}

int bg_step_objective_host(float* u, const float* actions, const float* F, int n_act, int n_envs, int N, float dx, float dt,
                           float nu, long n_substeps, float* obs, double* ssq_sum, int* status, int objective) {
    Args a;
    if (const int rc = step_args("bg_step_objective_host", false, u, actions, F, n_act, n_envs, N, 0, dx, dt, nu,
                                 n_substeps, nullptr, objective, a))
        return rc;
    a.obs = obs; a.ssq_sum = ssq_sum; a.status = status;
    dispatch(N, objective, HostStep{a});
    return 0;
}

int bg_reward_rows_host(const float* u, const float* phi, const float* actions, const float* F, int M, int N, int A, double dx,
                        double nu, double* reward) {
    RewardArgs a;
    if (const int rc = reward_args("bg_reward_rows_host", u, phi, actions, F, M, N, A, dx, nu, reward, a)) return rc;
    for (long row = 0; row < M; ++row) {
        double sd = 0.0, sp = 0.0;
        reward_row_share(a, row, 0, 1, sd, sp);
        reward[row] = reward_row_finish(sd, sp, N, a.nu_d);
    }
    return 0;
}

}  // extern "C"
