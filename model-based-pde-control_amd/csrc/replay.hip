// replay.hip -- the fused batch gather of the policy-update phase, and the append and episode returns of the
// device-resident replay (C ABI: include/replay_hip.h; binding: pdecontrol/mbrl/replay_hip.py).
//
// One launch assembles one SAC batch from several packed replays.  A wave owns a sample: it reads the sample's row in the
// concatenated row space, finds the source by comparing against the (at most RP_MAX_SOURCES) first rows -- the sources
// travel in the kernel arguments, so the search is a handful of wave-uniform selects on constant indices -- and copies the
// row with lanes along the columns: obs and nxtobs through the sensor and the observation coefficients, actions through
// the action coefficients, reward and terminated flag by lane 0.  float4 where the source allows it (see `vec` below).
//
// The affine map and the row copy (copy_row, copy_row4) are row_ops.h's, so the batch equals the host loader's bit for
// bit.  Plain vector stores only; nothing is stored through the scalar unit.
//
// rpd_moments reads the same rows the other way round: nothing is copied, the scaled state changes of all rows are
// reduced to per-column fp64 sums in two or three launches (partials per workgroup, then folds in index order).
// rpn_moments (include/replay/fit.h) is the same scheme over three fields of the rows at once: observations, actions and
// forced actions, the scaling fits of the offline evaluation.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/replay/fit.h"
#include "../../include/replay_hip.h"
#include "capi_error.h"
#include "place_rows.h"
#include "row_ops.h"

namespace {

struct GatherArgs {
    rp_source src[RP_MAX_SOURCES];
    long first[RP_MAX_SOURCES];        // first row of each source in the concatenated row space
    long total;                        // rows of all sources
    unsigned vec;                      // bit s: source s takes the float4 path
    int nsrc, B, obs_dim, act_dim;
    const long* rows;
    float* obs;
    float* actions;
    float* nxtobs;
    float* rewards;
    float* terminated;
};

__global__ __launch_bounds__(NT) void rp_gather_kernel(const GatherArgs g)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int b = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (b >= g.B) return;
    const long r = g.rows[b];
    float* __restrict__ obs = g.obs + (long)b * g.obs_dim;
    float* __restrict__ nxt = g.nxtobs + (long)b * g.obs_dim;
    float* __restrict__ act = g.actions + (long)b * g.act_dim;

    if (r < 0 || r >= g.total) {      // not a row of any source: read nothing, poison the sample
        for (int j = lane; j < g.obs_dim; j += WAVE) obs[j] = nxt[j] = NAN;
        if (lane < g.act_dim) act[lane] = NAN;
        if (lane == 0) g.rewards[b] = g.terminated[b] = NAN;
        return;
    }

    // wave-uniform selects over constant indices: the argument struct is never indexed dynamically
    rp_source s = g.src[0];
    long first = 0;
    bool vec = g.vec & 1u;
#pragma unroll
    for (int k = 1; k < RP_MAX_SOURCES; ++k) {
        if (k < g.nsrc && r >= g.first[k]) {
            s = g.src[k];
            first = g.first[k];
            vec = (g.vec >> k) & 1u;
        }
    }
    const long row = r - first;
    const float* __restrict__ src_obs = s.obs + row * s.obs_width;
    const float* __restrict__ src_nxt = s.nxtobs + row * s.obs_width;
    if (vec) {
        copy_row4(src_obs, s.obs_coef, obs, g.obs_dim, s.sensor_start, lane);
        copy_row4(src_nxt, s.obs_coef, nxt, g.obs_dim, s.sensor_start, lane);
    } else {
        copy_row(src_obs, s.obs_coef, obs, g.obs_dim, s.sensor_start, s.sensor_stride, lane);
        copy_row(src_nxt, s.obs_coef, nxt, g.obs_dim, s.sensor_start, s.sensor_stride, lane);
    }
    copy_row(s.actions + row * s.act_width, s.act_coef, act, g.act_dim, 0, 1, lane);
    if (lane == 0) {
        g.rewards[b] = s.rewards[row];
        g.terminated[b] = s.terminated[row] ? 1.0f : 0.0f;
    }
}

// ---- the device-resident replay: append of a rollout round, episode returns -----------------------------------------
struct AppendArgs {
    const float* traj;                 // [T_cap + 1][B][N]
    const float* actions;              // [T_cap][B][A]
    const float* rewards;              // [T_cap][B]
    const int* steps;                  // [T_cap][B]
    const long* dst;                   // [T][B]
    rp_slab slab;
    int T, B, N, A;
    int vec_obs, vec_act;
};

__global__ __launch_bounds__(NT) void rp_append_kernel(const AppendArgs a)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const long w = (long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (w >= (long)a.T * a.B) return;
    const long r = a.dst[w];
    if (r < 0 || r >= a.slab.rows) return;           // negative: skipped by contract; beyond the slab: never written
    const int t = (int)(w / a.B);
    place_row(a.traj + w * a.N, a.slab.obs + r * a.N, a.N, a.vec_obs, lane);
    place_row(a.traj + (w + a.B) * a.N, a.slab.nxtobs + r * a.N, a.N, a.vec_obs, lane);
    place_row(a.actions + w * a.A, a.slab.actions + r * a.A, a.A, a.vec_act, lane);
    if (lane == 0) {
        a.slab.rewards[r] = a.rewards[w];
        a.slab.steps[r] = a.steps[w];
        a.slab.terminated[r] = 0;
        a.slab.truncated[r] = t == a.T - 1 ? 1 : 0;
    }
}

__global__ __launch_bounds__(NT) void rp_episode_returns_kernel(const float* __restrict__ rewards, long slab_rows,
                                                                const long* __restrict__ rows, long nrows,
                                                                const long* __restrict__ offsets, int E, float* __restrict__ returns)
{
    const int e = blockIdx.x * NT + threadIdx.x;
    if (e >= E) return;
    const long lo = offsets[e], hi = offsets[e + 1];
    if (lo < 0 || hi < lo || hi > nrows) {
        returns[e] = NAN;
        return;
    }
    float acc = 0.0f;
    for (long i = lo; i < hi; ++i) {
        const long r = rows[i];
        acc = __fadd_rn(acc, r >= 0 && r < slab_rows ? rewards[r] : NAN);
    }
    returns[e] = acc;
}

// ---- the moments of the scaled state changes (update_delta_transform) -----------------------------------------------
struct DeltaArgs {
    const float* obs;                  // [slab_rows][obs_width]
    const float* nxtobs;
    const float* coef;                 // [4][obs_dim] or NULL
    const long* rows;                  // [n] or NULL: rows 0 ... n - 1
    long n, slab_rows;
    int obs_width, obs_dim, start, stride;
    float delta;
    double* ws;                        // [groups][2][obs_dim], then the rows of the middle launch
};

constexpr int TILE = 4 * WAVE;         // columns of one blockIdx.y: four per lane
constexpr int TURN = 4;                // rows a wave has in flight at a time
constexpr int FOLD = 32;               // partial rows one workgroup of the middle launch folds

__device__ __forceinline__ float scaled_delta(float nxt, float obs, float delta) { return __fdiv_rn(__fsub_rn(nxt, obs), delta); }

// A wave owns TURN consecutive rows of the list at a time -- their loads are issued together, which is what keeps enough
// bytes in flight -- and keeps sum d and sum d * d of its four columns of the tile in fp64 registers; the four waves'
// pairs meet in LDS and are added in wave order.  VEC: lane l holds columns 4 l ... 4 l + 3 of the tile (one float4 per
// field), else columns l, l + 64, l + 128, l + 192.
template <bool VEC>
__global__ __launch_bounds__(NT) void rpd_moments_kernel(const DeltaArgs a)
{
    __shared__ double part[WAVES][2][TILE];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const int j0 = blockIdx.y * TILE;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    for (long i0 = ((long)blockIdx.x * WAVES + wave) * TURN; i0 < a.n; i0 += (long)gridDim.x * WAVES * TURN) {
        long first[TURN];
        int state[TURN];               // 0: past the list, 1: a row of the slab, 2: outside it (read nothing, poison)
        float o[TURN][4], x[TURN][4];
#pragma unroll
        for (int t = 0; t < TURN; ++t) {
            const long i = i0 + t;
            const long r = i < a.n ? (a.rows ? a.rows[i] : i) : -1;
            const bool inside = r >= 0 && r < a.slab_rows;
            state[t] = i < a.n ? (inside ? 1 : 2) : 0;
            first[t] = inside ? r * a.obs_width + a.start : 0;
        }
#pragma unroll
        for (int t = 0; t < TURN; ++t) {
#pragma unroll
            for (int k = 0; k < 4; ++k) o[t][k] = x[t][k] = 0.0f;
            if (state[t] != 1) continue;
            if (VEC) {
                const int j = j0 + 4 * lane;
                if (j < a.obs_dim) {
                    const f4 vo = *reinterpret_cast<const f4*>(a.obs + first[t] + j);
                    const f4 vx = *reinterpret_cast<const f4*>(a.nxtobs + first[t] + j);
                    o[t][0] = vo.x, o[t][1] = vo.y, o[t][2] = vo.z, o[t][3] = vo.w;
                    x[t][0] = vx.x, x[t][1] = vx.y, x[t][2] = vx.z, x[t][3] = vx.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int j = j0 + lane + k * WAVE;
                    if (j0 + k * WAVE >= a.obs_dim) break;      // wave-uniform: a narrow row costs what it holds
                    if (j < a.obs_dim) {
                        o[t][k] = a.obs[first[t] + (long)j * a.stride];
                        x[t][k] = a.nxtobs[first[t] + (long)j * a.stride];
                    }
                }
            }
        }
#pragma unroll
        for (int t = 0; t < TURN; ++t) {
            if (state[t] == 0) continue;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = j0 + (VEC ? 4 * lane + k : lane + k * WAVE);
                if (!VEC && j0 + k * WAVE >= a.obs_dim) break;
                float d = 0.0f;
                if (state[t] == 2)
                    d = NAN;
                else if (j < a.obs_dim)
                    d = scaled_delta(affine_col(a.coef, a.obs_dim, j, x[t][k]), affine_col(a.coef, a.obs_dim, j, o[t][k]), a.delta);
                const double v = (double)d;
                s[k] += v;
                q[k] += v * v;         // the product of two fp32 values is exact in fp64
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = VEC ? 4 * lane + k : lane + k * WAVE;
        part[wave][0][c] = s[k];
        part[wave][1][c] = q[k];
    }
    __syncthreads();
    const int j = j0 + threadIdx.x;    // NT == TILE: a thread per column of the tile
    if (j < a.obs_dim) {
        double S = part[0][0][threadIdx.x], Q = part[0][1][threadIdx.x];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
            S += part[w][0][threadIdx.x];
            Q += part[w][1][threadIdx.x];
        }
        double* __restrict__ out = a.ws + (long)blockIdx.x * 2 * a.obs_dim;
        out[j] = S;
        out[a.obs_dim + j] = Q;
    }
}

// the middle launch: workgroup b adds the partial rows FOLD b ... FOLD b + FOLD - 1 of `in` (of `groups`) in index order
// into row b of `out`; a thread per column
__global__ __launch_bounds__(NT) void rpd_middle_kernel(const double* __restrict__ in, int groups, int obs_dim,
                                                             double* __restrict__ out)
{
    const int j = blockIdx.y * NT + threadIdx.x;
    if (j >= obs_dim) return;
    const int g0 = blockIdx.x * FOLD, g1 = g0 + FOLD < groups ? g0 + FOLD : groups;
    double S = 0.0, Q = 0.0;
#pragma unroll 8
    for (int g = g0; g < g1; ++g) {
        S += in[(long)g * 2 * obs_dim + j];
        Q += in[(long)g * 2 * obs_dim + obs_dim + j];
    }
    out[(long)blockIdx.x * 2 * obs_dim + j] = S;
    out[(long)blockIdx.x * 2 * obs_dim + obs_dim + j] = Q;
}

// mean and unbiased variance of m values from their fp64 sum and sum of squares, rounded once
__device__ __forceinline__ void write_stats(double S, double Q, double m, float* __restrict__ mean, float* __restrict__ var)
{
    *mean = (float)(S / m);
    *var = m < 2.0 ? NAN : (float)((Q - S * S / m) / (m - 1.0));
}

// the closing launch, one workgroup: the partial rows per column in index order, then the totals over the columns in
// column order
__global__ __launch_bounds__(NT) void rpd_fold_kernel(const double* __restrict__ ws, int groups, int obs_dim, long n,
                                                           double* __restrict__ sums, float* __restrict__ stats)
{
    __shared__ double col[2][RP_MAX_OBS_DIM];
    const int ld = obs_dim + 1;
    for (int j = threadIdx.x; j < obs_dim; j += NT) {
        double S = 0.0, Q = 0.0;
#pragma unroll 8
        for (int g = 0; g < groups; ++g) {
            S += ws[(long)g * 2 * obs_dim + j];
            Q += ws[(long)g * 2 * obs_dim + obs_dim + j];
        }
        col[0][j] = sums[j] = S;
        col[1][j] = sums[ld + j] = Q;
        write_stats(S, Q, (double)n, stats + j, stats + ld + j);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double S = 0.0, Q = 0.0;
        for (int j = 0; j < obs_dim; ++j) {
            S += col[0][j];
            Q += col[1][j];
        }
        sums[obs_dim] = S;
        sums[ld + obs_dim] = Q;
        write_stats(S, Q, (double)n * obs_dim, stats + obs_dim, stats + ld + obs_dim);
    }
}

// workgroups of rpd_moments for n rows: `groups`, or the default for 0 (a turn of rows per wave), at most
// RP_MAX_DELTA_GROUPS
int delta_groups(long n, int groups)
{
    const long most = RP_MAX_DELTA_GROUPS, per = WAVES * TURN;
    const long g = groups > 0 ? groups : (n + per - 1) / per;
    return (int)(g < most ? g : most);
}

// partial rows the middle launch leaves of G (0: there is no middle launch)
int delta_middle_rows(int G) { return G > FOLD ? (G + FOLD - 1) / FOLD : 0; }

// ---- the moments of observations, actions and forced actions (fit_scalings of the offline evaluation) --------------
struct FitArgs {
    const float* obs;                  // [slab_rows][N]
    const float* actions;              // [slab_rows][A]
    const float* F;                    // [A][N] or NULL: no forced field
    const long* rows;                  // [n] or NULL: rows 0 ... n - 1
    long n, slab_rows;
    int N, A, W;                       // W = N + A (+ N with F): columns of a workspace row
    double* ws;                        // [groups][2][W], then the rows of the middle launch
};

// The four waves' pairs of one field meet in LDS and are added in wave order into columns first + j0 ... of the
// workgroup's workspace row.  Every thread of the workgroup calls it.
template <bool VEC>
__device__ __forceinline__ void meet(double (*part)[2][TILE], const double* s, const double* q, int j0, int width, int first,
                                     double* __restrict__ out, int W)
{
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = VEC ? 4 * lane + k : lane + k * WAVE;
        part[wave][0][c] = s[k];
        part[wave][1][c] = q[k];
    }
    __syncthreads();
    const int j = j0 + threadIdx.x;    // NT == TILE: a thread per column of the tile
    if (j < width) {
        double S = part[0][0][threadIdx.x], Q = part[0][1][threadIdx.x];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
            S += part[w][0][threadIdx.x];
            Q += part[w][1][threadIdx.x];
        }
        out[first + j] = S;
        out[W + first + j] = Q;
    }
    __syncthreads();
}

// rpd_moments_kernel's shape: a wave owns TURN consecutive rows of the list at a time and keeps the sums of its four
// columns of the tile, per field, in fp64 registers.  The forced value of a column is forcing_col's chain over the row's
// A actions, which every lane reads (a wave-uniform address); the A action columns themselves are lanes 0 ... A - 1 of
// tile 0.
template <bool VEC>
__global__ __launch_bounds__(NT) void rpn_moments_kernel(const FitArgs a)
{
    __shared__ double part[WAVES][2][TILE];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const int j0 = blockIdx.y * TILE;
    const bool forced = a.F != nullptr, act_tile = blockIdx.y == 0;
    double so[4] = {0.0, 0.0, 0.0, 0.0}, qo[4] = {0.0, 0.0, 0.0, 0.0};
    double sf[4] = {0.0, 0.0, 0.0, 0.0}, qf[4] = {0.0, 0.0, 0.0, 0.0};
    double sa[4] = {0.0, 0.0, 0.0, 0.0}, qa[4] = {0.0, 0.0, 0.0, 0.0};     // entry 0 alone is used: a lane per action
    for (long i0 = ((long)blockIdx.x * WAVES + wave) * TURN; i0 < a.n; i0 += (long)gridDim.x * WAVES * TURN) {
        long row[TURN];
        int state[TURN];               // 0: past the list, 1: a row of the slab, 2: outside it (read nothing, poison)
        float o[TURN][4], f[TURN][4], u[TURN];
#pragma unroll
        for (int t = 0; t < TURN; ++t) {
            const long i = i0 + t;
            const long r = i < a.n ? (a.rows ? a.rows[i] : i) : -1;
            const bool inside = r >= 0 && r < a.slab_rows;
            state[t] = i < a.n ? (inside ? 1 : 2) : 0;
            row[t] = inside ? r : 0;
        }
#pragma unroll
        for (int t = 0; t < TURN; ++t) {
            u[t] = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[t][k] = f[t][k] = 0.0f;
            if (state[t] != 1) continue;
            const float* __restrict__ src = a.obs + row[t] * a.N;
            const float* __restrict__ act = a.actions + row[t] * a.A;
            if (act_tile && lane < a.A) u[t] = act[lane];
            if (VEC) {
                const int j = j0 + 4 * lane;
                if (j < a.N) {
                    const f4 vo = *reinterpret_cast<const f4*>(src + j);
                    o[t][0] = vo.x, o[t][1] = vo.y, o[t][2] = vo.z, o[t][3] = vo.w;
                    if (forced) {
                        const f4 vf = forcing_col4(nullptr, a.A, act, a.F + j, a.N);
                        f[t][0] = vf.x, f[t][1] = vf.y, f[t][2] = vf.z, f[t][3] = vf.w;
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int j = j0 + lane + k * WAVE;
                    if (j0 + k * WAVE >= a.N) break;            // wave-uniform: a narrow row costs what it holds
                    if (j < a.N) {
                        o[t][k] = src[j];
                        if (forced) f[t][k] = forcing_col(nullptr, a.A, act, a.F + j, a.N);
                    }
                }
            }
        }
#pragma unroll
        for (int t = 0; t < TURN; ++t) {
            if (state[t] == 0) continue;
            const bool poison = state[t] == 2;
            if (act_tile && lane < a.A) {
                const double v = poison ? (double)NAN : (double)u[t];
                sa[0] += v;
                qa[0] += v * v;        // the product of two fp32 values is exact in fp64
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = j0 + (VEC ? 4 * lane + k : lane + k * WAVE);
                if (!VEC && j0 + k * WAVE >= a.N) break;
                if (j >= a.N) continue;
                const double v = poison ? (double)NAN : (double)o[t][k];
                so[k] += v;
                qo[k] += v * v;
                if (forced) {
                    const double w = poison ? (double)NAN : (double)f[t][k];
                    sf[k] += w;
                    qf[k] += w * w;
                }
            }
        }
    }
    double* __restrict__ out = a.ws + (long)blockIdx.x * 2 * a.W;
    meet<VEC>(part, so, qo, j0, a.N, 0, out, a.W);
    if (act_tile) meet<false>(part, sa, qa, 0, a.A, a.N, out, a.W);        // blockIdx.y is uniform over the workgroup
    if (forced) meet<VEC>(part, sf, qf, j0, a.N, a.N + a.A, out, a.W);
}

// the closing launch, one workgroup: the partial rows per column in index order, then every field's total over its
// columns in column order, a thread per field.  Column j of the workspace row lies in field 0 (j < N), 1 (j < N + A) or
// 2, and goes to entry j + field of the output: each earlier field leaves a slot for its total.
__global__ __launch_bounds__(NT) void rpn_fold_kernel(const double* __restrict__ ws, int groups, int N, int A, int forced, long n,
                                                      double* __restrict__ sums, float* __restrict__ stats)
{
    __shared__ double col[2][2 * RP_MAX_OBS_DIM + RP_MAX_ACT_DIM];
    const int W = N + A + (forced ? N : 0), ld = W + (forced ? 3 : 2);
    for (int j = threadIdx.x; j < W; j += NT) {
        double S = 0.0, Q = 0.0;
#pragma unroll 8
        for (int g = 0; g < groups; ++g) {
            S += ws[(long)g * 2 * W + j];
            Q += ws[(long)g * 2 * W + W + j];
        }
        const int e = j + (j < N ? 0 : (j < N + A ? 1 : 2));
        col[0][j] = sums[e] = S;
        col[1][j] = sums[ld + e] = Q;
        write_stats(S, Q, (double)n, stats + e, stats + ld + e);
    }
    __syncthreads();
    if (threadIdx.x < (forced ? 3 : 2)) {
        const int field = threadIdx.x;
        const int first = field == 0 ? 0 : (field == 1 ? N : N + A), width = field == 1 ? A : N;
        double S = 0.0, Q = 0.0;
        for (int j = first; j < first + width; ++j) {
            S += col[0][j];
            Q += col[1][j];
        }
        const int e = first + width + field;
        sums[e] = S;
        sums[ld + e] = Q;
        write_stats(S, Q, (double)n * width, stats + e, stats + ld + e);
    }
}

int obs_dim_of(const rp_source& s) { return width_of(s.obs_width, s.sensor_start, s.sensor_stride); }

}  // namespace

extern "C" {

int rp_supported(int nsrc, const rp_source* srcs, int B)
{
    if (nsrc < 1 || nsrc > RP_MAX_SOURCES)
        return fail(-1, "rp_gather: %d sources (1 ... %d are supported)", nsrc, RP_MAX_SOURCES);
    if (!srcs) return fail(-2, "rp_gather: NULL source array");
    if (B < 1) return fail(-3, "rp_gather: batch size %d (at least 1)", B);
    for (int i = 0; i < nsrc; ++i) {
        const rp_source& s = srcs[i];
        if (!s.obs || !s.actions || !s.nxtobs || !s.rewards || !s.terminated)
            return fail(-2, "rp_gather: source %d has a NULL field pointer", i);
        if (s.sensor_stride < 1) return fail(-4, "rp_gather: source %d has sensor stride %d (at least 1)", i, s.sensor_stride);
        if (s.obs_width < 1 || s.sensor_start < 0 || s.sensor_start >= s.obs_width)
            return fail(-5, "rp_gather: source %d starts its sensor at column %d of %d", i, s.sensor_start, s.obs_width);
        if (s.act_width < 1 || s.act_width > RP_MAX_ACT_DIM)
            return fail(-6, "rp_gather: source %d has action width %d (1 ... %d are supported)", i, s.act_width, RP_MAX_ACT_DIM);
        if (obs_dim_of(s) > RP_MAX_OBS_DIM)
            return fail(-7, "rp_gather: source %d yields %d observation columns (1 ... %d are supported)", i, obs_dim_of(s),
                        RP_MAX_OBS_DIM);
        if (obs_dim_of(s) != obs_dim_of(srcs[0]) || s.act_width != srcs[0].act_width)
            return fail(-8, "rp_gather: source %d yields %d observation and %d action columns, source 0 yields %d and %d", i,
                        obs_dim_of(s), s.act_width, obs_dim_of(srcs[0]), srcs[0].act_width);
        if (s.rows < 1) return fail(-9, "rp_gather: source %d has %ld rows (at least 1)", i, s.rows);
    }
    return 0;
}

int rp_gather(void* stream, int nsrc, const rp_source* srcs, int B, const long* rows, float* obs, float* actions,
              float* nxtobs, float* rewards, float* terminated)
{
    const int rc = rp_supported(nsrc, srcs, B);
    if (rc != 0) return rc;
    if (!rows || !obs || !actions || !nxtobs || !rewards || !terminated)
        return fail(-10, "rp_gather: NULL rows or output pointer");
    GatherArgs g = {};
    g.nsrc = nsrc;
    g.B = B;
    g.obs_dim = obs_dim_of(srcs[0]);
    g.act_dim = srcs[0].act_width;
    g.rows = rows;
    g.obs = obs;
    g.actions = actions;
    g.nxtobs = nxtobs;
    g.rewards = rewards;
    g.terminated = terminated;
    const bool out4 = g.obs_dim % 4 == 0 && aligned16(obs) && aligned16(nxtobs);
    long first = 0;
    for (int i = 0; i < RP_MAX_SOURCES; ++i) {
        g.first[i] = first;
        if (i >= nsrc) continue;
        const rp_source& s = srcs[i];
        g.src[i] = s;
        first += s.rows;
        if (out4 && s.sensor_stride == 1 && s.obs_width % 4 == 0 && s.sensor_start % 4 == 0 && aligned16(s.obs) &&
            aligned16(s.nxtobs) && aligned16(s.obs_coef))
            g.vec |= 1u << i;
    }
    g.total = first;
    hipLaunchKernelGGL(rp_gather_kernel, dim3((B + WAVES - 1) / WAVES), dim3(NT), 0, static_cast<hipStream_t>(stream), g);
    return launch_status(-20, "rp_gather");
}

int rp_append(void* stream, const float* block, int T, int T_cap, int B, int N, int A, const long* dst, const long* dst_host,
              const rp_slab* slab)
{
    if (!block || !dst || !dst_host || !slab) return fail(-30, "rp_append: NULL block, dst, dst_host or slab");
    const PlaceRefusals refusals = {"rp_append", false, -30, -36, -37};
    if (const int rc = check_slab_fields(refusals, slab)) return rc;
    if (T < 1 || T > T_cap) return fail(-31, "rp_append: %d steps of a block laid out for %d (1 ... %d)", T, T_cap, T_cap);
    if (B < 1) return fail(-32, "rp_append: %d envs (at least 1)", B);
    if (N < 1 || N > RP_MAX_OBS_DIM) return fail(-33, "rp_append: observation width %d (1 ... %d are supported)", N, RP_MAX_OBS_DIM);
    if (A < 1 || A > RP_MAX_ACT_DIM) return fail(-34, "rp_append: action width %d (1 ... %d are supported)", A, RP_MAX_ACT_DIM);
    if (slab->rows < 1) return fail(-35, "rp_append: a slab of %ld rows (at least 1)", slab->rows);
    const long n = (long)T * B;
    if (const int rc = check_dst_rows(refusals, dst_host, n, slab->rows)) return rc;
    AppendArgs a = {};
    a.traj = block;
    a.actions = a.traj + (long)(T_cap + 1) * B * N;
    a.rewards = a.actions + (long)T_cap * B * A;
    a.steps = reinterpret_cast<const int*>(a.rewards + (long)T_cap * B);
    a.dst = dst;
    a.slab = *slab;
    a.T = T;
    a.B = B;
    a.N = N;
    a.A = A;
    a.vec_obs = N % 4 == 0 && aligned16(a.traj) && aligned16(slab->obs) && aligned16(slab->nxtobs);
    a.vec_act = A % 4 == 0 && aligned16(a.actions) && aligned16(slab->actions);
    hipLaunchKernelGGL(rp_append_kernel, dim3((unsigned)((n + WAVES - 1) / WAVES)), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    return launch_status(-40, "rp_append");
}

int rp_episode_returns(void* stream, const float* rewards, long slab_rows, const long* rows, long nrows, const long* offsets,
                       int E, float* returns)
{
    if (!rewards || !rows || !offsets || !returns) return fail(-50, "rp_episode_returns: NULL rewards, rows, offsets or returns");
    if (E < 1) return fail(-51, "rp_episode_returns: %d episodes (at least 1)", E);
    if (nrows < 1 || slab_rows < 1)
        return fail(-52, "rp_episode_returns: %ld rows of a slab of %ld (at least 1 each)", nrows, slab_rows);
    hipLaunchKernelGGL(rp_episode_returns_kernel, dim3((E + NT - 1) / NT), dim3(NT), 0, static_cast<hipStream_t>(stream), rewards,
                       slab_rows, rows, nrows, offsets, E, returns);
    return launch_status(-60, "rp_episode_returns");
}

long rpd_workspace_doubles(int obs_dim, long n, int groups)
{
    if (obs_dim < 1 || obs_dim > RP_MAX_OBS_DIM || n < 1 || groups < 0) return 0;
    const int G = delta_groups(n, groups);
    return (long)(G + delta_middle_rows(G)) * 2 * obs_dim;
}

int rpd_moments(void* stream, const float* obs, const float* nxtobs, long slab_rows, int obs_width, int sensor_start,
                     int sensor_stride, const float* obs_coef, const long* rows, long n, float delta, int groups,
                     double* workspace, double* sums, float* stats)
{
    if (!obs || !nxtobs || !workspace || !sums || !stats)
        return fail(-70, "rpd_moments: NULL obs, nxtobs, workspace, sums or stats");
    if (n < 1) return fail(-71, "rpd_moments: %ld rows (at least 1)", n);
    if (slab_rows < 1) return fail(-72, "rpd_moments: a slab of %ld rows (at least 1)", slab_rows);
    if (sensor_stride < 1) return fail(-73, "rpd_moments: sensor stride %d (at least 1)", sensor_stride);
    if (obs_width < 1 || sensor_start < 0 || sensor_start >= obs_width)
        return fail(-74, "rpd_moments: the sensor starts at column %d of %d", sensor_start, obs_width);
    const int obs_dim = width_of(obs_width, sensor_start, sensor_stride);
    if (obs_dim > RP_MAX_OBS_DIM)
        return fail(-75, "rpd_moments: %d observation columns (1 ... %d are supported)", obs_dim, RP_MAX_OBS_DIM);
    if (!(delta != 0.0f) || !std::isfinite(delta))
        return fail(-76, "rpd_moments: a step of %g to divide by (finite and not zero)", (double)delta);
    if (groups < 0) return fail(-77, "rpd_moments: %d workgroups (0 for the default, or at least 1)", groups);
    DeltaArgs a = {};
    a.obs = obs;
    a.nxtobs = nxtobs;
    a.coef = obs_coef;
    a.rows = rows;
    a.n = n;
    a.slab_rows = slab_rows;
    a.obs_width = obs_width;
    a.obs_dim = obs_dim;
    a.start = sensor_start;
    a.stride = sensor_stride;
    a.delta = delta;
    a.ws = workspace;
    const int G = delta_groups(n, groups);
    const dim3 grid(G, (obs_dim + TILE - 1) / TILE);
    // float4 puts four columns on a lane: worth it from 193 columns on, where a lane holds four either way; below, a
    // lane per column keeps the lanes busy (64 columns as float4 would leave 48 of 64 lanes idle through every division)
    const bool vec = obs_dim > 3 * WAVE && sensor_stride == 1 && obs_width % 4 == 0 && sensor_start % 4 == 0 && aligned16(obs) &&
                     aligned16(nxtobs) && aligned16(obs_coef);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec)
        hipLaunchKernelGGL(rpd_moments_kernel<true>, grid, dim3(NT), 0, s, a);
    else
        hipLaunchKernelGGL(rpd_moments_kernel<false>, grid, dim3(NT), 0, s, a);
    const int rc = launch_status(-80, "rpd_moments");
    if (rc != 0) return rc;
    const double* partials = workspace;
    int left = G;
    if (const int M = delta_middle_rows(G)) {
        double* middle = workspace + (long)G * 2 * obs_dim;
        hipLaunchKernelGGL(rpd_middle_kernel, dim3(M, (obs_dim + NT - 1) / NT), dim3(NT), 0, s, workspace, G, obs_dim, middle);
        partials = middle;
        left = M;
    }
    hipLaunchKernelGGL(rpd_fold_kernel, dim3(1), dim3(NT), 0, s, partials, left, obs_dim, n, sums, stats);
    return launch_status(-80, "rpd_moments");
}

long rpn_workspace_doubles(int N, int A, int forced, long n, int groups)
{
    if (N < 1 || N > RP_MAX_OBS_DIM || A < 1 || A > RP_MAX_ACT_DIM || n < 1 || groups < 0) return 0;
    const int G = delta_groups(n, groups);
    return (long)(G + delta_middle_rows(G)) * 2 * (N + A + (forced ? N : 0));
}

int rpn_moments(void* stream, const float* obs, const float* actions, long slab_rows, int N, int A, const float* F,
                const long* rows, long n, int groups, double* workspace, double* sums, float* stats)
{
    if (!obs || !actions || !workspace || !sums || !stats)
        return fail(-90, "rpn_moments: NULL obs, actions, workspace, sums or stats");
    if (n < 1) return fail(-91, "rpn_moments: %ld rows (at least 1)", n);
    if (slab_rows < 1) return fail(-92, "rpn_moments: a slab of %ld rows (at least 1)", slab_rows);
    if (N < 1 || N > RP_MAX_OBS_DIM) return fail(-93, "rpn_moments: observation width %d (1 ... %d are supported)", N, RP_MAX_OBS_DIM);
    if (A < 1 || A > RP_MAX_ACT_DIM) return fail(-94, "rpn_moments: action width %d (1 ... %d are supported)", A, RP_MAX_ACT_DIM);
    if (groups < 0) return fail(-95, "rpn_moments: %d workgroups (0 for the default, or at least 1)", groups);
    FitArgs a = {};
    a.obs = obs;
    a.actions = actions;
    a.F = F;
    a.rows = rows;
    a.n = n;
    a.slab_rows = slab_rows;
    a.N = N;
    a.A = A;
    a.W = N + A + (F ? N : 0);
    a.ws = workspace;
    const int G = delta_groups(n, groups);
    const dim3 grid(G, (N + TILE - 1) / TILE);
    // float4 under rpd_moments' conditions: from 193 columns on, every row and the forcing matrix 16-byte aligned
    const bool vec = N > 3 * WAVE && N % 4 == 0 && aligned16(obs) && aligned16(F);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec)
        hipLaunchKernelGGL(rpn_moments_kernel<true>, grid, dim3(NT), 0, s, a);
    else
        hipLaunchKernelGGL(rpn_moments_kernel<false>, grid, dim3(NT), 0, s, a);
    const int rc = launch_status(-100, "rpn_moments");
    if (rc != 0) return rc;
    const double* partials = workspace;
    int left = G;
    if (const int M = delta_middle_rows(G)) {
        double* middle = workspace + (long)G * 2 * a.W;
        hipLaunchKernelGGL(rpd_middle_kernel, dim3(M, (a.W + NT - 1) / NT), dim3(NT), 0, s, workspace, G, a.W, middle);
        partials = middle;
        left = M;
    }
    hipLaunchKernelGGL(rpn_fold_kernel, dim3(1), dim3(NT), 0, s, partials, left, N, A, F ? 1 : 0, n, sums, stats);
    return launch_status(-100, "rpn_moments");
}

const char* rp_last_error(void) { return g_err; }

}  // extern "C"
