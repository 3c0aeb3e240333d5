// replay.hip -- the fused batch gather of the policy-update phase, and the append and episode returns of the
// device-resident replay (C ABI: include/replay_hip.h; binding: pdecontrol/mbrl/replay_hip.py).
//
// One launch assembles one SAC batch from several packed replays.  A wave owns a sample: it reads the sample's row in the
// concatenated row space, finds the source by comparing against the (at most RP_MAX_SOURCES) first rows -- the sources
// travel in the kernel arguments, so the search is a handful of wave-uniform selects on constant indices -- and copies the
// row with lanes along the columns: obs and nxtobs through the sensor and the observation coefficients, actions through
// the action coefficients, reward and terminated flag by lane 0.  float4 where the source allows it (see `vec` below).
//
// The affine map is row_ops.h's, so the batch equals the host loader's bit for bit.  Plain vector stores only; nothing is
// stored through the scalar unit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/replay_hip.h"
#include "capi_error.h"
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

__device__ __forceinline__ void place_row(const float* __restrict__ in, float* __restrict__ out, int n, bool vec, int lane)
{
    if (vec) {
        for (int j = 4 * lane; j < n; j += 4 * WAVE) *reinterpret_cast<f4*>(out + j) = *reinterpret_cast<const f4*>(in + j);
    } else {
        for (int j = lane; j < n; j += WAVE) out[j] = in[j];
    }
}

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
    if (!slab->obs || !slab->actions || !slab->nxtobs || !slab->rewards || !slab->terminated || !slab->truncated || !slab->steps)
        return fail(-30, "rp_append: the slab has a NULL field pointer");
    if (T < 1 || T > T_cap) return fail(-31, "rp_append: %d steps of a block laid out for %d (1 ... %d)", T, T_cap, T_cap);
    if (B < 1) return fail(-32, "rp_append: %d envs (at least 1)", B);
    if (N < 1 || N > RP_MAX_OBS_DIM) return fail(-33, "rp_append: observation width %d (1 ... %d are supported)", N, RP_MAX_OBS_DIM);
    if (A < 1 || A > RP_MAX_ACT_DIM) return fail(-34, "rp_append: action width %d (1 ... %d are supported)", A, RP_MAX_ACT_DIM);
    if (slab->rows < 1) return fail(-35, "rp_append: a slab of %ld rows (at least 1)", slab->rows);
    const long n = (long)T * B;
    std::vector<bool> seen(static_cast<size_t>(slab->rows), false);
    for (long i = 0; i < n; ++i) {
        const long r = dst_host[i];
        if (r < 0) continue;
        if (r >= slab->rows) return fail(-36, "rp_append: dst[%ld] = %ld is beyond the slab's %ld rows", i, r, slab->rows);
        if (seen[r]) return fail(-37, "rp_append: row %ld is named twice (again at dst[%ld])", r, i);
        seen[r] = true;
    }
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

const char* rp_last_error(void) { return g_err; }

}  // extern "C"
