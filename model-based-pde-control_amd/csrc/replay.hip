// replay.hip -- the fused batch gather of the policy-update phase (C ABI: include/replay_hip.h; binding:
// pdecontrol/mbrl/replay_hip.py).
//
// One launch assembles one SAC batch from several packed replays.  A wave owns a sample: it reads the sample's row in the
// concatenated row space, finds the source by comparing against the (at most RP_MAX_SOURCES) first rows -- the sources
// travel in the kernel arguments, so the search is a handful of wave-uniform selects on constant indices -- and copies the
// row with lanes along the columns: obs and nxtobs through the sensor and the observation coefficients, actions through
// the action coefficients, reward and terminated flag by lane 0.  float4 where the source allows it (see `vec` below).
//
// The affine map is four separately rounded fp32 operations (__fsub_rn, __fdiv_rn, __fmul_rn, __fadd_rn; the file is also
// built with -ffp-contract=off), the operations of ScaleTransform._affine, so the batch equals the host loader's bit for
// bit.  Plain vector stores only; nothing is stored through the scalar unit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/replay_hip.h"
#include "capi_error.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int WAVE = 64;
constexpr int WAVES = 4;               // samples per workgroup
constexpr int NT = WAVE * WAVES;

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

__device__ __forceinline__ float affine(float v, float a, float ba, float dc, float c)
{
    return __fadd_rn(__fmul_rn(__fdiv_rn(__fsub_rn(v, a), ba), dc), c);
}

// n output columns of one row: out[j] = affine(in[start + j * stride]); coef is [4][n] or NULL
__device__ __forceinline__ void copy_row(const float* __restrict__ in, const float* __restrict__ coef, float* __restrict__ out,
                                         int n, int start, int stride, int lane)
{
    for (int j = lane; j < n; j += WAVE) {
        float v = in[start + (long)j * stride];
        if (coef) v = affine(v, coef[j], coef[n + j], coef[2 * n + j], coef[3 * n + j]);
        out[j] = v;
    }
}

// the same for stride 1 with every address a multiple of 16 bytes and n a multiple of 4
__device__ __forceinline__ void copy_row4(const float* __restrict__ in, const float* __restrict__ coef, float* __restrict__ out,
                                          int n, int start, int lane)
{
    for (int j = 4 * lane; j < n; j += 4 * WAVE) {
        f4 v = *reinterpret_cast<const f4*>(in + start + j);
        if (coef) {
            const f4 a = *reinterpret_cast<const f4*>(coef + j);
            const f4 ba = *reinterpret_cast<const f4*>(coef + n + j);
            const f4 dc = *reinterpret_cast<const f4*>(coef + 2 * n + j);
            const f4 c = *reinterpret_cast<const f4*>(coef + 3 * n + j);
            v.x = affine(v.x, a.x, ba.x, dc.x, c.x);
            v.y = affine(v.y, a.y, ba.y, dc.y, c.y);
            v.z = affine(v.z, a.z, ba.z, dc.z, c.z);
            v.w = affine(v.w, a.w, ba.w, dc.w, c.w);
        }
        *reinterpret_cast<f4*>(out + j) = v;
    }
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

int obs_dim_of(const rp_source& s)
{
    return (s.obs_width - s.sensor_start + s.sensor_stride - 1) / s.sensor_stride;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

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

const char* rp_last_error(void) { return g_err; }

}  // extern "C"
