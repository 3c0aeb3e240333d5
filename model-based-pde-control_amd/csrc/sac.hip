// sac.hip -- gfx950 kernels of the soft actor-critic agent (C ABI: include/sac_hip.h; binding: pdecontrol/sac/sac_hip.py).
//
// fp32 throughout.  The 256-wide layers run on v_mfma_f32_16x16x4_f32 (exact fp32: an fmaf chain in k order), four
// independent accumulators per wave.  A workgroup of four waves owns a tile of 16 samples whose activations stay in LDS;
// weights are streamed from L2 (all networks of the agent are about 1.5 MB).  The narrow heads (1 and act_dim <= 16
// outputs) are plain VALU dot products.
//
//   tile_linear   out[s][n] = act(b[n] + sum_k in[s][k] W[n][k]):  M = sample, N = unit, each lane group g = lane >> 4
//                 takes k = 16 kk + 4 g + j in step j of a 16-wide k block, so that both operands are read as float4 along
//                 k (the k order inside a block is a permutation; both operands use the same one).
//   tile_dgrad    out[s][k] = [act[s][k] > 0] sum_n dy[s][n] W[n][k]:  the same with the weight read down its columns.
//   sac_wgrad     dW[n][k] = sum_b dY[b][n] X[b][k] with M = n, N = k and the batch as the reduction: a wave owns a
//                 16 x 16 tile of one layer's dW (the bias is column K, its X is 1), walks the samples in order and applies
//                 Adam (and the target's Polyak average) to its tile, or stores the gradient (sac_grads).
//
// No float atomics anywhere; no kernel stores through the scalar unit.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/sac_hip.h"
#include "capi_error.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int HID = 256;      // hidden width
constexpr int TB = 16;        // samples per tile
constexpr int LDH = HID + 4;  // LDS row stride of a hidden activation tile
constexpr int LDX = 276;      // LDS row stride of an input tile: (256 + 16) + 4
constexpr int NT = 256;       // threads per workgroup
constexpr int SMALL = 1280;   // floats of per-tile scalars behind the activation tiles

struct PolicyP { const float *w1, *b1, *w2, *b2, *wm, *bm, *ws, *bs; };
struct QP { const float *w1, *b1, *w2, *b2, *w3, *b3; };

// ---------------------------------------------------------------------------------------------------------------------
// tile building blocks (all 256 threads call them; the caller synchronises between stages)
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void tile_linear(const float* in, int ldi, int K, const float* __restrict__ W,
                                            const float* __restrict__ bias, float* out, int ldo, bool relu)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    f4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (f4){0.f, 0.f, 0.f, 0.f};
    const int Kp = (K + 15) & ~15;
    const int Kv = (K & 3) == 0 ? (K & ~63) : 0;   // the part read as aligned float4 without guards, 64 wide steps
    const float* wrow[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) wrow[t] = W + (size_t)(64 * wave + 16 * t + r) * K;
    // branch-free bodies with a constant inner trip count: the sixteen float4 loads of a 64-wide step are in flight
    // before the first MFMA waits for one
    for (int k1 = 0; k1 < Kv; k1 += 64) {
        f4 a[4], b[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k1 + 16 * u + 4 * g;
            a[u] = *reinterpret_cast<const f4*>(in + r * ldi + k);
#pragma unroll
            for (int t = 0; t < 4; ++t) b[u][t] = *reinterpret_cast<const f4*>(wrow[t] + k);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][j], b[u][t][j], acc[t], 0, 0, 0);
    }
    for (int k0 = Kv; k0 < Kp; k0 += 16) {
        const int k = k0 + 4 * g;
        const f4 a = *reinterpret_cast<const f4*>(in + r * ldi + k);   // rows are zero-padded to Kp
        f4 b[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float w = wrow[t][min(k + j, K - 1)];              // clamped address, value masked
                b[t][j] = (k + j < K) ? w : 0.f;
            }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[t][j], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int n = 64 * wave + 16 * t + r;
        const float bv = bias[n];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float v = acc[t][q] + bv;
            if (relu) v = fmaxf(v, 0.f);
            out[(4 * g + q) * ldo + n] = v;
        }
    }
}

// out[s][k] = [act[s][k] > 0] * sum_n dy[s][n] W[n][k];  W is [256][256]
__device__ __forceinline__ void tile_dgrad(const float* dy, const float* __restrict__ W, const float* act, float* out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    f4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int n0 = 0; n0 < HID; n0 += 16) {
        const int n = n0 + 4 * g;
        const f4 a = *reinterpret_cast<const f4*>(dy + r * LDH + n);
        float b[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) b[t][j] = W[(size_t)(n + j) * HID + 64 * wave + 16 * t + r];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[t][j], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int k = 64 * wave + 16 * t + r;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int s = 4 * g + q;
            out[s * LDH + k] = act[s * LDH + k] > 0.f ? acc[t][q] : 0.f;
        }
    }
}

// q[s] = b3 + sum_k h[s][k] w3[k]: wave w takes samples 4w ... 4w+3
__device__ __forceinline__ void tile_qhead(const float* h, const float* __restrict__ w3, const float* __restrict__ b3, float* q)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int ss = 0; ss < 4; ++ss) {
        const int s = 4 * wave + ss;
        float v = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) v = fmaf(h[s * LDH + lane + 64 * c], w3[lane + 64 * c], v);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) q[s] = v + b3[0];
    }
}

// X[s][col0 + c] = src[s0 + s][c] (zero for samples past B)
__device__ __forceinline__ void load_tile(float* X, const float* __restrict__ src, int ncols, int col0, int s0, int B)
{
    for (int i = threadIdx.x; i < TB * ncols; i += NT) {
        const int s = i / ncols, c = i - s * ncols;
        X[s * LDX + col0 + c] = (s0 + s < B) ? src[(size_t)(s0 + s) * ncols + c] : 0.f;
    }
}

__device__ __forceinline__ void store_tile(float* __restrict__ dst, const float* T, int s0, int B)
{
    for (int i = threadIdx.x; i < TB * HID; i += NT) {
        const int s = i >> 8, c = i & 255;
        if (s0 + s < B) dst[(size_t)(s0 + s) * HID + c] = T[s * LDH + c];
    }
}

struct Head { float mean, lsraw, stdv, eps, y, om, sc, action, logp; };   // om = 1 - y^2

// the tanh-Gaussian head of sample s = t >> 4, action component j = t & 15 (j < A) from the second hidden tile h
__device__ __forceinline__ Head policy_head(const PolicyP& P, const float* h, int A, int s, int j, bool ok, const float* noise,
                                            size_t row, const float* scale, const float* bias)
{
    Head o;
    float m = P.bm[j], l = P.bs[j];
    const float* wm = P.wm + j * HID;
    const float* ws = P.ws + j * HID;
#pragma unroll 8
    for (int k = 0; k < HID; k += 4) {
        const f4 hv = *reinterpret_cast<const f4*>(h + s * LDH + k);
        const f4 a = *reinterpret_cast<const f4*>(wm + k);
        const f4 b = *reinterpret_cast<const f4*>(ws + k);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            m = fmaf(hv[c], a[c], m);
            l = fmaf(hv[c], b[c], l);
        }
    }
    o.mean = m;
    o.lsraw = l;
    const float ls = fminf(fmaxf(l, -20.f), 2.f);
    o.stdv = expf(ls);
    o.eps = (ok && noise != nullptr) ? noise[row * A + j] : 0.f;
    const float x = fmaf(o.stdv, o.eps, m);
    // tanh and 1 - tanh^2 = sech^2 from e = exp(-2|x|): 1 - y * y would cancel where the policy saturates, and the
    // log-probability takes its logarithm
    const float e = expf(-2.f * fabsf(x)), d = 1.f / (1.f + e);
    o.y = copysignf((1.f - e) * d, x);
    o.om = 4.f * e * d * d;
    o.sc = scale[j];
    o.action = fmaf(o.y, o.sc, bias[j]);
    o.logp = -0.5f * o.eps * o.eps - ls - 0.91893853320467274f - logf(o.sc * o.om + 1e-6f);
    return o;
}

// ---------------------------------------------------------------------------------------------------------------------
// launch 0: the policy alone (SAC.act)
// ---------------------------------------------------------------------------------------------------------------------
struct FArgs {
    PolicyP P;
    int O, A, B;
    const float *obs, *noise, *scale, *bias;
    float *action, *logp, *mean_action;
};

__global__ void __launch_bounds__(NT) sac_policy_fwd(FArgs a)
{
    extern __shared__ __align__(16) float lds[];
    float* X = lds;
    float* A1 = X + TB * LDX;
    float* A2 = A1 + TB * LDH;
    float* sm = A2 + TB * LDH;
    const int t = threadIdx.x, s0 = blockIdx.x * TB;
    for (int i = t; i < TB * LDX; i += NT) X[i] = 0.f;
    __syncthreads();
    load_tile(X, a.obs, a.O, 0, s0, a.B);
    __syncthreads();
    tile_linear(X, LDX, a.O, a.P.w1, a.P.b1, A1, LDH, true);
    __syncthreads();
    tile_linear(A1, LDH, HID, a.P.w2, a.P.b2, A2, LDH, true);
    __syncthreads();
    const int s = t >> 4, j = t & 15;
    const bool ok = s0 + s < a.B;
    float lp = 0.f;
    if (j < a.A) {
        const Head h = policy_head(a.P, A2, a.A, s, j, ok, a.noise, (size_t)(s0 + s), a.scale, a.bias);
        lp = h.logp;
        if (ok) {
            a.action[(size_t)(s0 + s) * a.A + j] = h.action;
            if (a.mean_action) a.mean_action[(size_t)(s0 + s) * a.A + j] = fmaf(tanhf(h.mean), h.sc, a.bias[j]);
        }
    }
    sm[t] = lp;
    __syncthreads();
    if (t < TB && s0 + t < a.B && a.logp) {
        float v = 0.f;
        for (int c = 0; c < a.A; ++c) v += sm[t * 16 + c];
        a.logp[s0 + t] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// launch 1: critic pass
// ---------------------------------------------------------------------------------------------------------------------
struct CArgs {
    PolicyP P;
    QP T[2], C[2];
    int O, A, B;
    float gamma;
    const float* alpha;
    const float *obs, *actions, *nxtobs, *rewards, *terminated, *noise, *scale, *bias;
    float *xu, *h1, *h2, *dh1, *dh2, *dq, *sq;   // h*, dh*: [2][B][256]; dq, sq: [2][B]
};

__global__ void __launch_bounds__(NT) sac_critic_pass(CArgs a)
{
    extern __shared__ __align__(16) float lds[];
    float* X = lds;
    float* A1 = X + TB * LDX;
    float* A2 = A1 + TB * LDH;
    float* A3 = A2 + TB * LDH;
    float* A4 = A3 + TB * LDH;
    float* sm = A4 + TB * LDH;
    float *lp = sm, *q = sm + 256, *yv = sm + 288, *dqs = sm + 304, *logp = sm + 320;
    const int t = threadIdx.x, s0 = blockIdx.x * TB, O = a.O, A = a.A, D = O + A, B = a.B;
    const float alpha = a.alpha[0];

    for (int i = t; i < TB * LDX; i += NT) X[i] = 0.f;
    __syncthreads();
    load_tile(X, a.nxtobs, O, 0, s0, B);
    __syncthreads();
    tile_linear(X, LDX, O, a.P.w1, a.P.b1, A1, LDH, true);
    __syncthreads();
    tile_linear(A1, LDH, HID, a.P.w2, a.P.b2, A2, LDH, true);
    __syncthreads();
    {
        const int s = t >> 4, j = t & 15;
        float v = 0.f;
        if (j < A) {
            const Head h = policy_head(a.P, A2, A, s, j, s0 + s < B, a.noise, (size_t)(s0 + s), a.scale, a.bias);
            X[s * LDX + O + j] = h.action;
            v = h.logp;
        }
        lp[t] = v;
    }
    __syncthreads();
    if (t < TB) {
        float v = 0.f;
        for (int c = 0; c < A; ++c) v += lp[t * 16 + c];
        logp[t] = v;
    }
    for (int i = 0; i < 2; ++i) {
        tile_linear(X, LDX, D, a.T[i].w1, a.T[i].b1, A1, LDH, true);
        __syncthreads();
        tile_linear(A1, LDH, HID, a.T[i].w2, a.T[i].b2, A2, LDH, true);
        __syncthreads();
        tile_qhead(A2, a.T[i].w3, a.T[i].b3, q + 16 * i);
        __syncthreads();
    }
    if (t < TB) {
        const bool ok = s0 + t < B;
        const float r = ok ? a.rewards[s0 + t] : 0.f, term = ok ? a.terminated[s0 + t] : 0.f;
        yv[t] = r + (1.f - term) * a.gamma * (fminf(q[t], q[16 + t]) - alpha * logp[t]);
    }
    __syncthreads();
    load_tile(X, a.obs, O, 0, s0, B);
    load_tile(X, a.actions, A, O, s0, B);
    __syncthreads();
    for (int i = t; i < TB * D; i += NT) {
        const int s = i / D, c = i - s * D;
        if (s0 + s < B) a.xu[(size_t)(s0 + s) * D + c] = X[s * LDX + c];
    }
    const float inv = 2.f / (float)B;
    for (int i = 0; i < 2; ++i) {
        tile_linear(X, LDX, D, a.C[i].w1, a.C[i].b1, A1, LDH, true);
        __syncthreads();
        tile_linear(A1, LDH, HID, a.C[i].w2, a.C[i].b2, A2, LDH, true);
        __syncthreads();
        tile_qhead(A2, a.C[i].w3, a.C[i].b3, q + 16 * i);
        __syncthreads();
        if (t < TB) {
            const bool ok = s0 + t < B;
            const float d = q[16 * i + t] - yv[t];
            dqs[t] = ok ? d * inv : 0.f;
            if (ok) {
                a.dq[(size_t)i * B + s0 + t] = d * inv;
                a.sq[(size_t)i * B + s0 + t] = d * d;
            }
        }
        __syncthreads();
        for (int e = t; e < TB * HID; e += NT) {
            const int s = e >> 8, n = e & 255;
            A3[s * LDH + n] = A2[s * LDH + n] > 0.f ? dqs[s] * a.C[i].w3[n] : 0.f;
        }
        __syncthreads();
        tile_dgrad(A3, a.C[i].w2, A1, A4);
        __syncthreads();
        const size_t off = (size_t)i * B * HID;
        store_tile(a.h1 + off, A1, s0, B);
        store_tile(a.h2 + off, A2, s0, B);
        store_tile(a.dh2 + off, A3, s0, B);
        store_tile(a.dh1 + off, A4, s0, B);
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// launch 3: policy pass
// ---------------------------------------------------------------------------------------------------------------------
struct PArgs {
    PolicyP P;
    QP C[2];
    int O, A, B;
    const float* alpha;
    const float *obs, *noise, *scale, *bias;
    float *h1, *h2, *dh1, *dh2, *dmean, *dls, *logpi, *minq;   // h*, dh*: [B][256]; dmean, dls: [B][A]
};

__global__ void __launch_bounds__(NT) sac_policy_pass(PArgs a)
{
    extern __shared__ __align__(16) float lds[];
    float* X = lds;
    float* A1 = X + TB * LDX;
    float* A2 = A1 + TB * LDH;
    float* A3 = A2 + TB * LDH;
    float* A4 = A3 + TB * LDH;
    float* A5 = A4 + TB * LDH;
    float* sm = A5 + TB * LDH;
    float *lp = sm, *q = sm + 256, *gu = sm + 288, *dm = lp, *dl = sm + 800;   // gu: [2][256]; dm reuses lp
    const int t = threadIdx.x, s0 = blockIdx.x * TB, O = a.O, A = a.A, D = O + A, B = a.B;
    const int s = t >> 4, j = t & 15;
    const bool ok = s0 + s < B;
    const float alpha = a.alpha[0], invB = 1.f / (float)B;

    for (int i = t; i < TB * LDX; i += NT) X[i] = 0.f;
    __syncthreads();
    load_tile(X, a.obs, O, 0, s0, B);
    __syncthreads();
    tile_linear(X, LDX, O, a.P.w1, a.P.b1, A1, LDH, true);
    __syncthreads();
    tile_linear(A1, LDH, HID, a.P.w2, a.P.b2, A2, LDH, true);
    __syncthreads();
    Head h = {};
    if (j < A) {
        h = policy_head(a.P, A2, A, s, j, ok, a.noise, (size_t)(s0 + s), a.scale, a.bias);
        X[s * LDX + O + j] = h.action;
    }
    lp[t] = h.logp;
    store_tile(a.h1, A1, s0, B);
    store_tile(a.h2, A2, s0, B);
    __syncthreads();
    if (t < TB && s0 + t < B) {
        float v = 0.f;
        for (int c = 0; c < A; ++c) v += lp[t * 16 + c];
        a.logpi[s0 + t] = v;
    }
    // both critic heads forward, and backward with a unit output gradient down to the action columns of the input
    for (int i = 0; i < 2; ++i) {
        tile_linear(X, LDX, D, a.C[i].w1, a.C[i].b1, A3, LDH, true);
        __syncthreads();
        tile_linear(A3, LDH, HID, a.C[i].w2, a.C[i].b2, A4, LDH, true);
        __syncthreads();
        tile_qhead(A4, a.C[i].w3, a.C[i].b3, q + 16 * i);
        __syncthreads();
        for (int e = t; e < TB * HID; e += NT) {
            const int ss = e >> 8, n = e & 255;
            A4[ss * LDH + n] = A4[ss * LDH + n] > 0.f ? a.C[i].w3[n] : 0.f;
        }
        __syncthreads();
        tile_dgrad(A4, a.C[i].w2, A3, A5);
        __syncthreads();
        float v = 0.f;
        if (j < A) {
            const float* w = a.C[i].w1 + O + j;
#pragma unroll 16
            for (int n = 0; n < HID; ++n) v = fmaf(A5[s * LDH + n], w[(size_t)n * D], v);
        }
        gu[256 * i + t] = v;
        __syncthreads();
    }
    {
        float dmean = 0.f, dls = 0.f;
        if (j < A && ok) {
            const float gpi = -invB * (q[s] <= q[16 + s] ? gu[t] : gu[256 + t]);
            const float om = h.om, u = h.sc * om + 1e-6f;
            const float dx = alpha * invB * (2.f * h.sc * h.y * om / u) + gpi * h.sc * om;
            dmean = dx;
            dls = (h.lsraw >= -20.f && h.lsraw <= 2.f) ? dx * h.stdv * h.eps - alpha * invB : 0.f;
            a.dmean[(size_t)(s0 + s) * A + j] = dmean;
            a.dls[(size_t)(s0 + s) * A + j] = dls;
        }
        dm[t] = dmean;   // (lp was consumed before the critic loop's first barrier)
        dl[t] = dls;
        if (t < TB && s0 + t < B) a.minq[s0 + t] = fminf(q[t], q[16 + t]);
    }
    __syncthreads();
    {
        float acc[TB];
#pragma unroll
        for (int ss = 0; ss < TB; ++ss) acc[ss] = 0.f;
        for (int c = 0; c < A; ++c) {
            const float wm = a.P.wm[c * HID + t], ws = a.P.ws[c * HID + t];
#pragma unroll
            for (int ss = 0; ss < TB; ++ss) acc[ss] = fmaf(dm[ss * 16 + c], wm, fmaf(dl[ss * 16 + c], ws, acc[ss]));
        }
#pragma unroll
        for (int ss = 0; ss < TB; ++ss) A3[ss * LDH + t] = A2[ss * LDH + t] > 0.f ? acc[ss] : 0.f;
    }
    __syncthreads();
    tile_dgrad(A3, a.P.w2, A1, A4);
    __syncthreads();
    store_tile(a.dh2, A3, s0, B);
    store_tile(a.dh1, A4, s0, B);
}

// ---------------------------------------------------------------------------------------------------------------------
// launches 2 and 4: weight gradients, Adam, Polyak
// ---------------------------------------------------------------------------------------------------------------------
constexpr int MAXJOBS = 6;

struct WJob {
    const float* dY;
    const float* X;
    float *W, *b, *mW, *mb, *vW, *vb, *tW, *tb, *gW, *gb;
    int ldy, ldx, N, K, strip0, kstrips;
};

struct WArgs {
    WJob job[MAXJOBS];
    int njobs, nstrips, B, grads_only, step_idx, interval;
    float lr, beta1, beta2, eps, tau;
    const int* counters;
};

__global__ void __launch_bounds__(NT) sac_wgrad(WArgs a)
{
    const int strip = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (strip >= a.nstrips) return;
    int ji = 0;
    for (int c = 1; c < a.njobs; ++c)
        if (strip >= a.job[c].strip0) ji = c;
    const WJob& J = a.job[ji];
    const int local = strip - J.strip0, n0 = (local / J.kstrips) * 16, kbase = (local % J.kstrips) * 16;
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const int N = J.N, K = J.K, B = a.B;
    // two accumulators (even and odd groups of four samples) keep the dependent MFMA chain off the critical path
    f4 acc0 = (f4){0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
    const bool n_ok = n0 + r < N;
    const int kcol = kbase + r;
    const bool k_ok = kcol < K;
    const float kone = kcol == K ? 1.f : 0.f;     // the bias column
    const float* dy = J.dY + min(n0 + r, N - 1);
    const float* x = J.X + min(kcol, K - 1);
    // clamped addresses and masked values keep the body branch-free; 64 loads of 128 samples are in flight at once (the
    // activations were written by other compute units: every load is a trip past this unit's L2 slice)
    constexpr int UN = 32;
    for (int b1 = 0; b1 < B; b1 += 4 * UN) {
        float av[UN], bv[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int bq = b1 + 4 * u + g, bb = min(bq, B - 1);
            const bool ok = bq < B;
            const float ar = dy[(size_t)bb * J.ldy], xr = x[(size_t)bb * J.ldx];
            av[u] = (ok && n_ok) ? ar : 0.f;
            bv[u] = !ok ? 0.f : (k_ok ? xr : kone);
        }
#pragma unroll
        for (int u = 0; u < UN; u += 2) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u + 1], bv[u + 1], acc1, 0, 0, 0);
        }
    }
    const f4 acc = acc0 + acc1;
    // Adam in torch.optim.Adam's form: step_size = lr / bc1, denom = sqrt(v) / sqrt(bc2) + eps, p -= step_size * m / denom
    const int step = a.counters[a.step_idx] + 1;
    const float step_size = (float)((double)a.lr / (1.0 - pow((double)a.beta1, (double)step)));
    const float bc2_sqrt = (float)sqrt(1.0 - pow((double)a.beta2, (double)step));
    const bool polyak = J.tW != nullptr && (a.counters[3] % a.interval) == 0;
    {
        const int k = kcol;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = n0 + 4 * g + q;
            if (n >= N || k > K) continue;
            const bool is_b = k == K;
            const size_t idx = is_b ? (size_t)n : (size_t)n * K + k;
            const float gr = acc[q];
            if (a.grads_only) {
                (is_b ? J.gb : J.gW)[idx] = gr;
                continue;
            }
            float* p = is_b ? J.b : J.W;
            float* m = is_b ? J.mb : J.mW;
            float* v = is_b ? J.vb : J.vW;
            const float m1 = m[idx] + (gr - m[idx]) * (1.f - a.beta1);
            const float v1 = v[idx] * a.beta2 + (1.f - a.beta2) * gr * gr;
            const float p1 = p[idx] - step_size * (m1 / (sqrtf(v1) / bc2_sqrt + a.eps));
            m[idx] = m1;
            v[idx] = v1;
            p[idx] = p1;
            if (polyak) {
                float* tp = is_b ? J.tb : J.tW;
                tp[idx] = tp[idx] * (1.f - a.tau) + p1 * a.tau;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// launch 5: statistics, log_alpha, counters
// ---------------------------------------------------------------------------------------------------------------------
struct ZArgs {
    const float *sq, *logpi, *minq, *rewards, *terminated;
    int B, auto_alpha, grads_only;
    float target_entropy, lr, beta1, beta2, eps;
    float *log_alpha, *log_alpha_m, *log_alpha_v, *alpha, *stats, *g_log_alpha;
    int* counters;
};

__device__ __forceinline__ float block_sum(const float* x, int n, float* red)
{
    float v = 0.f;
    for (int i = threadIdx.x; i < n; i += NT) v += x[i];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const float out = red[0];
    __syncthreads();
    return out;
}

__global__ void __launch_bounds__(NT) sac_finalize(ZArgs a)
{
    __shared__ float red[NT];
    const int B = a.B;
    const float invB = 1.f / (float)B;
    const float sq1 = block_sum(a.sq, B, red), sq2 = block_sum(a.sq + B, B, red);
    const float slp = block_sum(a.logpi, B, red), smq = block_sum(a.minq, B, red);
    const float srw = block_sum(a.rewards, B, red), stm = block_sum(a.terminated, B, red);
    if (threadIdx.x != 0) return;
    const float alpha = a.alpha[0];
    float alpha_loss = 0.f, alpha_out = alpha;
    if (a.auto_alpha) {
        const float la = a.log_alpha[0], mean_lp = slp * invB + a.target_entropy;
        const float gr = -mean_lp;
        alpha_loss = -(la * mean_lp);
        if (a.grads_only) {
            if (a.g_log_alpha) a.g_log_alpha[0] = gr;
        } else {
            const int step = a.counters[2] + 1;
            const float step_size = (float)((double)a.lr / (1.0 - pow((double)a.beta1, (double)step)));
            const float bc2_sqrt = (float)sqrt(1.0 - pow((double)a.beta2, (double)step));
            const float m1 = a.log_alpha_m[0] + (gr - a.log_alpha_m[0]) * (1.f - a.beta1);
            const float v1 = a.log_alpha_v[0] * a.beta2 + (1.f - a.beta2) * gr * gr;
            const float la1 = la - step_size * (m1 / (sqrtf(v1) / bc2_sqrt + a.eps));
            a.log_alpha_m[0] = m1;
            a.log_alpha_v[0] = v1;
            a.log_alpha[0] = la1;
            alpha_out = expf(la1);
            a.alpha[0] = alpha_out;
            a.counters[2] = step;
        }
    }
    a.stats[0] = sq1 * invB + sq2 * invB;
    a.stats[1] = (alpha * slp - smq) * invB;
    a.stats[2] = alpha_loss;
    a.stats[3] = alpha_out;
    a.stats[4] = srw * invB;
    a.stats[5] = stm;
    if (!a.grads_only) {
        a.counters[0] += 1;
        a.counters[1] += 1;
        a.counters[3] += 1;
        a.counters[4] += (int)stm;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
PolicyP policy_of(const sac_state* st)
{
    float* const* p = st->policy;
    return PolicyP{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]};
}

QP head_of(float* const* p, int i) { return QP{p[6 * i], p[6 * i + 1], p[6 * i + 2], p[6 * i + 3], p[6 * i + 4], p[6 * i + 5]}; }

template <typename K, typename Args>
int launch(K kernel, const char* name, int grid, size_t lds, hipStream_t stream, const Args& args)
{
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(NT), lds, stream, args);
    return launch_status(-20, name);
}

bool any_null(float* const* p, int n)
{
    for (int i = 0; i < n; ++i)
        if (p[i] == nullptr) return true;
    return false;
}

bool misaligned(float* const* p, int n)
{
    for (int i = 0; i < n; ++i)
        if (((uintptr_t)p[i] & 15) != 0 && (i & 1) == 0) return true;   // weights are read as float4
    return false;
}

struct Work {
    float *xu, *c_h1, *c_h2, *c_dh1, *c_dh2, *c_dq, *c_sq, *p_h1, *p_h2, *p_dh1, *p_dh2, *dmean, *dls, *logpi, *minq;
    long total;
};

Work carve(float* base, int O, int A, int B)
{
    Work w;
    long at = 0;
    auto take = [&](long n) { float* p = base ? base + at : nullptr; at += (n + 3) & ~3L; return p; };
    const long BH = (long)B * HID;
    w.xu = take((long)B * (O + A));
    w.c_h1 = take(2 * BH);
    w.c_h2 = take(2 * BH);
    w.c_dh1 = take(2 * BH);
    w.c_dh2 = take(2 * BH);
    w.c_dq = take(2L * B);
    w.c_sq = take(2L * B);
    w.p_h1 = take(BH);
    w.p_h2 = take(BH);
    w.p_dh1 = take(BH);
    w.p_dh2 = take(BH);
    w.dmean = take((long)B * A);
    w.dls = take((long)B * A);
    w.logpi = take(B);
    w.minq = take(B);
    w.total = at;
    return w;
}

void add_job(WArgs& wa, const float* dY, int ldy, const float* X, int ldx, int N, int K, float* const* p, float* const* m,
             float* const* v, float* const* tgt, float* const* grad, int at)
{
    WJob& J = wa.job[wa.njobs++];
    J.dY = dY; J.ldy = ldy; J.X = X; J.ldx = ldx; J.N = N; J.K = K;
    J.W = p[at]; J.b = p[at + 1];
    J.mW = m ? m[at] : nullptr; J.mb = m ? m[at + 1] : nullptr;
    J.vW = v ? v[at] : nullptr; J.vb = v ? v[at + 1] : nullptr;
    J.tW = tgt ? tgt[at] : nullptr; J.tb = tgt ? tgt[at + 1] : nullptr;
    J.gW = grad ? grad[at] : nullptr; J.gb = grad ? grad[at + 1] : nullptr;
    J.strip0 = wa.nstrips;
    J.kstrips = (K + 1 + 15) / 16;
    wa.nstrips += ((N + 15) / 16) * J.kstrips;
}

int check_common(const sac_config* cfg, const sac_state* st, int B)
{
    if (cfg == nullptr || st == nullptr) return fail(-10, "NULL configuration or state");
    if (B < 1) return fail(-11, "batch size %d: need B >= 1", B);
    const int rc = sac_supported(cfg->obs_dim, cfg->act_dim, cfg->hidden);
    if (rc != 0) return rc;
    if (any_null(st->policy, SAC_POLICY_TENSORS) || st->act_scale == nullptr || st->act_bias == nullptr)
        return fail(-12, "NULL policy parameter, action scale or action bias");
    if (misaligned(st->policy, SAC_POLICY_TENSORS)) return fail(-13, "policy weights must be 16-byte aligned");
    return 0;
}

int run_update(hipStream_t stream, const sac_config* cfg, const sac_state* st, int B, const float* obs, const float* actions,
               const float* nxtobs, const float* rewards, const float* terminated, const float* noise_next,
               const float* noise_cur, float* stats, float* work, int grads_only, float* const* g_critic,
               float* const* g_policy, float* g_log_alpha)
{
    int rc = check_common(cfg, st, B);
    if (rc != 0) return rc;
    if (!obs || !actions || !nxtobs || !rewards || !terminated || !noise_next || !noise_cur || !stats || !work)
        return fail(-12, "NULL batch, noise, statistics or workspace pointer");
    if (any_null(st->critic, SAC_CRITIC_TENSORS) || any_null(st->target, SAC_CRITIC_TENSORS) || !st->alpha || !st->counters)
        return fail(-12, "NULL critic or target parameter, alpha or counters");
    if (misaligned(st->critic, SAC_CRITIC_TENSORS) || misaligned(st->target, SAC_CRITIC_TENSORS))
        return fail(-13, "critic weights must be 16-byte aligned");
    if (cfg->auto_alpha && !st->log_alpha) return fail(-12, "automatic entropy tuning without log_alpha");
    if (cfg->target_update_interval < 1) return fail(-14, "target_update_interval %d: need >= 1", cfg->target_update_interval);
    if (grads_only) {
        if (!g_critic || !g_policy || any_null(g_critic, SAC_CRITIC_TENSORS) || any_null(g_policy, SAC_POLICY_TENSORS))
            return fail(-12, "NULL gradient buffer");
    } else {
        if (any_null(st->critic_m, SAC_CRITIC_TENSORS) || any_null(st->critic_v, SAC_CRITIC_TENSORS) ||
            any_null(st->policy_m, SAC_POLICY_TENSORS) || any_null(st->policy_v, SAC_POLICY_TENSORS) ||
            (cfg->auto_alpha && (!st->log_alpha_m || !st->log_alpha_v)))
            return fail(-12, "NULL Adam moment");
    }
    const int O = cfg->obs_dim, A = cfg->act_dim, tiles = (B + TB - 1) / TB;
    const Work w = carve(work, O, A, B);
    const PolicyP P = policy_of(st);

    CArgs ca;
    ca.P = P;
    for (int i = 0; i < 2; ++i) { ca.T[i] = head_of(st->target, i); ca.C[i] = head_of(st->critic, i); }
    ca.O = O; ca.A = A; ca.B = B; ca.gamma = cfg->gamma; ca.alpha = st->alpha;
    ca.obs = obs; ca.actions = actions; ca.nxtobs = nxtobs; ca.rewards = rewards; ca.terminated = terminated;
    ca.noise = noise_next; ca.scale = st->act_scale; ca.bias = st->act_bias;
    ca.xu = w.xu; ca.h1 = w.c_h1; ca.h2 = w.c_h2; ca.dh1 = w.c_dh1; ca.dh2 = w.c_dh2; ca.dq = w.c_dq; ca.sq = w.c_sq;
    rc = launch(sac_critic_pass, "sac_critic_pass", tiles, sizeof(float) * (TB * LDX + 4 * TB * LDH + SMALL), stream, ca);
    if (rc != 0) return rc;

    WArgs wa = {};
    wa.B = B; wa.grads_only = grads_only; wa.step_idx = 0; wa.interval = cfg->target_update_interval;
    wa.lr = cfg->lr[0]; wa.beta1 = cfg->beta1[0]; wa.beta2 = cfg->beta2[0]; wa.eps = cfg->eps[0]; wa.tau = cfg->tau;
    wa.counters = st->counters;
    const long BH = (long)B * HID;
    for (int i = 0; i < 2; ++i) {
        add_job(wa, w.c_dh1 + i * BH, HID, w.xu, O + A, HID, O + A, st->critic, st->critic_m, st->critic_v, st->target, g_critic, 6 * i);
        add_job(wa, w.c_dh2 + i * BH, HID, w.c_h1 + i * BH, HID, HID, HID, st->critic, st->critic_m, st->critic_v, st->target, g_critic, 6 * i + 2);
        add_job(wa, w.c_dq + (long)i * B, 1, w.c_h2 + i * BH, HID, 1, HID, st->critic, st->critic_m, st->critic_v, st->target, g_critic, 6 * i + 4);
    }
    rc = launch(sac_wgrad, "sac_wgrad (critic)", (wa.nstrips + 3) / 4, 0, stream, wa);
    if (rc != 0) return rc;

    PArgs pa;
    pa.P = P;
    for (int i = 0; i < 2; ++i) pa.C[i] = head_of(st->critic, i);
    pa.O = O; pa.A = A; pa.B = B; pa.alpha = st->alpha; pa.obs = obs; pa.noise = noise_cur;
    pa.scale = st->act_scale; pa.bias = st->act_bias;
    pa.h1 = w.p_h1; pa.h2 = w.p_h2; pa.dh1 = w.p_dh1; pa.dh2 = w.p_dh2; pa.dmean = w.dmean; pa.dls = w.dls;
    pa.logpi = w.logpi; pa.minq = w.minq;
    rc = launch(sac_policy_pass, "sac_policy_pass", tiles, sizeof(float) * (TB * LDX + 5 * TB * LDH + SMALL), stream, pa);
    if (rc != 0) return rc;

    WArgs wp = {};
    wp.B = B; wp.grads_only = grads_only; wp.step_idx = 1; wp.interval = 1;
    wp.lr = cfg->lr[1]; wp.beta1 = cfg->beta1[1]; wp.beta2 = cfg->beta2[1]; wp.eps = cfg->eps[1]; wp.tau = 0.f;
    wp.counters = st->counters;
    add_job(wp, w.p_dh1, HID, obs, O, HID, O, st->policy, st->policy_m, st->policy_v, nullptr, g_policy, 0);
    add_job(wp, w.p_dh2, HID, w.p_h1, HID, HID, HID, st->policy, st->policy_m, st->policy_v, nullptr, g_policy, 2);
    add_job(wp, w.dmean, A, w.p_h2, HID, A, HID, st->policy, st->policy_m, st->policy_v, nullptr, g_policy, 4);
    add_job(wp, w.dls, A, w.p_h2, HID, A, HID, st->policy, st->policy_m, st->policy_v, nullptr, g_policy, 6);
    rc = launch(sac_wgrad, "sac_wgrad (policy)", (wp.nstrips + 3) / 4, 0, stream, wp);
    if (rc != 0) return rc;

    ZArgs za;
    za.sq = w.c_sq; za.logpi = w.logpi; za.minq = w.minq; za.rewards = rewards; za.terminated = terminated;
    za.B = B; za.auto_alpha = cfg->auto_alpha; za.grads_only = grads_only; za.target_entropy = cfg->target_entropy;
    za.lr = cfg->lr[2]; za.beta1 = cfg->beta1[2]; za.beta2 = cfg->beta2[2]; za.eps = cfg->eps[2];
    za.log_alpha = st->log_alpha; za.log_alpha_m = st->log_alpha_m; za.log_alpha_v = st->log_alpha_v;
    za.alpha = st->alpha; za.stats = stats; za.g_log_alpha = g_log_alpha; za.counters = st->counters;
    return launch(sac_finalize, "sac_finalize", 1, 0, stream, za);
}

}  // namespace

extern "C" {

int sac_supported(int obs_dim, int act_dim, int hidden)
{
    if (hidden != HID) return fail(-1, "hidden size %d: the SAC kernels implement hidden = 256", hidden);
    if (obs_dim != 64 && obs_dim != 128 && obs_dim != 256)
        return fail(-2, "observation width %d: the SAC kernels implement 64, 128 and 256", obs_dim);
    if (act_dim < 1 || act_dim > 16) return fail(-3, "action width %d: the SAC kernels implement 1 to 16", act_dim);
    return 0;
}

long sac_workspace_floats(int obs_dim, int act_dim, int hidden, int B)
{
    const int rc = sac_supported(obs_dim, act_dim, hidden);
    if (rc != 0) return rc;
    if (B < 1) return fail(-11, "batch size %d: need B >= 1", B);
    return carve(nullptr, obs_dim, act_dim, B).total;
}

int sac_policy_forward(void* stream, const sac_config* cfg, const sac_state* st, int B, const float* obs, const float* noise,
                       float* action, float* logp, float* mean_action)
{
    const int rc = check_common(cfg, st, B);
    if (rc != 0) return rc;
    if (!obs || !action) return fail(-12, "NULL observation or action pointer");
    FArgs fa;
    fa.P = policy_of(st);
    fa.O = cfg->obs_dim; fa.A = cfg->act_dim; fa.B = B;
    fa.obs = obs; fa.noise = noise; fa.scale = st->act_scale; fa.bias = st->act_bias;
    fa.action = action; fa.logp = logp; fa.mean_action = mean_action;
    return launch(sac_policy_fwd, "sac_policy_fwd", (B + TB - 1) / TB, sizeof(float) * (TB * LDX + 2 * TB * LDH + SMALL),
                  (hipStream_t)stream, fa);
}

int sac_update(void* stream, const sac_config* cfg, const sac_state* st, int B, const float* obs, const float* actions,
               const float* nxtobs, const float* rewards, const float* terminated, const float* noise_next,
               const float* noise_cur, float* stats, float* work)
{
    return run_update((hipStream_t)stream, cfg, st, B, obs, actions, nxtobs, rewards, terminated, noise_next, noise_cur, stats,
                      work, 0, nullptr, nullptr, nullptr);
}

int sac_grads(void* stream, const sac_config* cfg, const sac_state* st, int B, const float* obs, const float* actions,
              const float* nxtobs, const float* rewards, const float* terminated, const float* noise_next,
              const float* noise_cur, float* stats, float* work, float* const* g_critic, float* const* g_policy,
              float* g_log_alpha)
{
    if (g_critic == nullptr || g_policy == nullptr) return fail(-12, "NULL gradient buffer");
    return run_update((hipStream_t)stream, cfg, st, B, obs, actions, nxtobs, rewards, terminated, noise_next, noise_cur, stats,
                      work, 1, g_critic, g_policy, g_log_alpha);
}

const char* sac_last_error(void) { return g_err; }

}  // extern "C"
