// Whole-rollout kernels of the delay-embedding CNN surrogate (KSDelayCNNSurrogateFactory): C ABI in include/delay_hip.h.
//
// One workgroup of 256 threads owns one sample and runs every step of the rollout in a loop; all activations live in
// LDS, the weights (39 830 fp32 = 156 KiB, one flat vector) are read through the caches.  Inside a step each layer is
// one pass over its outputs with a barrier after it: convolutions and LayerNorms one thread per output element, the
// Linear layers one wave per output row with the inner product split over the 64 lanes (coalesced weight rows) and a
// butterfly sum.
//
// Forward (dly_fwd_kernel), per step k:
//   x_k  = encoder(states_k) while teacher forcing (k < min(S, K)), encoder(output_{k-1}) afterwards
//   la_k = action encoder(actions_k)
//   the window [x_{k-2}, x_{k-1}, x_k] | [la_{k-2}, la_{k-1}, la_k]: a 3-slot ring, slot j lives at j mod 3 (the given
//          context's slot s is j = s - 3)
//   h_k  = MLP(window), d_k = decoder(h_k), output_k = base_k + delta * (d_k * mul + add)
// Backward (dly_bwd_kernel) walks the steps backwards per sample; nothing couples steps except the integration chain
// (g_k = d output_k + g_{k+1} while step k+1 is free running) and the window (d x_j collects slot 2 of step j, slot 1 of
// j + 1, slot 0 of j + 2; it is complete once step j is done, so the encoder / action-encoder backward of j runs right
// then).  Free-running inputs are detached (as in the reference), so their encoder backward is skipped.  Parameter
// gradients are added into the sample's own row of `work` (cleared by a memset on the stream first; each element by one
// fixed thread, steps in a fixed order);
// dly_reduce_kernel sums the rows in sample order.  No atomics anywhere: same inputs, bit-identical gradients.
//
// fp32 throughout with explicit fmaf.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../include/delay_hip.h"
#include "capi_error.h"

namespace {

constexpr int TPB = 256;
constexpr int NWAVE = TPB / 64;
constexpr int N = 64;                       // grid points
constexpr int NACT = 4;                     // raw actuator values
constexpr int DELAY = 3;
constexpr int XS = 64;                      // one encoded state: 8 channels x 8
constexpr int XA = 32;                      // one encoded action: 4 channels x 8
constexpr int SLOT = XS + XA;
constexpr int MIN = DELAY * SLOT;           // 288
constexpr int H1 = 96, H2 = 64, H3 = 64;
constexpr int ACT_NONE = 0, ACT_ELU = 1, ACT_TANH = 2;
constexpr float LN_EPS = 1e-5f;

// ---- the flat parameter vector (named_parameters() order of the factory's module tree) ------------------------------
struct Blk {                                 // one encoder ResidualBlock: offsets; ln < 0 when it has no LayerNorm
    int ci, li, co, ln, act;
    int c1w, n1g, n1b, c2w, n2g, n2b, skw, nsg, nsb, end;
};

constexpr Blk make_blk(int at, int ci, int li, int co, bool ln, int act) {
    Blk b{ci, li, co, ln ? li / 2 : -1, act, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int lo = li / 2;
    b.c1w = at; at += co * ci * 3;
    if (ln) { b.n1g = at; b.n1b = at + lo; at += 2 * lo; }
    b.c2w = at; at += co * co * 3;
    if (ln) { b.n2g = at; b.n2b = at + lo; at += 2 * lo; }
    b.skw = at; at += co * ci;
    if (ln) { b.nsg = at; b.nsb = at + lo; at += 2 * lo; }
    b.end = at;
    return b;
}

constexpr Blk EB0 = make_blk(0, 1, 64, 1, true, ACT_ELU);
constexpr Blk EB1 = make_blk(EB0.end, 1, 32, 4, true, ACT_ELU);
constexpr Blk EB2 = make_blk(EB1.end, 4, 16, 8, false, ACT_TANH);
// decoder: ConvTranspose1d (k3, s2, p1, op1) 8->8, 8->4, 4->1, then Conv1d k5 circular 1->1
constexpr int D0W = EB2.end, D0B = D0W + 8 * 8 * 3, D0G = D0B + 8, D0E = D0G + 16;
constexpr int D1W = D0E + 16, D1B = D1W + 8 * 4 * 3, D1G = D1B + 4, D1E = D1G + 32;
constexpr int D2W = D1E + 32, D2B = D2W + 4 * 1 * 3;
constexpr int D3W = D2B + 1, D3B = D3W + 5;
// action encoder: Linear 4->16 (ELU), 16->32 (Tanh)
constexpr int A0W = D3B + 1, A0B = A0W + 16 * 4, A1W = A0B + 16, A1B = A1W + 32 * 16;
// MLP: Linear 288->96 (ELU), 96->64 (ELU), 64->64 (Tanh)
constexpr int M0W = A1B + 32, M0B = M0W + H1 * MIN, M1W = M0B + H1, M1B = M1W + H2 * H1, M2W = M1B + H2, M2B = M2W + H3 * H2;
constexpr int NPARAM = M2B + H3;
static_assert(NPARAM == 39830, "parameter count of KSDelayCNNSurrogateFactory");

// ---- LDS -----------------------------------------------------------------------------------------------------------
struct EncAct { float a1[64], y1[64], a2[64], y2[64], sk[64], z[64], out[64]; };

struct Lds {
    EncAct enc[3];
    float x[N];                              // encoder input
    float ring_s[3][XS], ring_a[3][XA];      // the window (forward) / its slot gradients (backward)
    float ring_la[3][XA];                    // backward: action encodings of the window
    float in[MIN], z1[H1], z2[H2], h[H3];    // MLP
    float q0a[128], q0y[128], q1a[128], q1y[128], q2a[64], d[64];   // decoder
    float out[N], g[N], dd[N];
    float aq[16], ala[32], araw[NACT];       // action encoder
    float t1[MIN], t2[MIN], t3[MIN], t4[MIN];  // backward scratch
    float st[4 * 8];                         // LayerNorm row statistics
};

// ---- primitives: every one ends with a barrier ----------------------------------------------------------------------
// They are kept out of line (__noinline__): inlined into the two step loops, the backward kernel needed 256 VGPRs + 200
// AGPRs and produced wrong parameter gradients on gfx950 (a Linear weight-gradient pass lost the second sweep of three
// waves; encoder LayerNorm gradients off), which the out-of-line build does not.  The price is a 16-byte call frame per
// lane in scratch; nothing spills.
__device__ inline float activate(float x, int act) {
    return act == ACT_ELU ? (x > 0.0f ? x : expm1f(x)) : act == ACT_TANH ? tanhf(x) : x;
}

// d activation / d input, from the activation's output
__device__ inline float act_slope(float y, int act) {
    return act == ACT_ELU ? (y > 0.0f ? 1.0f : y + 1.0f) : act == ACT_TANH ? fmaf(-y, y, 1.0f) : 1.0f;
}

__device__ inline int wrap(int j, int n) { j %= n; return j < 0 ? j + n : j; }

__device__ void copy(float* dst, const float* src, int n, int tid) {
    for (int e = tid; e < n; e += TPB) dst[e] = src ? src[e] : 0.0f;
    __syncthreads();
}

// circular Conv1d (bias optional) + activation: in [ci][li] -> out [co][lo], lo = li / s
__device__ __noinline__ void conv_fwd(const float* __restrict__ w, const float* __restrict__ bias, const float* in, int ci, int li,
                         float* out, int co, int lo, int k, int s, int p, int act, int tid) {
    for (int e = tid; e < co * lo; e += TPB) {
        const int c = e / lo, o = e % lo;
        float acc = bias ? bias[c] : 0.0f;
        for (int i = 0; i < ci; ++i)
            for (int t = 0; t < k; ++t) acc = fmaf(w[(c * ci + i) * k + t], in[i * li + wrap(o * s + t - p, li)], acc);
        out[e] = activate(acc, act);
    }
    __syncthreads();
}

// data gradient of conv_fwd (before its activation): din [ci][li] (= or +=) from dout [co][lo]
__device__ __noinline__ void conv_dgrad(const float* __restrict__ w, const float* dout, float* din, int ci, int li, int co, int lo,
                           int k, int s, int p, bool accumulate, int tid) {
    for (int e = tid; e < ci * li; e += TPB) {
        const int i = e / li, j = e % li;
        float acc = accumulate ? din[e] : 0.0f;
        for (int c = 0; c < co; ++c)
            for (int t = 0; t < k; ++t) {
                const int q = wrap(j - t + p, li);
                if (q % s) continue;
                const int o = q / s;
                if (o < lo) acc = fmaf(w[(c * ci + i) * k + t], dout[c * lo + o], acc);
            }
        din[e] = acc;
    }
    __syncthreads();
}

// weight (and bias) gradient of conv_fwd, added into the gradient row
__device__ __noinline__ void conv_wgrad(float* gw, float* gb, const float* dout, const float* in, int ci, int li, int co, int lo, int k,
                           int s, int p, int tid) {
    for (int e = tid; e < co * ci * k; e += TPB) {
        const int c = e / (ci * k), i = (e / k) % ci, t = e % k;
        float acc = 0.0f;
        for (int o = 0; o < lo; ++o) acc = fmaf(dout[c * lo + o], in[i * li + wrap(o * s + t - p, li)], acc);
        gw[e] += acc;
    }
    if (gb)
        for (int c = tid; c < co; c += TPB) {
            float acc = 0.0f;
            for (int o = 0; o < lo; ++o) acc += dout[c * lo + o];
            gb[c] += acc;
        }
    __syncthreads();
}

// ConvTranspose1d (zero padded, k3, s2, p1, output_padding 1) + activation: in [ci][li] -> out [co][2 li]; w [ci][co][3]
__device__ __noinline__ void deconv_fwd(const float* __restrict__ w, const float* __restrict__ bias, const float* in, int ci, int li,
                           float* out, int co, int act, int tid) {
    const int lo = 2 * li;
    for (int e = tid; e < co * lo; e += TPB) {
        const int c = e / lo, o = e % lo;
        float acc = bias[c];
        for (int i = 0; i < ci; ++i)
            for (int t = 0; t < 3; ++t) {
                const int q = o + 1 - t;
                if (q < 0 || (q & 1) || (q >> 1) >= li) continue;
                acc = fmaf(w[(i * co + c) * 3 + t], in[i * li + (q >> 1)], acc);
            }
        out[e] = activate(acc, act);
    }
    __syncthreads();
}

__device__ __noinline__ void deconv_dgrad(const float* __restrict__ w, const float* dout, float* din, int ci, int li, int co, int tid) {
    const int lo = 2 * li;
    for (int e = tid; e < ci * li; e += TPB) {
        const int i = e / li, j = e % li;
        float acc = 0.0f;
        for (int c = 0; c < co; ++c)
            for (int t = 0; t < 3; ++t) {
                const int o = 2 * j - 1 + t;
                if (o >= 0 && o < lo) acc = fmaf(w[(i * co + c) * 3 + t], dout[c * lo + o], acc);
            }
        din[e] = acc;
    }
    __syncthreads();
}

__device__ __noinline__ void deconv_wgrad(float* gw, float* gb, const float* dout, const float* in, int ci, int li, int co, int tid) {
    const int lo = 2 * li;
    for (int e = tid; e < ci * co * 3; e += TPB) {
        const int i = e / (co * 3), c = (e / 3) % co, t = e % 3;
        float acc = 0.0f;
        for (int j = 0; j < li; ++j) {
            const int o = 2 * j - 1 + t;
            if (o >= 0 && o < lo) acc = fmaf(in[i * li + j], dout[c * lo + o], acc);
        }
        gw[e] += acc;
    }
    for (int c = tid; c < co; c += TPB) {
        float acc = 0.0f;
        for (int o = 0; o < lo; ++o) acc += dout[c * lo + o];
        gb[c] += acc;
    }
    __syncthreads();
}

// mean and 1/sqrt(biased var + eps) of each of the c rows of length l
__device__ __noinline__ void ln_stats(const float* a, int c, int l, float* st, int tid) {
    if (tid < c) {
        float m = 0.0f;
        for (int p = 0; p < l; ++p) m += a[tid * l + p];
        m /= (float)l;
        float v = 0.0f;
        for (int p = 0; p < l; ++p) {
            const float dv = a[tid * l + p] - m;
            v = fmaf(dv, dv, v);
        }
        v /= (float)l;
        st[4 * tid] = m;
        st[4 * tid + 1] = 1.0f / sqrtf(v + LN_EPS);
    }
    __syncthreads();
}

// LayerNorm over the last axis (affine g, b of length l); without one (g == nullptr) a copy
__device__ __noinline__ void ln_fwd(const float* a, float* y, int c, int l, const float* g, const float* b, float* st, int tid) {
    if (!g) { copy(y, a, c * l, tid); return; }
    ln_stats(a, c, l, st, tid);
    for (int e = tid; e < c * l; e += TPB) {
        const int r = e / l, p = e % l;
        y[e] = fmaf((a[e] - st[4 * r]) * st[4 * r + 1], g[p], b[p]);
    }
    __syncthreads();
}

// dx from dy through ln_fwd(a); adds d gamma / d beta into the gradient row
__device__ __noinline__ void ln_bwd(const float* a, const float* dy, float* dx, int c, int l, const float* g, float* gg, float* gb,
                       float* st, int tid) {
    if (!g) { copy(dx, dy, c * l, tid); return; }
    ln_stats(a, c, l, st, tid);
    if (tid < c) {
        const float m = st[4 * tid], rs = st[4 * tid + 1];
        float s1 = 0.0f, s2 = 0.0f;
        for (int p = 0; p < l; ++p) {
            const float dh = dy[tid * l + p] * g[p];
            s1 += dh;
            s2 = fmaf(dh, (a[tid * l + p] - m) * rs, s2);
        }
        st[4 * tid + 2] = s1 / (float)l;
        st[4 * tid + 3] = s2 / (float)l;
    }
    __syncthreads();
    for (int e = tid; e < c * l; e += TPB) {
        const int r = e / l, p = e % l;
        const float xh = (a[e] - st[4 * r]) * st[4 * r + 1];
        dx[e] = st[4 * r + 1] * (fmaf(dy[e], g[p], -st[4 * r + 2]) - xh * st[4 * r + 3]);
    }
    for (int p = tid; p < l; p += TPB) {
        float sg = 0.0f, sb = 0.0f;
        for (int r = 0; r < c; ++r) {
            sg = fmaf(dy[r * l + p], (a[r * l + p] - st[4 * r]) * st[4 * r + 1], sg);
            sb += dy[r * l + p];
        }
        gg[p] += sg;
        gb[p] += sb;
    }
    __syncthreads();
}

// dz *= slope of the activation at its output y (in place)
__device__ __noinline__ void act_bwd(const float* y, float* dz, int n, int act, int tid) {
    for (int e = tid; e < n; e += TPB) dz[e] *= act_slope(y[e], act);
    __syncthreads();
}

// nn.Linear + activation: out[o] = act(b[o] + sum_i w[o][i] in[i]); a wave per output row
__device__ __noinline__ void linear_fwd(const float* __restrict__ w, const float* __restrict__ bias, const float* in, int nin, float* out,
                           int nout, int act, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    for (int o = wave; o < nout; o += NWAVE) {
        float s = 0.0f;
        for (int i = lane; i < nin; i += 64) s = fmaf(w[o * nin + i], in[i], s);
        for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
        if (lane == 0) out[o] = activate(s + bias[o], act);
    }
    __syncthreads();
}

__device__ __noinline__ void linear_dgrad(const float* __restrict__ w, const float* dout, float* din, int nin, int nout, int tid) {
    for (int i = tid; i < nin; i += TPB) {
        float acc = 0.0f;
        for (int o = 0; o < nout; ++o) acc = fmaf(w[o * nin + i], dout[o], acc);
        din[i] = acc;
    }
    __syncthreads();
}

__device__ __noinline__ void linear_wgrad(float* gw, float* gb, const float* dout, const float* in, int nin, int nout, int tid) {
    for (int e = tid; e < nin * nout; e += TPB) {
        const int o = e / nin, i = e - o * nin;
        const float d = dout[o], x = in[i];
        gw[e] = fmaf(d, x, gw[e]);
    }
    for (int o = tid; o < nout; o += TPB) gb[o] += dout[o];
    __syncthreads();
}

// ---- modules -------------------------------------------------------------------------------------------------------
__device__ void block_fwd(const float* P, const Blk& b, const float* x, EncAct& A, float* st, int tid) {
    const int lo = b.li / 2;
    const bool ln = b.ln > 0;
    conv_fwd(P + b.c1w, nullptr, x, b.ci, b.li, A.a1, b.co, lo, 3, 2, 1, b.act, tid);
    ln_fwd(A.a1, A.y1, b.co, lo, ln ? P + b.n1g : nullptr, P + b.n1b, st, tid);
    conv_fwd(P + b.c2w, nullptr, A.y1, b.co, lo, A.a2, b.co, lo, 3, 1, 1, b.act, tid);
    ln_fwd(A.a2, A.y2, b.co, lo, ln ? P + b.n2g : nullptr, P + b.n2b, st, tid);
    conv_fwd(P + b.skw, nullptr, x, b.ci, b.li, A.sk, b.co, lo, 1, 2, 0, ACT_NONE, tid);
    for (int e = tid; e < b.co * lo; e += TPB) A.z[e] = A.y2[e] + A.sk[e];
    __syncthreads();
    ln_fwd(A.z, A.out, b.co, lo, ln ? P + b.nsg : nullptr, P + b.nsb, st, tid);
}

// dout [co][lo] -> dx [ci][li]; scratch u, v of 64
__device__ void block_bwd(const float* P, float* G, const Blk& b, const float* x, const EncAct& A, const float* dout, float* dx,
                          float* u, float* v, float* st, int tid) {
    const int lo = b.li / 2, n = b.co * lo;
    const bool ln = b.ln > 0;
    ln_bwd(A.z, dout, u, b.co, lo, ln ? P + b.nsg : nullptr, G + b.nsg, G + b.nsb, st, tid);           // u = d z
    conv_wgrad(G + b.skw, nullptr, u, x, b.ci, b.li, b.co, lo, 1, 2, 0, tid);
    conv_dgrad(P + b.skw, u, dx, b.ci, b.li, b.co, lo, 1, 2, 0, false, tid);
    ln_bwd(A.a2, u, v, b.co, lo, ln ? P + b.n2g : nullptr, G + b.n2g, G + b.n2b, st, tid);            // v = d a2
    act_bwd(A.a2, v, n, b.act, tid);
    conv_wgrad(G + b.c2w, nullptr, v, A.y1, b.co, lo, b.co, lo, 3, 1, 1, tid);
    conv_dgrad(P + b.c2w, v, u, b.co, lo, b.co, lo, 3, 1, 1, false, tid);                              // u = d y1
    ln_bwd(A.a1, u, v, b.co, lo, ln ? P + b.n1g : nullptr, G + b.n1g, G + b.n1b, st, tid);            // v = d a1
    act_bwd(A.a1, v, n, b.act, tid);
    conv_wgrad(G + b.c1w, nullptr, v, x, b.ci, b.li, b.co, lo, 3, 2, 1, tid);
    conv_dgrad(P + b.c1w, v, dx, b.ci, b.li, b.co, lo, 3, 2, 1, true, tid);
}

// L.x [64] -> L.enc[2].out [8][8]
__device__ void encoder_fwd(const float* P, Lds& L, int tid) {
    block_fwd(P, EB0, L.x, L.enc[0], L.st, tid);
    block_fwd(P, EB1, L.enc[0].out, L.enc[1], L.st, tid);
    block_fwd(P, EB2, L.enc[1].out, L.enc[2], L.st, tid);
}

// d L.enc[2].out (in dz [64]) -> d x (in dx [64]); needs encoder_fwd's activations
__device__ void encoder_bwd(const float* P, float* G, Lds& L, const float* dz, float* dx, int tid) {
    block_bwd(P, G, EB2, L.enc[1].out, L.enc[2], dz, L.t1, L.t2, L.t3, L.st, tid);
    block_bwd(P, G, EB1, L.enc[0].out, L.enc[1], L.t1, L.t4, L.t2, L.t3, L.st, tid);
    block_bwd(P, G, EB0, L.x, L.enc[0], L.t4, dx, L.t2, L.t3, L.st, tid);
}

// L.araw [4] -> L.aq [16] -> L.ala [32]
__device__ void action_fwd(const float* P, Lds& L, const float* a, int tid) {
    if (tid < NACT) L.araw[tid] = a[tid];
    __syncthreads();
    linear_fwd(P + A0W, P + A0B, L.araw, NACT, L.aq, 16, ACT_ELU, tid);
    linear_fwd(P + A1W, P + A1B, L.aq, 16, L.ala, XA, ACT_TANH, tid);
}

// d L.ala (in dla, overwritten) -> d raw actions (da, may be null)
__device__ void action_bwd(const float* P, float* G, Lds& L, float* dla, float* da, int tid) {
    act_bwd(L.ala, dla, XA, ACT_TANH, tid);
    linear_wgrad(G + A1W, G + A1B, dla, L.aq, 16, XA, tid);
    linear_dgrad(P + A1W, dla, L.t3, 16, XA, tid);
    act_bwd(L.aq, L.t3, 16, ACT_ELU, tid);
    linear_wgrad(G + A0W, G + A0B, L.t3, L.araw, NACT, 16, tid);
    linear_dgrad(P + A0W, L.t3, L.t2, NACT, 16, tid);
    if (da && tid < NACT) da[tid] = L.t2[tid];
    __syncthreads();
}

// L.in [288] -> L.z1, L.z2, L.h
__device__ void mlp_fwd(const float* P, Lds& L, int tid) {
    linear_fwd(P + M0W, P + M0B, L.in, MIN, L.z1, H1, ACT_ELU, tid);
    linear_fwd(P + M1W, P + M1B, L.z1, H1, L.z2, H2, ACT_ELU, tid);
    linear_fwd(P + M2W, P + M2B, L.z2, H2, L.h, H3, ACT_TANH, tid);
}

// d h (in dh, overwritten) -> d in (L.t1 [288])
__device__ void mlp_bwd(const float* P, float* G, Lds& L, float* dh, int tid) {
    act_bwd(L.h, dh, H3, ACT_TANH, tid);
    linear_wgrad(G + M2W, G + M2B, dh, L.z2, H2, H3, tid);
    linear_dgrad(P + M2W, dh, L.t2, H2, H3, tid);
    act_bwd(L.z2, L.t2, H2, ACT_ELU, tid);
    linear_wgrad(G + M1W, G + M1B, L.t2, L.z1, H1, H2, tid);
    linear_dgrad(P + M1W, L.t2, L.t3, H1, H2, tid);
    act_bwd(L.z1, L.t3, H1, ACT_ELU, tid);
    linear_wgrad(G + M0W, G + M0B, L.t3, L.in, MIN, H1, tid);
    linear_dgrad(P + M0W, L.t3, L.t1, MIN, H1, tid);
}

// L.h [8][8] -> L.d [64]
__device__ void decoder_fwd(const float* P, Lds& L, int tid) {
    deconv_fwd(P + D0W, P + D0B, L.h, 8, 8, L.q0a, 8, ACT_ELU, tid);
    ln_fwd(L.q0a, L.q0y, 8, 16, P + D0G, P + D0G + 16, L.st, tid);
    deconv_fwd(P + D1W, P + D1B, L.q0y, 8, 16, L.q1a, 4, ACT_ELU, tid);
    ln_fwd(L.q1a, L.q1y, 4, 32, P + D1G, P + D1G + 32, L.st, tid);
    deconv_fwd(P + D2W, P + D2B, L.q1y, 4, 32, L.q2a, 1, ACT_ELU, tid);
    conv_fwd(P + D3W, P + D3B, L.q2a, 1, N, L.d, 1, N, 5, 1, 2, ACT_TANH, tid);
}

// d L.d (in L.dd, overwritten) -> d h (dh [64])
__device__ void decoder_bwd(const float* P, float* G, Lds& L, float* dh, int tid) {
    act_bwd(L.d, L.dd, N, ACT_TANH, tid);
    conv_wgrad(G + D3W, G + D3B, L.dd, L.q2a, 1, N, 1, N, 5, 1, 2, tid);
    conv_dgrad(P + D3W, L.dd, L.t1, 1, N, 1, N, 5, 1, 2, false, tid);
    act_bwd(L.q2a, L.t1, N, ACT_ELU, tid);
    deconv_wgrad(G + D2W, G + D2B, L.t1, L.q1y, 4, 32, 1, tid);
    deconv_dgrad(P + D2W, L.t1, L.t2, 4, 32, 1, tid);
    ln_bwd(L.q1a, L.t2, L.t3, 4, 32, P + D1G, G + D1G, G + D1G + 32, L.st, tid);
    act_bwd(L.q1a, L.t3, 128, ACT_ELU, tid);
    deconv_wgrad(G + D1W, G + D1B, L.t3, L.q0y, 8, 16, 4, tid);
    deconv_dgrad(P + D1W, L.t3, L.t2, 8, 16, 4, tid);
    ln_bwd(L.q0a, L.t2, L.t3, 8, 16, P + D0G, G + D0G, G + D0G + 16, L.st, tid);
    act_bwd(L.q0a, L.t3, 128, ACT_ELU, tid);
    deconv_wgrad(G + D0W, G + D0B, L.t3, L.h, 8, 8, 8, tid);
    deconv_dgrad(P + D0W, L.t3, dh, 8, 8, 8, tid);
}

// ---- kernels -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB) dly_fwd_kernel(const float* __restrict__ P, int S, int K, int su,
                                                      const float* __restrict__ states, const float* __restrict__ actions,
                                                      const float* __restrict__ cs_in, const float* __restrict__ ca_in,
                                                      float delta, float mul, float add, float* __restrict__ outputs,
                                                      float* __restrict__ deltas, float* __restrict__ inlat,
                                                      float* __restrict__ outlat, float* __restrict__ cs_out,
                                                      float* __restrict__ ca_out) {
    __shared__ Lds L;
    const int b = blockIdx.x, tid = threadIdx.x;
    // the given context: slot s is j = s - 3, i.e. ring slot s
    copy(&L.ring_s[0][0], cs_in ? cs_in + (size_t)b * DELAY * XS : nullptr, DELAY * XS, tid);
    copy(&L.ring_a[0][0], ca_in ? ca_in + (size_t)b * DELAY * XA : nullptr, DELAY * XA, tid);
    for (int k = 0; k < K; ++k) {
        const size_t row = ((size_t)b * K + k) * N;
        const float* base = k < su ? states + ((size_t)b * S + k) * N : L.out;
        copy(L.x, base, N, tid);
        encoder_fwd(P, L, tid);
        const int r = k % 3;
        for (int e = tid; e < XS; e += TPB) {
            L.ring_s[r][e] = L.enc[2].out[e];
            inlat[row + e] = L.enc[2].out[e];
        }
        action_fwd(P, L, actions + ((size_t)b * K + k) * NACT, tid);
        for (int e = tid; e < XA; e += TPB) L.ring_a[r][e] = L.ala[e];
        __syncthreads();
        for (int e = tid; e < MIN; e += TPB) {
            const int s = e / SLOT, w = e % SLOT, rs = (k + 1 + s) % 3;
            L.in[e] = w < XS ? L.ring_s[rs][w] : L.ring_a[rs][w - XS];
        }
        __syncthreads();
        mlp_fwd(P, L, tid);
        decoder_fwd(P, L, tid);
        for (int e = tid; e < N; e += TPB) {
            const float o = fmaf(delta, fmaf(L.d[e], mul, add), L.x[e]);   // L.x still holds base_k
            outlat[row + e] = L.h[e];
            deltas[row + e] = L.d[e];
            outputs[row + e] = o;
            L.out[e] = o;
        }
        __syncthreads();
        (void)base;
    }
    // final context: slot i is j = K - 3 + i
    for (int e = tid; e < DELAY * XS; e += TPB) cs_out[(size_t)b * DELAY * XS + e] = L.ring_s[(K + e / XS) % 3][e % XS];
    for (int e = tid; e < DELAY * XA; e += TPB) ca_out[(size_t)b * DELAY * XA + e] = L.ring_a[(K + e / XA) % 3][e % XA];
}

__global__ void __launch_bounds__(TPB) dly_bwd_kernel(const float* __restrict__ P, int S, int K, int su,
                                                      const float* __restrict__ states, const float* __restrict__ actions,
                                                      const float* __restrict__ cs_in, const float* __restrict__ ca_in,
                                                      const float* __restrict__ inlat, const float* __restrict__ outlat,
                                                      float delta, float mul, const float* __restrict__ d_out,
                                                      const float* __restrict__ d_del, const float* __restrict__ d_inl,
                                                      const float* __restrict__ d_outl, const float* __restrict__ d_cs_out,
                                                      const float* __restrict__ d_ca_out, float* __restrict__ d_states,
                                                      float* __restrict__ d_actions, float* __restrict__ d_cs_in,
                                                      float* __restrict__ d_ca_in, float* __restrict__ work) {
    __shared__ Lds L;
    const int b = blockIdx.x, tid = threadIdx.x;
    float* G = work + (size_t)b * NPARAM;      // zeroed by dly_backward before the launch; each element of G is only ever
                                               // read and written by one fixed thread (the same loop over the same range)
    // slot gradients: ring slot j mod 3 collects d x_j / d la_j; the returned context's slot i is j = K - 3 + i
    for (int e = tid; e < DELAY * XS; e += TPB)
        L.ring_s[(K + e / XS) % 3][e % XS] = d_cs_out ? d_cs_out[(size_t)b * DELAY * XS + e] : 0.0f;
    for (int e = tid; e < DELAY * XA; e += TPB)
        L.ring_a[(K + e / XA) % 3][e % XA] = d_ca_out ? d_ca_out[(size_t)b * DELAY * XA + e] : 0.0f;
    for (int e = tid; e < N; e += TPB) L.g[e] = 0.0f;
    __syncthreads();
    // action encodings of the window of the last step
    for (int j = K - 3; j < K; ++j) {
        if (j < 0) continue;
        action_fwd(P, L, actions + ((size_t)b * K + j) * NACT, tid);
        copy(L.ring_la[j % 3], L.ala, XA, tid);
    }
    for (int k = K - 1; k >= 0; --k) {
        const size_t row = ((size_t)b * K + k) * N;
        const bool carry = k + 1 < K && k + 1 >= su;
        for (int e = tid; e < N; e += TPB) {
            const float g = (d_out ? d_out[row + e] : 0.0f) + (carry ? L.g[e] : 0.0f);
            L.g[e] = g;
            L.dd[e] = fmaf(delta * mul, g, d_del ? d_del[row + e] : 0.0f);
            L.h[e] = outlat[row + e];
        }
        __syncthreads();
        decoder_fwd(P, L, tid);
        decoder_bwd(P, G, L, L.t4, tid);                     // t4 = d h from the decoder
        // the window of step k
        for (int e = tid; e < MIN; e += TPB) {
            const int s = e / SLOT, w = e % SLOT, j = k - 2 + s;
            float v;
            if (w < XS) v = j >= 0 ? inlat[((size_t)b * K + j) * N + w] : (cs_in ? cs_in[((size_t)b * DELAY + j + 3) * XS + w] : 0.0f);
            else v = j >= 0 ? L.ring_la[j % 3][w - XS] : (ca_in ? ca_in[((size_t)b * DELAY + j + 3) * XA + w - XS] : 0.0f);
            L.in[e] = v;
        }
        __syncthreads();
        mlp_fwd(P, L, tid);
        for (int e = tid; e < H3; e += TPB) L.dd[e] = L.t4[e] + (d_outl ? d_outl[row + e] : 0.0f);
        __syncthreads();
        mlp_bwd(P, G, L, L.dd, tid);                         // t1 = d window
        for (int e = tid; e < MIN; e += TPB) {
            const int s = e / SLOT, w = e % SLOT, r = wrap(k - 2 + s, 3);
            if (w < XS) L.ring_s[r][w] += L.t1[e];
            else L.ring_a[r][w - XS] += L.t1[e];
        }
        __syncthreads();
        // step k's slot gradients are complete
        const int r = k % 3;
        if (k < su) {
            for (int e = tid; e < XS; e += TPB) L.t4[e] = L.ring_s[r][e] + (d_inl ? d_inl[row + e] : 0.0f);
            copy(L.x, states + ((size_t)b * S + k) * N, N, tid);
            encoder_fwd(P, L, tid);
            encoder_bwd(P, G, L, L.t4, L.dd, tid);           // dd = d state_k through the encoder
            if (d_states)
                for (int e = tid; e < N; e += TPB) d_states[((size_t)b * S + k) * N + e] = L.g[e] + L.dd[e];
        }
        action_fwd(P, L, actions + ((size_t)b * K + k) * NACT, tid);
        copy(L.t4, L.ring_a[r], XA, tid);
        action_bwd(P, G, L, L.t4, d_actions ? d_actions + ((size_t)b * K + k) * NACT : nullptr, tid);
        for (int e = tid; e < XS; e += TPB) L.ring_s[r][e] = 0.0f;
        for (int e = tid; e < XA; e += TPB) L.ring_a[r][e] = 0.0f;
        __syncthreads();
        if (k >= 3) {
            action_fwd(P, L, actions + ((size_t)b * K + k - 3) * NACT, tid);
            copy(L.ring_la[r], L.ala, XA, tid);
        }
    }
    if (d_states)
        for (int e = tid; e < (S - su) * N; e += TPB) d_states[((size_t)b * S + su) * N + e] = 0.0f;
    // the given context: slot s is j = s - 3 (slot 0 never reaches an output)
    if (d_cs_in)
        for (int e = tid; e < DELAY * XS; e += TPB)
            d_cs_in[(size_t)b * DELAY * XS + e] = e < XS ? 0.0f : L.ring_s[e / XS][e % XS];
    if (d_ca_in)
        for (int e = tid; e < DELAY * XA; e += TPB)
            d_ca_in[(size_t)b * DELAY * XA + e] = e < XA ? 0.0f : L.ring_a[e / XA][e % XA];
}

// out[p] = sum over rows b = 0 .. B-1 of rows[b][p], in that order
__global__ void __launch_bounds__(TPB) dly_reduce_kernel(const float* __restrict__ rows, int B, float* __restrict__ out) {
    const int p = blockIdx.x * TPB + threadIdx.x;
    if (p >= NPARAM) return;
    float s = 0.0f;
    for (int b = 0; b < B; ++b) s += rows[(size_t)b * NPARAM + p];
    out[p] = s;
}

}  // namespace

extern "C" {

int dly_param_count(void) { return NPARAM; }

int dly_supported(int n, int delay, int schannels, int ssize, int achannels, int asize, int actions, int nparams) {
    if (n != N) return fail(-4, "dly: grid width %d (the kernels are built for N = %d)", n, N);
    if (delay != DELAY) return fail(-4, "dly: delay %d (the kernels are built for delay = %d)", delay, DELAY);
    if (schannels * ssize != XS || ssize != 8 || achannels * asize != XA || asize != 8)
        return fail(-4, "dly: latent %d x %d / action latent %d x %d (the kernels take 8 x 8 / 4 x 8)", schannels, ssize,
                    achannels, asize);
    if (actions != NACT) return fail(-4, "dly: %d actuator values (the kernels take %d)", actions, NACT);
    if (nparams != NPARAM) return fail(-4, "dly: %d parameters (the kernels take %d)", nparams, NPARAM);
    return 0;
}

long dly_workspace_floats(int B) { return B > 0 ? (long)B * NPARAM : 0; }

int dly_forward(void* stream, const float* params, int B, int S, int K, const float* states, const float* actions,
                const float* ctx_s_in, const float* ctx_a_in, float delta, float mul, float add, float* outputs,
                float* deltas, float* inlatents, float* outlatents, float* ctx_s_out, float* ctx_a_out) {
    if (!params || !states || !actions || !outputs || !deltas || !inlatents || !outlatents || !ctx_s_out || !ctx_a_out ||
        B <= 0 || S <= 0 || K <= 0)
        return fail(-1, "dly_forward: bad argument");
    const int su = S < K ? S : K;
    hipLaunchKernelGGL(dly_fwd_kernel, dim3(B), dim3(TPB), 0, (hipStream_t)stream, params, S, K, su, states, actions,
                       ctx_s_in, ctx_a_in, delta, mul, add, outputs, deltas, inlatents, outlatents, ctx_s_out, ctx_a_out);
    return launch_status(-2, "dly_forward");
}

int dly_backward(void* stream, const float* params, int B, int S, int K, const float* states, const float* actions,
                 const float* ctx_s_in, const float* ctx_a_in, const float* inlatents, const float* outlatents, float delta,
                 float mul, const float* d_outputs, const float* d_deltas, const float* d_inlatents,
                 const float* d_outlatents, const float* d_ctx_s_out, const float* d_ctx_a_out, float* d_states,
                 float* d_actions, float* d_ctx_s_in, float* d_ctx_a_in, float* d_params, float* work) {
    if (!params || !states || !actions || !inlatents || !outlatents || !d_params || B <= 0 || S <= 0 || K <= 0)
        return fail(-1, "dly_backward: bad argument");
    if (!work) return fail(-1, "dly_backward: no workspace (dly_workspace_floats(B) floats)");
    const int su = S < K ? S : K;
    if (hipMemsetAsync(work, 0, sizeof(float) * (size_t)B * NPARAM, (hipStream_t)stream) != hipSuccess)
        return fail(-2, "dly_backward: clearing the workspace failed");
    hipLaunchKernelGGL(dly_bwd_kernel, dim3(B), dim3(TPB), 0, (hipStream_t)stream, params, S, K, su, states, actions,
                       ctx_s_in, ctx_a_in, inlatents, outlatents, delta, mul, d_outputs, d_deltas, d_inlatents,
                       d_outlatents, d_ctx_s_out, d_ctx_a_out, d_states, d_actions, d_ctx_s_in, d_ctx_a_in, work);
    int rc = launch_status(-2, "dly_backward");
    if (rc) return rc;
    hipLaunchKernelGGL(dly_reduce_kernel, dim3((NPARAM + TPB - 1) / TPB), dim3(TPB), 0, (hipStream_t)stream, work, B,
                       d_params);
    return launch_status(-2, "dly_backward (reduce)");
}

const char* dly_last_error(void) { return g_err; }

}  // extern "C"
