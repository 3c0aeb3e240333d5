// sur_narrow.h -- the narrow residual block (every channel count <= 4), one wave per sample on the VALU: enc_narrow, the nr_*
// device functions, nr_block_forward / nr_block_backward and the per-wave LDS sizers.
// Needs sur_common.h, sur_gemm.h (the MFMA tile type) and surrogate_hip.h.
#ifndef SUR_NARROW_H
#define SUR_NARROW_H

#include "../../include/surrogate_hip.h"
#include "sur_common.h"
#include "sur_gemm.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Narrow residual block: every channel count <= 4 (the action encoder, 1 -> 2 -> 4 -> 4) -- on the VALU, ONE WAVE PER SAMPLE.
// The MFMA gather-GEMM path spends its instructions on tile bookkeeping, index functors and masks whatever the channel
// counts: ~11 k wave-instructions per sample and block backward for ~10 k useful multiply-adds, and these kernels are
// instruction-issue bound.  Here a lane owns the positions p = lane + 64 e of every channel, keeps
// its values in registers, reads convolution neighbours from a wave-private LDS copy; LayerNorm statistics of all channels
// go through one halving butterfly (nr_wave_totals), a convolution's weight gradient is ONE MFMA tile whose reduction
// dimension is the position (nr_wgrad); the four waves of a workgroup handle four samples independently (no workgroup
// barrier inside a pass), sharing the staged weights.  Records in `saved`, outputs and partial-gradient rows are laid out
// exactly as the MFMA path leaves them, so either path can consume the other's.
// ---------------------------------------------------------------------------------------------
constexpr int NR_C = 4;   // channels
// positions per lane: at most 2 (block outputs are <= 128 wide, inputs that need a gradient too: N <= 256)

__host__ __device__ inline bool enc_narrow(const sur_encoder_params& p) {
    // block 0: 1 -> <= 2 channels onto <= 128 positions (tile 2 x 2, no input gradient); block 1: <= 2 -> <= 4 channels, <= 128 ->
    // <= 64 positions; block 2: <= 4 -> <= 4 channels on <= 64 positions
    if (p.c[0] != 1 || p.c[1] > 2 || p.c[2] > NR_C || p.c[3] > NR_C) return false;
    for (int b = 0; b < 3; ++b)
        if (p.stride[b] != 1 && p.stride[b] != 2) return false;
    const int h1 = p.n / p.stride[0], h2 = h1 / p.stride[1], h3 = h2 / p.stride[2];
    return h1 <= 128 && h2 <= 64 && h3 <= 64 && h3 == h2 && (h1 & 7) == 0 && (h2 & 7) == 0;
}

// LDS traffic between the lanes of ONE wave: make the wave's own writes visible to its later reads
#define NR_WAVE_SYNC()                                           \
    do {                                                          \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");    \
        __builtin_amdgcn_wave_barrier();                          \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");    \
    } while (0)

// Totals over the whole wave of M (4 or 8) per-lane values, returned wave-uniform (SGPRs).  A halving butterfly: in a stage two
// lanes that differ in one bit of the lane id split a PAIR of values between them -- each keeps one, hands the other over and
// adds what it receives -- so a lane carries half as many values afterwards; M values cost ~M exchanges instead of 6 M, in six
// dependent stages instead of 6 M / 2 (a wave that owns a whole sample has nothing to hide that chain behind; LayerNorm sums
// were half of the narrow kernels' instructions).  Lane bits 0 and 1 by DPP quad permutes, bit 4 by v_permlane16_swap (which
// IS the keep-one-hand-one-over exchange between even and odd rows of 16), then plain all-reduce steps on the one value left:
// bits 3, 2 by row rotations, bit 5 by v_permlane32_swap.  Every lane ends up with the total of the value its bits (4,1,0)
// name; v_readlane hands them out.
template <int CTRL>
__device__ __forceinline__ float nr_halve(bool upper, float lo, float hi) {
    return (upper ? hi : lo) + dpp_rot<CTRL>(upper ? lo : hi);
}
template <int M>
__device__ __forceinline__ void nr_wave_totals(float (&v)[M], int lane) {
    static_assert(M == 4 || M == 8, "two or four channels, two sums each");
    const bool b0 = lane & 1, b1 = lane & 2;
    float w[M / 2], x[M / 4];
#pragma unroll
    for (int i = 0; i < M / 2; ++i) w[i] = nr_halve<0xB1>(b0, v[2 * i], v[2 * i + 1]);     // quad_perm:[1,0,3,2]
#pragma unroll
    for (int i = 0; i < M / 4; ++i) x[i] = nr_halve<0x4E>(b1, w[2 * i], w[2 * i + 1]);     // quad_perm:[2,3,0,1]
    // rows 1, 3 of the first operand <-> rows 0, 2 of the second: even rows collect x[0], odd rows x[M / 4 - 1]
    const swap_u2 r16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(x[0]), __float_as_uint(x[M / 4 - 1]), false, false);
    float t = __uint_as_float(r16[0]) + __uint_as_float(r16[1]);
    t += dpp_rot<0x128>(t);  // row_ror:8
    t += dpp_rot<0x124>(t);  // row_ror:4: with the step before, the four lanes of the row that share bits 0 and 1
    t = swap_add32(t);
#pragma unroll
    for (int m = 0; m < M; ++m)
        v[m] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t), (m & 3) + (M == 8 ? 16 * (m >> 2) : 0)));
}

// A lane's values of a [C][H] activation: channels c < TC, positions lane + 64 e, e < TE.  TC / TE are compile-time bounds
// (the kernels instantiate the three shapes of the 1 -> 2 -> 4 -> 4 encoder and a generic 4 x 2 fallback): a tile is 4 to 8
// registers, so the residual block's working set stays far below the 128-VGPR budget the MFMA path of the same kernel has.
template <int TC, int TE>
struct NrTile {
    float v[TC][TE];
};

// a value every lane of the wave holds alike (a staged weight read from LDS): kept in an SGPR instead of a VGPR per weight
__device__ __forceinline__ float nr_uniform(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }

template <int TC, int TE>
__device__ __forceinline__ void nr_load(const float* buf, int C, int H, int lane, NrTile<TC, TE>& t) {
#pragma unroll
    for (int c = 0; c < TC; ++c)
#pragma unroll
        for (int e = 0; e < TE; ++e) {
            const int p = lane + 64 * e;
            t.v[c][e] = (c < C && p < H) ? buf[c * H + p] : 0.0f;
        }
}
template <int TC, int TE>
__device__ __forceinline__ void nr_store(float* buf, int C, int H, int lane, const NrTile<TC, TE>& t) {
#pragma unroll
    for (int c = 0; c < TC; ++c)
#pragma unroll
        for (int e = 0; e < TE; ++e) {
            const int p = lane + 64 * e;
            if (c < C && p < H) buf[c * H + p] = t.v[c][e];
        }
}

// out[o][p] = sum_{ci,k} W[o][ci][k] * in[ci][(p*stride + k - pad) mod hin] for the lane's own output positions (IC >= cin)
template <int K, int IC, int TC, int TE>
__device__ __forceinline__ void nr_conv(const float* in, int cin, int hin, const float* W, int cout, int stride, int pad, int hout,
                                        int lane, NrTile<TC, TE>& out) {
#pragma unroll
    for (int e = 0; e < TE; ++e) {
        const int p = lane + 64 * e;
        int idx[K];
#pragma unroll
        for (int k = 0; k < K; ++k) idx[k] = wrapi((p < hout ? p : 0) * stride + k - pad, hin);
        float x[IC][K];
#pragma unroll
        for (int ci = 0; ci < IC; ++ci)
#pragma unroll
            for (int k = 0; k < K; ++k) x[ci][k] = ci < cin ? in[ci * hin + idx[k]] : 0.0f;
#pragma unroll
        for (int o = 0; o < TC; ++o) {
            float acc = 0.0f;
            if (o < cout) {
#pragma unroll
                for (int ci = 0; ci < IC; ++ci)
                    if (ci < cin) {
#pragma unroll
                        for (int k = 0; k < K; ++k) acc = fmaf(nr_uniform(W[(o * cin + ci) * K + k]), x[ci][k], acc);
                    }
            }
            out.v[o][e] = p < hout ? acc : 0.0f;
        }
    }
}

// The narrow LayerNorm centres its variance too, but keeps ONE butterfly for all channels' sums: every value is taken relative
// to the row's FIRST value (position 0 sits in lane 0: one v_readlane, wave-uniform) before the joint reduction, var = E[t^2] -
// E[t]^2 with t = y - y[0].  E[t]^2 / var is then at most H, whatever offset the row rides on (one value cannot lie further
// from the mean than sqrt(H) deviations); a second butterfly for a two-pass variance (sur_layernorm.h) would double the
// cross-lane work of a wave that has nothing to hide it behind.
__device__ __forceinline__ float nr_row_first(float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)); }

// y = LayerNorm_H(act(x)) * gamma + beta, rows = channels, statistics over the 64 lanes x TE positions
template <int TC, int TE>
__device__ __forceinline__ void nr_ln_fwd(const NrTile<TC, TE>& x, int C, int H, const float* gamma, const float* beta, bool silu,
                                          int lane, NrTile<TC, TE>& y) {
    const float inv_h = 1.0f / H;
    float a[TC][TE], st[2 * TC];
#pragma unroll
    for (int c = 0; c < TC; ++c) {
        float s = 0.0f, ss = 0.0f;
#pragma unroll
        for (int e = 0; e < TE; ++e) {
            const bool live = c < C && lane + 64 * e < H;
            const float v = x.v[c][e];
            a[c][e] = live ? (silu ? v * sigmoid_(v) : v) : 0.0f;
        }
        const float a0 = nr_row_first(a[c][0]);
#pragma unroll
        for (int e = 0; e < TE; ++e) {
            if (c < C && lane + 64 * e < H) a[c][e] -= a0;
            s += a[c][e];
            ss = fmaf(a[c][e], a[c][e], ss);
        }
        st[2 * c] = s;
        st[2 * c + 1] = ss;
    }
    nr_wave_totals(st, lane);
#pragma unroll
    for (int c = 0; c < TC; ++c) {
        const float mean = st[2 * c] * inv_h;
        const float rstd = rsqrtf(fmaxf(fmaf(-mean, mean, st[2 * c + 1] * inv_h), 0.0f) + LN_EPS);
#pragma unroll
        for (int e = 0; e < TE; ++e) {
            const int p = lane + 64 * e;
            y.v[c][e] = (c < C && p < H) ? fmaf((a[c][e] - mean) * rstd, gamma[p], beta[p]) : 0.0f;
        }
    }
}

// backward of nr_ln_fwd: dpre from dout; the lane adds its own positions' gamma / beta gradients to the wave's accumulators
template <int TC, int TE>
__device__ __forceinline__ void nr_ln_bwd(const NrTile<TC, TE>& dout, const NrTile<TC, TE>& pre, int C, int H, const float* gamma,
                                          bool silu, int lane, NrTile<TC, TE>& dpre, float* ggamma, float* gbeta) {
    const float inv_h = 1.0f / H;
    float y[TC][TE], dxh[TC][TE], st[2 * TC], rstd[TC];
#pragma unroll
    for (int c = 0; c < TC; ++c) {
        float s = 0.0f, ss = 0.0f;
#pragma unroll
        for (int e = 0; e < TE; ++e) {
            const int p = lane + 64 * e;
            const bool live = c < C && p < H;
            const float v = pre.v[c][e];
            y[c][e] = live ? (silu ? v * sigmoid_(v) : v) : 0.0f;
            dxh[c][e] = live ? dout.v[c][e] * gamma[p] : 0.0f;
        }
        const float y0 = nr_row_first(y[c][0]);
#pragma unroll
        for (int e = 0; e < TE; ++e) {
            if (c < C && lane + 64 * e < H) y[c][e] -= y0;
            s += y[c][e];
            ss = fmaf(y[c][e], y[c][e], ss);
        }
        st[2 * c] = s;
        st[2 * c + 1] = ss;
    }
    nr_wave_totals(st, lane);
#pragma unroll
    for (int c = 0; c < TC; ++c) {
        const float mean = st[2 * c] * inv_h;
        rstd[c] = rsqrtf(fmaxf(fmaf(-mean, mean, st[2 * c + 1] * inv_h), 0.0f) + LN_EPS);
        float m1 = 0.0f, m2 = 0.0f;
#pragma unroll
        for (int e = 0; e < TE; ++e) {
            const bool live = c < C && lane + 64 * e < H;
            y[c][e] = live ? (y[c][e] - mean) * rstd[c] : 0.0f;     // xhat
            m1 += dxh[c][e];
            m2 = fmaf(dxh[c][e], y[c][e], m2);
        }
        st[2 * c] = m1;
        st[2 * c + 1] = m2;
    }
    nr_wave_totals(st, lane);
    float gg[TE], gb[TE];
#pragma unroll
    for (int e = 0; e < TE; ++e) gg[e] = gb[e] = 0.0f;
#pragma unroll
    for (int c = 0; c < TC; ++c) {
        const float m1 = st[2 * c] * inv_h, m2 = st[2 * c + 1] * inv_h;
#pragma unroll
        for (int e = 0; e < TE; ++e) {
            const bool live = c < C && lane + 64 * e < H;
            float dy = rstd[c] * (dxh[c][e] - m1 - y[c][e] * m2);
            if (silu) {
                const float v = pre.v[c][e], sg = sigmoid_(v);
                dy *= sg * (1.0f + v * (1.0f - sg));
            }
            dpre.v[c][e] = live ? dy : 0.0f;
            if (live) {
                gg[e] = fmaf(dout.v[c][e], y[c][e], gg[e]);
                gb[e] += dout.v[c][e];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < TE; ++e) {
        const int p = lane + 64 * e;
        if (p < H) {
            ggamma[p] += gg[e];
            gbeta[p] += gb[e];
        }
    }
}

// gW[o][ci][k] += sum_p dout[o][p] * in[ci][(p*stride + k - pad) mod hin]   (dout [cout][hout] and in [cin][hin]: this wave's LDS)
// One 16 x 16 MFMA tile: rows = output channels (cout <= 4 of 16), columns = (ci, k) (cin * K <= 12 of 16), reduction over the
// positions four at a time.  Mostly empty, and still ~50 instructions where 64-lane reductions of every weight's partial
// products took ~700: the tile does the cross-lane summation.  hout is a multiple of 8 (enc_narrow).
template <int K>
__device__ __forceinline__ void nr_wgrad(const float* dout, const float* in, int cin, int hin, int cout, int stride, int pad, int hout,
                                         int lane, float* gW) {
    const int r = lane & 15, q = lane >> 4, ncol = cin * K;
    const bool a_ok = r < cout, b_ok = r < ncol;
    const int ci = b_ok ? r / K : 0, k = b_ok ? r - ci * K : 0;
    const float* ap = dout + (a_ok ? r : 0) * hout;
    const float* bp = in + ci * hin;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int p0 = 0; p0 < hout; p0 += 8) {
        const int pa = p0 + q, pb = p0 + 4 + q;
        const float a0 = ap[pa], b0 = bp[wrapi(pa * stride + k - pad, hin)];
        const float a1 = ap[pb], b1 = bp[wrapi(pb * stride + k - pad, hin)];
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a_ok ? a0 : 0.f, b_ok ? b0 : 0.f, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a_ok ? a1 : 0.f, b_ok ? b1 : 0.f, acc1, 0, 0, 0);
    }
    if (q == 0 && b_ok) {        // rows 0..3 of the tile live in lanes 0..15
#pragma unroll
        for (int o = 0; o < NR_C; ++o)
            if (o < cout) gW[o * ncol + r] += acc0[o] + acc1[o];
    }
}

// din[ci][j] (+)= sum_{o,k : (p*stride + k - pad) mod hin == j} W[o][ci][k] * dout[o][p]   (dout: LDS, din: own positions; OC >= cout)
template <int K, int OC, int IC, int IE>
__device__ __forceinline__ void nr_dgrad(const float* dout, int cout, int hin, const float* W, int cin, int stride, int pad, int hout,
                                         int lane, NrTile<IC, IE>& din, bool accumulate) {
#pragma unroll
    for (int e = 0; e < IE; ++e) {
        const int j = lane + 64 * e;
        const bool live = j < hin;
        float acc[IC];
#pragma unroll
        for (int ci = 0; ci < IC; ++ci) acc[ci] = accumulate ? din.v[ci][e] : 0.0f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int t = wrapi((live ? j : 0) - k + pad, hin);
            if ((t & (stride - 1)) == 0) {
                const int pp = t >> (stride - 1);
#pragma unroll
                for (int o = 0; o < OC; ++o) {
                    if (o >= cout) break;
                    const float d = dout[o * hout + pp];
#pragma unroll
                    for (int ci = 0; ci < IC; ++ci)
                        if (ci < cin) acc[ci] = fmaf(nr_uniform(W[(o * cin + ci) * K + k]), d, acc[ci]);
                }
            }
        }
#pragma unroll
        for (int ci = 0; ci < IC; ++ci) din.v[ci][e] = (ci < cin && live) ? acc[ci] : 0.0f;
    }
}

// floats of one wave's LDS region
__host__ __device__ inline int nr_fwd_wave_floats(int cin, int hin, int cout, int hout) { return cin * hin + 7 * cout * hout; }
__host__ __device__ inline int nr_bwd_wave_floats(int cin, int hin, int cout, int hout, int psize_blk) {
    return cin * hin + 6 * cout * hout + ((psize_blk + 3) & ~3);   // in | a1pre a1 a2pre | s | dout | gbuf | gradient accumulators
}

// forward of one block for one sample: `wl` = this wave's LDS region; record layout skip | a1pre | a1 | a2pre | a2 | s | out
template <int IC, int TC, int TE>
__device__ __forceinline__ void nr_block_forward_t(int cin, int hin, int cout, int hout, int stride, const float* const* w, float* wl,
                                                   const float* __restrict__ src, float* __restrict__ rec_out, float* __restrict__ z,
                                                   int lane) {
    typedef NrTile<TC, TE> T;
    const int a = cout * hout, nin = cin * hin;
    float* in = wl;
    float* skip = in + nin;
    float *a1pre = skip + a, *a1 = skip + 2 * a, *a2pre = skip + 3 * a, *a2 = skip + 4 * a, *sb = skip + 5 * a, *out = skip + 6 * a;
    for (int i = lane; i < nin; i += 64) in[i] = src[i];
    NR_WAVE_SYNC();
    T t_skip, t_pre, t_act;
    nr_conv<1, IC>(in, cin, hin, w[SUR_RB_SKIP], cout, stride, 0, hout, lane, t_skip);
    nr_conv<3, IC>(in, cin, hin, w[SUR_RB_CONV1], cout, stride, 1, hout, lane, t_pre);
    nr_store(skip, cout, hout, lane, t_skip);
    nr_store(a1pre, cout, hout, lane, t_pre);
    nr_ln_fwd(t_pre, cout, hout, w[SUR_RB_LN1_W], w[SUR_RB_LN1_B], true, lane, t_act);
    nr_store(a1, cout, hout, lane, t_act);
    NR_WAVE_SYNC();
    nr_conv<3, TC>(a1, cout, hout, w[SUR_RB_CONV2], cout, 1, 1, hout, lane, t_pre);
    nr_store(a2pre, cout, hout, lane, t_pre);
    nr_ln_fwd(t_pre, cout, hout, w[SUR_RB_LN2_W], w[SUR_RB_LN2_B], true, lane, t_act);
    nr_store(a2, cout, hout, lane, t_act);
#pragma unroll
    for (int c = 0; c < TC; ++c)
#pragma unroll
        for (int e = 0; e < TE; ++e) t_act.v[c][e] += t_skip.v[c][e];
    nr_store(sb, cout, hout, lane, t_act);
    nr_ln_fwd(t_act, cout, hout, w[SUR_RB_LN3_W], w[SUR_RB_LN3_B], false, lane, t_pre);
    nr_store(out, cout, hout, lane, t_pre);
    NR_WAVE_SYNC();
    for (int i = lane; i < (7 * a) >> 2; i += 64) reinterpret_cast<float4*>(rec_out)[i] = reinterpret_cast<const float4*>(skip)[i];
    if (z)
        for (int i = lane; i < a; i += 64) z[i] = out[i];
    NR_WAVE_SYNC();      // the region is reused by this wave's next sample
}

__device__ __forceinline__ void nr_block_forward(int cin, int hin, int cout, int hout, int stride, const float* const* w, float* wl,
                                                 const float* __restrict__ src, float* __restrict__ rec_out, float* __restrict__ z, int lane) {
    if (cin <= 1 && cout <= 2) nr_block_forward_t<1, 2, 2>(cin, hin, cout, hout, stride, w, wl, src, rec_out, z, lane);
    else nr_block_forward_t<4, 4, 1>(cin, hin, cout, hout, stride, w, wl, src, rec_out, z, lane);      // hout <= 64 (enc_narrow)
}

// backward of one block for one sample; g[] = this wave's gradient accumulators (LDS)
template <int TC, int TE, int IC, int IE>
__device__ __forceinline__ void nr_block_backward_t(int cin, int hin, int cout, int hout, int stride, const float* const* w, float* const* g,
                                                    float* wl, const float* __restrict__ in_src, const float* __restrict__ rec_blk,
                                                    const float* __restrict__ dsrc, float* __restrict__ din_dst, bool need_din, int lane) {
    typedef NrTile<TC, TE> T;
    const int a = cout * hout, nin = cin * hin;
    float* in = wl;
    float* a1pre = in + nin;
    float *a1 = a1pre + a, *a2pre = a1pre + 2 * a, *sb = a1pre + 3 * a, *dout = a1pre + 4 * a, *gbuf = a1pre + 5 * a;
    for (int i = lane; i < nin; i += 64) in[i] = in_src[i];
    for (int i = lane; i < 3 * a; i += 64) a1pre[i] = rec_blk[a + i];            // a1pre | a1 | a2pre
    for (int i = lane; i < a; i += 64) {
        sb[i] = rec_blk[5 * a + i];
        dout[i] = dsrc[i];
    }
    NR_WAVE_SYNC();
    T t_d, t_x, t_g;
    NrTile<IC, IE> t_din;
    nr_load(dout, cout, hout, lane, t_d);
    nr_load(sb, cout, hout, lane, t_x);
    nr_ln_bwd(t_d, t_x, cout, hout, w[SUR_RB_LN3_W], false, lane, t_g, g[SUR_RB_LN3_W], g[SUR_RB_LN3_B]);       // g1
    nr_store(gbuf, cout, hout, lane, t_g);
    NR_WAVE_SYNC();
    nr_wgrad<1>(gbuf, in, cin, hin, cout, stride, 0, hout, lane, g[SUR_RB_SKIP]);
    if (need_din) nr_dgrad<1, TC>(gbuf, cout, hin, w[SUR_RB_SKIP], cin, stride, 0, hout, lane, t_din, false);
    nr_load(a2pre, cout, hout, lane, t_x);
    nr_ln_bwd(t_g, t_x, cout, hout, w[SUR_RB_LN2_W], true, lane, t_d, g[SUR_RB_LN2_W], g[SUR_RB_LN2_B]);         // g2 (in t_d)
    NR_WAVE_SYNC();       // every lane has read g1 from gbuf
    nr_store(gbuf, cout, hout, lane, t_d);
    NR_WAVE_SYNC();
    nr_wgrad<3>(gbuf, a1, cout, hout, cout, 1, 1, hout, lane, g[SUR_RB_CONV2]);
    nr_dgrad<3, TC>(gbuf, cout, hout, w[SUR_RB_CONV2], cout, 1, 1, hout, lane, t_g, false);                        // g3 (in t_g)
    nr_load(a1pre, cout, hout, lane, t_x);
    nr_ln_bwd(t_g, t_x, cout, hout, w[SUR_RB_LN1_W], true, lane, t_d, g[SUR_RB_LN1_W], g[SUR_RB_LN1_B]);         // g1' (in t_d)
    NR_WAVE_SYNC();
    nr_store(gbuf, cout, hout, lane, t_d);
    NR_WAVE_SYNC();
    nr_wgrad<3>(gbuf, in, cin, hin, cout, stride, 1, hout, lane, g[SUR_RB_CONV1]);
    if (need_din) {
        nr_dgrad<3, TC>(gbuf, cout, hin, w[SUR_RB_CONV1], cin, stride, 1, hout, lane, t_din, true);
#pragma unroll
        for (int c = 0; c < IC; ++c)
#pragma unroll
            for (int e = 0; e < IE; ++e) {
                const int j = lane + 64 * e;
                if (c < cin && j < hin) din_dst[c * hin + j] = t_din.v[c][e];
            }
    }
    NR_WAVE_SYNC();
}

__device__ __forceinline__ void nr_block_backward(int cin, int hin, int cout, int hout, int stride, const float* const* w, float* const* g,
                                                  float* wl, const float* __restrict__ in_src, const float* __restrict__ rec_blk,
                                                  const float* __restrict__ dsrc, float* __restrict__ din_dst, bool need_din, int lane) {
    // the three shapes of the 1 -> 2 -> 4 -> 4 encoder (N <= 256); enc_narrow() admits nothing else
    if (!need_din && cin <= 1 && cout <= 2)
        nr_block_backward_t<2, 2, 1, 1>(cin, hin, cout, hout, stride, w, g, wl, in_src, rec_blk, dsrc, din_dst, false, lane);
    else if (hout <= 64 && cin <= 2 && hin <= 128)
        nr_block_backward_t<4, 1, 2, 2>(cin, hin, cout, hout, stride, w, g, wl, in_src, rec_blk, dsrc, din_dst, need_din, lane);
    else      // hout <= 64, hin <= 64 (enc_narrow)
        nr_block_backward_t<4, 1, 4, 1>(cin, hin, cout, hout, stride, w, g, wl, in_src, rec_blk, dsrc, din_dst, need_din, lane);
}

}  // namespace

#endif  // SUR_NARROW_H
