// sur_layernorm.h -- LayerNorm over the spatial axis fused with the preceding activation, forward and backward (act_ln_fwd,
// act_ln_bwd), and LN_MAX_EPL, the row width they support.  Needs sur_common.h.
#ifndef SUR_LAYERNORM_H
#define SUR_LAYERNORM_H

#include "sur_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// LayerNorm over the spatial axis fused with the preceding activation.  A channel is handled by a
// group of LPC = min(64, H) lanes (64/LPC channels per wavefront at a time), each lane keeping its
// H/LPC activated values in registers; sums go through DPP row rotations inside 16-lane rows and one
// lane swap per doubling beyond a row (group_sum1 / group_sum2).
// The variance is TWO-PASS: the mean first, then E[(y - mean)^2] from the registers the values sit in; the centred
// values are the ones the normalisation needs anyway, so this costs no instruction over var = E[y^2] - mean^2 from one
// joint reduction, only the second reduction's latency.  That one-pass form loses mean^2 / var ulps to its
// cancellation: a row riding on an offset (a state on a constant background through the bias-free encoder blocks, a
// decoder bias in front of SiLU) came out 1e-2 of scale wrong ("The LayerNorm variance is centred").
// Forward and backward take the statistics in the same way, so the recomputing and the saved-activation backward see
// the same bits.
// ---------------------------------------------------------------------------------------------
constexpr int LN_MAX_EPL = 4;  // H <= 256

// out = LayerNorm_H(act(pre)) * gamma[p] + beta[p], act = SiLU or identity
__device__ void act_ln_fwd(const float* pre, int C, int H, const float* gamma, const float* beta, bool silu,
                           float* out) {
    const int lpc = H < 64 ? H : 64, gpw = 64 / lpc, epl = H / lpc;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int grp = lane / lpc, gl = lane - grp * lpc;
    const float inv_h = 1.0f / H;
    for (int c0 = 0; c0 < C; c0 += nw * gpw) {
        const int c = c0 + wave * gpw + grp;
        const bool live = c < C;
        const float* x = pre + (live ? c : 0) * H;
        float y[LN_MAX_EPL];
        float s = 0.0f, ss = 0.0f;
#pragma unroll
        for (int e = 0; e < LN_MAX_EPL; ++e) {
            if (e < epl) {
                const float v = x[gl + e * lpc];
                y[e] = silu ? v * sigmoid_(v) : v;
            }
        }
#pragma unroll
        for (int e = 0; e < LN_MAX_EPL; ++e)
            if (e < epl) s += y[e];
        group_sum1(s, lpc);
        const float mean = s * inv_h;
#pragma unroll
        for (int e = 0; e < LN_MAX_EPL; ++e) {
            if (e < epl) {
                y[e] -= mean;
                ss = fmaf(y[e], y[e], ss);
            }
        }
        group_sum1(ss, lpc);
        const float rstd = rsqrtf(ss * inv_h + LN_EPS);
        if (live) {
#pragma unroll
            for (int e = 0; e < LN_MAX_EPL; ++e) {
                if (e < epl) {
                    const int p = gl + e * lpc;
                    out[c * H + p] = fmaf(y[e] * rstd, gamma[p], beta[p]);
                }
            }
        }
    }
    __syncthreads();
}

// backward of act_ln_fwd: dpre from dout; accumulates ggamma / gbeta.  xhat_scratch: [C][H] work space.
template <class GP>
__device__ void act_ln_bwd(const float* dout, const float* pre, int C, int H, const float* gamma, bool silu,
                           float* dpre, float* xhat_scratch, GP ggamma, GP gbeta) {
    const int lpc = H < 64 ? H : 64, gpw = 64 / lpc, epl = H / lpc;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int grp = lane / lpc, gl = lane - grp * lpc;
    const float inv_h = 1.0f / H;
    for (int c0 = 0; c0 < C; c0 += nw * gpw) {
        const int c = c0 + wave * gpw + grp;
        const bool live = c < C;
        const int cc = live ? c : 0;
        const float* x = pre + cc * H;
        float y[LN_MAX_EPL], v_[LN_MAX_EPL], dxh[LN_MAX_EPL];
        float s = 0.0f, ss = 0.0f;
#pragma unroll
        for (int e = 0; e < LN_MAX_EPL; ++e) {
            if (e < epl) {
                const int p = gl + e * lpc;
                v_[e] = x[p];
                y[e] = silu ? v_[e] * sigmoid_(v_[e]) : v_[e];
                dxh[e] = dout[cc * H + p] * gamma[p];
            }
        }
#pragma unroll
        for (int e = 0; e < LN_MAX_EPL; ++e)
            if (e < epl) s += y[e];
        group_sum1(s, lpc);
        const float mean = s * inv_h;
#pragma unroll
        for (int e = 0; e < LN_MAX_EPL; ++e) {
            if (e < epl) {
                y[e] -= mean;
                ss = fmaf(y[e], y[e], ss);
            }
        }
        group_sum1(ss, lpc);
        const float rstd = rsqrtf(ss * inv_h + LN_EPS);
        float m1 = 0.0f, m2 = 0.0f;
#pragma unroll
        for (int e = 0; e < LN_MAX_EPL; ++e) {
            if (e < epl) {
                y[e] *= rstd;  // xhat
                m1 += dxh[e];
                m2 = fmaf(dxh[e], y[e], m2);
            }
        }
        group_sum2(m1, m2, lpc);
        m1 *= inv_h;
        m2 *= inv_h;
        if (live) {
#pragma unroll
            for (int e = 0; e < LN_MAX_EPL; ++e) {
                if (e < epl) {
                    const int p = gl + e * lpc;
                    float dy = rstd * (dxh[e] - m1 - y[e] * m2);
                    if (silu) {
                        const float sg = sigmoid_(v_[e]);
                        dy *= sg * (1.0f + v_[e] * (1.0f - sg));
                    }
                    xhat_scratch[c * H + p] = y[e];
                    dpre[c * H + p] = dy;
                }
            }
        }
    }
    __syncthreads();
    for (int p = threadIdx.x; p < H; p += blockDim.x) {
        float gg0 = 0.0f, gg1 = 0.0f, gb0 = 0.0f, gb1 = 0.0f;
        int c = 0;
        for (; c + 2 <= C; c += 2) {
            const float d0 = dout[c * H + p], d1 = dout[(c + 1) * H + p];
            gg0 = fmaf(d0, xhat_scratch[c * H + p], gg0);
            gg1 = fmaf(d1, xhat_scratch[(c + 1) * H + p], gg1);
            gb0 += d0;
            gb1 += d1;
        }
        for (; c < C; ++c) {
            const float d0 = dout[c * H + p];
            gg0 = fmaf(d0, xhat_scratch[c * H + p], gg0);
            gb0 += d0;
        }
        ggamma[p] += gg0 + gg1;
        gbeta[p] += gb0 + gb1;
    }
    __syncthreads();
}

}  // namespace

#endif  // SUR_LAYERNORM_H
