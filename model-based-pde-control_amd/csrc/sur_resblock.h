// sur_resblock.h -- the wide (MFMA) residual block on LDS-resident activations: RBBuf, rb_forward, rb_backward.
// Needs sur_gemm.h, sur_layernorm.h and the SUR_RB_* parameter order of surrogate_hip.h.
#ifndef SUR_RESBLOCK_H
#define SUR_RESBLOCK_H

#include "../../include/surrogate_hip.h"
#include "sur_gemm.h"
#include "sur_layernorm.h"

namespace {

// ---------------------------------------------------------------------------------------------
// encoder: three residual blocks
// ---------------------------------------------------------------------------------------------
struct RBBuf {  // LDS pointers of one block's forward intermediates
    float *in, *skip, *a1pre, *a1, *a2pre, *a2, *s, *out;
    int cin, cout, hin, hout, stride;
};

__device__ void rb_forward(const RBBuf& b, const float* const* w) {
    conv_fwd<1>(b.in, b.cin, b.hin, w[SUR_RB_SKIP], nullptr, b.cout, b.stride, 0, b.skip, false, lower_half(), false);
    conv_fwd<3>(b.in, b.cin, b.hin, w[SUR_RB_CONV1], nullptr, b.cout, b.stride, 1, b.a1pre, false, upper_half(), true);
    act_ln_fwd(b.a1pre, b.cout, b.hout, w[SUR_RB_LN1_W], w[SUR_RB_LN1_B], true, b.a1);
    conv_fwd<3>(b.a1, b.cout, b.hout, w[SUR_RB_CONV2], nullptr, b.cout, 1, 1, b.a2pre, false);
    act_ln_fwd(b.a2pre, b.cout, b.hout, w[SUR_RB_LN2_W], w[SUR_RB_LN2_B], true, b.a2);
    const int n = b.cout * b.hout;
    for (int i = threadIdx.x; i < n; i += blockDim.x) b.s[i] = b.a2[i] + b.skip[i];
    __syncthreads();
    act_ln_fwd(b.s, b.cout, b.hout, w[SUR_RB_LN3_W], w[SUR_RB_LN3_B], false, b.out);
}

// dout [cout][hout] -> din [cin][hin]; g1, g2, g3, xh: scratch of cout*hout floats each
// need_din = false (the encoder's first block: its input is data): the two data-gradient GEMMs onto the block input are
// skipped -- with cin = 1 they fill one row of every 16-row MFMA tile and were the longest phase of that block.
template <class GP>
__device__ void rb_backward(const RBBuf& b, const float* const* w, const GP* g, const float* dout, float* din,
                            float* g1, float* g2, float* g3, float* xh, int sb = -1, bool need_din = true) {
#ifdef SUR_STAMP
#define RB_STAMP(i) do { if (sb >= 0) STAMP(sb + (i)); } while (0)
#else
#define RB_STAMP(i) do { } while (0)
#endif
    act_ln_bwd(dout, b.s, b.cout, b.hout, w[SUR_RB_LN3_W], false, g1, xh, g[SUR_RB_LN3_W], g[SUR_RB_LN3_B]);
    RB_STAMP(0);
    // skip path
    if (need_din) {
        conv_bwd_weight<1>(g1, b.cout, b.in, b.cin, b.hin, b.stride, 0, g[SUR_RB_SKIP], GP(nullptr), lower_half(), false);
        conv_bwd_data<1>(g1, b.cout, b.hin, w[SUR_RB_SKIP], b.cin, b.stride, 0, din, false, upper_half(), true);
    } else {
        conv_bwd_weight<1>(g1, b.cout, b.in, b.cin, b.hin, b.stride, 0, g[SUR_RB_SKIP], GP(nullptr), all_waves(), false);
        // no barrier: the next phase reads g1 / a2pre and writes g2, xh and the LayerNorm accumulators only
    }
    RB_STAMP(1);
    // residual path
    act_ln_bwd(g1, b.a2pre, b.cout, b.hout, w[SUR_RB_LN2_W], true, g2, xh, g[SUR_RB_LN2_W], g[SUR_RB_LN2_B]);
    RB_STAMP(2);
    conv_bwd_weight<3>(g2, b.cout, b.a1, b.cout, b.hout, 1, 1, g[SUR_RB_CONV2], GP(nullptr), lower_half(), false);
    conv_bwd_data<3>(g2, b.cout, b.hout, w[SUR_RB_CONV2], b.cout, 1, 1, g3, false, upper_half(), true);
    RB_STAMP(3);
    act_ln_bwd(g3, b.a1pre, b.cout, b.hout, w[SUR_RB_LN1_W], true, g1, xh, g[SUR_RB_LN1_W], g[SUR_RB_LN1_B]);
    RB_STAMP(4);
    if (need_din) {
        conv_bwd_weight<3>(g1, b.cout, b.in, b.cin, b.hin, b.stride, 1, g[SUR_RB_CONV1], GP(nullptr), lower_half(), false);
        conv_bwd_data<3>(g1, b.cout, b.hin, w[SUR_RB_CONV1], b.cin, b.stride, 1, din, true, upper_half(), true);
    } else {
        conv_bwd_weight<3>(g1, b.cout, b.in, b.cin, b.hin, b.stride, 1, g[SUR_RB_CONV1], GP(nullptr), all_waves(), true);
    }
    RB_STAMP(5);
#undef RB_STAMP
}

}  // namespace

#endif  // SUR_RESBLOCK_H
