// sur_cell.h -- the device functions of one TBPTT step: StepLayout, the sizes of a step's saved record, cell_forward*,
// decoder_forward / decoder_backward, cell_dh_gemm, cell_wgrad_gemms.  The kernels that run them are sur_chunk.h's.
// Needs sur_gemm.h, sur_layernorm.h and surrogate_hip.h.
#ifndef SUR_CELL_H
#define SUR_CELL_H

#include "../../include/surrogate_hip.h"
#include "sur_gemm.h"
#include "sur_layernorm.h"

namespace {

// ---------------------------------------------------------------------------------------------
// One step of a TBPTT chunk: the ConvLSTM cell and the decoder as device functions on LDS-resident activations.  No
// kernel here and no time loop: the cell chain kernels of sur_chunk.h carry the recurrence, its (step, sample)-parallel
// kernels everything else.
// ---------------------------------------------------------------------------------------------
struct StepLayout {
    float *x, *h, *c, *gates, *cnew, *hnew, *p0, *a0, *p1, *a1, *p2, *a2, *d, *outv;
    // backward only
    float *dgates, *dh, *gA, *gB, *xh, *dx, *dhin, *dh_carry, *dc_carry, *dout_carry;
    float* end;
    int n;  // N = 4*hq
};

__host__ __device__ inline int step_max_act(const sur_chunk_params& p) {
    const int a = p.cs * 2 * p.hq, b = p.c_mid * 4 * p.hq;
    return a > b ? a : b;
}

// Floats of one step's forward intermediates as the forward kernel can save them for the backward kernel:
// the LDS block [gates .. a2] (activated gates, c_k, h_k, decoder pre-/post-LayerNorm activations), padded to
// whole 1 KiB pieces because the backward kernel fetches it by LDS-DMA (one wave instruction = 64 x 16 B).
constexpr int DMA_PIECE = 256;  // floats per global_load_lds_dwordx4 wave instruction
__host__ __device__ inline int step_block_floats(const sur_chunk_params& p) {
    const int s = p.cs * p.hq, n = 4 * p.hq;
    return 6 * s + 2 * p.cs * 2 * p.hq + 2 * p.c_mid * n + 2 * n;
}
__host__ __device__ inline int step_saved_floats(const sur_chunk_params& p) {
    return (step_block_floats(p) + DMA_PIECE - 1) / DMA_PIECE * DMA_PIECE;
}

// ConvLSTM cell with the gate non-linearities in the GEMM epilogue (4 * T waves, cs = 16): wave group w = wave & 3 owns
// channels 4w .. 4w+3 and its 16 tile rows are (channel, gate) pairs, so after the K loop lane (q, n) holds the four gate
// pre-activations of channel 4w+q at position n in its four accumulator registers -- i, f, g, o, c' and h' are finished
// in registers: no second pass over LDS, one barrier per step instead of two.  The hq / 16 column tiles are spread over
// the T = blockDim / 256 wave sets (the chain runs ONE workgroup per sample on a quarter of the CUs: at hq = 64 sixteen
// waves finish the recurrent step's GEMM in one tile each instead of four in a row).
template <int NSETS>
__device__ void cell_forward_fused(const sur_chunk_params& p, const StepLayout& L, const float* const* w) {
    const int s = p.cs * p.hq, hq = p.hq, ca = p.ca, cs = p.cs;
    const int lane = threadIdx.x & 63, wave = (threadIdx.x >> 6) & 3, tset = NSETS > 1 ? threadIdx.x >> 8 : 0;
    constexpr int nsets = NSETS;
    const int r = lane & 15, q = lane >> 4;
    const int gate_stride = (int)(w[SUR_ST_WXF] - w[SUR_ST_WXI]);
    const int gate_r = r & 3, ch_r = 4 * wave + (r >> 2);                 // identity of this lane's A row
    const float* ax = w[SUR_ST_WXI] + gate_r * gate_stride + ch_r * (ca * 3);   // W_g[(o*cin + ci)*3 + tap]
    const float* ah = w[SUR_ST_WHI] + gate_r * gate_stride + ch_r * (cs * 3);
    const int ch = 4 * wave + q;                                           // channel of this lane's accumulators
    const float bi = w[SUR_ST_BXI][ch], bf = (w[SUR_ST_BXI] + gate_stride)[ch], bc = (w[SUR_ST_BXI] + 2 * gate_stride)[ch],
                bo = (w[SUR_ST_BXI] + 3 * gate_stride)[ch];
    for (int n0 = 16 * tset; n0 < hq; n0 += 16 * nsets) {
        const int n = n0 + r;
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tap = 0; tap < 3; ++tap) {
            const int col = wrapi((n < hq ? n : 0) + tap - 1, hq);
            {   // latent action channels (ca <= 4: one K step)
                const bool ok = q < ca;
                const float a = ax[(ok ? q : 0) * 3 + tap], bv = L.x[(ok ? q : 0) * hq + col];
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ok ? a : 0.f, ok ? bv : 0.f, acc0, 0, 0, 0);
            }
#pragma unroll
            for (int c0 = 0; c0 < 16; c0 += 8) {   // hidden channels (cs = 16): two independent accumulators
                const float a0 = ah[(c0 + q) * 3 + tap], b0 = L.h[(c0 + q) * hq + col];
                const float a1 = ah[(c0 + 4 + q) * 3 + tap], b1 = L.h[(c0 + 4 + q) * hq + col];
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc1, 0, 0, 0);
            }
        }
        if (n < hq) {
            const int idx = ch * hq + n;
            const float gi = sigmoid_(acc0[0] + acc1[0] + bi), gf = sigmoid_(acc0[1] + acc1[1] + bf),
                        gg = tanh_(acc0[2] + acc1[2] + bc), go = sigmoid_(acc0[3] + acc1[3] + bo);
            L.gates[idx] = gi;
            L.gates[s + idx] = gf;
            L.gates[2 * s + idx] = gg;
            L.gates[3 * s + idx] = go;
            const float cn = fmaf(gf, L.c[idx], gi * gg);
            L.cnew[idx] = cn;
            L.hnew[idx] = go * tanh_(cn);
        }
    }
    __syncthreads();
}

// ConvLSTM cell on LDS-resident x, h, c: fills gates (activated), cnew, hnew.  BLOCK = blockDim.x when it is known at
// compile time (the chain kernels), 0 otherwise.
template <int BLOCK = 0>
__device__ void cell_forward(const sur_chunk_params& p, const StepLayout& L, const float* const* w) {
    const int s = p.cs * p.hq;
    if constexpr (BLOCK >= 256 && (BLOCK & 255) == 0) {
        if (p.cs == 16 && p.ca <= 4) {
            cell_forward_fused<BLOCK / 256>(p, L, w);
            return;
        }
    } else {
        if (blockDim.x == 256 && p.cs == 16 && p.ca <= 4) {
            cell_forward_fused<1>(p, L, w);
            return;
        }
    }
    STAMP(0);
    // all four gates' pre-activations in ONE gather-GEMM: rows = (gate, channel), K = 3*(ca + cs).
    // The four gates' weights are consecutive in the LDS copy (Wx_g, b_g, Wh_g per gate), so the
    // row stride between gates is constant.
    {
        const int gate_stride = (int)(w[SUR_ST_WXF] - w[SUR_ST_WXI]);
        const GemmSeg seg[2] = {{w[SUR_ST_WXI], p.ca * 3, 3, L.x, p.hq, p.ca}, {w[SUR_ST_WHI], p.cs * 3, 3, L.h, p.hq, p.cs}};
        const int cs = p.cs, hq = p.hq, ca = p.ca;
        // row m = g*cs + o lives at gate g's weight block: fold the gate offset into a_sm arithmetic by
        // running one GEMM per gate tile row-block (cs is a multiple of 16 for this model family)
        const int nwg = blockDim.x >> 6;
        for (int g = 0; g < 4; ++g) {
            const GemmSeg sg[2] = {{seg[0].a + g * gate_stride, ca * 3, 3, L.x, hq, ca},
                                   {seg[1].a + g * gate_stride, cs * 3, 3, L.h, hq, cs}};
            const float* bias = w[SUR_ST_BXI] + g * gate_stride;
            float* outg = L.gates + g * s;
            // gate g on its own wave quarter (all waves if the workgroup has fewer than 4)
            const WaveSet ws = nwg >= 4 ? WaveSet{g * (nwg / 4), nwg / 4} : WaveSet{0, nwg};
            gemm_taps<3, 2>(ws, false, cs, hq, sg, [&](int, int tap, int n) { return wrapi(n + tap - 1, hq); },
                            [&](int m, int n, float v) {
                                if (m < cs) outg[m * hq + n] = v + bias[m];
                            });
        }
        __syncthreads();
    }
    STAMP(1);
    for (int i = threadIdx.x; i < s; i += blockDim.x) {
        const float gi = sigmoid_(L.gates[i]), gf = sigmoid_(L.gates[s + i]), gg = tanh_(L.gates[2 * s + i]),
                    go = sigmoid_(L.gates[3 * s + i]);
        L.gates[i] = gi;
        L.gates[s + i] = gf;
        L.gates[2 * s + i] = gg;
        L.gates[3 * s + i] = go;
        const float cn = fmaf(gf, L.c[i], gi * gg);
        L.cnew[i] = cn;
        L.hnew[i] = go * tanh_(cn);
    }
    __syncthreads();
    STAMP(2);
}

// state decoder on LDS-resident hnew: fills p0, a0, p1, a1, p2, a2 and d
__device__ void decoder_forward(const sur_chunk_params& p, const StepLayout& L, const float* const* w) {
    deconv_fwd(L.hnew, p.cs, p.hq, w[SUR_ST_DC0_W], w[SUR_ST_DC0_B], p.cs, L.p0);
    STAMP(3);
    act_ln_fwd(L.p0, p.cs, 2 * p.hq, w[SUR_ST_LN0_W], w[SUR_ST_LN0_B], true, L.a0);
    STAMP(4);
    deconv_fwd(L.a0, p.cs, 2 * p.hq, w[SUR_ST_DC1_W], w[SUR_ST_DC1_B], p.c_mid, L.p1);
    STAMP(5);
    act_ln_fwd(L.p1, p.c_mid, L.n, w[SUR_ST_LN1_W], w[SUR_ST_LN1_B], true, L.a1);
    STAMP(6);
    conv_fwd<7>(L.a1, p.c_mid, L.n, w[SUR_ST_CV2_W], w[SUR_ST_CV2_B], 1, 1, 3, L.p2, false);
    STAMP(7);
    act_ln_fwd(L.p2, 1, L.n, w[SUR_ST_LN2_W], w[SUR_ST_LN2_B], true, L.a2);
    STAMP(8);
    conv_fwd<5>(L.a2, 1, L.n, w[SUR_ST_CV3_W], w[SUR_ST_CV3_B], 1, 1, 2, L.d, false);
    STAMP(9);
}

// decoder backward on LDS-resident activations: L.gA holds d loss / d d on entry, L.dh the gradient wrt hnew on exit.
// LDS is what limits the (step, sample)-parallel kernel's residency at N = 256, so nothing is allocated that a dead buffer
// can serve (dec_bwd_kernel lays the buffers out): the LayerNorm backward's normalised-activation scratch lives in the
// post-LayerNorm activation that was consumed just before (a2 for the last norm, a1 -- dead after the 7-tap weight
// gradient -- for the other two), L.dh aliases L.gB, and two activations arrive LATE from registers: p0 into p1's
// buffer once the middle norm's backward has read p1 (`late_p0`), h into a0's buffer once the second transposed
// convolution's weight gradient has read a0 (`late_h`).  Each is stored right after a barrier that retires the old
// contents and at least one barrier before its first reader.
template <class GP, typename StoreP0, typename StoreH>
__device__ void decoder_backward(const sur_chunk_params& p, const StepLayout& L, const float* const* w, const GP* g,
                                 StoreP0 late_p0, StoreH late_h) {
    const int n = L.n;
    // single-channel gradients fill the first n floats of gA: the rest of the buffer is the weight gradients' scratch
    float* const wg_scratch = L.gA + n;
    const int wg_floats = step_max_act(p) - n;
    conv_bwd_weight<5>(L.gA, 1, L.a2, 1, n, 1, 2, g[SUR_ST_CV3_W], g[SUR_ST_CV3_B], all_waves(), false, wg_scratch, wg_floats);
    STAMP(12);
    conv_bwd_data<5>(L.gA, 1, n, w[SUR_ST_CV3_W], 1, 1, 2, L.gB, false);
    STAMP(13);
    act_ln_bwd(L.gB, L.p2, 1, n, w[SUR_ST_LN2_W], true, L.gA, L.a2, g[SUR_ST_LN2_W], g[SUR_ST_LN2_B]);
    STAMP(14);
    conv_bwd_weight<7>(L.gA, 1, L.a1, p.c_mid, n, 1, 3, g[SUR_ST_CV2_W], g[SUR_ST_CV2_B], all_waves(), false, wg_scratch, wg_floats);
    STAMP(15);
    conv_bwd_data<7>(L.gA, 1, n, w[SUR_ST_CV2_W], p.c_mid, 1, 3, L.gB, false);
    STAMP(16);
    act_ln_bwd(L.gB, L.p1, p.c_mid, n, w[SUR_ST_LN1_W], true, L.gA, L.a1, g[SUR_ST_LN1_W], g[SUR_ST_LN1_B]);
    STAMP(17);
    late_p0();      // p1 is dead (act_ln_bwd ends with a barrier); first reader: the act_ln_bwd two barriers below
    deconv_bwd_weight(L.gA, p.c_mid, L.a0, p.cs, 2 * p.hq, g[SUR_ST_DC1_W], g[SUR_ST_DC1_B], lower_half(), false);
    STAMP(18);
    deconv_bwd_data(L.gA, p.c_mid, 2 * p.hq, w[SUR_ST_DC1_W], p.cs, L.gB, upper_half(), true);
    STAMP(19);
    late_h();       // a0 is dead; first reader: deconv_bwd_weight below, behind act_ln_bwd's barrier
    act_ln_bwd(L.gB, L.p0, p.cs, 2 * p.hq, w[SUR_ST_LN0_W], true, L.gA, L.a1, g[SUR_ST_LN0_W], g[SUR_ST_LN0_B]);
    STAMP(26);
    deconv_bwd_weight(L.gA, p.cs, L.hnew, p.cs, p.hq, g[SUR_ST_DC0_W], g[SUR_ST_DC0_B], lower_half(), false);
    STAMP(27);
    deconv_bwd_data(L.gA, p.cs, p.hq, w[SUR_ST_DC0_W], p.cs, L.dh, upper_half(), true);

}

// Cell backward, recurrent part: dh_in [cs][hq] = sum_g Wh_g^T * dG_g.  The K = 4 * cs * 3 contraction is split by gate
// over the wave quarters (each writes its partial tile to part[g]); the caller adds the four partials.
__device__ void cell_dh_gemm(const sur_chunk_params& p, const StepLayout& L, const float* const* w, float* part) {
    const int s = p.cs * p.hq, nwg = blockDim.x >> 6, cs = p.cs, hq = p.hq;
    const int gate_stride = (int)(w[SUR_ST_WXF] - w[SUR_ST_WXI]);
    auto tap_col = [&](int, int tap, int j) { return wrapi(j - tap + 1, hq); };  // stride 1, pad 1
    const float* wh = w[SUR_ST_WHI];
    for (int gt = 0; gt < 4; ++gt) {   // A[m=ci][c=o][tap] = W_g[(o*cin + ci)*3 + tap];  B = dG_g[o][col]
        const GemmSeg sh[1] = {{wh + gt * gate_stride, 3, cs * 3, L.dgates + gt * s, hq, cs}};
        float* dst = part + gt * s;
        const WaveSet ws = nwg >= 4 ? WaveSet{gt * (nwg / 4), nwg / 4} : all_waves();
        gemm_taps<3, 1>(ws, false, cs, hq, sh, tap_col, [&](int m, int j, float v) {
            if (m < cs) dst[m * hq + j] = v;
        });
    }
    __syncthreads();
}

// Cell backward, non-recurrent part for one (step, sample): dx [ca][hq] = sum_g Wx_g^T * dG_g and the LSTM weight /
// bias gradients dG_g x {x, h_in}.  dx on the first wave, the weight-gradient tiles on the others.
// `hs`: floats between consecutive rows of L.x, L.h and L.dgates (>= hq).  With hs = hq = 64 the sixteen tile rows a GEMM operand
// is gathered from start in the same LDS bank (SQ_LDS_BANK_CONFLICT was 79 % of the LDS-active cycles of this kernel);
// hs = hq + 4 staggers them by four banks and keeps rows 16-byte aligned.
template <class GP>
__device__ void cell_wgrad_gemms(const sur_chunk_params& p, const StepLayout& L, const float* const* w, const GP* g, int hs) {
    const int s = p.cs * hs, nwg = blockDim.x >> 6, cs = p.cs, ca = p.ca, hq = p.hq;
    const int gate_stride = (int)(w[SUR_ST_WXF] - w[SUR_ST_WXI]);     // between the gates' Wx as staged (cell_wgrad_kernel: back to back)
    const int ggate_stride = (int)(g[SUR_ST_WXF] - g[SUR_ST_WXI]);    // between the gates' accumulators (parameter order)
    const WaveSet w_dx = nwg >= 4 ? WaveSet{0, 1} : all_waves();
    const WaveSet w_gw = nwg >= 4 ? WaveSet{1, nwg - 1} : all_waves();
    auto tap_col = [&](int, int tap, int j) { return wrapi(j - tap + 1, hq); };
    {
        const float* wx = w[SUR_ST_WXI];
        const GemmSeg sx[4] = {{wx, 3, ca * 3, L.dgates, hs, cs},
                               {wx + gate_stride, 3, ca * 3, L.dgates + s, hs, cs},
                               {wx + 2 * gate_stride, 3, ca * 3, L.dgates + 2 * s, hs, cs},
                               {wx + 3 * gate_stride, 3, ca * 3, L.dgates + 3 * s, hs, cs}};
        float* dxp = L.dx;
        gemm_taps<3, 4>(w_dx, false, ca, hq, sx, tap_col, [&](int m, int j, float v) {
            if (m < ca) dxp[m * hq + j] = v;
        });
    }
    struct St { const float* row; int off; };
    {   // weight gradients, all gates in one GEMM each: rows m = (gate, o)
        const GP gx = g[SUR_ST_WXI];
        const float* xin = L.x;
        const int ncols = ca * 3;
        gemm_pos(w_gw, false, 4 * cs, ncols, hq, L.dgates, hs,
                 [&](int n) { const int ci = n / 3, k = n - ci * 3; return St{xin + ci * hs, k - 1}; },
                 [&](const St& st, int pp) { return st.row[wrapi(pp + st.off, hq)]; },
                 [&](int m, int n, float v) {
                     if (m < 4 * cs && n < ncols) {
                         const int gt = m / cs, o = m - gt * cs;
                         gx[gt * ggate_stride + o * ncols + n] += v;
                     }
                 });
        const GP gh = g[SUR_ST_WHI];
        const float* hin_ = L.h;
        const int ncols_h = cs * 3;
        gemm_pos(w_gw, false, 4 * cs, ncols_h, hq, L.dgates, hs,
                 [&](int n) { const int ci = n / 3, k = n - ci * 3; return St{hin_ + ci * hs, k - 1}; },
                 [&](const St& st, int pp) { return st.row[wrapi(pp + st.off, hq)]; },
                 [&](int m, int n, float v) {
                     if (m < 4 * cs && n < ncols_h) {
                         const int gt = m / cs, o = m - gt * cs;
                         gh[gt * ggate_stride + o * ncols_h + n] += v;
                     }
                 });
        // bias gradients: one 16-lane group per (gate, channel) row of dG
        const GP gbx = g[SUR_ST_BXI];
        const int group = threadIdx.x >> 4, gl = threadIdx.x & 15, ngroups = blockDim.x >> 4;
        for (int r0 = 0; r0 < 4 * cs; r0 += ngroups) {
            const int r = r0 + group;
            float a0 = 0.0f, a1 = 0.0f;
            if (r < 4 * cs)
                for (int pp = gl; pp < hq; pp += 32) {
                    a0 += L.dgates[r * hs + pp];
                    if (pp + 16 < hq) a1 += L.dgates[r * hs + pp + 16];
                }
            group_sum2(a0, a1, 16);
            if (gl == 0 && r < 4 * cs) {
                const int gt = r / cs, o = r - gt * cs;
                gbx[gt * ggate_stride + o] += a0 + a1;
            }
        }
    }
    __syncthreads();
}

}  // namespace

#endif  // SUR_CELL_H
