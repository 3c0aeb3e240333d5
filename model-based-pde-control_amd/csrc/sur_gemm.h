// sur_gemm.h -- the gather-GEMM core on v_mfma_f32_16x16x4_f32 (GemmSeg, WaveSet, gemm_taps, gemm_pos) and every conv-like
// layer built on it: circular Conv1d and zero-padded ConvTranspose1d, forward, data gradient and weight gradient.
// Needs sur_common.h.
#ifndef SUR_GEMM_H
#define SUR_GEMM_H

#include "sur_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// block-cooperative layer primitives on LDS-resident activations [C][H] (row-major, H contiguous).
// Every primitive ends with __syncthreads().
// ---------------------------------------------------------------------------------------------

// ---------------------------------------------------------------------------------------------
// Every convolution-like layer (forward, data-gradient, weight-gradient; strided circular Conv1d and
// zero-padded ConvTranspose1d) is a small GEMM  C[M][N] (+)= sum_k A(m,k) * B(k,n)  whose operands are
// *gathered* from LDS-resident activations / weights through index functors.  The GEMM itself runs
// on the matrix cores with v_mfma_f32_16x16x4_f32 (exact fp32: bit-for-bit an fmaf chain in k order),
// one 16x16 output tile per wavefront at a time, so a layer costs ~2 LDS reads + 1 MFMA per 1024
// MACs instead of ~5 VALU/LDS instructions per 64.  Lane map (guide, section 3): A[l&15][k=l>>4],
// B[k=l>>4][l&15], result reg i of lane l = C[4*(l>>4)+i][l&15].
// ---------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) float lds_f;   // a float the compiler KNOWS to be in LDS (ds_read / ds_write, 32-bit address)

// Flavour 1 -- reduction over (segment, tap, channel):
//   C[m][n] = sum_seg sum_{t<T} sum_{c<cin} A_seg[m*a_sm + c*a_sc + t] * B_seg[c*b_sc + col(seg, t, n)]
// col() returns the gathered column of B for tap t and output column n, or -1 when that tap does not
// contribute (zero padding / stride parity).  Per tap the channel loop is affine in both operands, so
// the loads of successive MFMAs are independent of each other (no div/mod/wrap inside the loop).
struct GemmSeg {
    const float* a;
    int a_sm, a_sc;
    const float* b;
    int b_sc, cin;
};

// A subset of the workgroup's wavefronts.  Independent small GEMMs are issued back to back on
// disjoint wave sets WITHOUT a barrier in between (sync = false) so that they run concurrently; the
// last one of a group (or an explicit __syncthreads()) closes the phase.
struct WaveSet {
    int lo, cnt;
};
__device__ __forceinline__ WaveSet all_waves() { return WaveSet{0, (int)(blockDim.x >> 6)}; }
__device__ __forceinline__ WaveSet lower_half() { const int nw = blockDim.x >> 6; return WaveSet{0, nw > 1 ? nw / 2 : 1}; }
__device__ __forceinline__ WaveSet upper_half() {
    const int nw = blockDim.x >> 6;
    return nw > 1 ? WaveSet{nw / 2, nw - nw / 2} : WaveSet{0, 1};
}

template <int T, int NSEG, class ColFn, class PutFn>
__device__ __forceinline__ void gemm_taps(WaveSet ws, bool sync, int M, int N, const GemmSeg (&seg)[NSEG], ColFn col,
                                          PutFn put) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (wid >= ws.lo && wid < ws.lo + ws.cnt) {
        const int nwg = blockDim.x >> 6;
        const int wave = wid - ws.lo, nw = ws.cnt < nwg ? ws.cnt : nwg;
        const int r = lane & 15, q = lane >> 4;
        const int tn_count = (N + 15) >> 4, tiles = ((M + 15) >> 4) * tn_count;
        for (int t = wave; t < tiles; t += nw) {
            const int m0 = (t / tn_count) << 4, n0 = (t % tn_count) << 4;
            const int m = m0 + r, n = n0 + r;
            const bool m_ok = m < M;
            const int m_safe = m_ok ? m : M - 1;
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int sg = 0; sg < NSEG; ++sg) {
                const GemmSeg& S = seg[sg];
#pragma unroll
                for (int tap = 0; tap < T; ++tap) {
                    const int cidx = (n < N) ? col(sg, tap, n) : -1;
                    const float* ap = S.a + m_safe * S.a_sm + tap;
                    const float* bp = S.b + (cidx >= 0 ? cidx : 0);
                    const bool b_ok = cidx >= 0;
                    if (__builtin_amdgcn_ballot_w64(b_ok) == 0) continue;   // this tap reaches none of the tile's columns
                    int c0 = 0;
                    for (; c0 + 8 <= S.cin; c0 += 8) {  // 2 MFMAs per trip on independent accumulators
                        const float a0 = ap[(c0 + q) * S.a_sc], b0 = bp[(c0 + q) * S.b_sc];
                        const float a1 = ap[(c0 + 4 + q) * S.a_sc], b1 = bp[(c0 + 4 + q) * S.b_sc];
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(m_ok ? a0 : 0.f, b_ok ? b0 : 0.f, acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(m_ok ? a1 : 0.f, b_ok ? b1 : 0.f, acc1, 0, 0, 0);
                    }
                    for (; c0 < S.cin; c0 += 4) {
                        const int c = c0 + q;
                        const bool c_ok = c < S.cin;
                        const int cs_ = c_ok ? c : S.cin - 1;
                        const float a0 = ap[cs_ * S.a_sc], b0 = bp[cs_ * S.b_sc];
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32((m_ok && c_ok) ? a0 : 0.f, (b_ok && c_ok) ? b0 : 0.f, acc0,
                                                                    0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) put(m0 + q * 4 + i, n0 + r, acc0[i] + acc1[i]);
        }
    }
    if (sync) __syncthreads();
}

// Flavour 2 -- reduction over positions p (P a multiple of 4):
//   C[m][n] = sum_p A[m*a_sm + p] * b_at(state(n), p);   state(n) decodes the output column once.
template <class PrepFn, class FetchFn, class PutFn>
__device__ __forceinline__ void gemm_pos(WaveSet ws, bool sync, int M, int N, int P, const float* a, int a_sm,
                                         PrepFn prep, FetchFn fetch, PutFn put, int t_lo = 0, int t_hi = 1 << 30) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (wid >= ws.lo && wid < ws.lo + ws.cnt) {
        const int nwg = blockDim.x >> 6;
        const int wave = wid - ws.lo, nw = ws.cnt < nwg ? ws.cnt : nwg;
        const int r = lane & 15, q = lane >> 4;
        const int tn_count = (N + 15) >> 4, tiles_all = ((M + 15) >> 4) * tn_count;
        const int tiles = tiles_all < t_hi ? tiles_all : t_hi;  // only tiles [t_lo, t_hi): lets a caller share one GEMM between wave sets
        for (int t = t_lo + wave; t < tiles; t += nw) {
            const int m0 = (t / tn_count) << 4, n0 = (t % tn_count) << 4;
            const int m = m0 + r, n = n0 + r;
            const bool m_ok = m < M, n_ok = n < N;
            const float* ap = a + (m_ok ? m : M - 1) * a_sm;
            const auto st = prep(n_ok ? n : N - 1);
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
            int p = 0;
            for (; p + 8 <= P; p += 8) {
                const float a0 = ap[p + q], b0 = fetch(st, p + q);
                const float a1 = ap[p + 4 + q], b1 = fetch(st, p + 4 + q);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(m_ok ? a0 : 0.f, n_ok ? b0 : 0.f, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(m_ok ? a1 : 0.f, n_ok ? b1 : 0.f, acc1, 0, 0, 0);
            }
            for (; p < P; p += 4) {
                const float a0 = ap[p + q], b0 = fetch(st, p + q);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(m_ok ? a0 : 0.f, n_ok ? b0 : 0.f, acc0, 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) put(m0 + q * 4 + i, n0 + r, acc0[i] + acc1[i]);
        }
    }
    if (sync) __syncthreads();
}

// circular Conv1d forward: out[o][p] (+)= bias[o] + sum_{ci,k} W[o][ci][k] * in[ci][(p*stride + k - pad) mod hin]
template <int K>
__device__ void conv_fwd(const float* in, int cin, int hin, const float* W, const float* bias, int cout, int stride,
                         int pad, float* out, bool accumulate, WaveSet ws = WaveSet{0, 1 << 20}, bool sync = true) {
    const int hout = hin / stride;
    if (cout == 1) {  // a single output row would waste 15/16 of an MFMA tile: split-lane VALU reduction
        const int total = hout;
        int split = 1;
        while (split < 8 && total * split * 2 <= (int)blockDim.x && cin % (split * 2) == 0) split *= 2;
        const int cper = cin / split;
        for (int base = 0; base < total * split; base += blockDim.x) {
            const int t = base + threadIdx.x;
            const bool live = t < total * split;
            const int p = live ? t / split : 0, part = t % split;
            float acc = 0.0f;
            for (int ci = part * cper; ci < (part + 1) * cper; ++ci) {
#pragma unroll
                for (int k = 0; k < K; ++k) acc = fmaf(W[ci * K + k], in[ci * hin + wrapi(p * stride + k - pad, hin)], acc);
            }
            for (int m = 1; m < split; m <<= 1) acc += __shfl_xor(acc, m, 64);
            if (live && part == 0) {
                if (bias) acc += bias[0];
                out[p] = accumulate ? out[p] + acc : acc;
            }
        }
        if (sync) __syncthreads();
        return;
    }
    const GemmSeg seg[1] = {{W, cin * K, K, in, hin, cin}};
    gemm_taps<K, 1>(ws, sync, cout, hout, seg, [&](int, int tap, int n) { return wrapi(n * stride + tap - pad, hin); },
                    [&](int m, int n, float v) {
                        if (m < cout) {
                            if (bias) v += bias[m];
                            out[m * hout + n] = accumulate ? out[m * hout + n] + v : v;
                        }
                    });
}

// din[ci][j] (+)= sum_{o,k : (p*stride + k - pad) mod hin == j} W[o][ci][k] * dout[o][p]
template <int K>
__device__ void conv_bwd_data(const float* dout, int cout, int hin, const float* W, int cin, int stride, int pad,
                              float* din, bool accumulate, WaveSet ws = WaveSet{0, 1 << 20}, bool sync = true) {
    const int hout = hin / stride;
    if (cout == 1 && stride == 1 && cin == 1) {   // one K-tap stencil: a position per thread on the VALU
        const int wid = threadIdx.x >> 6, nwg = blockDim.x >> 6;
        const int nw = ws.cnt < nwg ? ws.cnt : nwg;
        if (wid >= ws.lo && wid < ws.lo + nw)
            for (int j = threadIdx.x - 64 * ws.lo; j < hin; j += 64 * nw) {
                float acc = accumulate ? din[j] : 0.0f;
#pragma unroll
                for (int k = 0; k < K; ++k) acc = fmaf(W[k], dout[wrapi(j - k + pad, hin)], acc);
                din[j] = acc;
            }
        if (sync) __syncthreads();
        return;
    }
    if (cout == 1 && stride == 1 && cin <= 16 && K <= 8 && (hin & 15) == 0) {
        // din[ci][j] = sum_k W[ci][k] * dout[(j - k + pad) mod hin]: the TAPS are the reduction dimension -- rows = input
        // channels, columns = 16 positions, ceil(K / 4) MFMA steps per tile.  (The generic gather-GEMM reduces over
        // (output channel, tap) with the channels four at a time: with one output channel K steps per tile, three of
        // four k-slots empty -- 7 k cycles for the decoder's 7-tap layer at N = 256.)
        const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nwg = blockDim.x >> 6;
        const int nw = ws.cnt < nwg ? ws.cnt : nwg;
        if (wid >= ws.lo && wid < ws.lo + nw) {
            const int r = lane & 15, q = lane >> 4;
            const float w0 = (r < cin && q < K) ? W[r * K + q] : 0.0f;
            const float w1 = (r < cin && 4 + q < K) ? W[r * K + 4 + q] : 0.0f;
            for (int t = wid - ws.lo; t < (hin >> 4); t += nw) {
                const int j = 16 * t + r;
                const float d0 = q < K ? dout[wrapi(j - q + pad, hin)] : 0.0f;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w0, d0, acc, 0, 0, 0);
                if (K > 4) {
                    const float d1 = 4 + q < K ? dout[wrapi(j - 4 - q + pad, hin)] : 0.0f;
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w1, d1, acc, 0, 0, 0);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int ci = 4 * q + i;
                    if (ci < cin) din[ci * hin + j] = accumulate ? din[ci * hin + j] + acc[i] : acc[i];
                }
            }
        }
        if (sync) __syncthreads();
        return;
    }
    const GemmSeg seg[1] = {{W, K, cin * K, dout, hout, cout}};  // A[m=ci][c=o][tap] = W[(o*cin + ci)*K + tap]
    // stride 2: an input position receives from the taps of one parity only.  As in deconv_fwd the GEMM's columns are the even
    // positions followed by the odd ones (hin a multiple of 32), so a tile of 16 is of one parity and gemm_taps skips the taps
    // that reach none of its columns (half of the MFMA steps of the strided block's data gradients).
    const bool sorted = stride == 2 && (hin & 31) == 0;
    const int half = hin >> 1;
    auto pos = [&](int n) { return sorted ? (n < half ? 2 * n : 2 * (n - half) + 1) : n; };
    gemm_taps<K, 1>(ws, sync, cin, hin, seg,
                    [&](int, int tap, int n) {
                        const int t = wrapi(pos(n) - tap + pad, hin);
                        return (t % stride) ? -1 : t / stride;
                    },
                    [&](int m, int n, float v) {
                        const int j = pos(n);
                        if (m < cin) din[m * hin + j] = accumulate ? din[m * hin + j] + v : v;
                    });
}

// gW[o][ci][k] += sum_p dout[o][p] * in[ci][(p*stride + k - pad) mod hin];  gb[o] += sum_p dout[o][p]
// `scratch` (LDS, scratch_floats floats, not aliasing any operand): lets the single-output-channel case run as an MFMA tile.
// GP: the accumulators' pointer type -- `lds_f*` when the kernel knows them to be in LDS (plain ds_read / ds_write), `float*` when
// they may be the partial row in global memory (a generic pointer: flat_load / flat_store, whose s_waitcnt also drains every
// outstanding global load and store of the wave).
template <int K, class GP>
__device__ void conv_bwd_weight(const float* dout, int cout, const float* in, int cin, int hin, int stride, int pad,
                                GP gW, GP gb, WaveSet ws = WaveSet{0, 1 << 20}, bool sync = true, float* scratch = nullptr,
                                int scratch_floats = 0) {
    const int hout = hin / stride, ncols = cin * K;
    if (cout == 1 && stride == 1 && K <= 16 && cin < 16 && (cin + 1) * K <= 64 && scratch_floats >= 64 && (hin & 3) == 0) {
        // gW[ci][k] = sum_j dout[(j - k + pad) mod hin] * in[ci][j]: ONE tile with the taps as rows, the input channels (and
        // a column of ones: the bias) as columns, reduced over the input positions four at a time -- the positions split
        // over the waves, their partial tiles added in wave order through `scratch`.  hin / 16 MFMA steps per wave where the
        // 16-lane dot products below took 13 k cycles for the decoder's 7-tap layer at N = 256.
        const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nwg = blockDim.x >> 6;
        const int r = lane & 15, q = lane >> 4;
        int nw = ws.cnt < nwg ? ws.cnt : nwg;
        if (nw > scratch_floats >> 6) nw = scratch_floats >> 6;
        const int steps = hin >> 2, per = (steps + nw - 1) / nw;
        if (wid >= ws.lo && wid < ws.lo + nw) {
            const int wv = wid - ws.lo;
            const bool a_ok = r < K, b_in = r < cin;
            const float b_const = (r == cin && gb) ? 1.0f : 0.0f;
            const float* brow = in + (b_in ? r : 0) * hin;
            const int shift = pad - (a_ok ? r : 0);
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
            const int s1 = (wv + 1) * per < steps ? (wv + 1) * per : steps;
            int st = wv * per;
            for (; st + 2 <= s1; st += 2) {
                const int ja = 4 * st + q, jb = ja + 4;
                const float a0 = dout[wrapi(ja + shift, hin)], b0 = b_in ? brow[ja] : b_const;
                const float a1 = dout[wrapi(jb + shift, hin)], b1 = b_in ? brow[jb] : b_const;
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a_ok ? a0 : 0.f, b0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a_ok ? a1 : 0.f, b1, acc1, 0, 0, 0);
            }
            if (st < s1) {
                const int ja = 4 * st + q;
                const float a0 = dout[wrapi(ja + shift, hin)], b0 = b_in ? brow[ja] : b_const;
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a_ok ? a0 : 0.f, b0, acc0, 0, 0, 0);
            }
            if (r <= cin) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (4 * q + i < K) scratch[wv * 64 + r * K + 4 * q + i] = acc0[i] + acc1[i];
            }
        }
        __syncthreads();
        for (int t = threadIdx.x; t < ncols + (gb ? 1 : 0); t += blockDim.x) {
            float v = 0.0f;
            for (int wv = 0; wv < nw; ++wv) v += scratch[wv * 64 + t];
            if (t < ncols) gW[t] += v;
            else gb[0] += v;      // t = cin * K: row 0 of the ones column
        }
        if (sync) __syncthreads();
        return;
    }
    if (cout == 1) {
        // ncols + 1 dot products of length hout (the weight taps and the bias): one per 16-lane group, positions
        // strided over the group's lanes, partial sums folded with DPP row rotations.  (One thread per dot product
        // with a serial loop over hout cost 8 k cycles per call: the slowest phase of the decoder backward.)
        const int group = threadIdx.x >> 4, gl = threadIdx.x & 15, ngroups = blockDim.x >> 4;
        const int nout = ncols + (gb ? 1 : 0);
        for (int idx0 = 0; idx0 < nout; idx0 += ngroups) {
            const int idx = idx0 + group;
            float a0 = 0.0f, a1 = 0.0f;
            if (idx < ncols) {
                const int ci = idx / K, k = idx - ci * K;
                const float* row = in + ci * hin;
                for (int p = gl; p < hout; p += 32) {
                    a0 = fmaf(dout[p], row[wrapi(p * stride + k - pad, hin)], a0);
                    if (p + 16 < hout) a1 = fmaf(dout[p + 16], row[wrapi((p + 16) * stride + k - pad, hin)], a1);
                }
            } else if (idx == ncols && gb) {
                for (int p = gl; p < hout; p += 32) {
                    a0 += dout[p];
                    if (p + 16 < hout) a1 += dout[p + 16];
                }
            }
            group_sum2(a0, a1, 16);
            if (gl == 0) {
                if (idx < ncols) gW[idx] += a0 + a1;
                else if (idx == ncols && gb) gb[0] += a0 + a1;
            }
        }
        if (sync) __syncthreads();
        return;
    }
    if (gb) {
        // bias gradient: one 16-lane group per output channel
        const int group = threadIdx.x >> 4, gl = threadIdx.x & 15, ngroups = blockDim.x >> 4;
        for (int o0 = 0; o0 < cout; o0 += ngroups) {
            const int o = o0 + group;
            float a0 = 0.0f, a1 = 0.0f;
            if (o < cout)
                for (int p = gl; p < hout; p += 32) {
                    a0 += dout[o * hout + p];
                    if (p + 16 < hout) a1 += dout[o * hout + p + 16];
                }
            group_sum2(a0, a1, 16);
            if (gl == 0 && o < cout) gb[o] += a0 + a1;
        }
    }
    struct St { const float* row; int off; };
    gemm_pos(ws, sync, cout, ncols, hout, dout, hout,
             [&](int n) {
                 const int ci = n / K, k = n - ci * K;
                 return St{in + ci * hin, k - pad};
             },
             [&](const St& st, int p) { return st.row[wrapi(p * stride + st.off, hin)]; },
             [&](int m, int n, float v) {
                 if (m < cout && n < ncols) gW[m * ncols + n] += v;
             });
}

// ConvTranspose1d(k=3, stride=2, padding=1, output_padding=1), zero padded; W[ci][o][k]; hout = 2*hin
// out[o][j] = b[o] + sum_{ci,k : j = 2i - 1 + k} W[ci][o][k] * in[ci][i]
__device__ void deconv_fwd(const float* in, int cin, int hin, const float* W, const float* bias, int cout,
                           float* out, WaveSet ws = WaveSet{0, 1 << 20}, bool sync = true) {
    const int hout = 2 * hin;
    const GemmSeg seg[1] = {{W, 3, cout * 3, in, hin, cin}};  // A[m=o][c=ci][tap] = W[(ci*cout + o)*3 + tap]
    // An even output position takes the middle tap only, an odd one the outer two.  With the GEMM's columns in output
    // order every tile of 16 holds both parities and issues all three taps, half of them on zeros; with the even positions
    // in the first hin columns and the odd ones behind them (hin a multiple of 16) a tile is of one parity and gemm_taps
    // skips the taps that reach none of its columns: 1 or 2 tap passes per tile instead of 3.
    const bool sorted = (hin & 15) == 0;
    auto pos = [&](int n) { return sorted ? (n < hin ? 2 * n : 2 * (n - hin) + 1) : n; };
    gemm_taps<3, 1>(ws, sync, cout, hout, seg,
                    [&](int, int tap, int n) {
                        const int t = pos(n) + 1 - tap;
                        return (t < 0 || (t & 1) || (t >> 1) >= hin) ? -1 : (t >> 1);
                    },
                    [&](int m, int n, float v) {
                        if (m < cout) out[m * hout + pos(n)] = v + bias[m];
                    });
}

__device__ void deconv_bwd_data(const float* dout, int cout, int hin, const float* W, int cin, float* din,
                                WaveSet ws = WaveSet{0, 1 << 20}, bool sync = true) {
    const int hout = 2 * hin;
    const GemmSeg seg[1] = {{W, cout * 3, 3, dout, hout, cout}};  // A[m=ci][c=o][tap] = W[(ci*cout + o)*3 + tap]
    gemm_taps<3, 1>(ws, sync, cin, hin, seg,
                    [&](int, int tap, int i) {
                        const int j = 2 * i - 1 + tap;
                        return (j < 0 || j >= hout) ? -1 : j;
                    },
                    [&](int m, int i, float v) {
                        if (m < cin) din[m * hin + i] = v;
                    });
}

template <class GP>
__device__ void deconv_bwd_weight(const float* dout, int cout, const float* in, int cin, int hin, GP gW, GP gb,
                                  WaveSet ws = WaveSet{0, 1 << 20}, bool sync = true) {
    const int hout = 2 * hin, ncols = cout * 3;
    {
        // bias gradient: one 16-lane group per output channel, positions strided over the group's lanes.  (One thread per
        // channel with a serial loop over hout was 16 k cycles at hout = 256 -- a fifth of the decoder backward -- all of
        // it in the wave that then starts on the first tile of the GEMM below.)
        const int group = threadIdx.x >> 4, gl = threadIdx.x & 15, ngroups = blockDim.x >> 4;
        for (int o0 = 0; o0 < cout; o0 += ngroups) {
            const int o = o0 + group;
            float a0 = 0.0f, a1 = 0.0f;
            if (o < cout)
                for (int j = gl; j < hout; j += 32) {
                    a0 += dout[o * hout + j];
                    if (j + 16 < hout) a1 += dout[o * hout + j + 16];
                }
            group_sum2(a0, a1, 16);
            if (gl == 0 && o < cout) gb[o] += a0 + a1;
        }
    }
    struct St { const float* row; int off; };
    gemm_pos(ws, sync, cin, ncols, hin, in, hin,
             [&](int n) {
                 const int o = n / 3, k = n - o * 3;
                 return St{dout + o * hout, k - 1};
             },
             [&](const St& st, int i) {
                 const int j = 2 * i + st.off;
                 return (j < 0 || j >= hout) ? 0.0f : st.row[j];
             },
             [&](int m, int n, float v) {
                 if (m < cin && n < ncols) gW[m * ncols + n] += v;
             });
}

}  // namespace

#endif  // SUR_GEMM_H
