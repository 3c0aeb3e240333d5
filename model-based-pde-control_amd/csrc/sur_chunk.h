// sur_chunk.h -- the split-path kernels of a TBPTT chunk: the cell chains (cell_fwd_kernel, cell_bwd_kernel), the scans over time
// (integrate, dgrad_scan, latent_scan / _dscan), the (step, sample)-parallel dec_fwd / dec_bwd / cell_wgrad kernels, add_into,
// and their LDS sizers.  Needs sur_cell.h and sur_params.h.
#ifndef SUR_CHUNK_H
#define SUR_CHUNK_H

#include <type_traits>

#include "../../include/surrogate_hip.h"
#include "sur_cell.h"
#include "sur_params.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Split path: only the ConvLSTM cell is a recurrence.  The decoder of step k reads h_k and feeds nothing back
// into step k+1 (the reference's transition ignores the re-encoded prediction, transition.py:285-296; teacher
// forcing replaces H by the encoded true state), so it is evaluated for ALL (step, sample) pairs in parallel,
// forward and backward, by persistent workgroups on every CU, while the chain kernels (one workgroup per
// sample) carry only the cell.  Layout of a saved block (step_saved_floats per (step, sample)):
//   [ gates 4s | c_k s | h_k s | p0 | a0 | p1 | a1 | p2 | a2 ]     cell part = first 6s floats
// ---------------------------------------------------------------------------------------------
#ifndef PAR_OCC
#define PAR_OCC 2   // resident workgroups per CU the (step, sample)-parallel kernels are built for
#endif
constexpr int ST_NLSTM = SUR_ST_DC0_W;              // the LSTM parameters come first in the chunk parameter order
constexpr int ST_NDEC = SUR_ST_NPARAM - ST_NLSTM;

__host__ __device__ inline int cell_part_floats(const sur_chunk_params& p) { return 6 * p.cs * p.hq; }
// threads of a cell-chain workgroup: one 256-thread wave set per 16-wide column tile of the latent, at most four
inline int cell_chain_threads(const sur_chunk_params& p) {
    const int sets = p.hq / 16;
    return TPB * (sets < 1 ? 1 : (sets > 4 ? 4 : sets));
}
__host__ __device__ inline int dec_part_floats(const sur_chunk_params& p) { return step_block_floats(p) - cell_part_floats(p); }
__host__ __device__ inline int cell_fwd_act_floats(const sur_chunk_params& p) { return p.ca * p.hq + 8 * p.cs * p.hq; }
__host__ __device__ inline int cell_bwd_act_floats(const sur_chunk_params& p) {
    const int s = p.cs * p.hq;   // [gates | c_k] twice (ping-pong DMA targets), dgates, four dh partials
    return 2 * 5 * s + 4 * s + 4 * s;
}
__host__ __device__ inline int cell_wgrad_act_floats(const sur_chunk_params& p) {
    return p.ca * p.hq + (p.ca + 5 * p.cs) * (p.hq + 4);   // dx | x, h_in, dgates with rows hq + 4 apart (cell_wgrad_gemms)
}
__host__ __device__ inline int dec_act_floats(const sur_chunk_params& p, bool backward) {
    const int s = p.cs * p.hq, n = 4 * p.hq;
    // backward (dec_bwd_kernel): three activation buffers [a0 -> h | p1 -> p0 | a1], gA, gB (dh, and p2 / a2 in its tail)
    if (backward) return 5 * step_max_act(p);
    return s + dec_part_floats(p) + n;                                    // hnew, p0..a2, d
}

template <int NP>
__device__ __forceinline__ void stage_range(const sur_chunk_params& p, int first, float* lds_w, const float** w) {
    ParamViews<NP> v;
    stage_weights<NP>(p.w + first, p.size + first, lds_w, v);
#pragma unroll
    for (int i = 0; i < NP; ++i) w[first + i] = v.w[i];
}

// (the chain kernels are instantiated per workgroup size: the 256-thread build keeps its register budget)
// The whole forward chain of one sample with the state in registers (cs = 16, ca <= 4, hq = 16 * NSETS: exactly one
// (channel, position) element per thread).  Per step and lane: 15 MFMAs whose A operands -- the gate weights -- were read
// from global memory ONCE into 15 registers before the time loop, B operands gathered from the x / h buffers in LDS;
// i, f, g, o, c', h' finished in the accumulator registers (same row <-> (channel, gate) map and the same summation order
// as cell_forward_fused), c carried in a register, h' and the next step's x written to the OTHER of two LDS buffers and
// every output stored to HBM straight from registers: ONE barrier per step, no LDS copy of h / c / gates, no weights in
// LDS.  The next step's latent action and (teacher forcing) encoded state are fetched one step ahead.
template <int NSETS>
__device__ __forceinline__ void cell_chain_forward(const sur_chunk_params& p, float* lds, const float* __restrict__ xlat_t,
                                                   const float* __restrict__ lstates_t, const float* __restrict__ h0,
                                                   const float* __restrict__ c0, int hc_bstride, int K, int S, int B, int b,
                                                   float* __restrict__ h_all, float* __restrict__ c_all,
                                                   float* __restrict__ saved) {
    const int hq = p.hq, ca = p.ca, s = 16 * hq, nx = ca * hq;
    // LDS-typed pointers: through a generic `float*` picked from an array by (k & 1) the operand reads of the time loop were
    // flat_load_dword -- 64-bit address arithmetic per read and, because a flat access may be a global one, an
    // s_waitcnt vmcnt(0) in front of every MFMA group: each step waited for its own prefetch and the previous step's stores
    lds_f* const xbase = (lds_f*)lds;
    lds_f* const hbase = xbase + 2 * nx;
    const int tid = threadIdx.x, lane = tid & 63, wave = (tid >> 6) & 3, tset = NSETS > 1 ? tid >> 8 : 0;
    const int r = lane & 15, q = lane >> 4;
    const int n = 16 * tset + r, ch = 4 * wave + q, idx = ch * hq + n;
    // A operands: row r of this wave's tile = (gate r & 3, channel 4 * wave + (r >> 2)); lane (r, q) feeds k = q of each K block
    const int gate_r = r & 3, ch_r = 4 * wave + (r >> 2);
    const bool xq = q < ca;
    float ax[3], ah[4][3];
    {
        const float* wx = p.w[SUR_ST_WXI + 3 * gate_r] + (ch_r * ca + (xq ? q : 0)) * 3;   // W_g[(o*cin + ci)*3 + tap]
        const float* wh = p.w[SUR_ST_WHI + 3 * gate_r] + ch_r * 16 * 3;
#pragma unroll
        for (int tap = 0; tap < 3; ++tap) {
            ax[tap] = xq ? wx[tap] : 0.0f;
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) ah[c4][tap] = wh[(4 * c4 + q) * 3 + tap];
        }
    }
    const float bi = p.w[SUR_ST_BXI][ch], bf = p.w[SUR_ST_BXF][ch], bc = p.w[SUR_ST_BXC][ch], bo = p.w[SUR_ST_BXO][ch];
    float c_reg = c0[(size_t)b * hc_bstride + idx];
    hbase[idx] = S > 0 ? lstates_t[(size_t)b * s + idx] : h0[(size_t)b * hc_bstride + idx];
    if (tid < nx) xbase[tid] = xlat_t[(size_t)b * nx + tid];
    const size_t save_stride = step_saved_floats(p);
    int colx[3];
#pragma unroll
    for (int tap = 0; tap < 3; ++tap) colx[tap] = wrapi(n + tap - 1, hq);
    __syncthreads();
    for (int k = 0; k < K; ++k) {
        const size_t kb = (size_t)k * B + b;
        const bool nxt = k + 1 < K, next_forced = nxt && k + 1 < S;
        float xnext = 0.0f, hforced = 0.0f;
        if (nxt && tid < nx) xnext = xlat_t[(kb + B) * nx + tid];
        if (next_forced) hforced = lstates_t[(kb + B) * s + idx];
        const lds_f* xc = xbase + (k & 1) * nx;
        const lds_f* hc = hbase + (k & 1) * s;
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tap = 0; tap < 3; ++tap) {
            const int col = colx[tap];
            const float bx = xc[(xq ? q : 0) * hq + col];
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ax[tap], xq ? bx : 0.f, acc0, 0, 0, 0);
#pragma unroll
            for (int c0_ = 0; c0_ < 4; c0_ += 2) {
                const float b0 = hc[(4 * c0_ + q) * hq + col], b1 = hc[(4 * c0_ + 4 + q) * hq + col];
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[c0_][tap], b0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[c0_ + 1][tap], b1, acc1, 0, 0, 0);
            }
        }
        const float gi = sigmoid_(acc0[0] + acc1[0] + bi), gf = sigmoid_(acc0[1] + acc1[1] + bf),
                    gg = tanh_(acc0[2] + acc1[2] + bc), go = sigmoid_(acc0[3] + acc1[3] + bo);
        const float cn = fmaf(gf, c_reg, gi * gg);
        const float hn = go * tanh_(cn);
        c_reg = cn;
        h_all[kb * s + idx] = hn;
        c_all[kb * s + idx] = cn;
        if (saved) {   // [gates | c_k | h_k]
            float* dst = saved + kb * save_stride + idx;
            dst[0] = gi;
            dst[s] = gf;
            dst[2 * s] = gg;
            dst[3 * s] = go;
            dst[4 * s] = cn;
            dst[5 * s] = hn;
        }
        if (nxt) {
            hbase[((k + 1) & 1) * s + idx] = next_forced ? hforced : hn;   // teacher forcing replaces H
            if (tid < nx) xbase[((k + 1) & 1) * nx + tid] = xnext;
        }
        __syncthreads();
    }
}

template <int MAXT>
__global__ void __launch_bounds__(MAXT)
cell_fwd_kernel(const sur_chunk_params p, const float* __restrict__ xlat_t, const float* __restrict__ lstates_t,
                const float* __restrict__ h0, const float* __restrict__ c0, int hc_bstride, int K, int S, int B,
                float* __restrict__ h_all, float* __restrict__ c_all, float* __restrict__ saved) {
    extern __shared__ __align__(16) float lds[];
    const int b = blockIdx.x, s = p.cs * p.hq, nx = p.ca * p.hq;
#ifndef SUR_STAMP
    if constexpr ((MAXT & 255) == 0) {
        if (p.cs == 16 && p.ca <= 4 && p.hq * 16 == MAXT) {   // one (channel, position) element per thread
            cell_chain_forward<MAXT / 256>(p, lds, xlat_t, lstates_t, h0, c0, hc_bstride, K, S, B, b, h_all, c_all, saved);
            return;
        }
    }
#endif
    StepLayout L{};
    L.x = lds;
    L.h = L.x + nx;
    L.c = L.h + s;
    L.gates = L.c + s;
    L.cnew = L.gates + 4 * s;
    L.hnew = L.cnew + s;
    const float* w[SUR_ST_NPARAM];
    stage_range<ST_NLSTM>(p, 0, L.hnew + s, w);
    const size_t save_stride = step_saved_floats(p);
    for (int i = threadIdx.x; i < s; i += blockDim.x) {
        L.hnew[i] = h0[(size_t)b * hc_bstride + i];   // hc_bstride = 0: one initial state shared by the batch
        L.cnew[i] = c0[(size_t)b * hc_bstride + i];
    }
    STAMP(109);
    // the next step's latent action is fetched while this step computes
    float xn[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
        xn[u] = threadIdx.x + u * MAXT < nx ? xlat_t[(size_t)b * nx + threadIdx.x + u * MAXT] : 0.0f;
    __syncthreads();
    for (int k = 0; k < K; ++k) {
        const size_t kb = (size_t)k * B + b;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (threadIdx.x + u * MAXT < nx) L.x[threadIdx.x + u * MAXT] = xn[u];
        for (int i = threadIdx.x + 4 * MAXT; i < nx; i += MAXT) L.x[i] = xlat_t[kb * nx + i];
        for (int i = threadIdx.x; i < s; i += blockDim.x) {
            L.h[i] = (k < S) ? lstates_t[kb * s + i] : L.hnew[i];  // teacher forcing replaces H
            L.c[i] = L.cnew[i];
        }
        __syncthreads();
        STAMP(k < S ? 110 : 111);
        if (k + 1 < K) {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (threadIdx.x + u * MAXT < nx) xn[u] = xlat_t[(kb + B) * nx + threadIdx.x + u * MAXT];
        }
        cell_forward<MAXT>(p, L, w);
        STAMP(112);
        for (int i = threadIdx.x; i < s; i += blockDim.x) {
            h_all[kb * s + i] = L.hnew[i];
            c_all[kb * s + i] = L.cnew[i];
        }
        if (saved) {   // [gates | c_k | h_k]
            float4* dst = reinterpret_cast<float4*>(saved + kb * save_stride);
            const float4* src = reinterpret_cast<const float4*>(L.gates);
            for (int i = threadIdx.x; i < (6 * s) >> 2; i += blockDim.x) dst[i] = src[i];
        }
        __syncthreads();
        STAMP(113);
    }
}

// decoder of every (step, sample) pair m: d_all[m] from h_all[m]; persistent workgroups
__global__ void __launch_bounds__(TPB, PAR_OCC)
dec_fwd_kernel(const sur_chunk_params p, const float* __restrict__ h_all, int M, float* __restrict__ d_all,
               float* __restrict__ saved) {
    extern __shared__ __align__(16) float lds[];
    const int s = p.cs * p.hq, n = 4 * p.hq;
    StepLayout L{};
    L.n = n;
    L.hnew = lds;
    L.p0 = L.hnew + s;
    L.a0 = L.p0 + p.cs * 2 * p.hq;
    L.p1 = L.a0 + p.cs * 2 * p.hq;
    L.a1 = L.p1 + p.c_mid * n;
    L.p2 = L.a1 + p.c_mid * n;
    L.a2 = L.p2 + n;
    L.d = L.a2 + n;
    const float* w[SUR_ST_NPARAM];
    stage_range<ST_NDEC>(p, ST_NLSTM, L.d + n, w);
    const size_t save_stride = step_saved_floats(p);
    const int ndec4 = dec_part_floats(p) >> 2;
    for (int m = blockIdx.x; m < M; m += gridDim.x) {
        lds_load_v4(L.hnew, h_all + (size_t)m * s, s >> 2);
        decoder_forward(p, L, w);
        for (int i = threadIdx.x; i < n; i += blockDim.x) d_all[(size_t)m * n + i] = L.d[i];
        if (saved) {
            float4* dst = reinterpret_cast<float4*>(saved + (size_t)m * save_stride + 6 * s);
            const float4* src = reinterpret_cast<const float4*>(L.p0);
            for (int i = threadIdx.x; i < ndec4; i += blockDim.x) dst[i] = src[i];
        }
        __syncthreads();
    }
}

// out_k = base_k + delta * (d_k * mul + add); base_k = the given state while teacher forcing, else out_{k-1}
__global__ void __launch_bounds__(TPB)
integrate_kernel(const float* __restrict__ states_t, const float* __restrict__ d_all, int K, int S, int B, int n, float delta,
                 float mul, float add, float* __restrict__ out_all) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= B * n) return;
    float prev = 0.0f;
    for (int k = 0; k < K; ++k) {
        const size_t idx = (size_t)k * B * n + e;
        const float base = k < S ? states_t[idx] : prev;
        prev = base + delta * fmaf(d_all[idx], mul, add);
        out_all[idx] = prev;
    }
}

// total gradient wrt d_k: direct + through out_k (and through the outputs after it while free running)
__global__ void __launch_bounds__(TPB)
dgrad_scan_kernel(const float* __restrict__ dd_all, const float* __restrict__ dout_all, int K, int S, int B, int n, float scale,
                  float* __restrict__ ga_all) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= B * n) return;
    float carry = 0.0f;
    for (int k = K - 1; k >= 0; --k) {
        const size_t idx = (size_t)k * B * n + e;
        const float go = (dout_all ? dout_all[idx] : 0.0f) + carry;
        ga_all[idx] = fmaf(scale, go, dd_all ? dd_all[idx] : 0.0f);
        carry = (k >= S) ? go : 0.0f;   // out_{k-1} is the base of step k only while free running
    }
}

// Latent-space rollout (LatentAutoRegPDESurrogate): z_k = z_{k-1} + delta * h_k from z_{-1} = lstates_t[0] (the encoded
// first given state); the decoder reads z_k.  With `saved`, z_k also replaces h_k in the h slot of the pair's saved block,
// where dec_bwd_kernel takes the decoder's input from: cell_bwd_kernel reads only [gates | c], cell_wgrad_kernel reads h_all.
__global__ void __launch_bounds__(TPB)
latent_scan_kernel(const float* __restrict__ h_all, const float* __restrict__ z0, int K, int B, int sl, float delta,
                   float* __restrict__ z_all, float* __restrict__ saved, int save_stride) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= B * sl) return;
    const int b = e / sl, i = e - b * sl;
    float z = z0[e];
    for (int k = 0; k < K; ++k) {
        const size_t idx = (size_t)k * B * sl + e;
        z = fmaf(delta, h_all[idx], z);
        z_all[idx] = z;
        if (saved) saved[((size_t)k * B + b) * save_stride + 5 * sl + i] = z;
    }
}

// Backward of latent_scan_kernel: G_k = dz_dec_k + dz_all_k + G_{k+1} (d loss / d z_k); the cell chain receives
// d loss / d h_k = delta * G_k, written over dz_dec in place.  G_0 = d loss / d z_{-1} goes to dz0 (may be NULL).
__global__ void __launch_bounds__(TPB)
latent_dscan_kernel(float* __restrict__ dh_dec, const float* __restrict__ dz_all, int K, int B, int sl, float delta,
                    float* __restrict__ dz0) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= B * sl) return;
    float carry = 0.0f;
    for (int k = K - 1; k >= 0; --k) {
        const size_t idx = (size_t)k * B * sl + e;
        carry += dh_dec[idx] + (dz_all ? dz_all[idx] : 0.0f);
        dh_dec[idx] = delta * carry;
    }
    if (dz0) dz0[e] = carry;
}

// dst += src over n floats (d z_{-1} onto the teacher-forcing gradient cell_bwd_kernel wrote into dlstates_t[0])
__global__ void __launch_bounds__(TPB) add_into_kernel(float* __restrict__ dst, const float* __restrict__ src, int n) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) dst[e] += src[e];
}

// decoder backward of every (step, sample) pair: dh_dec[m] = d loss / d h_m through the decoder; decoder parameter
// gradients into this workgroup's partial row.  Built for DEC_BWD_OCC workgroups per CU: at N = 256 the LDS layout below
// is 52 KB (round 2: 75 KB, two per CU), so three workgroups share a CU and the 640 pairs of a 10-step chunk are ONE round
// of workgroups.  Saved block of a pair: [gates 4s | c s | h s | p0 | a0 | p1 | a1 | p2 | a2].
//   LDS: X2 = a0 (later h) | X1 = p1 (later p0) | X0 = a1 | gA | gB (dh; p2, a2 in its last 2n floats: phase 1 only uses
//        the first n floats of gB, and p2 / a2 are dead when the 7-tap data gradient fills it)
// p0 and h wait in registers (2 + 1 float4 per thread at N = 256) until their buffers are free (decoder_backward).
#ifndef DEC_BWD_OCC
#define DEC_BWD_OCC 3
#endif
constexpr int DEC_LATE_P0 = 2;   // float4 registers per thread for the late p0: cs * 2 hq <= 2 * 4 * TPB
constexpr int DEC_LATE_H = 1;    //                                  ... for the late h:  cs * hq <= 4 * TPB
// GL: the gradient accumulators are in LDS (behind the staged weights) -- known at compile time, so that they are LDS-typed
// pointers (see conv_bwd_weight); GL = false accumulates straight into the workgroup's partial row.
template <bool GL>
__global__ void __launch_bounds__(TPB, DEC_BWD_OCC)
dec_bwd_kernel(const sur_chunk_params p, const float* __restrict__ saved, const float* __restrict__ ga_all, int M,
               float* __restrict__ dh_dec, int row_base) {
    extern __shared__ __align__(16) float lds[];
    const int s = p.cs * p.hq, n = 4 * p.hq, mx = step_max_act(p);
    const int a0f = p.cs * 2 * p.hq, a1f = p.c_mid * n;
    StepLayout L{};
    L.n = n;
    float* X2 = lds;
    float* X1 = X2 + mx;
    float* X0 = X1 + mx;
    L.a0 = X2;
    L.hnew = X2;
    L.p1 = X1;
    L.p0 = X1;
    L.a1 = X0;
    L.gA = X0 + mx;
    L.gB = L.gA + mx;
    L.dh = L.gB;              // s <= mx: the first LayerNorm's backward has consumed gB before dh is written
    L.p2 = L.gB + mx - 2 * n;
    L.a2 = L.p2 + n;
    float* wbase = L.gB + mx;
    const float* w[SUR_ST_NPARAM];
    stage_range<ST_NDEC>(p, ST_NLSTM, wbase, w);
    int off_dec = 0, psize_dec = 0;
    for (int i = 0; i < ST_NLSTM; ++i) off_dec += p.size[i];
    for (int i = ST_NLSTM; i < SUR_ST_NPARAM; ++i) psize_dec += p.size[i];
    const int psize = off_dec + psize_dec;
    float* row = p.partial + (size_t)(row_base + blockIdx.x) * psize + off_dec;
    typedef typename std::conditional<GL, lds_f*, float*>::type GP;
    GP gacc;
    if constexpr (GL) gacc = (lds_f*)(wbase + psize_dec);
    else gacc = row;
    GP g[SUR_ST_NPARAM];
    {
        int off = 0;
        for (int i = ST_NLSTM; i < SUR_ST_NPARAM; ++i) {
            g[i] = gacc + off;
            off += p.size[i];
        }
        if (GL)
            for (int j = threadIdx.x; j < psize_dec; j += blockDim.x) gacc[j] = 0.0f;
    }
    __syncthreads();
    const size_t save_stride = step_saved_floats(p);
    for (int m = blockIdx.x; m < M; m += gridDim.x) {
        const float* blk = saved + (size_t)m * save_stride + 5 * s;        // [h | p0 | a0 | p1 | a1 | p2 | a2]
        // the late activations start their trip now and land in registers
        float4 rp0[DEC_LATE_P0], rh[DEC_LATE_H];
#pragma unroll
        for (int u = 0; u < DEC_LATE_P0; ++u) {
            const int i = threadIdx.x + u * TPB;
            rp0[u] = i < (a0f >> 2) ? reinterpret_cast<const float4*>(blk + s)[i] : float4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < DEC_LATE_H; ++u) {
            const int i = threadIdx.x + u * TPB;
            rh[u] = i < (s >> 2) ? reinterpret_cast<const float4*>(blk)[i] : float4{0.f, 0.f, 0.f, 0.f};
        }
        for (int i = threadIdx.x; i < n; i += blockDim.x) L.gA[i] = ga_all[(size_t)m * n + i];
        for (int i = threadIdx.x; i < (2 * n) >> 2; i += blockDim.x)
            reinterpret_cast<float4*>(L.p2)[i] = reinterpret_cast<const float4*>(blk + s + 2 * a0f + 2 * a1f)[i];
        for (int i = threadIdx.x; i < (a0f >> 2); i += blockDim.x)
            reinterpret_cast<float4*>(X2)[i] = reinterpret_cast<const float4*>(blk + s + a0f)[i];
        lds_load_v4(X1, blk + s + 2 * a0f, a1f >> 2);                      // p1 (ends with a barrier)
        lds_load_v4(X0, blk + s + 2 * a0f + a1f, a1f >> 2);                // a1
        decoder_backward(p, L, w, g,
                         [&] {
#pragma unroll
                             for (int u = 0; u < DEC_LATE_P0; ++u) {
                                 const int i = threadIdx.x + u * TPB;
                                 if (i < (a0f >> 2)) reinterpret_cast<float4*>(X1)[i] = rp0[u];
                             }
                         },
                         [&] {
#pragma unroll
                             for (int u = 0; u < DEC_LATE_H; ++u) {
                                 const int i = threadIdx.x + u * TPB;
                                 if (i < (s >> 2)) reinterpret_cast<float4*>(X2)[i] = rh[u];
                             }
                         });
        for (int i = threadIdx.x; i < s; i += blockDim.x) dh_dec[(size_t)m * s + i] = L.dh[i];
        __syncthreads();
    }
    if constexpr (GL) add_to_row(row, (const float*)gacc, psize_dec);
}

// BPTT through the cell chain of one sample: consumes dh_dec (decoder) and the upstream dh / dc gradients, emits the
// gate gradients dG_k of every step (for cell_wgrad_kernel) and the gradient wrt the teacher-forced hidden inputs.
// Only what is recurrent stays here: the gate derivative and dh_{k-1} = sum_g Wh_g^T dG_g.  Two barriers per step:
//   A  element-wise: every thread owns the same elements in every step, so dc_carry lives in registers; the incoming
//      dh is the sum of the four partial tiles the previous step's GEMM left in LDS; the next step's c_{k-1} and
//      dh_dec were prefetched into registers, its [gates | c] block arrived by LDS-DMA in the other block buffer
//   B  issue the prefetches for step k-1, then the dh GEMM (K split by gate over the wave quarters)
constexpr int CELL_EPT = 4;   // elements per thread: cs * hq <= 4 * 256
struct ChunkSpans {
    sur_chunk_span sp[SUR_MAX_SPANS];
    int n;
};
// The backward chain of one (chunk, sample) for cs = 16, hq = 16 * NSETS (one (channel, position) element per thread), built
// like cell_chain_forward: the recurrent weights Wh_g^T are read from global memory ONCE into 12 registers per lane (wave
// group g = wave / NSETS contracts gate g, K = 48, for the column tile wave % NSETS), LDS holds only the gate derivatives
// and the four partial dh tiles, and everything a step reads from HBM -- its activated gates and c_k (saved by the forward),
// c_{k-1}, the decoder's dh -- is fetched TWO steps ahead into registers, so no step waits for memory (with one step of
// lead, LDS-DMA + prefetch, the loads landed ~1 us after they were needed).  Two barriers per step remain: the gate
// derivatives of all channels feed every wave's GEMM, and the four gates' partial tiles are summed by the next step.
struct CellBwdIn {
    float g[5], cp, dhd;   // activated gates i f g o, c_k; c_{k-1}; d loss / d h_k from the decoder
};

template <int NSETS>
__device__ __forceinline__ void cell_chain_backward(const sur_chunk_params& p, float* lds, const sur_chunk_span& sp, int b, int B,
                                                    const float* __restrict__ c_all, const float* __restrict__ saved,
                                                    const float* __restrict__ dh_dec, const float* __restrict__ dh_all,
                                                    const float* __restrict__ dc_all, float* __restrict__ dg_all,
                                                    float* __restrict__ dh0, float* __restrict__ dc0) {
    const int hq = p.hq, s = 16 * hq;
    const int K0 = sp.k0, K = sp.k1, S = sp.k0 + sp.s;
    const float* __restrict__ c0 = sp.c0;
    const int hc_bstride = sp.hc_bstride;
    float* __restrict__ dlstates_t = sp.dlstates_t;
    lds_f* const dgates = (lds_f*)lds;    // [4][s]   LDS-typed: as generic pointers these were flat accesses, whose
    lds_f* const part = dgates + 4 * s;   // [4][s]   s_waitcnt vmcnt(0) drained the two-steps-ahead prefetch every step
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int gt = wid / NSETS, n0 = 16 * (wid % NSETS);
    const size_t save_stride = step_saved_floats(p);
    // A[m = ci][k = o][tap] = Wh_g[(o * 16 + ci) * 3 + tap]; lane (r, q): row ci = r, k = q of each block of four o
    float a[3][4];
    {
        const float* wh = p.w[SUR_ST_WHI + 3 * gt];
#pragma unroll
        for (int tap = 0; tap < 3; ++tap)
#pragma unroll
            for (int blk = 0; blk < 4; ++blk) a[tap][blk] = wh[((4 * blk + q) * 16 + r) * 3 + tap];
    }
    int colj[3];
#pragma unroll
    for (int tap = 0; tap < 3; ++tap) colj[tap] = wrapi(n0 + r - tap + 1, hq);
    const int i = tid;   // this thread's element of [cs][hq]
    auto fetch = [&](int kk, CellBwdIn& in) {
        const float* rec = saved + ((size_t)kk * B + b) * save_stride + i;
#pragma unroll
        for (int j = 0; j < 5; ++j) in.g[j] = rec[(size_t)j * s];
        in.cp = kk > K0 ? c_all[((size_t)(kk - 1) * B + b) * s + i] : c0[(size_t)b * hc_bstride + i];
        in.dhd = dh_dec[((size_t)kk * B + b) * s + i];
    };
    CellBwdIn cur{}, nx1{}, nx2{};
    fetch(K - 1, cur);
    if (K - 2 >= K0) fetch(K - 2, nx1);
    float dcc = 0.0f;
    for (int k = K - 1; k >= K0 - 1; --k) {
        if (k - 2 >= K0) fetch(k - 2, nx2);
        // ---- A: what step k+1's GEMM produced, then (k >= K0) this step's gate derivative ----
        const bool have_prev = k + 1 < K, prev_forced = have_prev && k + 1 < S;
        float dh_in = 0.0f;
        if (have_prev) {
            const float v_ = (part[i] + part[s + i]) + (part[2 * s + i] + part[3 * s + i]);
            if (prev_forced) {
                if (dlstates_t) dlstates_t[((size_t)(k + 1 - K0) * B + b) * s + i] = v_;
            } else {
                dh_in = v_;
            }
        }
        if (k < K0) {   // past the first step: what is left goes to the initial state
            if (dh0) dh0[(size_t)b * s + i] = dh_in;
            if (dc0) dc0[(size_t)b * s + i] = dcc;
            break;
        }
        const size_t kb = (size_t)k * B + b;
        const float dhn = cur.dhd + dh_in + (dh_all ? dh_all[kb * s + i] : 0.0f);
        const float gi = cur.g[0], gf = cur.g[1], gg = cur.g[2], go = cur.g[3];
        const float tc = tanh_(cur.g[4]);
        const float dcn = dcc + (dc_all ? dc_all[kb * s + i] : 0.0f) + dhn * go * (1.0f - tc * tc);
        const float d0 = dcn * gg * gi * (1.0f - gi), d1 = dcn * cur.cp * gf * (1.0f - gf),
                    d2 = dcn * gi * (1.0f - gg * gg), d3 = dhn * tc * go * (1.0f - go);
        dgates[i] = d0;
        dgates[s + i] = d1;
        dgates[2 * s + i] = d2;
        dgates[3 * s + i] = d3;
        float* dg = dg_all + kb * 4 * s;
        dg[i] = d0;
        dg[s + i] = d1;
        dg[2 * s + i] = d2;
        dg[3 * s + i] = d3;
        dcc = dcn * gf;   // gradient wrt c_{k-1}
        __syncthreads();
        // ---- B: dh_{k-1} partial of gate gt, column tile n0: sum_{o, tap} Wh_gt[o][ci][tap] * dG_gt[o][j - tap + 1] ----
        {
            const lds_f* bsrc = dgates + gt * s;
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int tap = 0; tap < 3; ++tap) {
                const lds_f* bp = bsrc + colj[tap];
#pragma unroll
                for (int blk = 0; blk < 4; blk += 2) {
                    const float b0 = bp[(4 * blk + q) * hq], b1 = bp[(4 * blk + 4 + q) * hq];
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[tap][blk], b0, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[tap][blk + 1], b1, acc1, 0, 0, 0);
                }
            }
            lds_f* dst = part + gt * s + n0 + r;
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[(4 * q + e) * hq] = acc0[e] + acc1[e];
        }
        cur = nx1;
        nx1 = nx2;
        __syncthreads();
    }
}

template <int MAXT>
__global__ void __launch_bounds__(MAXT)
cell_bwd_kernel(const sur_chunk_params p, const ChunkSpans spans, const float* __restrict__ c_all,
                const float* __restrict__ saved, const float* __restrict__ dh_dec, const float* __restrict__ dh_all,
                const float* __restrict__ dc_all, int B, float* __restrict__ dg_all, float* __restrict__ dh0,
                float* __restrict__ dc0) {
    extern __shared__ __align__(16) float lds[];
    // workgroup -> (chunk of the time axis, sample): the chunks' chains are independent (TBPTT cuts the graph)
    const sur_chunk_span sp = spans.sp[blockIdx.x / B];
    const int b = blockIdx.x % B, s = p.cs * p.hq;
#ifndef SUR_STAMP
    if constexpr ((MAXT & 255) == 0) {
        if (p.cs == 16 && p.hq * 16 == MAXT) {   // one (channel, position) element per thread
            cell_chain_backward<MAXT / 256>(p, lds, sp, b, B, c_all, saved, dh_dec, dh_all, dc_all, dg_all, dh0, dc0);
            return;
        }
    }
#endif
    const int K0 = sp.k0, K = sp.k1, S = sp.k0 + sp.s;   // steps K0 .. K-1 (global time index), the first sp.s teacher forced
    const float* __restrict__ c0 = sp.c0;
    const int hc_bstride = sp.hc_bstride;
    float* __restrict__ dlstates_t = sp.dlstates_t;
    StepLayout L{};
    float* blk[2] = {lds, lds + 5 * s};   // [gates | c_k] of the step at hand / of the next one (ping-pong)
    L.dgates = lds + 10 * s;
    float* part = L.dgates + 4 * s;        // four partial dh tiles
    float* wbase = part + 4 * s;
    const size_t save_stride = step_saved_floats(p);
    const int npieces = (5 * s) / DMA_PIECE;   // a whole number: checked on the host
    auto fetch_block = [&](int kk) {
        const float* src = saved + ((size_t)kk * B + b) * save_stride;
        float* dst = blk[kk & 1];
        const int lane = threadIdx.x & 63;
        for (int j = threadIdx.x >> 6; j < npieces; j += blockDim.x >> 6)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + j * DMA_PIECE + lane * 4),
                                             (__attribute__((address_space(3))) void*)(dst + j * DMA_PIECE + lane * 4), 16, 0, 0);
    };
    float cp[CELL_EPT], dhd[CELL_EPT], dcc[CELL_EPT];
    auto prefetch = [&](int kk) {   // c_{kk-1} and the decoder's dh of step kk
#pragma unroll
        for (int e = 0; e < CELL_EPT; ++e) {
            const int i = threadIdx.x + e * MAXT;
            if (i < s) {
                cp[e] = (kk > K0) ? c_all[((size_t)(kk - 1) * B + b) * s + i] : c0[(size_t)b * hc_bstride + i];
                dhd[e] = dh_dec[((size_t)kk * B + b) * s + i];
            }
        }
    };
    fetch_block(K - 1);
    prefetch(K - 1);
    const float* w[SUR_ST_NPARAM];
    stage_range<ST_NLSTM>(p, 0, wbase, w);
#pragma unroll
    for (int e = 0; e < CELL_EPT; ++e) dcc[e] = 0.0f;
    __syncthreads();

    for (int k = K - 1; k >= K0 - 1; --k) {
        // ---- A: what step k+1's GEMM produced, then (k >= K0) this step's gate derivative ----
        const bool have_prev = k + 1 < K;               // part[] holds d loss / d h_in of step k+1
        const bool prev_forced = have_prev && k + 1 < S; // ... which was the encoded given state, not h_k
        const float* g_ = k >= K0 ? blk[k & 1] : nullptr;
#pragma unroll
        for (int e = 0; e < CELL_EPT; ++e) {
            const int i = threadIdx.x + e * MAXT;
            if (i >= s) continue;
            float dh_in = 0.0f;
            if (have_prev) {
                const float v_ = (part[i] + part[s + i]) + (part[2 * s + i] + part[3 * s + i]);
                if (prev_forced) {
                    if (dlstates_t) dlstates_t[((size_t)(k + 1 - K0) * B + b) * s + i] = v_;
                } else {
                    dh_in = v_;
                }
            }
            if (k < K0) {   // past the first step: what is left goes to the initial state
                if (dh0) dh0[(size_t)b * s + i] = dh_in;  // non-zero only if step 0 was free running (S == 0)
                if (dc0) dc0[(size_t)b * s + i] = dcc[e];
                continue;
            }
            const size_t kb = (size_t)k * B + b;
            const float dhn = dhd[e] + dh_in + (dh_all ? dh_all[kb * s + i] : 0.0f);
            const float gi = g_[i], gf = g_[s + i], gg = g_[2 * s + i], go = g_[3 * s + i];
            const float tc = tanh_(g_[4 * s + i]);
            const float dcn = dcc[e] + (dc_all ? dc_all[kb * s + i] : 0.0f) + dhn * go * (1.0f - tc * tc);
            const float d0 = dcn * gg * gi * (1.0f - gi), d1 = dcn * cp[e] * gf * (1.0f - gf),
                        d2 = dcn * gi * (1.0f - gg * gg), d3 = dhn * tc * go * (1.0f - go);
            L.dgates[i] = d0;
            L.dgates[s + i] = d1;
            L.dgates[2 * s + i] = d2;
            L.dgates[3 * s + i] = d3;
            float* dg = dg_all + kb * 4 * s;
            dg[i] = d0;
            dg[s + i] = d1;
            dg[2 * s + i] = d2;
            dg[3 * s + i] = d3;
            dcc[e] = dcn * gf;  // gradient wrt c_{k-1}
        }
        if (k < K0) break;
        __syncthreads();
        STAMP(120);
        // ---- B: prefetches for step k-1, then dh_{k-1} partials ----
        if (k > K0) {
            fetch_block(k - 1);
            prefetch(k - 1);
        }
        STAMP(121);
        cell_dh_gemm(p, L, w, part);   // ends with the barrier that also retires the DMA
        STAMP(122);
    }
}

// Everything of the cell backward that is not recurrent, for all (step, sample) pairs in parallel: the gradient wrt
// the latent action and the LSTM weight / bias gradients (into this workgroup's partial row).
template <bool GL>      // as dec_bwd_kernel
__global__ void __launch_bounds__(TPB, PAR_OCC)
cell_wgrad_kernel(const sur_chunk_params p, const ChunkSpans spans, const float* __restrict__ xlat_t,
                  const float* __restrict__ h_all, const float* __restrict__ dg_all, int K, int B,
                  float* __restrict__ dxlat_t, int row_base) {
    extern __shared__ __align__(16) float lds[];
    const int s = p.cs * p.hq, nx = p.ca * p.hq, M = K * B, hq = p.hq, hs = hq + 4;
    StepLayout L{};
    L.dx = lds;
    L.x = L.dx + nx;
    L.h = L.x + p.ca * hs;
    L.dgates = L.h + p.cs * hs;
    float* wbase = L.dgates + 4 * p.cs * hs;
    // of the LSTM's weights only the four Wx_g are read here (dx); staged back to back.  (All twelve tensors were 15.6 KB: with
    // the padded rows one workgroup too many for three per CU -- measured: 0.571 instead of 0.541 ms per step.)
    const float* w[SUR_ST_NPARAM] = {};
    int wx_floats = 0;
    for (int gt = 0; gt < 4; ++gt) {
        const int i = SUR_ST_WXI + 3 * gt;     // parameter order: Wx_g, b_g, Wh_g per gate
        for (int j = threadIdx.x; j < p.size[i]; j += blockDim.x) wbase[wx_floats + j] = p.w[i][j];
        w[i] = wbase + wx_floats;
        wx_floats += p.size[i];
    }
    int psize_lstm = 0;
    for (int i = 0; i < ST_NLSTM; ++i) psize_lstm += p.size[i];
    int psize = psize_lstm;
    for (int i = ST_NLSTM; i < SUR_ST_NPARAM; ++i) psize += p.size[i];
    float* row = p.partial + (size_t)(row_base + blockIdx.x) * psize;
    typedef typename std::conditional<GL, lds_f*, float*>::type GP;
    GP gacc;
    if constexpr (GL) gacc = (lds_f*)(wbase + wx_floats);
    else gacc = row;
    GP g[SUR_ST_NPARAM];
    {
        int off = 0;
        for (int i = 0; i < ST_NLSTM; ++i) {
            g[i] = gacc + off;
            off += p.size[i];
        }
        if (GL)
            for (int j = threadIdx.x; j < psize_lstm; j += blockDim.x) gacc[j] = 0.0f;
    }
    __syncthreads();
    for (int m = blockIdx.x; m < M; m += gridDim.x) {
        const int k = m / B, b = m - k * B;
        int si = 0;
        for (int j = 1; j < spans.n; ++j) si = k >= spans.sp[j].k0 ? j : si;
        const sur_chunk_span sp = spans.sp[si];
        const float* hin = (k - sp.k0 < sp.s) ? sp.lstates_t + ((size_t)(k - sp.k0) * B + b) * s
                                               : (k > sp.k0 ? h_all + ((size_t)(k - 1) * B + b) * s : sp.h0 + (size_t)b * sp.hc_bstride);
        // rows land hs floats apart (float4 granules: hq is a multiple of 4)
        const int q4 = hq >> 2;
        auto padded = [&](int i4) { const int row = i4 / q4; return row * hs + 4 * (i4 - row * q4); };
        {
            const float4* xs = reinterpret_cast<const float4*>(xlat_t + (size_t)m * nx);
            const float4* hsrc = reinterpret_cast<const float4*>(hin);
            const float4* gs = reinterpret_cast<const float4*>(dg_all + (size_t)m * 4 * s);
            for (int i = threadIdx.x; i < (nx >> 2); i += blockDim.x) *reinterpret_cast<float4*>(L.x + padded(i)) = xs[i];
            for (int i = threadIdx.x; i < (s >> 2); i += blockDim.x) *reinterpret_cast<float4*>(L.h + padded(i)) = hsrc[i];
            constexpr int U = 4;    // all of a thread's loads of a round in flight before the first store (lds_load_v4)
            for (int i0 = threadIdx.x; i0 < s; i0 += U * TPB) {
                float4 v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) v[u] = gs[i0 + u * TPB < s ? i0 + u * TPB : i0];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (i0 + u * TPB < s) *reinterpret_cast<float4*>(L.dgates + padded(i0 + u * TPB)) = v[u];
            }
            __syncthreads();
        }
        cell_wgrad_gemms(p, L, w, g, hs);
        if (dxlat_t)
            for (int i = threadIdx.x; i < nx; i += blockDim.x) dxlat_t[(size_t)m * nx + i] = L.dx[i];
        __syncthreads();
    }
    if constexpr (GL) add_to_row(row, (const float*)gacc, psize_lstm);
}

}  // namespace

#endif  // SUR_CHUNK_H
