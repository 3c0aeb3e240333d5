// sur_encoder.h -- the encoder kernels: the whole-encoder forward / backward (enc_fwd_kernel, enc_bwd_kernel, enc_bwd_multi_kernel
// and their LDS layout), and the one-residual-block-per-launch kernels with their geometry (EncBlockGeom), their wide jobs
// (EncBlockJob, EncFwdJob) and the narrow job that rides behind them (NarrowJob, narrow_job).
// Needs sur_params.h, sur_resblock.h and sur_narrow.h.
#ifndef SUR_ENCODER_H
#define SUR_ENCODER_H

#include <type_traits>

#include "../../include/surrogate_hip.h"
#include "sur_narrow.h"
#include "sur_params.h"
#include "sur_resblock.h"

namespace {

struct EncLayout {
    RBBuf rb[3];
    float *g1, *g2, *g3, *xh, *dA, *dB, *end;
};

__host__ __device__ inline int enc_max_act(const sur_encoder_params& p) {
    int h = p.n, m = p.c[0] * p.n;
    for (int b = 0; b < 3; ++b) {
        h /= p.stride[b];
        const int a = p.c[b + 1] * h;
        m = a > m ? a : m;
    }
    return m;
}

__host__ __device__ inline int enc_act_floats(const sur_encoder_params& p, bool backward) {
    int h = p.n, total = p.c[0] * p.n;
    for (int b = 0; b < 3; ++b) {
        h /= p.stride[b];
        total += 7 * p.c[b + 1] * h;
    }
    if (backward) total += 6 * enc_max_act(p);
    return total;
}

__device__ void enc_layout(const sur_encoder_params& p, float* lds, bool backward, EncLayout& L) {
    float* cur = lds;
    int h = p.n;
    float* in = cur;
    cur += p.c[0] * p.n;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        RBBuf& r = L.rb[b];
        r.cin = p.c[b];
        r.cout = p.c[b + 1];
        r.hin = h;
        r.stride = p.stride[b];
        h /= p.stride[b];
        r.hout = h;
        const int a = r.cout * r.hout;
        r.in = in;
        r.skip = cur;
        r.a1pre = cur + a;
        r.a1 = cur + 2 * a;
        r.a2pre = cur + 3 * a;
        r.a2 = cur + 4 * a;
        r.s = cur + 5 * a;
        r.out = cur + 6 * a;
        cur += 7 * a;
        in = r.out;
    }
    if (backward) {
        const int m = enc_max_act(p);
        L.g1 = cur;
        L.g2 = cur + m;
        L.g3 = cur + 2 * m;
        L.xh = cur + 3 * m;
        L.dA = cur + 4 * m;
        L.dB = cur + 5 * m;
        cur += 6 * m;
    }
    L.end = cur;
}

// floats of one sample's forward intermediates (everything after the input in the LDS layout), as enc_fwd_kernel can
// save them for enc_bwd_kernel
__host__ __device__ inline int enc_saved_floats(const sur_encoder_params& p) { return enc_act_floats(p, false) - p.c[0] * p.n; }

__global__ void __launch_bounds__(TPB) enc_fwd_kernel(const sur_encoder_params p, const float* __restrict__ x, int m_total,
                                                      float* __restrict__ z, float* __restrict__ saved) {
    extern __shared__ __align__(16) float lds[];
    EncLayout L;
    enc_layout(p, lds, false, L);
    ParamViews<SUR_ENC_NPARAM> v;
    stage_weights<SUR_ENC_NPARAM>(p.w, p.size, L.end, v);
    const int nin = p.c[0] * p.n, nout = L.rb[2].cout * L.rb[2].hout;
    for (int m = blockIdx.x; m < m_total; m += gridDim.x) {
        lds_load(L.rb[0].in, x + (size_t)m * nin, nin);
#pragma unroll
        for (int b = 0; b < 3; ++b) rb_forward(L.rb[b], v.w + b * SUR_RB_NPARAM);
        if (saved) {  // every intermediate of the three blocks: the backward kernel then skips its forward recomputation
            const int n4 = enc_saved_floats(p) >> 2;
            float4* dst = reinterpret_cast<float4*>(saved + (size_t)m * (n4 << 2));
            const float4* src = reinterpret_cast<const float4*>(L.rb[0].skip);
            for (int i = threadIdx.x; i < n4; i += blockDim.x) dst[i] = src[i];
        }
        lds_store(z + (size_t)m * nout, L.rb[2].out, nout);
    }
}

// Two workgroups per CU (2 waves per SIMD): the kernel is bound by dependent-phase latency, so a second resident
// workgroup fills the issue slots the first one leaves empty.  Costs ~118 spilled dwords, measured +10 % on the step.
#ifndef ENC_BWD_OCC
#define ENC_BWD_OCC 2
#endif
// body of the encoder backward for the workgroup `wg` of `nwg` working on one encoder (job)
__device__ __forceinline__ void enc_bwd_body(const sur_encoder_params& p, const float* __restrict__ x,
                                             const float* __restrict__ dz, int m_total, float* __restrict__ dx, int grads_in_lds,
                                             int row_base, const float* __restrict__ saved, int wg, int nwg, float* lds) {
    STAMP(32);
    EncLayout L;
    enc_layout(p, lds, true, L);
    ParamViews<SUR_ENC_NPARAM> v;
    stage_weights<SUR_ENC_NPARAM>(p.w, p.size, L.end, v);
    STAMP(33);
    const int psize = psize_of<SUR_ENC_NPARAM>(p.size);
    float* row = p.partial + (size_t)(row_base + wg) * psize;
    float* gacc = grads_in_lds ? L.end + psize : row;
    setup_grads<SUR_ENC_NPARAM>(p.size, gacc, grads_in_lds != 0, v);
    STAMP(34);
    const int nin = p.c[0] * p.n, nout = L.rb[2].cout * L.rb[2].hout;
    for (int m = wg; m < m_total; m += nwg) {
        lds_load(L.rb[0].in, x + (size_t)m * nin, nin);
        STAMP(35);
        if (saved) {  // the second workgroup resident on this CU covers the load latency
            const int nsv = enc_saved_floats(p);
            lds_load_v4(L.rb[0].skip, saved + (size_t)m * nsv, nsv >> 2);
        } else {
#pragma unroll
            for (int b = 0; b < 3; ++b) rb_forward(L.rb[b], v.w + b * SUR_RB_NPARAM);
        }
        STAMP(36);
        lds_load(L.dA, dz + (size_t)m * nout, nout);
        STAMP(37);
        float *dout = L.dA, *din = L.dB;
#pragma unroll
        for (int b = 2; b >= 0; --b) {
            rb_backward(L.rb[b], v.w + b * SUR_RB_NPARAM, v.g + b * SUR_RB_NPARAM, dout, din, L.g1, L.g2, L.g3, L.xh);
            STAMP(38 + b);
            float* t = dout;
            dout = din;
            din = t;
        }
        if (dx) lds_store(dx + (size_t)m * nin, dout, nin);
        STAMP(41);
    }
    if (grads_in_lds) {
        add_to_row(row, gacc, psize);
    }
    STAMP(42);
}

__global__ void __launch_bounds__(TPB, ENC_BWD_OCC) enc_bwd_kernel(const sur_encoder_params p, const float* __restrict__ x,
                                                      const float* __restrict__ dz, int m_total, float* __restrict__ dx,
                                                      int grads_in_lds, int row_base, const float* __restrict__ saved) {
    extern __shared__ __align__(16) float lds[];
    enc_bwd_body(p, x, dz, m_total, dx, grads_in_lds, row_base, saved, blockIdx.x, gridDim.x, lds);
}

// Several encoder backward jobs (different encoders / inputs) in ONE launch: the workgroups of all jobs are
// dispatched together, so a long job never queues behind a short one on the same hardware queue.
struct EncBwdJob {
    sur_encoder_params p;
    const float* x;
    const float* dz;
    const float* saved;
    int m, row_base, wg_begin, wg_count, grads_in_lds;
};

__global__ void __launch_bounds__(TPB, ENC_BWD_OCC) enc_bwd_multi_kernel(const EncBwdJob j0, const EncBwdJob j1, const EncBwdJob j2,
                                                                         int njobs) {
    extern __shared__ __align__(16) float lds[];
    const int wg = blockIdx.x;
    if (njobs > 2 && wg >= j2.wg_begin)
        enc_bwd_body(j2.p, j2.x, j2.dz, j2.m, nullptr, j2.grads_in_lds, j2.row_base, j2.saved, wg - j2.wg_begin, j2.wg_count, lds);
    else if (njobs > 1 && wg >= j1.wg_begin)
        enc_bwd_body(j1.p, j1.x, j1.dz, j1.m, nullptr, j1.grads_in_lds, j1.row_base, j1.saved, wg - j1.wg_begin, j1.wg_count, lds);
    else
        enc_bwd_body(j0.p, j0.x, j0.dz, j0.m, nullptr, j0.grads_in_lds, j0.row_base, j0.saved, wg, j0.wg_count, lds);
}

// ---------------------------------------------------------------------------------------------
// Encoder backward, one residual block per launch (block 2, then 1, then 0): a third of the code and of the LDS
// of the whole-encoder kernel per launch, so it no longer sits at the 256-VGPR cap and more workgroups share a CU.
// The blocks' forward intermediates come from the `saved` buffer of enc_fwd_kernel; the gradient between blocks
// travels through a small workspace ([M, c1*h1 + c2*h2] floats).
// ---------------------------------------------------------------------------------------------
struct EncBlockGeom {
    int cin, cout, hin, hout, stride;
    int saved_off;      // offset of this block's 7 intermediates in a sample's saved record
    int in_saved_off;   // offset of this block's INPUT (= previous block's `out`) in the record, -1: the raw input x
    int param_off;      // column of this block's parameters in a partial-gradient row
    int psize_blk;      // their total size
};

__host__ __device__ inline EncBlockGeom enc_block_geom(const sur_encoder_params& p, int blk) {
    EncBlockGeom g{};
    int h = p.n, off = 0, prev_out = -1;
    for (int b = 0; b <= blk; ++b) {
        g.cin = p.c[b];
        g.cout = p.c[b + 1];
        g.hin = h;
        g.stride = p.stride[b];
        h /= p.stride[b];
        g.hout = h;
        g.saved_off = off;
        g.in_saved_off = prev_out;
        const int a = g.cout * g.hout;
        prev_out = off + 6 * a;
        off += 7 * a;
    }
    g.param_off = 0;
    for (int i = 0; i < SUR_RB_NPARAM * blk; ++i) g.param_off += p.size[i];
    g.psize_blk = 0;
    for (int i = 0; i < SUR_RB_NPARAM; ++i) g.psize_blk += p.size[SUR_RB_NPARAM * blk + i];
    return g;
}

// workspace floats per sample: the gradients wrt the inputs of blocks 1 and 2
__host__ __device__ inline int enc_ws_floats(const sur_encoder_params& p) {
    const int h1 = p.n / p.stride[0], h2 = h1 / p.stride[1];
    return p.c[1] * h1 + p.c[2] * h2;
}

// LDS of the block backward: only what rb_backward reads is resident -- the input, four of the seven saved intermediates
// (a1pre, a1, a2pre: contiguous in the record; s), and scratch that reuses dead buffers (g2 over dout, g3 over s).
// 2 nin + 7 a floats instead of 2 nin + 13 a: at N = 256 a third workgroup fits a CU.
__host__ __device__ inline int enc_block_act_floats(const EncBlockGeom& g) {
    const int a = g.cout * g.hout, nin = g.cin * g.hin;
    return nin + 4 * a + 2 * a + a + nin;   // in, {a1pre a1 a2pre s}, {g1 xh}, dout (= g2), din
}

struct EncBlockJob {
    sur_encoder_params p;
    const float* x;
    const float* dz;
    const float* saved;
    float* ws;
    int m, row_base, wg_begin, wg_count, grads_in_lds;
};

template <bool GL>     // GL: this job's gradient accumulators are in LDS (j.grads_in_lds), as LDS-typed pointers (conv_bwd_weight)
__device__ __forceinline__ void enc_block_bwd_body(const EncBlockJob& j, int blk, int wg, float* lds) {
    const sur_encoder_params& p = j.p;
    const EncBlockGeom gm = enc_block_geom(p, blk);
    const int a = gm.cout * gm.hout, nin = gm.cin * gm.hin;
    RBBuf rb{};
    rb.cin = gm.cin; rb.cout = gm.cout; rb.hin = gm.hin; rb.hout = gm.hout; rb.stride = gm.stride;
    float* cur = lds;
    rb.in = cur; cur += nin;
    rb.a1pre = cur; rb.a1 = cur + a; rb.a2pre = cur + 2 * a; rb.s = cur + 3 * a; cur += 4 * a;   // skip, a2, out: not read
    float *g1 = cur, *xh = cur + a;
    cur += 2 * a;
    float* dout = cur; cur += a;
    float* g2 = dout;     // dout is consumed by the first LayerNorm backward, before g2 is written
    float* g3 = rb.s;     // likewise s
    float* din = cur; cur += nin;
    ParamViews<SUR_RB_NPARAM> v;
    const int sbase = 64 + 16 * blk;   // SUR_STAMP ids of this block's phases
    (void)sbase;
    STAMP(sbase + 0);
    stage_weights<SUR_RB_NPARAM>(p.w + SUR_RB_NPARAM * blk, p.size + SUR_RB_NPARAM * blk, cur, v);
    const int psize = psize_of<SUR_ENC_NPARAM>(p.size);
    float* row = p.partial + (size_t)(j.row_base + wg) * psize + gm.param_off;
    typedef typename std::conditional<GL, lds_f*, float*>::type GP;
    GP gacc, g[SUR_RB_NPARAM];
    if constexpr (GL) gacc = (lds_f*)(cur + gm.psize_blk);
    else gacc = row;
    {
        int off = 0;
#pragma unroll
        for (int i = 0; i < SUR_RB_NPARAM; ++i) {
            g[i] = gacc + off;
            off += p.size[SUR_RB_NPARAM * blk + i];
        }
        if (GL)
            for (int t = threadIdx.x; t < off; t += blockDim.x) gacc[t] = 0.0f;
        __syncthreads();
    }
    STAMP(sbase + 1);
    const int nsv = enc_saved_floats(p), nws = enc_ws_floats(p);
    const int h1 = p.n / p.stride[0];
    const int ws_in_off = blk == 2 ? p.c[1] * h1 : 0;       // where this block writes d loss / d its input (blocks 2, 1)
    const int ws_out_off = blk == 1 ? p.c[1] * h1 : 0;      // where block 1 reads d loss / d its output (written by block 2)
    for (int m = wg; m < j.m; m += j.wg_count) {
        const float* rec = j.saved + (size_t)m * nsv;
        const float* dsrc = blk == 2 ? j.dz + (size_t)m * a : j.ws + (size_t)m * nws + (blk == 1 ? ws_out_off : 0);
        // this block's input, four of its seven intermediates, the gradient wrt its output.  record: skip | a1pre a1 a2pre | a2 | s | out
        // (one loader with every load of the sample in flight and a single barrier measured 3 % SLOWER on the whole step than
        // these four: 40 more live registers spill in a 128-VGPR kernel, and the co-resident workgroups cover the round trips)
        // by LDS-DMA: all four in flight at once, one wait + barrier (through registers each was a round trip of its own -- a sixth of
        // the block's time -- and holding them all in registers spilled; the DMA needs none)
        if (gm.in_saved_off < 0) lds_dma_v4(rb.in, j.x + (size_t)m * nin, nin >> 2);
        else lds_dma_v4(rb.in, rec + gm.in_saved_off, nin >> 2);
        lds_dma_v4(rb.a1pre, rec + gm.saved_off + a, (3 * a) >> 2);
        lds_dma_v4(rb.s, rec + gm.saved_off + 5 * a, a >> 2);
        lds_dma_v4(dout, dsrc, a >> 2);
        lds_dma_wait();
        STAMP(sbase + 2);
        rb_backward(rb, v.w, g, dout, din, g1, g2, g3, xh, sbase + 3, blk > 0);
        if (blk > 0) {
            float* dst = j.ws + (size_t)m * nws + (blk == 2 ? ws_in_off : 0);
            for (int i = threadIdx.x; i < nin; i += blockDim.x) dst[i] = din[i];
        }
        __syncthreads();
        STAMP(sbase + 9);
    }
    if constexpr (GL) add_to_row(row, (const float*)gacc, gm.psize_blk);
    STAMP(sbase + 10);
}


// A narrow job (one wave per sample, see "Narrow residual block") has a flat argument block whose arrays are only ever indexed
// by constants (as members of the wide jobs' structs -- indexed by the block number -- they went through scratch: 3 KB per
// lane).  Its workgroups ride BEHIND the wide jobs' in the same launch (`narrow_begin` of the multi kernels: as launches of
// their own, serialized behind the wide ones, the narrow kernels lost what they had gained); a launch set without a wide job
// uses the standalone kernels below.
struct NarrowJob {
    const float* w[SUR_RB_NPARAM];   // this block's weights (global)
    int size[SUR_RB_NPARAM];
    int cin, hin, cout, hout, stride;
    int nsv, nws;                    // floats per sample of the saved record / of the inter-block gradient workspace
    int saved_off, in_saved_off;     // this block's intermediates / its input inside a record (-1: the raw input x)
    int ws_in_off, ws_out_off;       // where the block writes d loss / d input, reads d loss / d output (blocks 1, 0)
    int blk, m, wg_count, psize_blk, need_din;
    const float* x;
    const float* dz;                 // backward, block 2: d loss / d z
    float* z;                        // forward, block 2: the encoder output
    float* saved;
    float* ws;
    float* rows;                     // backward: &partial[row_base][param_off]; workgroup wg adds to rows + wg * row_stride
    int row_stride;
};

__device__ __forceinline__ void narrow_stage(const NarrowJob& j, float* dst, const float** w) {
    int off = 0;
#pragma unroll
    for (int i = 0; i < SUR_RB_NPARAM; ++i) {
        w[i] = dst + off;
        for (int t = threadIdx.x; t < j.size[i]; t += blockDim.x) dst[off + t] = j.w[i][t];
        off += j.size[i];
    }
    __syncthreads();
}

__device__ __forceinline__ void enc_narrow_fwd_run(const NarrowJob& j, int wg, float* lds) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwv = blockDim.x >> 6;
    const int a = j.cout * j.hout, nin = j.cin * j.hin;
    const int wf = nr_fwd_wave_floats(j.cin, j.hin, j.cout, j.hout);
    const float* w[SUR_RB_NPARAM];
    narrow_stage(j, lds + nwv * wf, w);
    const int passes = (j.m + nwv - 1) / nwv;
    for (int mp = wg; mp < passes; mp += j.wg_count) {
        const int m = mp * nwv + wave;
        if (m < j.m) {
            float* rec = j.saved + (size_t)m * j.nsv;
            const float* src = j.in_saved_off < 0 ? j.x + (size_t)m * nin : rec + j.in_saved_off;
            nr_block_forward(j.cin, j.hin, j.cout, j.hout, j.stride, w, lds + wave * wf, src, rec + j.saved_off,
                             j.z ? j.z + (size_t)m * a : nullptr, lane);
        }
    }
}

__global__ void __launch_bounds__(TPB) enc_narrow_fwd_kernel(const NarrowJob j) {
    extern __shared__ __align__(16) float lds[];
    enc_narrow_fwd_run(j, blockIdx.x, lds);
}

__device__ __forceinline__ void enc_narrow_bwd_run(const NarrowJob& j, int wg, float* lds) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwv = blockDim.x >> 6;
    const int a = j.cout * j.hout, nin = j.cin * j.hin;
    const int wf = nr_bwd_wave_floats(j.cin, j.hin, j.cout, j.hout, j.psize_blk);
    float* wl = lds + wave * wf;
    float* gacc = wl + nin + 6 * a;
    const float* w[SUR_RB_NPARAM];
    float* g[SUR_RB_NPARAM];
    {
        int off = 0;
#pragma unroll
        for (int i = 0; i < SUR_RB_NPARAM; ++i) {
            g[i] = gacc + off;
            off += j.size[i];
        }
        for (int i = lane; i < j.psize_blk; i += 64) gacc[i] = 0.0f;
    }
    narrow_stage(j, lds + nwv * wf, w);
    const int passes = (j.m + nwv - 1) / nwv;
    for (int mp = wg; mp < passes; mp += j.wg_count) {
        const int m = mp * nwv + wave;
        if (m < j.m) {
            const float* rec = j.saved + (size_t)m * j.nsv;
            const float* in_src = j.in_saved_off < 0 ? j.x + (size_t)m * nin : rec + j.in_saved_off;
            const float* dsrc = j.blk == 2 ? j.dz + (size_t)m * a : j.ws + (size_t)m * j.nws + j.ws_out_off;
            float* din_dst = j.need_din ? j.ws + (size_t)m * j.nws + j.ws_in_off : nullptr;
            nr_block_backward(j.cin, j.hin, j.cout, j.hout, j.stride, w, g, wl, in_src, rec + j.saved_off, dsrc, din_dst, j.need_din != 0,
                              lane);
        }
    }
    __syncthreads();
    float* row = j.rows + (size_t)wg * j.row_stride;
    for (int i = threadIdx.x; i < j.psize_blk; i += blockDim.x) {
        float t = 0.0f;
        for (int wv = 0; wv < nwv; ++wv) t += lds[wv * wf + nin + 6 * a + i];
        row[i] += t;
    }
}

__global__ void __launch_bounds__(TPB) enc_narrow_bwd_kernel(const NarrowJob j) {
    extern __shared__ __align__(16) float lds[];
    enc_narrow_bwd_run(j, blockIdx.x, lds);
}

static NarrowJob narrow_job(const sur_encoder_params& p, int blk, int m) {
    NarrowJob j{};
    const EncBlockGeom gm = enc_block_geom(p, blk);
    for (int i = 0; i < SUR_RB_NPARAM; ++i) {
        j.w[i] = p.w[SUR_RB_NPARAM * blk + i];
        j.size[i] = p.size[SUR_RB_NPARAM * blk + i];
    }
    j.cin = gm.cin; j.hin = gm.hin; j.cout = gm.cout; j.hout = gm.hout; j.stride = gm.stride;
    j.nsv = enc_saved_floats(p);
    j.nws = enc_ws_floats(p);
    j.saved_off = gm.saved_off;
    j.in_saved_off = gm.in_saved_off;
    const int h1 = p.n / p.stride[0];
    j.ws_in_off = blk == 2 ? p.c[1] * h1 : 0;
    j.ws_out_off = blk == 1 ? p.c[1] * h1 : 0;
    j.blk = blk;
    j.m = m;
    j.psize_blk = gm.psize_blk;
    j.need_din = blk > 0 ? 1 : 0;
    return j;
}

#ifndef ENC_BLK_OCC
#define ENC_BLK_OCC 3   // 168 VGPRs, no spills.  Four per CU (128 VGPRs, ~30 spilled dwords) measured best while the action encoder's
                        // 640 samples went through these workgroups too; with those on the narrow path a launch is <= 480 workgroups
                        // and the spills cost more than the residency gives: 0.496 vs 0.511 ms per step at N = 256 (2 per CU: 0.499)
#endif
template <bool GL>     // every wide job keeps its accumulators in LDS (the host clears grads_in_lds of all of them otherwise)
__global__ void __launch_bounds__(TPB, ENC_BLK_OCC)
enc_block_bwd_multi_kernel(const EncBlockJob j0, const EncBlockJob j1, const EncBlockJob j2, int njobs, int blk, const NarrowJob nj,
                           int narrow_begin) {
    extern __shared__ __align__(16) float lds[];
    const int wg = blockIdx.x;
    if (wg >= narrow_begin) {      // the workgroups behind the wide jobs' carry the narrow job (one wave per sample)
        enc_narrow_bwd_run(nj, wg - narrow_begin, lds);
        return;
    }
    if (njobs > 2 && wg >= j2.wg_begin) enc_block_bwd_body<GL>(j2, blk, wg - j2.wg_begin, lds);
    else if (njobs > 1 && wg >= j1.wg_begin) enc_block_bwd_body<GL>(j1, blk, wg - j1.wg_begin, lds);
    else enc_block_bwd_body<GL>(j0, blk, wg, lds);
}

// Encoder forward, one residual block per launch (block 0, 1, 2), several jobs per launch: for large sample counts the
// same trade as in the backward pass -- a third of the registers and LDS per launch, more workgroups per CU.  Each
// block reads its input from the previous block's record in `saved` and writes its own seven intermediates there.
struct EncFwdJob {
    sur_encoder_params p;
    const float* x;
    float* z;
    float* saved;
    int m, wg_begin, wg_count;
};

__device__ __forceinline__ void enc_block_fwd_body(const EncFwdJob& j, int blk, int wg, float* lds) {
    const sur_encoder_params& p = j.p;
    const EncBlockGeom gm = enc_block_geom(p, blk);
    const int a = gm.cout * gm.hout, nin = gm.cin * gm.hin;
    RBBuf rb{};
    rb.cin = gm.cin; rb.cout = gm.cout; rb.hin = gm.hin; rb.hout = gm.hout; rb.stride = gm.stride;
    float* cur = lds;
    rb.in = cur; cur += nin;
    rb.skip = cur; rb.a1pre = cur + a; rb.a1 = cur + 2 * a; rb.a2pre = cur + 3 * a; rb.a2 = cur + 4 * a; rb.s = cur + 5 * a;
    rb.out = cur + 6 * a; cur += 7 * a;
    ParamViews<SUR_RB_NPARAM> v;
    stage_weights<SUR_RB_NPARAM>(p.w + SUR_RB_NPARAM * blk, p.size + SUR_RB_NPARAM * blk, cur, v);
    const int nsv = enc_saved_floats(p);
    for (int m = wg; m < j.m; m += j.wg_count) {
        float* rec = j.saved + (size_t)m * nsv;
        if (gm.in_saved_off < 0) lds_load(rb.in, j.x + (size_t)m * nin, nin);
        else lds_load_v4(rb.in, rec + gm.in_saved_off, nin >> 2);
        rb_forward(rb, v.w);
        float4* dst = reinterpret_cast<float4*>(rec + gm.saved_off);
        const float4* src = reinterpret_cast<const float4*>(rb.skip);
        for (int i = threadIdx.x; i < (7 * a) >> 2; i += blockDim.x) dst[i] = src[i];
        if (blk == 2)
            for (int i = threadIdx.x; i < a; i += blockDim.x) j.z[(size_t)m * a + i] = rb.out[i];
        __syncthreads();
    }
}


__global__ void __launch_bounds__(TPB, ENC_BLK_OCC)
enc_block_fwd_multi_kernel(const EncFwdJob j0, const EncFwdJob j1, int njobs, int blk, const NarrowJob nj, int narrow_begin) {
    extern __shared__ __align__(16) float lds[];
    const int wg = blockIdx.x;
    if (wg >= narrow_begin) {
        enc_narrow_fwd_run(nj, wg - narrow_begin, lds);
        return;
    }
    if (njobs > 1 && wg >= j1.wg_begin) enc_block_fwd_body(j1, blk, wg - j1.wg_begin, lds);
    else enc_block_fwd_body(j0, blk, wg, lds);
}

}  // namespace

#endif  // SUR_ENCODER_H
