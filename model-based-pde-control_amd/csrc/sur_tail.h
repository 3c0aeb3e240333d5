// sur_tail.h -- the tail of a step: the gradient reduction over partial rows with or without Adam (flush_*), the row fold
// (fold_rows_kernel), Adam from g[] (adam_all_kernel) and the clipped update (flush_all_sumsq_kernel, clip_adam_kernel).
// Needs sur_common.h and surrogate_hip.h.
#ifndef SUR_TAIL_H
#define SUR_TAIL_H

#include "../../include/surrogate_hip.h"
#include "sur_common.h"

namespace {

// Adam's bias correction 1 - beta^step.  1.0f - powf(beta, step) cancels at small step counts: beta^step lies within a few
// (1 - beta) of 1, where fp32 resolves 2^-24, so at step 2 of beta = 0.999 the difference 0.002 keeps 15 of its 24 bits
// and the step multiplier sqrt(bc2) / bc1 is off by tens of units of its last place (measured: 3.8 of the 4 units the
// tests allow p' at steps 2 .. 4, against 0.9 with this form).  -expm1(step log(beta)) has no subtraction.
// (1.0 - pow((double)beta, step), the spelling of sac.hip, gives the same units in tests/test_surrogate_tail_gpu.py and a
// flush launch 1 us longer: profiles/sur_tail_adam_ab.json.)
__device__ __forceinline__ float adam_bias_correction(float beta, int step) {
    return -expm1f((float)step * logf(beta));
}

// g[i][j] += sum_r partial[r][off_i + j]; the partial rows are re-zeroed.  With an Adam descriptor the reduced gradient is
// consumed on the spot: g = sum (not accumulated), then the torch.optim.Adam update of the parameter element
// (no weight decay, no amsgrad): m' = beta1 m + (1 - beta1) g, v' = beta2 v + (1 - beta2) g^2,
// p' = p - lr / bc1 * m' / (sqrt(v') / sqrt(bc2) + eps), torch's formula in fp32 with the bias corrections
// bc = 1 - beta^step of adam_bias_correction above -- the optimizer costs no extra launch and the gradients need no
// zeroing pass.
#ifndef FLUSH_TPB
#define FLUSH_TPB 1024   // the reduction over rows is a latency chain (rows / FLUSH_RG / 8 rounds of loads): 1024 threads = 32 row groups
#endif
constexpr int FLUSH_COLS = 32, FLUSH_RG = FLUSH_TPB / FLUSH_COLS;   // 16 columns (twice the blocks) measured slower: 34 vs 26 us
__host__ __device__ inline int flush_blocks(int psize) { return (psize + FLUSH_COLS - 1) / FLUSH_COLS; }

// The pieces the reductions and the two Adam launches share.
//
// One thread's share of a column of partial rows: the sum of rows rg, rg + FLUSH_RG, ... below `rows` (`stride` floats
// apart), which are re-zeroed.  The loads of a round are all in flight before the first add / re-zero; the additions keep
// row order.
__device__ __forceinline__ float column_sum_rezero(float* col, int rows, int stride, int rg) {
    constexpr int U = 8;
    float acc = 0.0f;
    for (int r0 = rg; r0 < rows; r0 += FLUSH_RG * U) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int r = r0 + FLUSH_RG * u;
            v[u] = r < rows ? col[(size_t)r * stride] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int r = r0 + FLUSH_RG * u;
            if (r < rows) {
                acc += v[u];
                col[(size_t)r * stride] = 0.0f;
            }
        }
    }
    return acc;
}

// a column's total from the row groups' sums in LDS, in row-group order
__device__ __forceinline__ float combine_row_groups(const float (*part)[FLUSH_COLS + 1], int col) {
    float tot = 0.0f;
#pragma unroll
    for (int i = 0; i < FLUSH_RG; ++i) tot += part[i][col];
    return tot;
}

// element t of a pack's flat parameter order: where its gradient and its weight live
template <int NP, typename Params>
__device__ __forceinline__ void locate_param(const Params& p, int t, float*& g, float*& w) {
    int off = 0;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        if (t >= off && t < off + p.size[i]) {
            g = p.g[i] + (t - off);
            w = const_cast<float*>(p.w[i]) + (t - off);
        }
        off += p.size[i];
    }
}

// the torch.optim.Adam update of element t from its old moments and weight: stores m', v' and p'
__device__ __forceinline__ void adam_update(const sur_adam& adam, int t, float* w, float m_old, float v_old, float w_old, float g,
                                            float lr, float bc1, float bc2) {
    const float m = adam.beta1 * m_old + (1.0f - adam.beta1) * g;
    const float v = adam.beta2 * v_old + (1.0f - adam.beta2) * g * g;
    adam.m[t] = m;
    adam.v[t] = v;
    const float denom = sqrtf(v) / sqrtf(bc2) + adam.eps;
    *w = w_old - (lr / bc1) * (m / denom);
}

// The workgroup that takes the last of a launch's nblk tickets advances the step counter and clears the ticket: like every
// other workgroup it has read the step count before it took its ticket.
__device__ __forceinline__ void adam_finish_step(const sur_adam& adam, int step, int nblk) {
    __syncthreads();
    if (threadIdx.x == 0 && atomicAdd(adam.ticket, 1u) == (unsigned)(nblk - 1)) {
        *adam.step = step;
        *adam.ticket = 0u;
    }
}

// SUMSQ: `sumsq` receives the fp64 sum of the squares of the block's FLUSH_COLS column totals, columns past the pack's end
// counting as 0: the square of an fp32 value is exact in fp64, and the 32 squares -- held by lanes 0 .. 31 of the block's
// first wavefront -- are added by a butterfly over partners 16, 8, 4, 2, 1 lanes apart (five roundings deep).  A template
// switch, so that the instantiations without it are the code they have always been.  SUMSQ squares the column total, which
// is the stored gradient only when the total overwrites g: a SUMSQ caller passes overwrite = true and no Adam descriptor.
template <int NP, typename Params, bool SUMSQ = false>
__device__ __forceinline__ void flush_grads_body(const Params& p, int psize, const sur_adam& adam, bool overwrite, int blk,
                                                 int nblk, double* sumsq = nullptr) {
    // block = FLUSH_COLS columns x FLUSH_RG row groups: each thread sums every FLUSH_RG-th row of its column, LDS combines
    // the partials (a wave reads 2 rows x 128 contiguous bytes per load instruction).  The kernel is a chain of memory
    // round trips (rows -> LDS -> Adam state -> ticket), so whatever does not depend on the sum is fetched FIRST: the row
    // group 0 threads -- the ones that finish a column -- locate their parameter and load its moments / weight before
    // the row loop.
    __shared__ float part[FLUSH_RG][FLUSH_COLS + 1];
    const int col = threadIdx.x & (FLUSH_COLS - 1), rg = threadIdx.x / FLUSH_COLS;
    const int t = blk * FLUSH_COLS + col;
    const int step = adam.m ? *adam.step + 1 : 0;   // read before this block takes its ticket (adam_finish_step)
    const float lr = adam.m ? *adam.lr : 0.0f;      // device scalar: a scheduler can change it between graph replays
    const bool finisher = rg == 0 && t < psize;
    float* gdst = nullptr;
    float* wdst = nullptr;
    float m_old = 0.0f, v_old = 0.0f, w_old = 0.0f, bc1 = 1.0f, bc2 = 1.0f;
    if (finisher) {
        locate_param<NP>(p, t, gdst, wdst);
        if (adam.m) {
            m_old = adam.m[t];
            v_old = adam.v[t];
            w_old = *wdst;
            bc1 = adam_bias_correction(adam.beta1, step);   // independent of the sum: before the row loop
            bc2 = adam_bias_correction(adam.beta2, step);
        }
    }
    part[rg][col] = t < psize ? column_sum_rezero(p.partial + t, p.rows, psize, rg) : 0.0f;
    __syncthreads();
    if (finisher) {
        const float tot = combine_row_groups(part, col);
        if (adam.m) {
            *gdst = tot;
            adam_update(adam, t, wdst, m_old, v_old, w_old, tot, lr, bc1, bc2);
        } else if (overwrite) {
            *gdst = tot;
        } else {
            *gdst += tot;
        }
    }
    if constexpr (SUMSQ) {
        static_assert(FLUSH_COLS == 32, "the butterfly below spans the 32 finishers of a block");
        if (threadIdx.x < 64) {   // the first wavefront: row groups 0 (the finishers) and 1 (whose lanes add 0)
            double sq = 0.0;
            if (finisher) {
                const float tot = combine_row_groups(part, col);   // the bits just stored: LDS has not changed since
                sq = (double)tot * (double)tot;
            }
#pragma unroll
            for (int off = FLUSH_COLS / 2; off > 0; off >>= 1) sq += __shfl_xor(sq, off);
            if (threadIdx.x == 0) *sumsq = sq;
        }
    }
    if (adam.m) adam_finish_step(adam, step, nblk);
}

template <int NP, typename Params>
__global__ void __launch_bounds__(FLUSH_TPB) flush_grads_kernel(const Params p, int psize, const sur_adam adam, int overwrite) {
    flush_grads_body<NP, Params>(p, psize, adam, overwrite != 0, blockIdx.x, gridDim.x);
}

// the three gradient reductions of a surrogate (state encoder, action encoder, chunk) in one launch
__global__ void __launch_bounds__(FLUSH_TPB)
flush_all_kernel(const sur_encoder_params e0, const sur_adam a0, int n0, const sur_encoder_params e1, const sur_adam a1, int n1,
                 const sur_chunk_params c2, const sur_adam a2, int n2, int overwrite_mask) {
    const int b0 = flush_blocks(n0), b1 = flush_blocks(n1), b2 = flush_blocks(n2);
    const int blk = blockIdx.x;
    if (blk < b0) flush_grads_body<SUR_ENC_NPARAM, sur_encoder_params>(e0, n0, a0, overwrite_mask & 1, blk, b0);
    else if (blk < b0 + b1) flush_grads_body<SUR_ENC_NPARAM, sur_encoder_params>(e1, n1, a1, overwrite_mask & 2, blk - b0, b1);
    else flush_grads_body<SUR_ST_NPARAM, sur_chunk_params>(c2, n2, a2, overwrite_mask & 4, blk - b0 - b1, b2);
}

// flush_all_kernel without Adam, g = sum of the rows, and block k's sum of squares in sumsq[k]: the first of the two launches
// of a step whose gradient norm is clipped (clip_adam_kernel below is the second)
__global__ void __launch_bounds__(FLUSH_TPB)
flush_all_sumsq_kernel(const sur_encoder_params e0, int n0, const sur_encoder_params e1, int n1, const sur_chunk_params c2, int n2,
                       double* __restrict__ sumsq) {
    const int b0 = flush_blocks(n0), b1 = flush_blocks(n1), b2 = flush_blocks(n2);
    const int blk = blockIdx.x;
    const sur_adam none{};
    if (blk < b0) flush_grads_body<SUR_ENC_NPARAM, sur_encoder_params, true>(e0, n0, none, true, blk, b0, sumsq + blk);
    else if (blk < b0 + b1) flush_grads_body<SUR_ENC_NPARAM, sur_encoder_params, true>(e1, n1, none, true, blk - b0, b1, sumsq + blk);
    else flush_grads_body<SUR_ST_NPARAM, sur_chunk_params, true>(c2, n2, none, true, blk - b0 - b1, b2, sumsq + blk);
}

// Fold the partial-gradient rows [base, base + count) of up to three packs into ONE row each (dst += their sum, fixed order)
// and re-zero them: what a backward branch that finishes early does with its own rows, so that the reduction at the end
// of the step (flush) reads one row per branch instead of hundreds (hipops.fused_tbptt_train).
struct FoldJob {
    float* partial;
    int psize, base, count, dst;
};

__device__ __forceinline__ void fold_rows_body(const FoldJob& j, int blk) {
    __shared__ float part[FLUSH_RG][FLUSH_COLS + 1];
    const int col = threadIdx.x & (FLUSH_COLS - 1), rg = threadIdx.x / FLUSH_COLS;
    const int t = blk * FLUSH_COLS + col;
    part[rg][col] = t < j.psize ? column_sum_rezero(j.partial + (size_t)j.base * j.psize + t, j.count, j.psize, rg) : 0.0f;
    __syncthreads();
    if (rg == 0 && t < j.psize) j.partial[(size_t)j.dst * j.psize + t] += combine_row_groups(part, col);
}

__global__ void __launch_bounds__(FLUSH_TPB) fold_rows_kernel(const FoldJob j0, const FoldJob j1, const FoldJob j2) {
    const int b0 = flush_blocks(j0.psize), b1 = flush_blocks(j1.psize);
    const int blk = blockIdx.x;
    if (blk < b0) fold_rows_body(j0, blk);
    else if (blk < b0 + b1) fold_rows_body(j1, blk - b0);
    else fold_rows_body(j2, blk - b0 - b1);
}

// torch.optim.Adam (no weight decay / amsgrad) of a whole parameter pack from its gradient tensors: the optimizer of the
// EAGER fused path (pdecontrol.surrogates.hipops.PackAdam) -- one launch instead of torch's per-step Python bookkeeping.
// The update of the Adam branch of flush_grads_body (adam_update), fed from g[] instead of the row sum.
template <int NP, typename Params>
__device__ __forceinline__ void adam_apply_body(const Params& p, int psize, const sur_adam& adam, int blk, int nblk) {
    const int t = blk * TPB + threadIdx.x;
    const int step = *adam.step + 1;   // read before this block takes its ticket
    const float lr = *adam.lr;
    if (t < psize) {
        const float bc1 = adam_bias_correction(adam.beta1, step), bc2 = adam_bias_correction(adam.beta2, step);
        float* g = nullptr;
        float* w = nullptr;
        locate_param<NP>(p, t, g, w);
        adam_update(adam, t, w, adam.m[t], adam.v[t], *w, *g, lr, bc1, bc2);
    }
    adam_finish_step(adam, step, nblk);
}

__global__ void __launch_bounds__(TPB)
adam_all_kernel(const sur_encoder_params e0, const sur_adam a0, int n0, const sur_encoder_params e1, const sur_adam a1, int n1,
                const sur_chunk_params c2, const sur_adam a2, int n2) {
    const int b0 = (n0 + TPB - 1) / TPB, b1 = (n1 + TPB - 1) / TPB, b2 = (n2 + TPB - 1) / TPB;
    const int blk = blockIdx.x;
    if (blk < b0) adam_apply_body<SUR_ENC_NPARAM, sur_encoder_params>(e0, n0, a0, blk, b0);
    else if (blk < b0 + b1) adam_apply_body<SUR_ENC_NPARAM, sur_encoder_params>(e1, n1, a1, blk - b0, b1);
    else adam_apply_body<SUR_ST_NPARAM, sur_chunk_params>(c2, n2, a2, blk - b0 - b1, b2);
}

// torch.nn.utils.clip_grad_norm_ over the three packs together, then adam_all_kernel's update, in one launch.  Every block
// folds the per-block sums of squares of flush_all_sumsq_kernel itself, in one fixed order (include/surrogate_hip.h), so all
// blocks scale by the same bits and nothing waits for another block: thread j adds sumsq[j], sumsq[j + TPB], ... in ascending
// order, a butterfly (partners 32 .. 1 lanes apart) combines the 64 threads of a wavefront, the wavefronts' sums are added in
// ascending order.
__device__ __forceinline__ double fold_sumsq(const double* __restrict__ sumsq, int count) {
    __shared__ double wave_sum[TPB / 64];
    double acc = 0.0;
    for (int i = threadIdx.x; i < count; i += TPB) acc += sumsq[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x / 64] = acc;
    __syncthreads();
    double total = 0.0;
#pragma unroll
    for (int w = 0; w < TPB / 64; ++w) total += wave_sum[w];
    return total;
}

// g *= coef (always multiplied, as torch does), then the update of adam_apply_body from the scaled gradient; a pack without
// a descriptor is scaled only
template <int NP, typename Params>
__device__ __forceinline__ void clip_adam_body(const Params& p, int psize, const sur_adam& adam, float coef, int blk, int nblk) {
    const int t = blk * TPB + threadIdx.x;
    if (t < psize) {
        float* g = nullptr;
        float* w = nullptr;
        locate_param<NP>(p, t, g, w);
        *g = *g * coef;
    }
    if (adam.m) adam_apply_body<NP, Params>(p, psize, adam, blk, nblk);   // each thread reads back the element it has just stored
}

__global__ void __launch_bounds__(TPB)
clip_adam_kernel(const sur_encoder_params e0, const sur_adam a0, int n0, const sur_encoder_params e1, const sur_adam a1, int n1,
                 const sur_chunk_params c2, const sur_adam a2, int n2, const double* __restrict__ sumsq, int count, float max_norm,
                 float* __restrict__ total_norm) {
    const float total = (float)sqrt(fold_sumsq(sumsq, count));
    float coef = max_norm / (total + 1e-6f);
    coef = coef > 1.0f ? 1.0f : coef;
    const int b0 = (n0 + TPB - 1) / TPB, b1 = (n1 + TPB - 1) / TPB, b2 = (n2 + TPB - 1) / TPB;
    const int blk = blockIdx.x;
    if (total_norm != nullptr && blk == 0 && threadIdx.x == 0) *total_norm = total;
    if (blk < b0) clip_adam_body<SUR_ENC_NPARAM, sur_encoder_params>(e0, n0, a0, coef, blk, b0);
    else if (blk < b0 + b1) clip_adam_body<SUR_ENC_NPARAM, sur_encoder_params>(e1, n1, a1, coef, blk - b0, b1);
    else clip_adam_body<SUR_ST_NPARAM, sur_chunk_params>(c2, n2, a2, coef, blk - b0 - b1, b2);
}

}  // namespace

#endif  // SUR_TAIL_H
