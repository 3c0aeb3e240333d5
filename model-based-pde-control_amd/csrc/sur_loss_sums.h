// sur_loss_sums.h -- the `partial` / `ticket` convention of the one-launch losses of libsurrogate_hip.so, spelled once:
// sur_loss.h (delta loss, validation loss: a part of sur_kernels.hip) and sur_decoded.hip (decoded loss) both end their
// workgroups with it.
//
// Every workgroup of a loss adds its terms in fp64 per thread, reduces them here in a fixed order and stores the sums in
// its own slot of the caller's `partial` scratch with plain stores; then it fences and takes a ticket.  The workgroup
// that takes the last ticket fences again and reads every slot with relaxed agent-scope atomic loads (they bypass its
// CU's L1), adds them in a fixed order, writes the results and leaves the ticket at zero for the next launch or replay.
// The ticket add is the only atomic; no floating-point atomics anywhere.
#pragma once

#include <hip/hip_runtime.h>

constexpr int LOSS_TPB = 256;   // threads per loss workgroup

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// The end of a loss workgroup: its NSUM fp64 sums (waves first, then the waves' sums in wave order) go to `out`, the
// workgroup's slot of the partial sums; then, unless the caller finishes the loss in a launch of its own, the workgroup takes
// a ticket.  True for the workgroup that takes the last of `tickets`: every slot is visible to it once it has fenced.
template <int NSUM>
__device__ __forceinline__ bool loss_block_sums(const double (&acc)[NSUM], double* __restrict__ out, unsigned int* __restrict__ ticket,
                                                int tickets, bool take_ticket = true) {
    __shared__ double red[LOSS_TPB / 64][NSUM];
    __shared__ bool last;
#pragma unroll
    for (int j = 0; j < NSUM; ++j) {
        const double w = wave_sum(acc[j]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][j] = w;
    }
    __syncthreads();
    if (threadIdx.x < NSUM) {
        double v = 0.0;
        for (int w = 0; w < LOSS_TPB / 64; ++w) v += red[w][threadIdx.x];
        out[threadIdx.x] = v;
    }
    if (!take_ticket) return false;
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) last = (atomicAdd(ticket, 1u) == (unsigned)(tickets - 1));
    __syncthreads();
    return last;
}
