// ks_record.hip -- ks_record_device (include/kspde.h): the transitions of a collection segment written from the stepper's
// own outputs into the slabs of the device-resident replay.  The device form of KSBatchedVecEnv._finish_step plus
// Sample.split for T steps without a truncation.
//
// A wave owns a transition (t, e), lanes run along the columns (place_rows.h, rp_append's shape): obs = traj[t][e],
// nxtobs = traj[t + 1][e], the action row, and by lane 0 the reward, the steps and the two zero flags.  The reward is
// (float)((scale * ssq) / substeps): one fp64 multiply, one correctly rounded fp64 division, one round-to-nearest-even
// conversion -- numpy's  (-1.0) * (1 / N) * ssq / cfg_steps  cast to fp32, bit for bit (the library is built
// -ffp-contract=off; the intrinsics pin the three roundings).  Plain vector stores only: no LDS, no scratch, no atomics.
#include <hip/hip_runtime.h>

#include "ks_internal.h"
#include "place_rows.h"

namespace {

__global__ __launch_bounds__(NT) void ks_record_kernel(const ks::RecordArgs a)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const long w = (long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (w >= a.n) return;
    const long r = a.dst[w];
    if (r < 0 || r >= a.rows) return;                // negative: skipped by contract; beyond the slab: never written
    place_row(a.traj + w * a.N, a.obs + r * a.N, a.N, a.vec_obs, lane);
    place_row(a.traj + (w + a.E) * a.N, a.nxtobs + r * a.N, a.N, a.vec_obs, lane);
    place_row(a.actions + w * a.A, a.act + r * a.A, a.A, a.vec_act, lane);
    if (lane == 0) {
        a.rewards[r] = __double2float_rn(__ddiv_rn(__dmul_rn(a.scale, a.ssq[w]), a.substeps));
        a.out_steps[r] = a.steps[w];
        a.terminated[r] = 0;
        a.truncated[r] = 0;
    }
}

}  // namespace

namespace ks {

hipError_t launch_record(const RecordArgs& args, hipStream_t stream)
{
    RecordArgs a = args;
    a.vec_obs = a.N % 4 == 0 && aligned16(a.traj) && aligned16(a.obs) && aligned16(a.nxtobs);
    a.vec_act = a.A % 4 == 0 && aligned16(a.actions) && aligned16(a.act);
    hipLaunchKernelGGL(ks_record_kernel, dim3((unsigned)((a.n + WAVES - 1) / WAVES)), dim3(NT), 0, stream, a);
    return hipGetLastError();
}

}  // namespace ks
