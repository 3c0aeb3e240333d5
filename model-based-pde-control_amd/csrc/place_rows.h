// place_rows.h -- what the three kernels that place a segment's transitions into the slabs of a device-resident replay
// share (include/replay/slabs.h): rp_append_kernel (replay.hip), ks_record_kernel (ks_record.hip) and bg_record_kernel
// (burgers.hip).  A wave owns a transition, lanes run along the columns; each kernel keeps its argument struct and its
// lane-0 tail (the reward expression and the truncated flag are what differ).  place_row is the device half; the host half
// is the two refusals every entry point makes from the slab struct and from dst_host before any HIP call, worded and
// numbered by the caller.  The three place_row calls of a kernel stay three calls in the kernel: folded into one inline
// function they compile to other code objects (profiles/segment_path_isa.txt).
#ifndef PLACE_ROWS_H
#define PLACE_ROWS_H

#include <vector>

#include "../../include/replay/slabs.h"
#include "capi_error.h"
#include "row_ops.h"

namespace {

// n columns of one row, unchanged: float4 where the caller found n a multiple of 4 and both bases 16-byte aligned
__device__ __forceinline__ void place_row(const float* __restrict__ in, float* __restrict__ out, int n, bool vec, int lane)
{
    if (vec) {
        for (int j = 4 * lane; j < n; j += 4 * WAVE) *reinterpret_cast<f4*>(out + j) = *reinterpret_cast<const f4*>(in + j);
    } else {
        for (int j = lane; j < n; j += WAVE) out[j] = in[j];
    }
}

// How an entry point words and numbers the two refusals: `who` starts the message, `plural` says "the slabs have" /
// "the slabs'" where the header speaks of slabs (rp_append: "the slab has" / "the slab's").
struct PlaceRefusals {
    const char* who;
    bool plural;
    int null_field, beyond, twice;
};

// 0, or the refusal of a slab struct with a NULL field pointer
inline int check_slab_fields(const PlaceRefusals& p, const replay_slabs* s)
{
    if (!s->obs || !s->actions || !s->nxtobs || !s->rewards || !s->terminated || !s->truncated || !s->steps)
        return fail(p.null_field, "%s: the %s a NULL field pointer", p.who, p.plural ? "slabs have" : "slab has");
    return 0;
}

// 0, or the refusal of the first of the n entries of dst_host that lies beyond the slabs or names a row a second time
// (negative entries are skipped by contract)
inline int check_dst_rows(const PlaceRefusals& p, const long* dst_host, long n, long rows)
{
    std::vector<bool> seen(static_cast<size_t>(rows), false);
    for (long i = 0; i < n; ++i) {
        const long r = dst_host[i];
        if (r < 0) continue;
        if (r >= rows)
            return fail(p.beyond, "%s: dst[%ld] = %ld is beyond the %s %ld rows", p.who, i, r, p.plural ? "slabs'" : "slab's", rows);
        if (seen[r]) return fail(p.twice, "%s: row %ld is named twice (again at dst[%ld])", p.who, r, i);
        seen[r] = true;
    }
    return 0;
}

}  // namespace

#endif
