// gsage_weighted_dev.h -- the draw from a weighted adjacency's row (include/gsage.h, "Weighted adjacency"), shared by the
// edge-weight sampler (gsage_weighted.hip) and the weighted steps of the importance walks (gsage_importance.hip).
#pragma once
#include "gsage_common.h"

namespace gsage {

// the two 32-bit words of a Philox block that make draw `odd` of it (a block holds two draws); selects, not
// r.v[2 * odd]: no scratch
__device__ __forceinline__ uint64_t philox_r64(const philox4 &r, bool odd)
{
    return ((uint64_t)(odd ? r.v[2] : r.v[0]) << 32) | (uint64_t)(odd ? r.v[3] : r.v[1]);
}

// first edge e of the row [beg, end) with cdf[e] > x.  The caller has x < cdf[end - 1] (x = umul64hi(r64, T) with
// T = cdf[end - 1] > 0): the answer is in [beg, end - 1]
__device__ __forceinline__ int64_t cdf_first_above(const uint64_t *__restrict__ cdf, int64_t beg, int64_t end, uint64_t x)
{
    int64_t lo = beg, hi = end - 1;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (cdf[mid] > x) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

}  // namespace gsage
