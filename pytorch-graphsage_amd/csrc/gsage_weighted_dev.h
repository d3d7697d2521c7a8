// gsage_weighted_dev.h -- the draw from a weighted adjacency's row (include/gsage.h, "Weighted adjacency"), shared by the
// edge-weight sampler (gsage_weighted.hip) and the weighted steps of the importance walks (gsage_importance.hip).
#pragma once
#include "gsage_common.h"

namespace gsage {

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

// The same entry found eight ways at a time: seven evenly spaced probes per round, their loads issued together, then the
// eighth of the range that holds the answer -- ceil(log8(deg)) dependent rounds instead of ceil(log2(deg)).  cdf is
// non-decreasing inside a row, so "first entry above x" is one entry however it is found.
__device__ __forceinline__ int64_t cdf_first_above_k8(const uint64_t *__restrict__ cdf, int64_t beg, int64_t end, uint64_t x)
{
    int64_t lo = beg, hi = end - 1;                   // the answer is in [lo, hi]; cdf[hi] > x
    while (lo < hi) {
        const int64_t span = hi - lo;                 // probes lo + floor(span * j / 8), j = 1..7: all in [lo, hi)
        uint64_t c[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) c[j] = cdf[lo + ((span * (j + 1)) >> 3)];
        int64_t nlo = lo, nhi = hi;
#pragma unroll
        for (int j = 0; j < 7; ++j) {                 // ascending probes: the last one not above x, the first one above
            const int64_t q = lo + ((span * (j + 1)) >> 3);
            if (c[j] <= x) nlo = q + 1;
            else if (q < nhi) nhi = q;
        }
        lo = nlo; hi = nhi;
    }
    return lo;
}

}  // namespace gsage
