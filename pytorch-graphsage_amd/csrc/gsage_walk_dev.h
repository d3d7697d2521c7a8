// gsage_walk_dev.h -- the second-order (node2vec) step's shared parts (include/gsage.h, "Biased walks"): the accept
// thresholds, the wave-cooperative membership test and the class / accept decision, used by the biased batch builder
// (gsage_unsup.hip) and the biased importance walks (gsage_importance.hip).
#pragma once
#include <cmath>

#include "gsage_common.h"

namespace gsage {

constexpr int WALK_ROUNDS = 32;                      // proposals per second-order step; the last one is taken regardless

// theta_return, theta_near, theta_far (accept iff the round's 32-bit word < theta of the proposal's class; 2^32: always)
// and their derived bounds: a word below `lo` accepts any x != t, one at or above `hi` rejects it, without a scan
struct WalkBias {
    uint64_t ret, near_, far_, lo, hi, restart;
    int32_t neutral;                                 // every class threshold is 2^32: round 0 always accepts
};

// host: the thresholds of the definition, in double.  false: a parameter outside its limits (NaN included)
inline bool walk_bias_make(double p, double q, double restart, WalkBias &b)
{
    if (!(p >= 0.125 && p <= 8.0) || !(q >= 0.125 && q <= 8.0) || !(restart >= 0.0 && restart < 1.0)) return false;
    const double a[3] = {1.0 / p, 1.0, 1.0 / q};
    const double a_max = a[0] > a[1] ? (a[0] > a[2] ? a[0] : a[2]) : (a[1] > a[2] ? a[1] : a[2]);
    uint64_t th[3];
    for (int c = 0; c < 3; ++c)
        th[c] = a[c] == a_max ? (1ull << 32) : (uint64_t)std::floor((a[c] / a_max) * 4294967296.0);
    b.ret = th[0]; b.near_ = th[1]; b.far_ = th[2];
    b.lo = th[1] < th[2] ? th[1] : th[2];
    b.hi = th[1] < th[2] ? th[2] : th[1];
    b.restart = (uint64_t)std::floor(restart * 4294967296.0);
    b.neutral = (th[0] == (1ull << 32) && b.lo == (1ull << 32)) ? 1 : 0;
    return true;
}

// Does x occur among the stored columns of the row [beg, end)?  beg, end, x wave-uniform; the 64 lanes read 64 stored
// columns per load and ballot; the first trip with a hit ends the scan.  A trip is four such loads, issued together
// (an index past the row reads the row's last entry and does not count): a row of 420 columns is two dependent round
// trips instead of seven.  Wave-uniform result.
__device__ __forceinline__ bool wave_row_contains(const int32_t *__restrict__ col, int64_t beg, int64_t end, int32_t x,
                                                  int lane)
{
    for (int64_t base = beg; base < end; base += 256) {
        int32_t c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t e = base + 64 * u + lane;
            c[u] = col[e < end ? e : end - 1];
        }
        bool hit = false;
#pragma unroll
        for (int u = 0; u < 4; ++u) hit = hit || (base + 64 * u + lane < end && c[u] == x);
        if (__ballot(hit) != 0ull) return true;
    }
    return false;
}

// What the acceptance word decides about a proposal x after the previous node t, before any scan:
//   1 accept, 0 reject, -1 only the row of t can tell (the word lies between the near and the far threshold)
__device__ __forceinline__ int walk_accept_early(const WalkBias &b, uint32_t word, bool is_return)
{
    if (is_return) return (uint64_t)word < b.ret ? 1 : 0;
    if ((uint64_t)word < b.lo) return 1;
    if ((uint64_t)word >= b.hi) return 0;
    return -1;
}

// ... and after the scan said whether x is stored in the row of t
__device__ __forceinline__ bool walk_accept_scanned(const WalkBias &b, uint32_t word, bool near_)
{
    return (uint64_t)word < (near_ ? b.near_ : b.far_);
}

}  // namespace gsage
