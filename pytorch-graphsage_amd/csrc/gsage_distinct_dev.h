// gsage_distinct_dev.h -- the distinct-draw neighbour sampler's device body (include/gsage.h, "Distinct neighbours"),
// shared by the per-hop kernel and the all-hops kernel of gsage_distinct.hip.
//
// A workgroup of 256 lanes works in TRIPS of whole parents: with n samples per parent a trip takes
// P = 256 / n parents, lane l < P * n is slot j = l % n of the trip's parent l / n.  A parent's slots therefore never
// straddle two trips, and a trip is two passes with one LDS barrier between them:
//   pass 1   every lane loads its row's extent, draws its Philox word and stores its t_j (slot 0 of a row of degree
//            <= n: the rotation r) into the trip's 256-word LDS buffer;
//   pass 2   every lane chases its offset through its parent's earlier t in LDS and issues its one col load.
// The row's extent stays in registers across the barrier: rowptr and the one col load are the only global reads.
// The buffers of consecutive trips alternate (tbuf + 256 * (trip & 1)): a lane still chasing in trip i's buffer while
// another already writes trip i + 1's touches other words, and trip i + 2's writers have passed trip i + 1's barrier,
// which every lane reaches only after its trip-i chase.  One barrier per trip.
#pragma once
#include "gsage_common.h"

namespace gsage {

constexpr uint32_t DISTINCT_TAG = 0x44000000u;   // xored into the key's high word: a stream of its own

// One trip of the calling workgroup.  EVERY lane of the workgroup calls it (it holds a barrier); `active` lanes carry
// slot j of parent `id`, whose slot 0 sits in lane threadIdx.x - j of this trip, and draw global sample g.  tbuf: this
// trip's 256 words.  -> the child (0: the dummy, for an inactive lane too).
__device__ __forceinline__ int64_t distinct_trip(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                 int64_t n_rows, bool active, int64_t id, uint32_t j, uint32_t n,
                                                 uint64_t g, uint64_t call, uint32_t seed_lo, uint32_t seed_hi,
                                                 int32_t *err_flag, uint32_t *tbuf)
{
    int64_t beg = 0;
    uint32_t deg = 0;                                   // 0: this lane yields the dummy
    if (active) {
        if ((uint64_t)id >= (uint64_t)n_rows) {         // checked before rowptr is read (the reference raises IndexError)
            if (err_flag) *err_flag = 1;
        } else {
            beg = rowptr[id];
            const int64_t d = rowptr[id + 1] - beg;
            if (d > 0xffffffffLL) {                     // no adjacency of this project: stated so that 64 bits are exact
                if (err_flag) *err_flag = 1;
            } else if (d > 0) {
                deg = (uint32_t)d;
            }
        }
        if (deg > n) {                                  // t_j = j + floor(w_j (deg - j) / 2^32), in [j, deg)
            tbuf[threadIdx.x] = j + philox_below(philox_word(g, call, seed_lo, seed_hi ^ DISTINCT_TAG), deg - j);
        } else if (deg && j == 0) {                     // every neighbour: the rotation r, in [0, deg)
            tbuf[threadIdx.x] = philox_below(philox_word(g, call, seed_lo, seed_hi ^ DISTINCT_TAG), deg);
        }
    }
    lds_barrier();
    if (!deg) return 0;
    const uint32_t *tp = tbuf + (threadIdx.x - j);      // the parent's t_0 .. t_{n-1}
    uint32_t x;
    if (deg <= n) {
        x = (j + tp[0]) % deg;
    } else {
        // the value of a[t_j] after steps 0 .. j-1 of the shuffle: the last earlier step that wrote a[x] moved a[i]
        // there, whose value is found the same way among the steps before i -- one descending scan (no barrier
        // inside: its length differs per lane)
        x = tp[j];
        for (int i = (int)j - 1; i >= 0; --i)
            if (tp[i] == x) x = (uint32_t)i;
    }
    return (int64_t)col[beg + (int64_t)x];
}

}  // namespace gsage
