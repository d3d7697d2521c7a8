// gsage_temporal_dev.h -- the temporal sampler's device body (include/gsage.h, "Temporal neighbours"), shared by the
// hop kernel and the count kernel of gsage_temporal.hip.
//
// A TEAM is 16 consecutive lanes of a wave (four teams per wave, sixteen per 256-lane workgroup) and holds one row
// at a time.  The row is in time order, so "the number of edges before t" is the position of the first edge at or
// after t: the team finds it together, one count per parent however many samples the parent takes.
//   a window of <= 16 edges   one load per lane, cnt = lo + popcount of the team's 16 bits of __ballot(etime < t)
//   a longer window           cut into 16 chunks of step = ceil(len / 16) edges; lane l probes the LAST edge of
//                             chunk l; the probes are monotone, so their popcount k says that chunks 0 .. k-1 lie
//                             before t and the boundary is in chunk k: the window shrinks 16-fold per round
// -- one round up to 16 edges, two up to 256, three up to 4096.  No LDS and no barrier.
//
// __ballot is wave-wide and the four teams of a wave hold rows of different lengths, so the round loop is
// WAVE-UNIFORM: every lane of the wave runs every round until the longest row of the wave is done, and the lanes of a
// finished (or idle) team contribute false.  Every lane of a wave must therefore call temporal_count together.
#pragma once
#include "gsage_common.h"

namespace gsage {

constexpr uint32_t TEMPORAL_TAG = 0x54000000u;   // xored into the key's high word: a stream of its own
constexpr int TEAM = 16;

// The row's extent.  live: this team carries a row; v: its id.  -> deg (0: nothing to search), beg through `beg`.
// A row outside the graph, or one of 2^32 edges or more, has deg 0 and raises the flag.
__device__ __forceinline__ uint32_t temporal_row(const int64_t *__restrict__ rowptr, int64_t n_rows, bool live, int64_t v,
                                                 int64_t &beg, int32_t *err_flag)
{
    beg = 0;
    if (!live) return 0;
    if ((uint64_t)v >= (uint64_t)n_rows) {              // checked before rowptr is read
        if (err_flag) *err_flag = 1;
        return 0;
    }
    beg = rowptr[v];
    const int64_t d = rowptr[v + 1] - beg;
    if (d > 0xffffffffLL) {                             // no adjacency of this project: stated so that 32 bits are exact
        if (err_flag) *err_flag = 1;
        return 0;
    }
    return d > 0 ? (uint32_t)d : 0u;
}

// cnt = |{e in [beg, beg + deg): etime[e] < t}| for the calling lane's team.  EVERY lane of the wave calls it (the
// loop is wave-uniform around __ballot); a team without a row passes deg = 0.  beg, deg and t are team-uniform.
__device__ __forceinline__ uint32_t temporal_count(const int64_t *__restrict__ etime, int64_t beg, uint32_t deg, int64_t t)
{
    const uint32_t l = threadIdx.x & (TEAM - 1);                     // lane of the team
    const uint32_t shift = threadIdx.x & 63u & ~(uint32_t)(TEAM - 1);     // the team's 16 bits of the wave's ballot
    uint32_t lo = 0, len = deg;          // positions < lo are before t, positions >= lo + len are not
    bool done = deg == 0;
    for (;;) {
        const bool last = len <= (uint32_t)TEAM;
        const uint32_t step = last ? 1u : (uint32_t)(((uint64_t)len + TEAM - 1) / TEAM);     // (len + 15 may pass 2^32)
        const uint64_t p = (uint64_t)(l + 1) * step - 1;             // the last edge of chunk l, from lo on
        bool before = false;
        if (!done && p < len) before = etime[beg + (int64_t)((uint64_t)lo + p)] < t;    // a signed 64-bit compare
        const uint64_t b = __ballot(before);
        const uint32_t k = (uint32_t)__popc((uint32_t)(b >> shift) & 0xffffu);
        if (!done) {                     // chunks 0 .. k-1 lie before t (k * step <= len: chunk k-1's probe was in range)
            const uint32_t adv = k * step;
            lo += adv;
            len -= adv;
            if (len > step) len = step;
            done = last;
        }
        if (!__any(!done)) break;        // (uniform over the wave)
    }
    return lo;
}

}  // namespace gsage
