// gsage_temporal.hip -- neighbour sampling over the edges BEFORE a query time, and the snapshot "as of T" (gfx950).
//
// No reference counterpart: its samplers know no time.  A temporal CSR keeps every row in time order (etime int64 per
// stored edge, non-decreasing inside a row), so the edges a parent may see at time t are the first cnt positions of
// its row, cnt = |{e: etime[e] < t}| (include/gsage.h, "Temporal neighbours").
//
//   gsage_sample_csr_temporal   one launch per hop: a team of 16 lanes takes one parent per trip, finds cnt together
//                               (gsage_temporal_dev.h: 16-fold narrowing by __ballot, no LDS, no barrier) and then
//                               takes the parent's n samples in ceil(n / 16) trips, one col (and etime) load per sample
//   gsage_sample_hops_temporal  every hop of a frontier in ONE launch: frontier_walk
//                               (gsage_sample_dev.h: a workgroup per seed sub-tree, the previous hop in LDS) with the
//                               times of a hop in LDS beside its ids.  A hop runs in two phases: the teams COUNT (one
//                               search per parent, beg and cnt left in LDS), then one lane per SAMPLE draws -- at one
//                               seed per workgroup hop 1 has a single parent, whose 25 samples are 25 busy lanes
//                               instead of two trips of one team.  LDS: 44 bytes per id of the widest hop of a
//                               workgroup's seeds (ids and times, each twice: 32; a parent's beg: 8; its cnt: 4)
//   gsage_temporal_count        the same search, one count per row
//   gsage_temporal_compact      a row copy: a wave per row moves the first cnt entries of col and etime
#include "gsage_common.h"
#include "gsage_sample_dev.h"
#include "gsage_temporal_dev.h"

namespace gsage {

namespace {

constexpr int TEAMS = 256 / TEAM;                   // parents per trip of a workgroup

template <int STRATEGY, int INHERIT>
__global__ void __launch_bounds__(256)
k_sample_temporal(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int64_t *__restrict__ etime,
                  int64_t n_rows, const int64_t *__restrict__ ids, const int64_t *__restrict__ times, int64_t M, uint32_t n,
                  uint32_t seed_lo, uint32_t seed_hi, const uint64_t *__restrict__ call_ctr, uint64_t call_base,
                  uint64_t g0, int64_t *__restrict__ out, int64_t *__restrict__ out_time, int32_t *err_flag)
{
    const uint64_t call = call_base + (call_ctr ? *call_ctr : 0ull);
    const uint32_t team = threadIdx.x / TEAM, l = threadIdx.x & (TEAM - 1);
    const int64_t groups = (M + TEAMS - 1) / TEAMS;
    for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {           // (uniform over the workgroup)
        const int64_t i = grp * TEAMS + team;
        const bool live = i < M;
        const int64_t t = live ? times[i] : 0;
        int64_t beg;
        const uint32_t deg = temporal_row(rowptr, n_rows, live, live ? ids[i] : 0, beg, err_flag);
        const uint32_t cnt = temporal_count(etime, beg, deg, t);               // every lane of the wave
        if (!live) continue;
        const int64_t base = i * (int64_t)n;
        for (uint32_t j = l; j < n; j += TEAM) {
            int64_t v = 0, vt = t;
            if (cnt) {
                uint32_t off;
                if (STRATEGY == GSAGE_TEMPORAL_RECENT)
                    off = cnt - 1 - j % cnt;
                else
                    off = philox_below(philox_word(g0 + (uint64_t)(base + j), call, seed_lo, seed_hi ^ TEMPORAL_TAG), cnt);
                v = (int64_t)col[beg + (int64_t)off];
                if (INHERIT == GSAGE_TEMPORAL_INHERIT_EDGE) vt = etime[beg + (int64_t)off];
            }
            out[base + j] = v;
            out_time[base + j] = vt;
        }
    }
}

// All hops of a temporal frontier: the frontier walk of gsage_sample_dev.h with a second pair of ping-pong buffers for
// the times.  LDS, in entries of cap = spw * widest:
//   [ids cur | ids nxt | times cur | times nxt | beg per parent] int64, then [cnt per parent] uint32
constexpr size_t HOPS_TEMPORAL_LDS_PER_ID = 5 * sizeof(int64_t) + sizeof(uint32_t);      // 44 bytes

template <int STRATEGY, int INHERIT>
__global__ void __launch_bounds__(256)
k_sample_hops_temporal(const HopsParams p, const int64_t *__restrict__ etime, const int64_t *__restrict__ times,
                       const int64_t *__restrict__ time_queue, int64_t *__restrict__ out_times)
{
    extern __shared__ int64_t frontier[];
    Frontier f;
    // the seeds' times ride on the seeds' loop (f.cap is set by then): from the time queue beside a seed queue, else
    // from `times`; published as hop 0 of out_times
    const int64_t *__restrict__ seed_times = p.seed_queue ? time_queue : times;
    if (!frontier_setup<256>(p, (int)blockIdx.x, frontier, f, [&](int t, int64_t src) {
            const int64_t vt = seed_times[src];
            frontier[2 * f.cap + t] = vt;
            if (out_times) out_times[p.off[0] + f.seed0 + t] = vt;
        })) return;                                  // (uniform over the workgroup)
    int64_t *tcur = frontier + 2 * f.cap, *tnxt = frontier + 3 * f.cap, *pbeg = frontier + 4 * f.cap;
    uint32_t *pcnt = (uint32_t *)(frontier + 5 * f.cap);
    const uint32_t team = threadIdx.x / TEAM, l = threadIdx.x & (TEAM - 1);
    frontier_walk(p, f, [&](const Hop &h) {
        // phase 1, count: a team per parent; every lane of every wave runs every trip (temporal_count's ballots)
        for (int64_t i0 = 0; i0 < h.parents; i0 += TEAMS) {           // (uniform over the workgroup)
            const int64_t i = i0 + team;
            const bool live = i < h.parents;
            const int64_t t = live ? tcur[i] : 0;
            int64_t beg;
            const uint32_t deg = temporal_row(p.rowptr, p.n_rows, live, live ? f.cur[i] : 0, beg, p.err_flag);
            const uint32_t cnt = temporal_count(etime, beg, deg, t);
            if (live && l == 0) {
                pbeg[i] = beg;
                pcnt[i] = cnt;
            }
        }
        lds_barrier();
        // phase 2, draw: a lane per sample
        for (int64_t t = threadIdx.x; t < h.count; t += 256) {
            const uint32_t i = (uint32_t)t / h.n, j = (uint32_t)t - i * h.n;
            const uint32_t cnt = pcnt[i];
            const int64_t beg = pbeg[i];
            int64_t v = 0, vt = tcur[i];
            if (cnt) {
                uint32_t off;
                if (STRATEGY == GSAGE_TEMPORAL_RECENT)
                    off = cnt - 1 - j % cnt;
                else
                    off = philox_below(philox_word(hop_sample(p, h, t), h.call, p.seed_lo, p.seed_hi ^ TEMPORAL_TAG), cnt);
                v = (int64_t)p.col[beg + (int64_t)off];
                if (INHERIT == GSAGE_TEMPORAL_INHERIT_EDGE) vt = etime[beg + (int64_t)off];
            }
            hop_store(p, f, h, t, v);
            tnxt[t] = vt;
            if (out_times) out_times[p.off[h.k] + h.local0 + t] = vt;
        }
        int64_t *tmp = tcur; tcur = tnxt; tnxt = tmp;                 // (the walk swaps the ids' pair after its barrier)
    });
}

__global__ void __launch_bounds__(256)
k_temporal_count(const int64_t *__restrict__ rowptr, const int64_t *__restrict__ etime, int64_t n_rows,
                 const int64_t *__restrict__ ids, int64_t M, const int64_t *__restrict__ times, int64_t t_all,
                 int64_t *__restrict__ cnt, int32_t *err_flag)
{
    const uint32_t team = threadIdx.x / TEAM, l = threadIdx.x & (TEAM - 1);
    const int64_t groups = (M + TEAMS - 1) / TEAMS;
    for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {           // (uniform over the workgroup)
        const int64_t i = grp * TEAMS + team;
        const bool live = i < M;
        const int64_t t = live && times ? times[i] : t_all;
        int64_t beg;
        const uint32_t deg = temporal_row(rowptr, n_rows, live, live ? (ids ? ids[i] : i) : 0, beg, err_flag);
        const uint32_t c = temporal_count(etime, beg, deg, t);                 // every lane of the wave
        if (live && l == 0) cnt[i] = (int64_t)c;
    }
}

// a wave per row: the first min(cnt, deg) entries of the row, to prefix[v] on; nothing outside [0, out_nnz)
__global__ void __launch_bounds__(256)
k_temporal_compact(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int64_t *__restrict__ etime,
                   int64_t n_rows, const int64_t *__restrict__ cnt, const int64_t *__restrict__ prefix,
                   int32_t *__restrict__ out_col, int64_t *__restrict__ out_etime, int64_t out_nnz)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (int64_t v = (int64_t)blockIdx.x * 4 + threadIdx.x / 64; v < n_rows; v += (int64_t)gridDim.x * 4) {
        const int64_t beg = rowptr[v], deg = rowptr[v + 1] - beg, dst = prefix[v];
        int64_t c = cnt[v];
        if (c > deg) c = deg;
        if (dst < 0 || dst > out_nnz) continue;
        if (c > out_nnz - dst) c = out_nnz - dst;
        for (int64_t k = lane; k < c; k += 64) {
            out_col[dst + k] = col[beg + k];
            out_etime[dst + k] = etime[beg + k];
        }
    }
}

}  // namespace

}  // namespace gsage

using namespace gsage;

extern "C" {

int gsage_sample_csr_temporal(const int64_t *rowptr, const int32_t *col, const int64_t *etime, int64_t n_rows,
                              const int64_t *ids, const int64_t *times, int64_t M, int32_t n, int32_t strategy,
                              int32_t inherit, uint64_t seed, const uint64_t *call_ctr, uint64_t call_base, uint64_t g0,
                              int64_t *out, int64_t *out_time, int32_t *err_flag, void *stream)
{
    GSAGE_REQUIRE(n >= 1, "sample_csr_temporal: n (samples per parent) must be >= 1");
    GSAGE_REQUIRE(strategy == GSAGE_TEMPORAL_UNIFORM || strategy == GSAGE_TEMPORAL_RECENT,
                  "sample_csr_temporal: unknown strategy %d (0: uniform, 1: recent)", (int)strategy);
    GSAGE_REQUIRE(inherit == GSAGE_TEMPORAL_INHERIT_SEED || inherit == GSAGE_TEMPORAL_INHERIT_EDGE,
                  "sample_csr_temporal: unknown inherit rule %d (0: seed, 1: edge)", (int)inherit);
    GSAGE_REQUIRE(M >= 0 && n_rows >= 0, "sample_csr_temporal: negative size (M, n_rows)");
    if (M == 0) return GSAGE_OK;
    GSAGE_REQUIRE(rowptr && col && etime && ids && times && out && out_time,
                  "sample_csr_temporal: null pointer (rowptr, col, etime, ids, times, out, out_time)");
    int64_t grid = ceil_div(M, TEAMS);
    if (grid > 8192) grid = 8192;
    const bool recent = strategy == GSAGE_TEMPORAL_RECENT, edge = inherit == GSAGE_TEMPORAL_INHERIT_EDGE;
    auto kernel = recent ? (edge ? k_sample_temporal<1, 1> : k_sample_temporal<1, 0>)
                         : (edge ? k_sample_temporal<0, 1> : k_sample_temporal<0, 0>);
    launch(kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, rowptr, col, etime, n_rows, ids, times, M,
           (uint32_t)n, (uint32_t)seed, (uint32_t)(seed >> 32), call_ctr, call_base, g0, out, out_time, err_flag);
    return check_launch("sample_csr_temporal");
}

int gsage_sample_hops_temporal(const gsage_hops_desc *hops, const int64_t *etime, const int64_t *times,
                               const int64_t *time_queue, int32_t strategy, int32_t inherit, int64_t *out_times,
                               void *stream)
{
    GSAGE_REQUIRE(hops, "sample_hops_temporal: null descriptor (hops)");
    GSAGE_REQUIRE(etime, "sample_hops_temporal: null pointer (etime)");
    GSAGE_REQUIRE(!hops->sel, "sample_hops_temporal: sel must be NULL (the temporal sampler draws from Philox)");
    GSAGE_REQUIRE(!hops->dense_adj, "sample_hops_temporal: dense_adj must be NULL (the temporal sampler walks a CSR)");
    GSAGE_REQUIRE(hops->n_hops >= 1 && hops->n_hops <= 5, "sample_hops_temporal: n_hops must be in 1..5");
    for (int k = 0; k < hops->n_hops; ++k)
        GSAGE_REQUIRE(hops->fan[k] >= 1, "sample_hops_temporal: fan[%d] must be >= 1", k);
    GSAGE_REQUIRE(strategy == GSAGE_TEMPORAL_UNIFORM || strategy == GSAGE_TEMPORAL_RECENT,
                  "sample_hops_temporal: unknown strategy %d (0: uniform, 1: recent)", (int)strategy);
    GSAGE_REQUIRE(inherit == GSAGE_TEMPORAL_INHERIT_SEED || inherit == GSAGE_TEMPORAL_INHERIT_EDGE,
                  "sample_hops_temporal: unknown inherit rule %d (0: seed, 1: edge)", (int)inherit);
    GSAGE_REQUIRE(hops->rowptr && hops->col && hops->ids, "sample_hops_temporal: null pointer (rowptr, col, ids)");
    if (hops->seed_queue)
        GSAGE_REQUIRE(time_queue, "sample_hops_temporal: time_queue must not be NULL beside a seed_queue");
    else
        GSAGE_REQUIRE(times && !time_queue,
                      "sample_hops_temporal: without a seed_queue times must not be NULL and time_queue must be NULL");
    gsage_hops_desc d = *hops;
    d.max_deg = 1;                                        // ignored: a draw is scaled by its row's count
    for (int k = 1; k <= d.n_hops; ++k) {                 // (hop by hop: the first hop that no longer fits is named)
        const int64_t widest = hops_widest(d, k);
        GSAGE_REQUIRE(hops_lds_bytes(widest, HOPS_TEMPORAL_LDS_PER_ID, 0) <= HOPS_LDS_MAX,
                      "sample_hops_temporal: the product of fan[] is too large: the widest hop of a workgroup's seeds "
                      "(%lld ids, 44 bytes each) does not fit the LDS", (long long)(widest * hops_spw()));
    }
    HopsParams p;
    size_t lds = 0;
    int rc = fill_hops(p, lds, d, HOPS_TEMPORAL_LDS_PER_ID, 0);
    if (rc != GSAGE_OK || d.B == 0) return rc;
    const bool recent = strategy == GSAGE_TEMPORAL_RECENT, edge = inherit == GSAGE_TEMPORAL_INHERIT_EDGE;
    auto kernel = recent ? (edge ? k_sample_hops_temporal<1, 1> : k_sample_hops_temporal<1, 0>)
                         : (edge ? k_sample_hops_temporal<0, 1> : k_sample_hops_temporal<0, 0>);
    launch(kernel, dim3((unsigned)ceil_div(d.B, p.spw)), dim3(256), lds, (hipStream_t)stream, p, etime, times,
           time_queue, out_times);
    return check_launch("sample_hops_temporal");
}

int gsage_temporal_count(const int64_t *rowptr, const int64_t *etime, int64_t n_rows, const int64_t *ids, int64_t M,
                         const int64_t *times, int64_t t, int64_t *cnt, int32_t *err_flag, void *stream)
{
    GSAGE_REQUIRE(M >= 0 && n_rows >= 0, "temporal_count: negative size (M, n_rows)");
    GSAGE_REQUIRE(ids || M <= n_rows, "temporal_count: M must not exceed n_rows when ids is NULL (every row)");
    if (M == 0) return GSAGE_OK;
    GSAGE_REQUIRE(rowptr && etime && cnt, "temporal_count: null pointer (rowptr, etime, cnt)");
    int64_t grid = ceil_div(M, TEAMS);
    if (grid > 8192) grid = 8192;
    launch(k_temporal_count, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, rowptr, etime, n_rows, ids, M,
           times, t, cnt, err_flag);
    return check_launch("temporal_count");
}

int gsage_temporal_compact(const int64_t *rowptr, const int32_t *col, const int64_t *etime, int64_t n_rows,
                           const int64_t *cnt, const int64_t *prefix, int32_t *out_col, int64_t *out_etime,
                           int64_t out_nnz, void *stream)
{
    GSAGE_REQUIRE(n_rows >= 0 && out_nnz >= 0, "temporal_compact: negative size (n_rows, out_nnz)");
    if (n_rows == 0) return GSAGE_OK;
    GSAGE_REQUIRE(rowptr && cnt && prefix, "temporal_compact: null pointer (rowptr, cnt, prefix)");
    if (out_nnz == 0) return GSAGE_OK;
    GSAGE_REQUIRE(col && etime && out_col && out_etime, "temporal_compact: null pointer (col, etime, out_col, out_etime)");
    int64_t grid = ceil_div(n_rows, 4);
    if (grid > 8192) grid = 8192;
    launch(k_temporal_compact, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, rowptr, col, etime, n_rows, cnt,
           prefix, out_col, out_etime, out_nnz);
    return check_launch("temporal_compact");
}

}  // extern "C"
