// gsage_block.hip -- k-hop closure of a query set and its per-layer blocks (infer.closure / infer.query, gfx950).
//
// The exact full-neighbourhood answer for a query set needs, with L layers, the node sets S_L c ... c S_0:
//   S_L     = the queries, duplicates removed, in order of first appearance
//   S_{l-1} = S_l unchanged as a prefix, then the nodes of N(S_l) u {0} not yet present, in ascending id
// (global row 0, the dummy, is a member of every source set: a row of degree 0 reads it).  A node's position in its
// set is its LOCAL index; the prefix rule makes it the same number in every larger set, so one map
//   local   int32 [n_rows]   -1 = absent
// serves every level.  Block l (destinations S_l, sources S_{l-1}) is the stored rows of S_l, whole and in stored
// order, every id replaced by its local index (and the rows' cdf segments verbatim, for a weighted adjacency).
//
// One hop S_l -> S_{l-1}, seven launches whatever the sizes (the caller copies the set's prefix into the grown buffer in
// between), one readback between the two halves:
//   count   k_mark        a team per NEWEST member (S_l \ S_{l+1}: the older members' rows were walked before):
//                         atomicOr a bit per neighbour that has no local index yet into a bitmap of n_rows bits
//           k_span_sums   popcount of the bitmap words, summed per workgroup span      } phase 1 of two scans
//           k_span_sums   degrees of the rows of S_l, summed per workgroup span        }
//           k_scan_sums   phase 2 of both: one workgroup each scans the span sums; the totals (new members, the
//                         block's edge count) and the dummy's local index go to three words the host reads
//   write   k_compact     phase 3: rank inside the span + the span's offset -> the new ids in ascending order, their
//                         `local` entries; the words that were set are cleared (the bitmap is all zero again)
//           k_rowptr      phase 3 of the degree scan -> the block's rowptr
//           k_fill        a team per destination: col relabelled through `local`, cdf copied
// The scans are three-phase (span sums, scan of the sums, apply): no workgroup ever waits for another one inside a
// launch.  Integer arithmetic only, and the one atomic (a bitwise OR) commutes: the same inputs give the same sets.
// An id outside [0, n_rows) -- a query or a stored neighbour -- raises *err_flag and is dropped from the sets; in a
// block's col it reads the dummy.
#include "gsage_common.h"

namespace gsage {

namespace {

constexpr int BK_THREADS = 256;
constexpr int BK_ITEMS = 4;                          // consecutive items per thread
constexpr int BK_SPAN = BK_THREADS * BK_ITEMS;       // items per workgroup of a scan: 1024 (bitmap: 32 768 rows)
constexpr int BK_TEAM = 16;                          // lanes per row in k_mark / k_fill

// exclusive prefix of one value per thread over the workgroup; *total = the workgroup's sum (every thread calls)
__device__ __forceinline__ int64_t wg_exclusive_scan(int64_t v, int64_t *total)
{
    __shared__ int64_t wave_sum[BK_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    int64_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < BK_THREADS / 64; ++w) {
        if (w < wave) base += wave_sum[w];
        tot += wave_sum[w];
    }
    __syncthreads();                                 // (wave_sum is free for the next call)
    *total = tot;
    return base + inc - v;
}

// ---- what the three scans count -----------------------------------------------------------------
struct WordCount {                                   // item = bitmap word: its set bits
    const uint32_t *bitmap;
    __device__ __forceinline__ int64_t operator()(int64_t i) const { return __popc(bitmap[i]); }
};
struct RowDegree {                                   // item = member of the set: its stored degree
    const int64_t *rowptr;
    const int64_t *set;
    __device__ __forceinline__ int64_t operator()(int64_t i) const
    {
        const int64_t v = set[i];
        return rowptr[v + 1] - rowptr[v];
    }
};
struct QueryFirst {                                  // item = query: 1 where it is the first appearance of a valid id
    const int64_t *q;
    const int32_t *local;                            // (holds the smallest query index per id: k_query_first)
    int64_t n_rows;
    __device__ __forceinline__ int64_t operator()(int64_t i) const
    {
        const int64_t id = q[i];
        return (uint64_t)id < (uint64_t)n_rows && local[id] == (int32_t)i ? 1 : 0;
    }
};

// phase 1: sums[wg] = sum of f over the workgroup's span
template <typename F>
__global__ __launch_bounds__(BK_THREADS) void k_span_sums(F f, int64_t n, int64_t *__restrict__ sums)
{
    const int64_t base = (int64_t)blockIdx.x * BK_SPAN + (int64_t)threadIdx.x * BK_ITEMS;
    int64_t s = 0;
#pragma unroll
    for (int k = 0; k < BK_ITEMS; ++k)
        if (base + k < n) s += f(base + k);
    int64_t tot;
    wg_exclusive_scan(s, &tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// phase 2: a workgroup per job turns its span sums into exclusive offsets (in place) and writes the total.  The last
// word of `totals` gets the dummy's local index: its present one, or n_prev (it will be the first new member).
struct ScanJobs {
    int64_t *sums[2];
    int64_t n[2];
    int64_t *totals;                                 // [n_jobs + 1]
    const int32_t *local;                            // may be NULL (no dummy word)
    int64_t n_prev;
    int32_t n_jobs;
};
__global__ __launch_bounds__(BK_THREADS) void k_scan_sums(ScanJobs j)
{
    int64_t *s = j.sums[blockIdx.x];
    const int64_t n = j.n[blockIdx.x];
    int64_t carry = 0;
    for (int64_t b = 0; b < n; b += BK_THREADS) {
        const int64_t i = b + threadIdx.x;
        const int64_t v = i < n ? s[i] : 0;
        int64_t tot;
        const int64_t ex = wg_exclusive_scan(v, &tot);
        if (i < n) s[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) {
        j.totals[blockIdx.x] = carry;
        if (blockIdx.x == 0 && j.local) j.totals[j.n_jobs] = j.local[0] >= 0 ? (int64_t)j.local[0] : j.n_prev;
    }
}

// ---- the seed level ---------------------------------------------------------------------------
// local[id] = the smallest index of a query holding id (unsigned minimum over the -1 the map rests at)
__global__ __launch_bounds__(BK_THREADS) void k_query_first(const int64_t *__restrict__ q, int64_t nq, int64_t n_rows,
                                                            int32_t *local, int32_t *err)
{
    const int64_t i = (int64_t)blockIdx.x * BK_THREADS + threadIdx.x;
    if (i >= nq) return;
    const int64_t id = q[i];
    if ((uint64_t)id >= (uint64_t)n_rows) {
        if (err) *err = 1;
        return;
    }
    atomicMin(reinterpret_cast<unsigned int *>(local) + id, (unsigned int)i);
}

// phase 3 of the query scan: the first appearances, in query order (their `local` entries: k_assign_local, a launch
// of its own, because this one still compares them with the query indices)
__global__ __launch_bounds__(BK_THREADS) void k_query_compact(QueryFirst f, int64_t nq, const int64_t *__restrict__ sums,
                                                              int64_t *__restrict__ set)
{
    const int64_t base = (int64_t)blockIdx.x * BK_SPAN + (int64_t)threadIdx.x * BK_ITEMS;
    int64_t flag[BK_ITEMS], s = 0;
#pragma unroll
    for (int k = 0; k < BK_ITEMS; ++k) {
        flag[k] = base + k < nq ? f(base + k) : 0;
        s += flag[k];
    }
    int64_t tot;
    int64_t pos = sums[blockIdx.x] + wg_exclusive_scan(s, &tot);
#pragma unroll
    for (int k = 0; k < BK_ITEMS; ++k)
        if (flag[k]) set[pos++] = f.q[base + k];
}

__global__ __launch_bounds__(BK_THREADS) void k_assign_local(const int64_t *__restrict__ set, int64_t n,
                                                             int32_t *__restrict__ local, int32_t value_or_index)
{
    const int64_t i = (int64_t)blockIdx.x * BK_THREADS + threadIdx.x;
    if (i < n) local[set[i]] = value_or_index < 0 ? -1 : (int32_t)i;
}

__global__ __launch_bounds__(BK_THREADS) void k_lookup(const int64_t *__restrict__ q, int64_t nq, int64_t n_rows,
                                                       const int32_t *__restrict__ local, int64_t *__restrict__ pos)
{
    const int64_t i = (int64_t)blockIdx.x * BK_THREADS + threadIdx.x;
    if (i >= nq) return;
    const int64_t id = q[i];
    pos[i] = (uint64_t)id < (uint64_t)n_rows ? (int64_t)local[id] : -1;
}

// ---- one hop ----------------------------------------------------------------------------------
__global__ __launch_bounds__(BK_THREADS) void k_mark(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                     int64_t n_rows, const int64_t *__restrict__ set, int64_t lo,
                                                     int64_t hi, const int32_t *__restrict__ local, uint32_t *bitmap,
                                                     int32_t *err)
{
    if (blockIdx.x == 0 && threadIdx.x == 0 && local[0] < 0) atomicOr(bitmap, 1u);       // the dummy
    const int lane = threadIdx.x & (BK_TEAM - 1);
    const int64_t m = lo + (int64_t)blockIdx.x * (BK_THREADS / BK_TEAM) + threadIdx.x / BK_TEAM;
    if (m >= hi) return;
    const int64_t v = set[m];
    const int64_t beg = rowptr[v], end = rowptr[v + 1];
    for (int64_t e = beg + lane; e < end; e += BK_TEAM) {
        const int32_t id = col[e];
        if ((uint32_t)id >= (uint64_t)n_rows) {
            if (err) *err = 1;
            continue;
        }
        if (local[id] < 0) atomicOr(bitmap + (id >> 5), 1u << (id & 31));
    }
}

// phase 3 of the bitmap scan: the marked ids in ascending order behind the n_prev members there are
__global__ __launch_bounds__(BK_THREADS) void k_compact(uint32_t *__restrict__ bitmap, int64_t n_words,
                                                        const int64_t *__restrict__ sums, int64_t n_prev,
                                                        int64_t *__restrict__ set, int32_t *__restrict__ local)
{
    const int64_t base = (int64_t)blockIdx.x * BK_SPAN + (int64_t)threadIdx.x * BK_ITEMS;
    uint32_t w[BK_ITEMS];
    int64_t s = 0;
#pragma unroll
    for (int k = 0; k < BK_ITEMS; ++k) {
        w[k] = base + k < n_words ? bitmap[base + k] : 0u;
        s += __popc(w[k]);
    }
    int64_t tot;
    int64_t pos = n_prev + sums[blockIdx.x] + wg_exclusive_scan(s, &tot);
#pragma unroll
    for (int k = 0; k < BK_ITEMS; ++k) {
        uint32_t word = w[k];
        if (word == 0) continue;
        bitmap[base + k] = 0u;
        while (word) {
            const int64_t id = (base + k) * 32 + (__ffs(word) - 1);
            word &= word - 1;
            set[pos] = id;
            local[id] = (int32_t)pos;
            ++pos;
        }
    }
}

// phase 3 of the degree scan: the block's rowptr
__global__ __launch_bounds__(BK_THREADS) void k_rowptr(RowDegree f, int64_t n_dst, const int64_t *__restrict__ sums,
                                                       int64_t *__restrict__ out)
{
    const int64_t base = (int64_t)blockIdx.x * BK_SPAN + (int64_t)threadIdx.x * BK_ITEMS;
    int64_t d[BK_ITEMS], s = 0;
#pragma unroll
    for (int k = 0; k < BK_ITEMS; ++k) {
        d[k] = base + k < n_dst ? f(base + k) : 0;
        s += d[k];
    }
    int64_t tot;
    int64_t pos = sums[blockIdx.x] + wg_exclusive_scan(s, &tot);
#pragma unroll
    for (int k = 0; k < BK_ITEMS; ++k) {
        if (base + k < n_dst) {
            out[base + k] = pos;
            pos += d[k];
            if (base + k == n_dst - 1) out[n_dst] = pos;
        }
    }
}

__global__ __launch_bounds__(BK_THREADS) void k_fill(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                     const uint64_t *__restrict__ cdf, int64_t n_rows,
                                                     const int64_t *__restrict__ set, int64_t n_dst,
                                                     const int64_t *__restrict__ brow, const int32_t *__restrict__ local,
                                                     int32_t *__restrict__ bcol, uint64_t *__restrict__ bcdf, int32_t *err)
{
    const int lane = threadIdx.x & (BK_TEAM - 1);
    const int64_t m = (int64_t)blockIdx.x * (BK_THREADS / BK_TEAM) + threadIdx.x / BK_TEAM;
    if (m >= n_dst) return;
    const int64_t v = set[m];
    const int64_t beg = rowptr[v], deg = rowptr[v + 1] - beg, ob = brow[m];
    const int32_t dummy = local[0];
    for (int64_t j = lane; j < deg; j += BK_TEAM) {
        const int32_t id = col[beg + j];
        int32_t loc = dummy;
        if ((uint32_t)id >= (uint64_t)n_rows) {
            if (err) *err = 1;
        } else {
            loc = local[id];
        }
        bcol[ob + j] = loc;
        if (cdf) bcdf[ob + j] = cdf[beg + j];
    }
}

inline uint32_t grid_of(int64_t n, int64_t per) { return (uint32_t)std::max<int64_t>(1, ceil_div(n, per)); }

}  // namespace

}  // namespace gsage

using namespace gsage;

extern "C" {

int64_t gsage_closure_span(void) { return BK_SPAN; }

int gsage_closure_seed_count(const int64_t *queries, int64_t nq, int64_t n_rows, int32_t *local, int64_t *sums,
                             int64_t *counts, int32_t *err_flag, void *stream)
{
    GSAGE_REQUIRE(nq > 0 && nq < ((int64_t)1 << 31), "closure_seed_count: bad query count %lld", (long long)nq);
    GSAGE_REQUIRE(n_rows > 0 && n_rows < ((int64_t)1 << 31), "closure_seed_count: bad n_rows");
    GSAGE_REQUIRE(queries && local && sums && counts, "closure_seed_count: null pointer");
    hipStream_t s = (hipStream_t)stream;
    launch(k_query_first, dim3(grid_of(nq, BK_THREADS)), dim3(BK_THREADS), 0, s, queries, nq, n_rows, local, err_flag);
    int rc = check_launch("closure_query_first");
    if (rc != GSAGE_OK) return rc;
    QueryFirst f{queries, local, n_rows};
    launch(k_span_sums<QueryFirst>, dim3(grid_of(nq, BK_SPAN)), dim3(BK_THREADS), 0, s, f, nq, sums);
    rc = check_launch("closure_query_sums");
    if (rc != GSAGE_OK) return rc;
    ScanJobs j{};
    j.sums[0] = sums; j.n[0] = ceil_div(nq, BK_SPAN); j.totals = counts; j.local = nullptr; j.n_prev = 0; j.n_jobs = 1;
    launch(k_scan_sums, dim3(1), dim3(BK_THREADS), 0, s, j);
    return check_launch("closure_query_scan");
}

int gsage_closure_seed_write(const int64_t *queries, int64_t nq, int64_t n_rows, int32_t *local, const int64_t *sums,
                             int64_t *set, int64_t n_set, int64_t *pos, void *stream)
{
    GSAGE_REQUIRE(nq > 0 && nq < ((int64_t)1 << 31) && n_set >= 0 && n_set <= nq, "closure_seed_write: bad sizes");
    GSAGE_REQUIRE(n_rows > 0 && n_rows < ((int64_t)1 << 31), "closure_seed_write: bad n_rows");
    GSAGE_REQUIRE(queries && local && sums && pos && (set || n_set == 0), "closure_seed_write: null pointer");
    hipStream_t s = (hipStream_t)stream;
    QueryFirst f{queries, local, n_rows};
    launch(k_query_compact, dim3(grid_of(nq, BK_SPAN)), dim3(BK_THREADS), 0, s, f, nq, sums, set);
    int rc = check_launch("closure_query_compact");
    if (rc != GSAGE_OK) return rc;
    launch(k_assign_local, dim3(grid_of(n_set, BK_THREADS)), dim3(BK_THREADS), 0, s, (const int64_t *)set, n_set, local, 0);
    rc = check_launch("closure_assign_local");
    if (rc != GSAGE_OK) return rc;
    launch(k_lookup, dim3(grid_of(nq, BK_THREADS)), dim3(BK_THREADS), 0, s, queries, nq, n_rows, (const int32_t *)local, pos);
    return check_launch("closure_lookup");
}

int gsage_closure_expand_count(const int64_t *rowptr, const int32_t *col, int64_t n_rows, const int64_t *set, int64_t lo,
                               int64_t hi, const int32_t *local, uint32_t *bitmap, int64_t *sums_words,
                               int64_t *sums_rows, int64_t *counts, int32_t *err_flag, void *stream)
{
    GSAGE_REQUIRE(n_rows > 0 && n_rows < ((int64_t)1 << 31), "closure_expand_count: bad n_rows");
    GSAGE_REQUIRE(0 <= lo && lo <= hi && hi > 0 && hi <= n_rows, "closure_expand_count: bad member range");
    GSAGE_REQUIRE(rowptr && set && local && bitmap && sums_words && sums_rows && counts,
                  "closure_expand_count: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_words = ceil_div(n_rows, 32);
    launch(k_mark, dim3(grid_of(hi - lo, BK_THREADS / BK_TEAM)), dim3(BK_THREADS), 0, s, rowptr, col, n_rows, set, lo, hi,
           local, bitmap, err_flag);
    int rc = check_launch("closure_mark");
    if (rc != GSAGE_OK) return rc;
    WordCount wc{bitmap};
    launch(k_span_sums<WordCount>, dim3(grid_of(n_words, BK_SPAN)), dim3(BK_THREADS), 0, s, wc, n_words, sums_words);
    rc = check_launch("closure_word_sums");
    if (rc != GSAGE_OK) return rc;
    RowDegree rd{rowptr, set};
    launch(k_span_sums<RowDegree>, dim3(grid_of(hi, BK_SPAN)), dim3(BK_THREADS), 0, s, rd, hi, sums_rows);
    rc = check_launch("closure_degree_sums");
    if (rc != GSAGE_OK) return rc;
    ScanJobs j{};
    j.sums[0] = sums_words; j.n[0] = ceil_div(n_words, BK_SPAN);
    j.sums[1] = sums_rows; j.n[1] = ceil_div(hi, BK_SPAN);
    j.totals = counts; j.local = local; j.n_prev = hi; j.n_jobs = 2;
    launch(k_scan_sums, dim3(2), dim3(BK_THREADS), 0, s, j);
    return check_launch("closure_scan_sums");
}

int gsage_closure_expand_write(const int64_t *rowptr, const int32_t *col, const uint64_t *cdf, int64_t n_rows,
                               int64_t *set, int64_t n_dst, int32_t *local, uint32_t *bitmap, const int64_t *sums_words,
                               const int64_t *sums_rows, int64_t *blk_rowptr, int32_t *blk_col, uint64_t *blk_cdf,
                               int32_t *err_flag, void *stream)
{
    GSAGE_REQUIRE(n_rows > 0 && n_rows < ((int64_t)1 << 31), "closure_expand_write: bad n_rows");
    GSAGE_REQUIRE(n_dst > 0 && n_dst <= n_rows, "closure_expand_write: bad n_dst");
    GSAGE_REQUIRE(rowptr && set && local && bitmap && sums_words && sums_rows && blk_rowptr,
                  "closure_expand_write: null pointer");
    GSAGE_REQUIRE(!cdf || blk_cdf, "closure_expand_write: a weighted adjacency needs blk_cdf");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_words = ceil_div(n_rows, 32);
    launch(k_compact, dim3(grid_of(n_words, BK_SPAN)), dim3(BK_THREADS), 0, s, bitmap, n_words, sums_words, n_dst, set, local);
    int rc = check_launch("closure_compact");
    if (rc != GSAGE_OK) return rc;
    RowDegree rd{rowptr, set};
    launch(k_rowptr, dim3(grid_of(n_dst, BK_SPAN)), dim3(BK_THREADS), 0, s, rd, n_dst, sums_rows, blk_rowptr);
    rc = check_launch("closure_rowptr");
    if (rc != GSAGE_OK) return rc;
    launch(k_fill, dim3(grid_of(n_dst, BK_THREADS / BK_TEAM)), dim3(BK_THREADS), 0, s, rowptr, col, cdf, n_rows,
           (const int64_t *)set, n_dst, (const int64_t *)blk_rowptr, (const int32_t *)local, blk_col, blk_cdf, err_flag);
    return check_launch("closure_fill");
}

int gsage_closure_restore(const int64_t *set, int64_t n, int32_t *local, void *stream)
{
    GSAGE_REQUIRE(n >= 0 && (n == 0 || (set && local)), "closure_restore: bad arguments");
    launch(k_assign_local, dim3(grid_of(n, BK_THREADS)), dim3(BK_THREADS), 0, (hipStream_t)stream, set, n, local, -1);
    return check_launch("closure_restore");
}

}  // extern "C"
