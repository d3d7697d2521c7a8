// gsage_build.hip -- graph construction on the device: edge list -> CSR, transpose, symmetrise (gfx950).
//
// Reference: utils/convert.py:100-126 (make_sparse_adjacency over a networkx graph) -- a Python dictionary loop, one
// add_edge per edge and one row walk per node.  Here the same definition (include/gsage.h, "Graph construction") is
// a fixed pipeline of streaming integer kernels around the library's own stable radix sort (gsage_sort_rows,
// gsage_rowsum.hip), which this file calls only through its C entry:
//
//   gsage_edges_expand       one packed key per RECORD (input edge i -> records 2i and 2i+1, or i when directed):
//                            key = row << b | neighbour (0-based ids), a sentinel above every valid key for a record
//                            that does not exist (self-loop's second record, an end outside `sel`, a bad id).  One
//                            16-byte store per undirected edge.
//   gsage_edges_expand_csr   the same from a CSR position: the transpose's key is the column alone (row-major
//                            enumeration already yields ascending sources, so ONE stable sort by column is the whole
//                            transposition), the symmetrised graph's keys are (r, c) and (c, r)
//   gsage_edges_mark         over SORTED keys: the first entry of every run of equal keys is the kept one (the sort is
//                            stable: the smallest record index); "sum" adds the run's weights in record order, one
//                            lane per run, sequentially -- no atomics, the same bits every run.  The verdict goes
//                            either to a flag per sorted entry ("id" order: the kept entries ARE the rows) or, indexed
//                            by record, to the row key of a second sort ("insertion" order: kept records by row, in
//                            record order; a dropped record's row key is the sentinel row, it sorts behind every row)
//   gsage_edges_row_keys     row key of every record through an optional permutation ("all" duplicates, and the
//                            time-then-row pair of sorts of a temporal build); gsage_edges_time_keys: time - t_min
//   gsage_edges_finish       col and the carried weight / time of every kept entry, at its rank among the kept ones
//   gsage_edges_rowptr       a lane per row: lower bound of the row among the sorted keys -> rowptr.  No histogram,
//                            no atomics anywhere in this file.
// Nothing is compacted between the sorts: a record that is dropped keeps travelling as a sentinel (a few percent of
// the records of a real edge list), so no launch needs a count from the device and the only readback of a build is
// the pair (nnz, max_deg) at its end.  Every kernel is one lane per entry, 8- and 16-byte accesses, no LDS.
#include "gsage_common.h"

namespace gsage {

namespace {

typedef long long ll2 __attribute__((ext_vector_type(2)));

__global__ void __launch_bounds__(256)
k_build_expand(const int64_t *__restrict__ src, const int64_t *__restrict__ dst, int64_t E, int64_t n_nodes,
               const uint8_t *__restrict__ sel, int directed, int b, int64_t sentinel, int64_t *__restrict__ keys,
               int32_t *err_flag)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= E) return;
    const int64_t u = src[i], v = dst[i];
    const bool ok = u >= 0 && u < n_nodes && v >= 0 && v < n_nodes;
    if (!ok && err_flag) *err_flag = 1;
    const bool live = ok && (!sel || (sel[u] && sel[v]));
    const int64_t k0 = live ? ((u << b) | v) : sentinel;
    if (directed) {
        keys[i] = k0;
    } else {
        ll2 o;
        o.x = k0;
        o.y = live && u != v ? ((v << b) | u) : sentinel;
        *reinterpret_cast<ll2 *>(keys + 2 * i) = o;              // (keys is 16-byte aligned: required by the entry)
    }
}

// the row of CSR position p: the last r with rowptr[r] <= p  (rowptr[0] == 0 <= p < rowptr[n_rows])
__device__ __forceinline__ int64_t row_of(const int64_t *__restrict__ rowptr, int64_t n_rows, int64_t p)
{
    int64_t lo = 0, hi = n_rows;                                 // invariant: rowptr[lo] <= p, (hi == n_rows or rowptr[hi] > p)
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (rowptr[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

template <int SYM>
__global__ void __launch_bounds__(256)
k_build_expand_csr(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t n_rows, int64_t nnz,
                   int b, int64_t sentinel, int64_t *__restrict__ keys, int32_t *__restrict__ rowof, int32_t *err_flag)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= nnz) return;
    const int64_t r = row_of(rowptr, n_rows, p), c = (int64_t)col[p];
    const bool ok = c >= 0 && c < n_rows;
    if (!ok && err_flag) *err_flag = 1;
    if (SYM) {
        ll2 o;
        o.x = ok ? ((r << b) | c) : sentinel;
        o.y = ok ? ((c << b) | r) : sentinel;
        *reinterpret_cast<ll2 *>(keys + 2 * p) = o;
    } else {
        keys[p] = ok ? c : sentinel;
        rowof[p] = (int32_t)r;
    }
}

__global__ void __launch_bounds__(256)
k_build_mark(const int64_t *__restrict__ ks, const int32_t *__restrict__ ps, int64_t n, int b, int64_t sentinel,
             int keep_all, int32_t *__restrict__ flag, int64_t *__restrict__ row_keys, int64_t sent_row,
             const float *__restrict__ weight, int eshift, float *__restrict__ wsum)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t key = ks[i];
    const bool kept = key < sentinel && (keep_all || i == 0 || ks[i - 1] != key);
    const int64_t at = row_keys ? (int64_t)ps[i] : i;            // by record / by sorted entry
    if (row_keys) row_keys[at] = kept ? (key >> b) : sent_row;
    else flag[at] = kept ? 1 : 0;
    if (wsum && kept) {
        float s = weight[(int64_t)ps[i] >> eshift];
        for (int64_t j = i + 1; j < n && ks[j] == key; ++j) s += weight[(int64_t)ps[j] >> eshift];
        wsum[at] = s;
    }
}

__global__ void __launch_bounds__(256)
k_build_row_keys(const int64_t *__restrict__ keys, const int32_t *__restrict__ perm, int64_t n, int b,
                 int64_t *__restrict__ row_keys)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    row_keys[j] = keys[perm ? (int64_t)perm[j] : j] >> b;        // (the sentinel's row is 2^b - 1: behind every row)
}

__global__ void __launch_bounds__(256)
k_build_time_keys(const int64_t *__restrict__ time, int64_t n, int eshift, int64_t t_min, int64_t *__restrict__ tkeys)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    tkeys[r] = (int64_t)((uint64_t)time[r >> eshift] - (uint64_t)t_min);
}

// entry i of the last sort is kept when its inclusive count steps (incl != NULL) or when its row is a row at all
// (incl == NULL: the dropped entries are sentinels behind every row, the rank of a kept entry is i itself)
__global__ void __launch_bounds__(256)
k_build_finish(const int64_t *__restrict__ ks, const int32_t *__restrict__ pos, const int32_t *__restrict__ perm,
               const int32_t *__restrict__ incl, int64_t n, int shift, int64_t n_lim, const int32_t *__restrict__ nbr32,
               const int64_t *__restrict__ nbr64, int64_t mask, int32_t col_add, const float *__restrict__ wsrc,
               const int64_t *__restrict__ tsrc, int eshift, int by_entry, int32_t *__restrict__ col,
               float *__restrict__ w, int64_t *__restrict__ t, int64_t cap)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t key = ks[i];
    int64_t o;
    if (incl) {
        const int32_t here = incl[i], before = i ? incl[i - 1] : 0;
        if (here == before) return;
        o = (int64_t)before;
    } else {
        if ((key >> shift) >= n_lim) return;
        o = i;
    }
    if (o < 0 || o >= cap) return;
    int64_t q = (int64_t)pos[i];
    if (perm) q = (int64_t)perm[q];
    col[o] = nbr32 ? nbr32[q] : (int32_t)(((nbr64 ? nbr64[q] : key) & mask) + col_add);
    const int64_t pay = by_entry ? i : (q >> eshift);
    if (wsrc) w[o] = wsrc[pay];
    if (tsrc) t[o] = tsrc[pay];
}

// rowptr[base + r], r = 0 .. n_lim: the number of kept entries in rows below r
__global__ void __launch_bounds__(256)
k_build_rowptr(const int64_t *__restrict__ ks, const int32_t *__restrict__ incl, int64_t n, int shift, int64_t n_lim,
               int64_t *__restrict__ rowptr, int base)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > n_lim) return;
    int64_t lo = 0, hi = n;                                      // first entry whose row is >= r
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if ((ks[mid] >> shift) < r) lo = mid + 1; else hi = mid;
    }
    rowptr[base + r] = incl ? (lo ? (int64_t)incl[lo - 1] : 0) : lo;
    if (r == 0 && base) rowptr[0] = 0;                           // (the dummy row of the reference's convention)
}

inline unsigned grid_for(int64_t n) { return (unsigned)ceil_div(n, 256); }

}  // namespace

}  // namespace gsage

using namespace gsage;

extern "C" {

int gsage_edges_expand(const int64_t *src, const int64_t *dst, int64_t E, int64_t n_nodes, const uint8_t *sel,
                       int32_t directed, int32_t b, int64_t *keys, int32_t *err_flag, void *stream)
{
    GSAGE_REQUIRE(E >= 0 && n_nodes >= 0, "edges_expand: negative size (E, n_nodes)");
    GSAGE_REQUIRE((directed ? E : 2 * E) < ((int64_t)1 << 31), "edges_expand: 2^31 records or more (the sort carries int32 positions)");
    GSAGE_REQUIRE(b >= 1 && b <= 31 && n_nodes < ((int64_t)1 << b),
                  "edges_expand: b must be in 1..31 with n_nodes < 2^b (the sentinel's row lies behind every row)");
    if (E == 0) return GSAGE_OK;
    GSAGE_REQUIRE(src && dst && keys, "edges_expand: null pointer (src, dst, keys)");
    GSAGE_REQUIRE(((uintptr_t)keys & 15) == 0, "edges_expand: keys must be 16-byte aligned");
    const int64_t sentinel = ((int64_t)1 << (2 * b)) - 1;
    launch(k_build_expand, dim3(grid_for(E)), dim3(256), 0, (hipStream_t)stream, src, dst, E, n_nodes, sel,
           (int)(directed != 0), (int)b, sentinel, keys, err_flag);
    return check_launch("edges_expand");
}

int gsage_edges_expand_csr(const int64_t *rowptr, const int32_t *col, int64_t n_rows, int64_t nnz, int32_t symmetric,
                           int32_t b, int64_t *keys, int32_t *rowof, int32_t *err_flag, void *stream)
{
    GSAGE_REQUIRE(n_rows >= 0 && nnz >= 0, "edges_expand_csr: negative size (n_rows, nnz)");
    GSAGE_REQUIRE((symmetric ? 2 * nnz : nnz) < ((int64_t)1 << 31),
                  "edges_expand_csr: 2^31 records or more (the sort carries int32 positions)");
    GSAGE_REQUIRE(b >= 1 && b <= 31 && n_rows < ((int64_t)1 << b),
                  "edges_expand_csr: b must be in 1..31 with n_rows < 2^b (the sentinel lies behind every row)");
    if (nnz == 0) return GSAGE_OK;
    GSAGE_REQUIRE(n_rows >= 1 && rowptr && col && keys, "edges_expand_csr: null pointer (rowptr, col, keys) or no rows");
    GSAGE_REQUIRE(((uintptr_t)keys & 15) == 0, "edges_expand_csr: keys must be 16-byte aligned");
    if (symmetric) {
        launch(k_build_expand_csr<1>, dim3(grid_for(nnz)), dim3(256), 0, (hipStream_t)stream, rowptr, col, n_rows, nnz,
               (int)b, ((int64_t)1 << (2 * b)) - 1, keys, rowof, err_flag);
    } else {
        GSAGE_REQUIRE(rowof, "edges_expand_csr: null pointer (rowof)");
        launch(k_build_expand_csr<0>, dim3(grid_for(nnz)), dim3(256), 0, (hipStream_t)stream, rowptr, col, n_rows, nnz,
               (int)b, ((int64_t)1 << b) - 1, keys, rowof, err_flag);
    }
    return check_launch("edges_expand_csr");
}

int gsage_edges_mark(const int64_t *keys_sorted, const int32_t *pos_sorted, int64_t n, int32_t b, int32_t keep_all,
                     int32_t *flag, int64_t *row_keys, const float *weight, int32_t eshift, float *wsum, void *stream)
{
    GSAGE_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "edges_mark: n outside [0, 2^31)");
    GSAGE_REQUIRE(b >= 1 && b <= 31, "edges_mark: b must be in 1..31");
    GSAGE_REQUIRE(eshift == 0 || eshift == 1, "edges_mark: eshift must be 0 (directed) or 1");
    GSAGE_REQUIRE((flag != nullptr) != (row_keys != nullptr), "edges_mark: exactly one of flag and row_keys");
    GSAGE_REQUIRE((weight != nullptr) == (wsum != nullptr), "edges_mark: weight and wsum go together");
    if (n == 0) return GSAGE_OK;
    GSAGE_REQUIRE(keys_sorted && pos_sorted, "edges_mark: null pointer (keys_sorted, pos_sorted)");
    launch(k_build_mark, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, keys_sorted, pos_sorted, n, (int)b,
           ((int64_t)1 << (2 * b)) - 1, (int)(keep_all != 0), flag, row_keys, ((int64_t)1 << b) - 1, weight, (int)eshift,
           wsum);
    return check_launch("edges_mark");
}

int gsage_edges_row_keys(const int64_t *keys, const int32_t *perm, int64_t n, int32_t b, int64_t *row_keys,
                         void *stream)
{
    GSAGE_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "edges_row_keys: n outside [0, 2^31)");
    GSAGE_REQUIRE(b >= 1 && b <= 31, "edges_row_keys: b must be in 1..31");
    if (n == 0) return GSAGE_OK;
    GSAGE_REQUIRE(keys && row_keys, "edges_row_keys: null pointer (keys, row_keys)");
    launch(k_build_row_keys, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, keys, perm, n, (int)b, row_keys);
    return check_launch("edges_row_keys");
}

int gsage_edges_time_keys(const int64_t *time, int64_t n, int32_t eshift, int64_t t_min, int64_t *time_keys,
                          void *stream)
{
    GSAGE_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "edges_time_keys: n outside [0, 2^31)");
    GSAGE_REQUIRE(eshift == 0 || eshift == 1, "edges_time_keys: eshift must be 0 (directed) or 1");
    if (n == 0) return GSAGE_OK;
    GSAGE_REQUIRE(time && time_keys, "edges_time_keys: null pointer (time, time_keys)");
    launch(k_build_time_keys, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, time, n, (int)eshift, t_min,
           time_keys);
    return check_launch("edges_time_keys");
}

int gsage_edges_finish(const int64_t *keys_sorted, const int32_t *pos_sorted, const int32_t *perm, const int32_t *incl,
                       int64_t n, int32_t shift, int64_t n_lim, const int32_t *nbr32, const int64_t *nbr64,
                       int32_t nbr_bits, int32_t col_add, const float *wsrc, const int64_t *tsrc, int32_t eshift,
                       int32_t by_entry, int32_t *col, float *w, int64_t *t, int64_t cap, void *stream)
{
    GSAGE_REQUIRE(n >= 0 && n < ((int64_t)1 << 31) && n_lim >= 0 && cap >= 0, "edges_finish: bad size (n, n_lim, cap)");
    GSAGE_REQUIRE(shift >= 0 && shift <= 31 && nbr_bits >= 1 && nbr_bits <= 31,
                  "edges_finish: shift must be in 0..31 and nbr_bits in 1..31");
    GSAGE_REQUIRE(eshift == 0 || eshift == 1, "edges_finish: eshift must be 0 (directed) or 1");
    GSAGE_REQUIRE((wsrc != nullptr) == (w != nullptr) && (tsrc != nullptr) == (t != nullptr),
                  "edges_finish: a payload's source and output go together (wsrc / w, tsrc / t)");
    if (n == 0 || cap == 0) return GSAGE_OK;
    GSAGE_REQUIRE(keys_sorted && pos_sorted && col, "edges_finish: null pointer (keys_sorted, pos_sorted, col)");
    launch(k_build_finish, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, keys_sorted, pos_sorted, perm, incl, n,
           (int)shift, n_lim, nbr32, nbr64, ((int64_t)1 << nbr_bits) - 1, col_add, wsrc, tsrc, (int)eshift,
           (int)(by_entry != 0), col, w, t, cap);
    return check_launch("edges_finish");
}

int gsage_edges_rowptr(const int64_t *keys_sorted, const int32_t *incl, int64_t n, int32_t shift, int64_t n_lim,
                       int64_t *rowptr, int32_t base, void *stream)
{
    GSAGE_REQUIRE(n >= 0 && n < ((int64_t)1 << 31) && n_lim >= 0, "edges_rowptr: bad size (n, n_lim)");
    GSAGE_REQUIRE(shift >= 0 && shift <= 31 && (base == 0 || base == 1), "edges_rowptr: shift in 0..31, base 0 or 1");
    GSAGE_REQUIRE(rowptr && (keys_sorted || n == 0), "edges_rowptr: null pointer (rowptr, keys_sorted)");
    launch(k_build_rowptr, dim3(grid_for(n_lim + 1)), dim3(256), 0, (hipStream_t)stream, keys_sorted, incl, n, (int)shift,
           n_lim, rowptr, (int)base);
    return check_launch("edges_rowptr");
}

}  // extern "C"
