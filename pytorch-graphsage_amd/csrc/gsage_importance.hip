// gsage_importance.hip -- importance neighbourhoods from random walks (gfx950): visit counts and their top-T.
//
// No reference counterpart.  From every source, n_walks walks of walk_len steps over a device CSR (uniform steps, or
// steps drawn from a weighted adjacency's per-edge table); the `top` most-visited nodes become the source's new row,
// their visit counts its edge weights (include/gsage.h, "Importance neighbourhoods").  The output is a pure function of
// (graph, source id, seed): no atomics, nothing that depends on the grid or on timing.
//
//   gsage_importance_walks    one WAVE (a workgroup of 64 lanes) per source, sources handed out grid-stride:
//     1  walks     lane l runs walks l, l + 64, ...: up to 64 dependent (rowptr -> col) chains in flight per wave.
//                  Step s of walk r owns slot r * walk_len + s of an LDS array that starts as 0xffffffff everywhere, and
//                  writes the node it lands on there unless that is the source -- no slot has two writers.
//     2  sort      bitonic sort of the n slots by id, n = the power of two >= max(n_walks * walk_len, 64); the empty
//                  slots sort behind every id (ids are int32).
//     3  count     the first slot of every run of equal ids finds the run's end by binary search and writes the key
//                  (count << 32) | (0xffffffff - id) to its own position of a second array; every other slot writes 0.
//     4  select    bitonic sort of the keys, descending: count descending, then id ascending -- a total order, so the
//                  first `top` keys are the row whatever order the landings were made in.  Lane j emits entry j.
//   Size classes by n: the LDS arrays (4 + 8 bytes per slot) are sized 256 / 1024 / 4096 slots = 3 / 12 / 48 KB per
//   workgroup (template parameter), the sorts' loops run over n itself (launch argument): 100 landings sort 128 slots.
//   gsage_importance_compact  the padded rows packed into a CSR: one lane per padded entry.
#include "gsage_common.h"
#include "gsage_walk_dev.h"
#include "gsage_weighted_dev.h"

namespace gsage {

namespace {

constexpr uint32_t IMPORTANCE_TAG = 0x49000000u;   // xored into the key's high word: no other sampler's stream
constexpr uint32_t EMPTY_SLOT = 0xffffffffu;
constexpr int IMPORTANCE_MAX_LANDINGS = 4096;

// ascending (DESC = false) or descending bitonic sort of s[0 .. n), n a power of two >= 64, by the one wave of the
// workgroup; ends with a barrier
template <typename T, bool DESC>
__device__ __forceinline__ void wave_bitonic_sort(T *s, int n, int lane)
{
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (n >> 1); t += 64) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));       // bit j clear; its partner has it set
                const int hi = lo | j;
                const bool up = ((lo & k) == 0) != DESC;
                const T a = s[lo], b = s[hi];
                if ((a > b) == up) {
                    s[lo] = b;
                    s[hi] = a;
                }
            }
            lds_barrier();
        }
    }
}

// steps 2-4 for source i: the landings in s_id[0 .. n) -> the source's padded row (every lane of the wave calls it)
__device__ __forceinline__ void importance_rank(uint32_t *s_id, uint64_t *s_key, int n, int32_t top, int lane, int64_t i,
                                                int32_t *__restrict__ out_col, float *__restrict__ out_w,
                                                int32_t *__restrict__ out_deg)
{
    lds_barrier();
    wave_bitonic_sort<uint32_t, false>(s_id, n, lane);
    for (int t = lane; t < n; t += 64) {
        const uint32_t id = s_id[t];
        uint64_t key = 0;
        if (id != EMPTY_SLOT && (t == 0 || s_id[t - 1] != id)) {
            int lo = t + 1, hi = n;                   // first slot in (t, n] that holds another id
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_id[mid] > id) hi = mid;
                else lo = mid + 1;
            }
            key = ((uint64_t)(uint32_t)(lo - t) << 32) | (uint64_t)(EMPTY_SLOT - id);
        }
        s_key[t] = key;
    }
    lds_barrier();
    wave_bitonic_sort<uint64_t, true>(s_key, n, lane);
    const uint64_t key = lane < top ? s_key[lane] : 0ull;         // top <= 64 <= n
    const bool live = key != 0;
    if (lane < top) {
        out_col[i * top + lane] = live ? (int32_t)(EMPTY_SLOT - (uint32_t)key) : 0;
        out_w[i * top + lane] = live ? (float)(uint32_t)(key >> 32) : 0.f;
    }
    const int k = __popcll(__ballot(live));
    if (lane == 0) out_deg[i] = k;
}

template <int P>
__global__ void __launch_bounds__(64)
k_importance_walks(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const uint64_t *__restrict__ cdf,
                   int64_t n_rows, const int64_t *__restrict__ ids, int64_t M, int32_t n_walks, int32_t walk_len,
                   int32_t top, int32_t n, uint32_t seed_lo, uint32_t seed_hi, int32_t *__restrict__ out_col,
                   float *__restrict__ out_w, int32_t *__restrict__ out_deg, int32_t *err_flag)
{
    __shared__ uint32_t s_id[P];
    __shared__ uint64_t s_key[P];
    const int lane = threadIdx.x;
    for (int64_t i = blockIdx.x; i < M; i += gridDim.x) {
        const int64_t v = ids[i];
        for (int t = lane; t < n; t += 64) s_id[t] = EMPTY_SLOT;
        lds_barrier();
        if ((uint64_t)v >= (uint64_t)n_rows) {            // (uniform over the wave) an empty row
            if (lane == 0 && err_flag) *err_flag = 1;
        } else {
            for (int r = lane; r < n_walks; r += 64) {
                int64_t u = v;
                philox4 w = {{0u, 0u, 0u, 0u}};
                for (int s = 0; s < walk_len; ++s) {
                    if (!(s & 1))
                        w = philox4x32_10((uint32_t)v, (uint32_t)r, (uint32_t)(s >> 1), 0u, seed_lo, seed_hi ^ IMPORTANCE_TAG);
                    const uint64_t r64 = philox_r64(w, (s & 1) != 0);
                    const int64_t beg = rowptr[u], end = rowptr[u + 1];
                    if (end <= beg) break;                // a row of degree 0: the walk ends
                    int64_t e;
                    if (cdf) {
                        const uint64_t Tu = cdf[end - 1];
                        if (Tu == 0) break;               // no drawable edge
                        e = cdf_first_above(cdf, beg, end, __umul64hi(r64, Tu));
                    } else {
                        e = beg + (int64_t)__umul64hi(r64, (uint64_t)(end - beg));
                    }
                    const int64_t nu = (int64_t)col[e];
                    if ((uint64_t)nu >= (uint64_t)n_rows) {           // a stored id outside the graph: not counted
                        if (err_flag) *err_flag = 1;
                        break;
                    }
                    u = nu;
                    if (u != v) s_id[r * walk_len + s] = (uint32_t)u;
                }
            }
        }
        importance_rank(s_id, s_key, n, top, lane, i, out_col, out_w, out_deg);
        lds_barrier();                                    // the keys are read: the next source may overwrite them
    }
}

// The walks of "Biased walks" (include/gsage.h): second-order steps by rejection, restarts.  A walk per lane, as above,
// but the lanes move in lock step -- step s, round k -- so that the wave can answer the membership queries together:
// every lane whose acceptance word falls between the near and the far threshold hands its (previous node, proposal)
// to the whole wave in turn, and the 64 lanes scan that row 64 stored columns per trip (wave_row_contains).  Every
// loop is wave-uniform and bounded: the walks' chunks, the steps, 32 rounds, the 64 bits of a ballot, a row's length.
template <int P>
__global__ void __launch_bounds__(64)
k_importance_walks_biased(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                          const uint64_t *__restrict__ cdf, int64_t n_rows, const int64_t *__restrict__ ids, int64_t M,
                          int32_t n_walks, int32_t walk_len, int32_t top, int32_t n, uint32_t seed_lo, uint32_t seed_hi,
                          const WalkBias b, int32_t *__restrict__ out_col, float *__restrict__ out_w,
                          int32_t *__restrict__ out_deg, int32_t *err_flag)
{
    __shared__ uint32_t s_id[P];
    __shared__ uint64_t s_key[P];
    const int lane = threadIdx.x;
    const uint32_t k1 = seed_hi ^ IMPORTANCE_TAG;
    for (int64_t i = blockIdx.x; i < M; i += gridDim.x) {
        const int64_t v = ids[i];
        for (int t = lane; t < n; t += 64) s_id[t] = EMPTY_SLOT;
        lds_barrier();
        if ((uint64_t)v >= (uint64_t)n_rows) {            // (uniform over the wave) an empty row
            if (lane == 0 && err_flag) *err_flag = 1;
        } else {
            for (int r0 = 0; r0 < n_walks; r0 += 64) {
                const int r = r0 + lane;
                bool alive = r < n_walks;
                int64_t u = v, prev = -1;                 // prev < 0: no previous node, the step is first-order
                philox4 w = {{0u, 0u, 0u, 0u}};
                for (int s = 0; s < walk_len; ++s) {
                    if (!(s & 1))
                        w = philox4x32_10((uint32_t)v, (uint32_t)r, (uint32_t)(s >> 1), 0u, seed_lo, k1);
                    philox4 nb0 = {{0u, 0u, 0u, 0u}};     // N(s, 0): round 0's acceptance word, the restart word
                    if (!b.neutral || (b.restart != 0 && s >= 1))
                        nb0 = philox4x32_10((uint32_t)v, (uint32_t)r, (uint32_t)s, 1u, seed_lo, k1);
                    bool moving = alive;
                    if (s >= 1 && moving && (uint64_t)nb0.v[3] < b.restart) {     // back on the source, nothing counted
                        u = v;
                        prev = -1;
                        moving = false;
                    }
                    int64_t beg = 0, end = 0;
                    uint64_t Tu = 0;
                    if (moving) {
                        beg = rowptr[u];
                        end = rowptr[u + 1];
                        if (end > beg && cdf) Tu = cdf[end - 1];
                        if (end <= beg || (cdf && Tu == 0)) alive = moving = false;       // the walk ends
                    }
                    bool pending = moving;
                    int64_t x = -1;
                    for (int k = 0; k < WALK_ROUNDS; ++k) {
                        if (__ballot(pending) == 0ull) break;
                        philox4 nb = nb0;
                        bool scan = false;
                        if (pending) {
                            if (k > 0) nb = philox4x32_10((uint32_t)v, (uint32_t)r, (uint32_t)s, (uint32_t)(1 + k), seed_lo, k1);
                            const uint64_t r64 = k == 0 ? philox_r64(w, (s & 1) != 0) : ((uint64_t)nb.v[0] << 32) | nb.v[1];
                            const int64_t e = cdf ? cdf_first_above(cdf, beg, end, __umul64hi(r64, Tu))
                                                  : beg + (int64_t)__umul64hi(r64, (uint64_t)(end - beg));
                            x = (int64_t)col[e];
                            if ((uint64_t)x >= (uint64_t)n_rows) {    // a stored id outside the graph: the walk ends
                                if (err_flag) *err_flag = 1;
                                alive = moving = pending = false;
                            } else if (prev < 0 || b.neutral) {
                                pending = false;                      // a first-order step
                            } else {
                                const int a = walk_accept_early(b, nb.v[2], x == prev);
                                if (a > 0) pending = false;
                                scan = a < 0;
                            }
                        }
                        uint64_t todo = __ballot(scan);               // the lanes only the row of prev can answer
                        while (todo != 0ull) {
                            const int src = __ffsll((unsigned long long)todo) - 1;
                            todo &= todo - 1;
                            const int64_t tq = (int64_t)__shfl((int)prev, src, 64);       // (ids are int32)
                            const int32_t xq = __shfl((int)x, src, 64);
                            const bool near_ = wave_row_contains(col, rowptr[tq], rowptr[tq + 1], xq, lane);
                            if (lane == src && walk_accept_scanned(b, nb.v[2], near_)) pending = false;
                        }
                    }
                    if (moving) {                         // (still pending after 32 rounds: round 31's proposal)
                        prev = u;
                        u = x;
                        if (u != v) s_id[r * walk_len + s] = (uint32_t)u;
                    }
                }
            }
        }
        importance_rank(s_id, s_key, n, top, lane, i, out_col, out_w, out_deg);
        lds_barrier();                                    // the keys are read: the next source may overwrite them
    }
}

__global__ void __launch_bounds__(256)
k_importance_compact(const int32_t *__restrict__ out_col, const float *__restrict__ out_w,
                     const int32_t *__restrict__ out_deg, const int64_t *__restrict__ rowptr_new, int64_t total,
                     uint32_t top, int32_t *__restrict__ col_new, float *__restrict__ w_new)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
        const int64_t i = (total <= 0xffffffffLL) ? (int64_t)((uint32_t)t / top) : t / (int64_t)top;
        const int64_t j = t - i * (int64_t)top;
        if (j < (int64_t)out_deg[i]) {
            const int64_t o = rowptr_new[i] + j;
            col_new[o] = out_col[t];
            w_new[o] = out_w[t];
        }
    }
}

inline int importance_grid(int64_t items, int64_t cap)
{
    return (int)(items < 1 ? 1 : items > cap ? cap : items);
}

// [host] what the two walk entries require, under the entry's name.  M == 0 passes (the caller then launches nothing)
// before the pointers are looked at.
int importance_check(const char *entry, const int64_t *rowptr, const int32_t *col, int64_t n_rows, const int64_t *ids,
                     int64_t M, int32_t n_walks, int32_t walk_len, int32_t top, const int32_t *out_col, const float *out_w,
                     const int32_t *out_deg)
{
    GSAGE_REQUIRE(n_walks >= 1, "%s: n_walks must be >= 1", entry);
    GSAGE_REQUIRE(walk_len >= 1 && walk_len <= 16, "%s: walk_len must be in 1..16", entry);
    GSAGE_REQUIRE(top >= 1 && top <= 64, "%s: top must be in 1..64", entry);
    GSAGE_REQUIRE((int64_t)n_walks * walk_len <= IMPORTANCE_MAX_LANDINGS,
                  "%s: n_walks * walk_len = %lld, more than %d landings per source", entry, (long long)n_walks * walk_len,
                  IMPORTANCE_MAX_LANDINGS);
    GSAGE_REQUIRE(M >= 0 && n_rows >= 0 && n_rows < (1LL << 31), "%s: bad sizes (node ids are int32)", entry);
    if (M == 0) return GSAGE_OK;
    GSAGE_REQUIRE(rowptr && col && ids && out_col && out_w && out_deg, "%s: null pointer", entry);
    return GSAGE_OK;
}

// slots the sorts run over: the power of two >= max(n_walks * walk_len, 64)
inline int importance_slots(int32_t n_walks, int32_t walk_len)
{
    int n = 64;
    while (n < n_walks * walk_len) n <<= 1;
    return n;
}

// The size classes: the kernel instantiated for 256 / 1024 / 4096 slots, whichever holds n, a wave per source up to the
// class's grid cap (a 256-slot workgroup holds 3 KB of LDS, a 4096-slot one 48: three of those fit a CU)
template <typename K, typename... Args>
void importance_launch(K k256, K k1024, K k4096, int64_t M, int n, void *stream, Args... args)
{
    if (n <= 256)
        launch(k256, dim3(importance_grid(M, 16384)), dim3(64), 0, (hipStream_t)stream, args...);
    else if (n <= 1024)
        launch(k1024, dim3(importance_grid(M, 8192)), dim3(64), 0, (hipStream_t)stream, args...);
    else
        launch(k4096, dim3(importance_grid(M, 2048)), dim3(64), 0, (hipStream_t)stream, args...);
}

}  // namespace

}  // namespace gsage

using namespace gsage;

extern "C" {

int gsage_importance_walks(const int64_t *rowptr, const int32_t *col, const uint64_t *cdf, int64_t n_rows,
                           const int64_t *ids, int64_t M, int32_t n_walks, int32_t walk_len, int32_t top, uint64_t seed,
                           int32_t *out_col, float *out_w, int32_t *out_deg, int32_t *err_flag, void *stream)
{
    int rc = importance_check("importance_walks", rowptr, col, n_rows, ids, M, n_walks, walk_len, top, out_col, out_w, out_deg);
    if (rc != GSAGE_OK || M == 0) return rc;
    const int n = importance_slots(n_walks, walk_len);
    importance_launch(k_importance_walks<256>, k_importance_walks<1024>, k_importance_walks<4096>, M, n, stream, rowptr, col,
                      cdf, n_rows, ids, M, n_walks, walk_len, top, n, (uint32_t)seed, (uint32_t)(seed >> 32), out_col, out_w,
                      out_deg, err_flag);
    return check_launch("importance_walks");
}

int gsage_importance_walks_biased(const int64_t *rowptr, const int32_t *col, const uint64_t *cdf, int64_t n_rows,
                                  const int64_t *ids, int64_t M, int32_t n_walks, int32_t walk_len, int32_t top,
                                  uint64_t seed, double p, double q, double restart, int32_t *out_col, float *out_w,
                                  int32_t *out_deg, int32_t *err_flag, void *stream)
{
    GSAGE_REQUIRE(p >= 0.125 && p <= 8.0, "importance_walks_biased: p must be in [1/8, 8] (got %g)", p);
    GSAGE_REQUIRE(q >= 0.125 && q <= 8.0, "importance_walks_biased: q must be in [1/8, 8] (got %g)", q);
    GSAGE_REQUIRE(restart >= 0.0 && restart < 1.0, "importance_walks_biased: restart must be in [0, 1) (got %g)", restart);
    int rc = importance_check("importance_walks_biased", rowptr, col, n_rows, ids, M, n_walks, walk_len, top, out_col,
                              out_w, out_deg);
    if (rc != GSAGE_OK || M == 0) return rc;
    WalkBias b;
    (void)walk_bias_make(p, q, restart, b);               // (the limits were checked above)
    const int n = importance_slots(n_walks, walk_len);
    importance_launch(k_importance_walks_biased<256>, k_importance_walks_biased<1024>, k_importance_walks_biased<4096>, M, n,
                      stream, rowptr, col, cdf, n_rows, ids, M, n_walks, walk_len, top, n, (uint32_t)seed,
                      (uint32_t)(seed >> 32), b, out_col, out_w, out_deg, err_flag);
    return check_launch("importance_walks_biased");
}

int gsage_importance_compact(const int32_t *out_col, const float *out_w, const int32_t *out_deg,
                             const int64_t *rowptr_new, int64_t M, int32_t top, int32_t *col_new, float *w_new,
                             void *stream)
{
    GSAGE_REQUIRE(top >= 1 && top <= 64, "importance_compact: top must be in 1..64");
    GSAGE_REQUIRE(M >= 0, "importance_compact: negative size");
    if (M == 0) return GSAGE_OK;
    GSAGE_REQUIRE(out_col && out_w && out_deg && rowptr_new, "importance_compact: null pointer");
    // (col_new / w_new may be NULL when every row is empty: nothing is written then)
    const int64_t total = M * (int64_t)top;
    launch(k_importance_compact, dim3(importance_grid(ceil_div(total, 256), 8192)), dim3(256), 0, (hipStream_t)stream,
           out_col, out_w, out_deg, rowptr_new, total, (uint32_t)top, col_new, w_new);
    return check_launch("importance_compact");
}

}  // extern "C"
