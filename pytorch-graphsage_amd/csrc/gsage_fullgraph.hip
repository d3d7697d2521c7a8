// gsage_fullgraph.hip -- CSR segment reduce for layer-wise full-neighbourhood inference (gfx950).
//
// out[v, c] = reduce_{u in N(v)} table[u, c] over the WHOLE neighbourhood of every row v (infer.py), with
// N(v) = col[rowptr[v] .. rowptr[v+1]) and the single neighbour 0 (the dummy) for a row of degree 0 -- what the
// sampler draws for such a row (gsage_sample_dev.h).  Four modes:
//   MEAN              (1/deg) sum_u table[u]
//   MAX               max_u table[u]
//   SOFTMAX_WEIGHTED  sum_u softmax_u(keys[u] . keys[v]) table[u]; keys are 32-wide fp32 rows, the score of a
//                     neighbour is its key dotted with the row's own key (the attention aggregator's query).
//   WEIGHTED_MEAN     sum_e (q_e / T_v) table[u_e] over a weighted adjacency's integer quanta (gsage_weighted.hip):
//                     q_e = cdf[e] - cdf[e - 1] < 2^24 is exact as a float and p_e = q_e / float(T_v) is one IEEE
//                     division per edge, so a row with a single drawable edge (p = 1) returns that neighbour's row
//                     bit for bit -- sum q_e x_u divided once at the end does not (round(q x) / q need not be x).  Short
//                     rows and slices accumulate fma(p_e, x_u, acc); the merge adds the slices' partials.  A row
//                     without a drawable edge (T_v == 0) reads the dummy like a row of degree 0
//                     (gsage_segment_reduce_weighted).
//
// Degree skew (Reddit-shaped graphs run from degree 0 to > 20,000): the caller's plan (infer.py, built once per
// adjacency) lists the rows of degree <= slice_len in DEGREE-DESCENDING order -- a wave holds 64 / team rows of
// similar length -- and cuts every longer row into slices of slice_len edges.  Launch 1 gives each short row and
// each slice a TEAM of lanes (one 16-byte column chunk per lane, several teams per wave when the row is narrow):
// short rows are written directly, slices write fp32 partials (sum | max | (acc, m, l)).  Launch 2 merges the
// partials of each long row in slice order.  No floating-point atomics anywhere: the same inputs give the same
// bits, and no team walks more than slice_len edges.
//
// Loads: 16 bytes per lane, 8 neighbour rows in flight per lane, the ids of the next batch requested before the
// rows of the current one (the idiom of gather_mean_chunk, gsage_gather.hip).  Columns >= D are never stored.
//
// Blocks (gsage_segment_reduce_block, infer.query): the same kernels over a block of a k-hop closure
// (csrc/gsage_block.hip) -- n_dst output rows reading a table and keys of n_src >= n_dst rows, ids bounded by n_src, and
// the dummy at a local index the caller names.  The whole-graph entry points are the case n_src = n_rows, dummy = 0.
#include "gsage_common.h"

namespace gsage {

namespace {

constexpr int FG_THREADS = 256;
constexpr int FG_BATCH = 8;

template <typename T> struct fg_io;
template <> struct fg_io<uint16_t> {
    static constexpr int VEC = 8;
    __device__ static __forceinline__ float elem(const vec16 &v, int e)
    {
        const uint32_t w = v[e >> 1];
        return __uint_as_float((e & 1) ? (w & 0xffff0000u) : (w << 16));
    }
    __device__ static __forceinline__ void put(uint16_t *p, float f) { *p = f32_to_bf16(f); }
};
template <> struct fg_io<float> {
    static constexpr int VEC = 4;
    __device__ static __forceinline__ float elem(const vec16 &v, int e) { return __uint_as_float(v[e]); }
    __device__ static __forceinline__ void put(float *p, float f) { *p = f; }
};

struct FgArgs {
    const void *table;
    int64_t ld;
    int32_t D, Dp;                  // logical width, width rounded up to the 16-byte chunk
    const float *keys;              // SOFTMAX_WEIGHTED: [n_rows, ldk] fp32, 32 columns used
    int64_t ldk;
    const int64_t *rowptr;
    const int32_t *col;
    int64_t n_rows;                 // output rows
    int64_t n_src;                  // rows of the table and keys: the bound of a neighbour id (a block: > n_rows)
    int32_t dummy;                  // the row a row without a (drawable) edge, or an id outside the table, reads
    const int32_t *order;           // short rows, degree-descending
    int64_t n_short;
    const int64_t *slices;          // [n_slices, 2]: (row, first edge)
    int64_t n_slices;
    const int64_t *long_rows;       // [n_long, 2]: (row, index of its first slice)
    int64_t n_long;
    int32_t slice_len;
    float *partials;                // [n_slices, ldp]: acc[Dp] | m | l
    int64_t ldp;
    void *out;
    int64_t out_ld;
    int32_t act;
    int32_t team;                   // lanes per row: 8, 16, 32 or 64
    int32_t *err;                   // set to 1 when a neighbour id is outside [0, n_src)
    const uint64_t *cdf;            // WEIGHTED_MEAN: the adjacency's inclusive per-row running sums of quanta [nnz]
};

// state of one lane's column chunk
template <int MODE, int VEC>
struct FgAcc {
    float a[VEC];
    float m, l;
    __device__ __forceinline__ void init()
    {
#pragma unroll
        for (int e = 0; e < VEC; ++e) a[e] = MODE == GSAGE_SEG_MAX ? -INFINITY : 0.f;
        m = -INFINITY;
        l = 0.f;
    }
};

__device__ __forceinline__ float team8_sum(float s)
{
    s += __shfl_xor(s, 1, 8);
    s += __shfl_xor(s, 2, 8);
    s += __shfl_xor(s, 4, 8);
    return s;
}

// Walk edges [beg, beg + cnt) of one row (cnt == 0: the dummy neighbour) for the column chunk at c0.  Every lane
// of the team runs this with the same beg / cnt (the score of SOFTMAX_WEIGHTED is a cross-lane sum); `live` lanes
// own a chunk inside Dp.
template <typename TI, int MODE>
__device__ __forceinline__ void fg_walk(const FgArgs &a, int64_t beg, int64_t cnt, int32_t c0, bool live,
                                        const float4 &q, int klane, FgAcc<MODE, fg_io<TI>::VEC> &s, int64_t row_beg, float Tf)
{
    constexpr int VEC = fg_io<TI>::VEC;
    const TI *table = (const TI *)a.table;
    const int32_t *col = a.col + beg;
    const int64_t n = cnt > 0 ? cnt : 1;
    const int32_t cc = live ? c0 : 0;
    auto id_at = [&](int64_t j) -> int32_t {
        if (cnt == 0) return a.dummy;
        int32_t id = col[min(j, cnt - 1)];
        if ((uint32_t)id >= (uint64_t)a.n_src) {
            if (a.err) *a.err = 1;
            id = a.dummy;
        }
        return id;
    };
    int32_t rc[FG_BATCH], rn[FG_BATCH];
#pragma unroll
    for (int u = 0; u < FG_BATCH; ++u) rn[u] = rc[u] = id_at(u);
    for (int64_t j = 0; j < n; j += FG_BATCH) {
        const int m = (int)min((int64_t)FG_BATCH, n - j);
        if (j + FG_BATCH < n) {
#pragma unroll
            for (int u = 0; u < FG_BATCH; ++u) rn[u] = id_at(j + FG_BATCH + u);
        }
        vec16 v[FG_BATCH];
#pragma unroll
        for (int u = 0; u < FG_BATCH; ++u) v[u] = *reinterpret_cast<const vec16 *>(table + (int64_t)rc[u] * a.ld + cc);
        if (MODE == GSAGE_SEG_SOFTMAX_WEIGHTED) {
            float sc[FG_BATCH];
#pragma unroll
            for (int u = 0; u < FG_BATCH; ++u) {
                const float4 k = *reinterpret_cast<const float4 *>(a.keys + (int64_t)rc[u] * a.ldk + klane * 4);
                sc[u] = k.x * q.x + k.y * q.y + k.z * q.z + k.w * q.w;
            }
            float bm = -INFINITY;
#pragma unroll
            for (int u = 0; u < FG_BATCH; ++u) {
                sc[u] = team8_sum(sc[u]);
                if (u < m) bm = fmaxf(bm, sc[u]);
            }
            const float mn = fmaxf(s.m, bm);
            const float scale = expf(s.m - mn);
            s.l *= scale;
#pragma unroll
            for (int e = 0; e < VEC; ++e) s.a[e] *= scale;
#pragma unroll
            for (int u = 0; u < FG_BATCH; ++u) {
                if (u < m) {
                    const float w = expf(sc[u] - mn);
                    s.l += w;
#pragma unroll
                    for (int e = 0; e < VEC; ++e) s.a[e] += w * fg_io<TI>::elem(v[u], e);
                }
            }
            s.m = mn;
        } else if (MODE == GSAGE_SEG_WEIGHTED_MEAN) {
            // the edge's quantum: the difference of two neighbouring table entries (the row's first edge subtracts 0),
            // over the row's total; the dummy neighbour of a row without a drawable edge (cnt == 0) has weight 1
            float w[FG_BATCH];
#pragma unroll
            for (int u = 0; u < FG_BATCH; ++u) {
                const int64_t e = beg + min(j + u, cnt - 1);
                w[u] = 1.f;
                if (cnt > 0) w[u] = (float)(uint32_t)(a.cdf[e] - (e > row_beg ? a.cdf[e - 1] : 0ull)) / Tf;
            }
#pragma unroll
            for (int u = 0; u < FG_BATCH; ++u) {
                if (u < m) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) s.a[e] = fmaf(w[u], fg_io<TI>::elem(v[u], e), s.a[e]);
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < FG_BATCH; ++u) {
                if (u < m) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        const float x = fg_io<TI>::elem(v[u], e);
                        s.a[e] = MODE == GSAGE_SEG_MAX ? fmaxf(s.a[e], x) : s.a[e] + x;
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < FG_BATCH; ++u) rc[u] = rn[u];
    }
}

template <typename TO, int VEC>
__device__ __forceinline__ void fg_store(const FgArgs &a, int64_t row, int32_t c0, float (&r)[VEC])
{
    TO *o = (TO *)a.out + row * a.out_ld + c0;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        if (c0 + e < a.D) {
            const float x = a.act == GSAGE_ACT_RELU ? fmaxf(r[e], 0.f) : r[e];
            fg_io<TO>::put(o + e, x);
        }
    }
}

// launch 1: one team per short row or slice
template <typename TI, typename TO, int MODE>
__global__ __launch_bounds__(FG_THREADS) void k_segment_reduce(FgArgs a)
{
    constexpr int VEC = fg_io<TI>::VEC;
    const int team = a.team;
    const int lane = threadIdx.x & (team - 1);
    const int64_t item = (int64_t)blockIdx.x * (FG_THREADS / team) + threadIdx.x / team;
    if (item >= a.n_short + a.n_slices) return;
    int64_t row, beg, cnt;
    float Tf = 1.f;                 // WEIGHTED_MEAN: the row's total
    const bool is_slice = item >= a.n_short;
    if (!is_slice) {
        row = a.order[item];
        beg = a.rowptr[row];
        cnt = a.rowptr[row + 1] - beg;
        if (MODE == GSAGE_SEG_WEIGHTED_MEAN) {
            const uint64_t T = cnt > 0 ? a.cdf[beg + cnt - 1] : 0ull;
            if (T == 0) cnt = 0;    // no drawable edge: the dummy, as a row of degree 0
            else Tf = (float)T;
        }
    } else {
        const int64_t s = item - a.n_short;
        row = a.slices[2 * s];
        beg = a.slices[2 * s + 1];
        cnt = min((int64_t)a.slice_len, a.rowptr[row + 1] - beg);
        // (a long row of zero weights: every quantum is 0, the partials are +-0 whatever Tf is; the merge reads the dummy)
        if (MODE == GSAGE_SEG_WEIGHTED_MEAN) Tf = fmaxf((float)a.cdf[a.rowptr[row + 1] - 1], 1.f);
    }
    const int klane = lane & 7;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (MODE == GSAGE_SEG_SOFTMAX_WEIGHTED) q = *reinterpret_cast<const float4 *>(a.keys + row * a.ldk + klane * 4);
    const int32_t chunks = a.Dp / VEC;
    for (int32_t g = 0; g < chunks; g += team) {
        const int32_t c0 = (g + lane) * VEC;
        const bool live = g + lane < chunks;
        FgAcc<MODE, VEC> s;
        s.init();
        fg_walk<TI, MODE>(a, beg, cnt, c0, live, q, klane, s, a.rowptr[row], Tf);
        if (!live) continue;
        if (is_slice) {
            float *p = a.partials + (item - a.n_short) * a.ldp;
#pragma unroll
            for (int e = 0; e < VEC; e += 4) {
                vec16 w;
                w[0] = __float_as_uint(s.a[e]); w[1] = __float_as_uint(s.a[e + 1]);
                w[2] = __float_as_uint(s.a[e + 2]); w[3] = __float_as_uint(s.a[e + 3]);
                *reinterpret_cast<vec16 *>(p + c0 + e) = w;
            }
            if (MODE == GSAGE_SEG_SOFTMAX_WEIGHTED && c0 == 0) {
                p[a.Dp] = s.m;
                p[a.Dp + 1] = s.l;
            }
        } else {
            float r[VEC];
            const float inv = MODE == GSAGE_SEG_MEAN ? (float)(cnt > 0 ? cnt : 1)
                              : MODE == GSAGE_SEG_SOFTMAX_WEIGHTED ? s.l : 1.f;
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                r[e] = MODE == GSAGE_SEG_MAX || MODE == GSAGE_SEG_WEIGHTED_MEAN ? s.a[e] : s.a[e] / inv;
            fg_store<TO, VEC>(a, row, c0, r);
        }
    }
}

// launch 2: one team per long row, its slices merged in slice order
template <typename TI, typename TO, int MODE>
__global__ __launch_bounds__(FG_THREADS) void k_segment_merge(FgArgs a)
{
    constexpr int VEC = fg_io<TI>::VEC;
    const int team = a.team;
    const int lane = threadIdx.x & (team - 1);
    const int64_t lr = (int64_t)blockIdx.x * (FG_THREADS / team) + threadIdx.x / team;
    if (lr >= a.n_long) return;
    const int64_t row = a.long_rows[2 * lr], s0 = a.long_rows[2 * lr + 1];
    const int64_t deg = a.rowptr[row + 1] - a.rowptr[row];
    const int64_t ns = (deg + a.slice_len - 1) / a.slice_len;
    const uint64_t T = MODE == GSAGE_SEG_WEIGHTED_MEAN ? a.cdf[a.rowptr[row + 1] - 1] : 1ull;
    float M = -INFINITY;
    if (MODE == GSAGE_SEG_SOFTMAX_WEIGHTED)
        for (int64_t s = 0; s < ns; ++s) M = fmaxf(M, a.partials[(s0 + s) * a.ldp + a.Dp]);
    const int32_t chunks = a.Dp / VEC;
    for (int32_t c = lane; c < chunks; c += team) {
        const int32_t c0 = c * VEC;
        float r[VEC], l = 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) r[e] = MODE == GSAGE_SEG_MAX ? -INFINITY : 0.f;
        for (int64_t s = 0; s < ns; ++s) {
            const float *p = a.partials + (s0 + s) * a.ldp;
            float w = 1.f;
            if (MODE == GSAGE_SEG_SOFTMAX_WEIGHTED) {
                w = expf(p[a.Dp] - M);
                l += w * p[a.Dp + 1];
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                r[e] = MODE == GSAGE_SEG_MAX ? fmaxf(r[e], p[c0 + e])
                       : MODE == GSAGE_SEG_SOFTMAX_WEIGHTED ? r[e] + w * p[c0 + e] : r[e] + p[c0 + e];
        }
        const float inv = MODE == GSAGE_SEG_MEAN ? (float)deg : MODE == GSAGE_SEG_SOFTMAX_WEIGHTED ? l : 1.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            r[e] = MODE == GSAGE_SEG_MAX || MODE == GSAGE_SEG_WEIGHTED_MEAN ? r[e] : r[e] / inv;
        if (MODE == GSAGE_SEG_WEIGHTED_MEAN && T == 0) {            // a long row of zero weights: the dummy's row
            const vec16 v0 = *reinterpret_cast<const vec16 *>((const TI *)a.table + (int64_t)a.dummy * a.ld + c0);
#pragma unroll
            for (int e = 0; e < VEC; ++e) r[e] = fg_io<TI>::elem(v0, e);
        }
        fg_store<TO, VEC>(a, row, c0, r);
    }
}

template <typename TI, typename TO, int MODE>
int launch_segment_reduce(const FgArgs &a, hipStream_t s)
{
    const int per_wg = FG_THREADS / a.team;
    const int64_t items = a.n_short + a.n_slices;
    launch(k_segment_reduce<TI, TO, MODE>, dim3((uint32_t)std::max<int64_t>(1, ceil_div(items, per_wg))),
           dim3(FG_THREADS), 0, s, a);
    int rc = check_launch("segment_reduce");
    if (rc != GSAGE_OK) return rc;
    // always launched (an empty grid exits at once): the launch count does not depend on the graph
    launch(k_segment_merge<TI, TO, MODE>, dim3((uint32_t)std::max<int64_t>(1, ceil_div(a.n_long, per_wg))),
           dim3(FG_THREADS), 0, s, a);
    return check_launch("segment_reduce_merge");
}

template <typename TI, typename TO>
int dispatch_mode(int mode, const FgArgs &a, hipStream_t s)
{
    switch (mode) {
    case GSAGE_SEG_MEAN: return launch_segment_reduce<TI, TO, GSAGE_SEG_MEAN>(a, s);
    case GSAGE_SEG_MAX: return launch_segment_reduce<TI, TO, GSAGE_SEG_MAX>(a, s);
    case GSAGE_SEG_WEIGHTED_MEAN: return launch_segment_reduce<TI, TO, GSAGE_SEG_WEIGHTED_MEAN>(a, s);
    default: return launch_segment_reduce<TI, TO, GSAGE_SEG_SOFTMAX_WEIGHTED>(a, s);
    }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

}  // namespace gsage

using namespace gsage;

extern "C" {

int64_t gsage_segment_reduce_ldp(int64_t D)
{
    if (D <= 0) return -1;
    return ceil_div(D, 8) * 8 + 4;
}

static int segment_reduce_any(int mode, const void *table, int dtype, int64_t ld, int64_t D, const float *keys,
                              int64_t ldk, const int64_t *rowptr, const int32_t *col, const uint64_t *cdf,
                              int64_t n_rows, int64_t n_src, int64_t dummy, const int32_t *order, int64_t n_short,
                              const int64_t *slices, int64_t n_slices, const int64_t *long_rows, int64_t n_long,
                              int32_t slice_len, float *partials, int64_t ldp, void *out, int out_dtype, int64_t out_ld,
                              int act, int32_t *err_flag, void *stream)
{
    GSAGE_REQUIRE(dtype == GSAGE_BF16 || dtype == GSAGE_F32, "segment_reduce: table dtype must be bf16 or fp32");
    GSAGE_REQUIRE(out_dtype == GSAGE_BF16 || out_dtype == GSAGE_F32, "segment_reduce: out dtype must be bf16 or fp32");
    GSAGE_REQUIRE(act == GSAGE_ACT_NONE || act == GSAGE_ACT_RELU, "segment_reduce: act must be none or relu");
    GSAGE_REQUIRE(D > 0 && D <= (1 << 20), "segment_reduce: bad width D=%lld", (long long)D);
    const int vec = dtype == GSAGE_BF16 ? 8 : 4;
    const int64_t Dp = ceil_div(D, vec) * vec;
    GSAGE_REQUIRE(ld % vec == 0 && Dp <= ld, "segment_reduce: ld must be a multiple of 16 bytes holding D");
    GSAGE_REQUIRE(out_ld >= D, "segment_reduce: out_ld smaller than D");
    GSAGE_REQUIRE(n_rows > 0 && n_rows < ((int64_t)1 << 31), "segment_reduce: bad n_rows");
    GSAGE_REQUIRE(n_src >= n_rows && n_src < ((int64_t)1 << 31) && dummy >= 0 && dummy < n_src,
                  "segment_reduce: a block needs n_dst <= n_src < 2^31 and a dummy inside the table");
    GSAGE_REQUIRE(n_short >= 0 && n_slices >= 0 && n_long >= 0 && n_short + n_long <= n_rows &&
                  n_long <= n_slices, "segment_reduce: bad plan sizes");
    GSAGE_REQUIRE(slice_len >= 8 && slice_len % 8 == 0, "segment_reduce: slice_len must be a positive multiple of 8");
    if (n_slices > 0)
        GSAGE_REQUIRE(partials && ldp >= gsage_segment_reduce_ldp(D) && ldp % 4 == 0 && aligned16(partials),
                      "segment_reduce: partials need [n_slices, ldp >= gsage_segment_reduce_ldp(D)] fp32, 16-byte aligned");
    if (mode == GSAGE_SEG_SOFTMAX_WEIGHTED)
        GSAGE_REQUIRE(keys && ldk >= 32 && ldk % 4 == 0 && aligned16(keys),
                      "segment_reduce: softmax mode needs 32-wide fp32 keys (ldk >= 32, 16-byte rows)");
    if (n_short + n_slices == 0) return GSAGE_OK;
    GSAGE_REQUIRE(table && rowptr && col && out && aligned16(table), "segment_reduce: null or misaligned pointer");
    GSAGE_REQUIRE(mode != GSAGE_SEG_WEIGHTED_MEAN || cdf, "segment_reduce_weighted: null cdf");
    GSAGE_REQUIRE(n_short == 0 || order, "segment_reduce: null order");
    GSAGE_REQUIRE(n_slices == 0 || (slices && long_rows), "segment_reduce: null slice plan");

    FgArgs a;
    a.table = table; a.ld = ld; a.D = (int32_t)D; a.Dp = (int32_t)Dp;
    a.keys = keys; a.ldk = ldk;
    a.rowptr = rowptr; a.col = col; a.n_rows = n_rows; a.n_src = n_src; a.dummy = (int32_t)dummy;
    a.order = order; a.n_short = n_short;
    a.slices = slices; a.n_slices = n_slices; a.long_rows = long_rows; a.n_long = n_long;
    a.slice_len = slice_len; a.partials = partials; a.ldp = ldp;
    a.out = out; a.out_ld = out_ld; a.act = act; a.err = err_flag; a.cdf = cdf;
    int team = 8;
    while (team < 64 && team * vec < Dp) team *= 2;
    a.team = team;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == GSAGE_BF16)
        return out_dtype == GSAGE_F32 ? dispatch_mode<uint16_t, float>(mode, a, s)
                                      : dispatch_mode<uint16_t, uint16_t>(mode, a, s);
    return out_dtype == GSAGE_F32 ? dispatch_mode<float, float>(mode, a, s) : dispatch_mode<float, uint16_t>(mode, a, s);
}

int gsage_segment_reduce(int mode, const void *table, int dtype, int64_t ld, int64_t D, const float *keys,
                         int64_t ldk, const int64_t *rowptr, const int32_t *col, int64_t n_rows,
                         const int32_t *order, int64_t n_short, const int64_t *slices, int64_t n_slices,
                         const int64_t *long_rows, int64_t n_long, int32_t slice_len, float *partials,
                         int64_t ldp, void *out, int out_dtype, int64_t out_ld, int act, int32_t *err_flag,
                         void *stream)
{
    GSAGE_REQUIRE(mode == GSAGE_SEG_MEAN || mode == GSAGE_SEG_MAX || mode == GSAGE_SEG_SOFTMAX_WEIGHTED,
                  "segment_reduce: unknown mode %d", mode);
    return segment_reduce_any(mode, table, dtype, ld, D, keys, ldk, rowptr, col, nullptr, n_rows, n_rows, 0, order, n_short,
                              slices, n_slices, long_rows, n_long, slice_len, partials, ldp, out, out_dtype, out_ld, act,
                              err_flag, stream);
}

int gsage_segment_reduce_weighted(const void *table, int dtype, int64_t ld, int64_t D, const int64_t *rowptr,
                                  const int32_t *col, const uint64_t *cdf, int64_t n_rows, const int32_t *order,
                                  int64_t n_short, const int64_t *slices, int64_t n_slices, const int64_t *long_rows,
                                  int64_t n_long, int32_t slice_len, float *partials, int64_t ldp, void *out,
                                  int out_dtype, int64_t out_ld, int act, int32_t *err_flag, void *stream)
{
    return segment_reduce_any(GSAGE_SEG_WEIGHTED_MEAN, table, dtype, ld, D, nullptr, 0, rowptr, col, cdf, n_rows, n_rows,
                              0, order, n_short, slices, n_slices, long_rows, n_long, slice_len, partials, ldp, out,
                              out_dtype, out_ld, act, err_flag, stream);
}

int gsage_segment_reduce_block(int mode, const void *table, int dtype, int64_t ld, int64_t D, const float *keys,
                               int64_t ldk, const int64_t *rowptr, const int32_t *col, const uint64_t *cdf,
                               int64_t n_dst, int64_t n_src, int64_t dummy, const int32_t *order, int64_t n_short,
                               const int64_t *slices, int64_t n_slices, const int64_t *long_rows, int64_t n_long,
                               int32_t slice_len, float *partials, int64_t ldp, void *out, int out_dtype,
                               int64_t out_ld, int act, int32_t *err_flag, void *stream)
{
    GSAGE_REQUIRE(mode == GSAGE_SEG_MEAN || mode == GSAGE_SEG_MAX || mode == GSAGE_SEG_SOFTMAX_WEIGHTED ||
                  mode == GSAGE_SEG_WEIGHTED_MEAN, "segment_reduce_block: unknown mode %d", mode);
    GSAGE_REQUIRE((mode == GSAGE_SEG_WEIGHTED_MEAN) == (cdf != nullptr),
                  "segment_reduce_block: cdf goes with the weighted mean, and only with it");
    return segment_reduce_any(mode, table, dtype, ld, D, keys, ldk, rowptr, col, cdf, n_dst, n_src, dummy, order, n_short,
                              slices, n_slices, long_rows, n_long, slice_len, partials, ldp, out, out_dtype, out_ld, act,
                              err_flag, stream);
}

}  // extern "C"
