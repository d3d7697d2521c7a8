// gsage_propagate.hip -- one step of label / residual propagation over a CSR adjacency (gfx950), fp32.
//
//     acc[v, c]  = sum_{e in [rowptr[v], rowptr[v+1])} y[col[e], c]       an empty row: 0 (NOT the dummy)
//     out[v, c]  = min(max(beta * base[v, c] + alpha * (a[v] * acc[v, c]), lo), hi)          c < C
//     yout[v, c] = b[v] * out[v, c]
//
// y is the PRE-SCALED iterate b (.) x, so the neighbour loop is a plain sum of 16-byte row chunks with no
// per-neighbour scale fetch, and the epilogue writes the next step's y next to the iterate itself: the caller
// (propagate.py) ping-pongs two buffers and issues nothing else per step.  With a = b = deg^-1/2 this is
// x' = clamp(beta * base + alpha * D^-1/2 A D^-1/2 x), the step of label propagation and of Correct and Smooth.
//
// Schedule and loads are those of the full-neighbourhood segment reduce (gsage_fullgraph.hip), over the same plan
// (infer.plan): short rows in degree-descending order, longer rows cut into slices of slice_len edges.  Launch 1 gives
// each short row and each slice a TEAM of 8 / 16 / 32 / 64 lanes -- one 16-byte column chunk (4 columns) per lane,
// several teams per wave when the row is narrow --, 8 neighbour rows in flight per lane, the ids of the next batch
// requested before the rows of the current one; short rows run the epilogue, slices write fp32 partial sums.
// Launch 2 adds the partials of each long row in slice order and runs the same epilogue.  No floating-point atomics:
// the same inputs give the same bits.  An id outside [0, n_rows) contributes 0 and raises *err_flag.
#include "gsage_common.h"

#include <math.h>

namespace gsage {

namespace {

constexpr int PG_THREADS = 256;
constexpr int PG_BATCH = 8;
constexpr int PG_VEC = 4;

struct PgArgs {
    const float *y;
    int64_t ldy;
    const float *base;              // may be null (beta == 0)
    int64_t ldb;
    const float *a, *b;             // per-row scales; null = 1
    float alpha, beta, lo, hi;
    int32_t C, Cp;                  // logical width, width rounded up to the 16-byte chunk
    const int64_t *rowptr;
    const int32_t *col;
    int64_t n_rows;
    const int32_t *order;           // short rows, degree-descending
    int64_t n_short;
    const int64_t *slices;          // [n_slices, 2]: (row, first edge)
    int64_t n_slices;
    const int64_t *long_rows;       // [n_long, 2]: (row, index of its first slice)
    int64_t n_long;
    int32_t slice_len;
    float *partials;                // [n_slices, ldp]
    int64_t ldp;
    float *out;                     // may be null
    int64_t ldo;
    float *yout;                    // may be null
    int64_t ldyo;
    int32_t team;                   // lanes per row: 8, 16, 32 or 64
    int32_t *err;                   // set to 1 when a neighbour id is outside [0, n_rows)
};

// s += sum of the chunk at column cc of the rows col[beg .. beg + cnt), cnt >= 1, in stored order.
__device__ __forceinline__ void pg_walk(const PgArgs &a, int64_t beg, int64_t cnt, int32_t cc, float (&s)[PG_VEC])
{
    const int32_t *col = a.col + beg;
    // an id outside the table: -1, which reads row 0 and is dropped from the sum
    auto id_at = [&](int64_t j) -> int32_t {
        int32_t id = col[min(j, cnt - 1)];
        if ((uint32_t)id >= (uint32_t)a.n_rows) {
            if (a.err) *a.err = 1;
            id = -1;
        }
        return id;
    };
    int32_t rc[PG_BATCH], rn[PG_BATCH];
#pragma unroll
    for (int u = 0; u < PG_BATCH; ++u) rn[u] = rc[u] = id_at(u);
    for (int64_t j = 0; j < cnt; j += PG_BATCH) {
        const int m = (int)min((int64_t)PG_BATCH, cnt - j);
        if (j + PG_BATCH < cnt) {
#pragma unroll
            for (int u = 0; u < PG_BATCH; ++u) rn[u] = id_at(j + PG_BATCH + u);
        }
        vec16 v[PG_BATCH];
#pragma unroll
        for (int u = 0; u < PG_BATCH; ++u)
            v[u] = *reinterpret_cast<const vec16 *>(a.y + (int64_t)max(rc[u], 0) * a.ldy + cc);
#pragma unroll
        for (int u = 0; u < PG_BATCH; ++u) {
            if (u < m && rc[u] >= 0) {
#pragma unroll
                for (int e = 0; e < PG_VEC; ++e) s[e] += __uint_as_float(v[u][e]);
            }
        }
#pragma unroll
        for (int u = 0; u < PG_BATCH; ++u) rc[u] = rn[u];
    }
}

// the epilogue of a finished row chunk: scale, residual, clamp; the iterate and / or the next step's y
__device__ __forceinline__ void pg_finish(const PgArgs &a, int64_t row, int32_t c0, const float (&s)[PG_VEC])
{
    const float av = a.a ? a.a[row] : 1.f;
    const float bv = a.b ? a.b[row] : 1.f;
    float r[PG_VEC];
#pragma unroll
    for (int e = 0; e < PG_VEC; ++e) r[e] = 0.f;
    if (a.base) {
        const vec16 w = *reinterpret_cast<const vec16 *>(a.base + row * a.ldb + c0);
#pragma unroll
        for (int e = 0; e < PG_VEC; ++e) r[e] = a.beta * __uint_as_float(w[e]);
    }
#pragma unroll
    for (int e = 0; e < PG_VEC; ++e) r[e] = fminf(fmaxf(r[e] + a.alpha * (av * s[e]), a.lo), a.hi);
    const bool whole = c0 + PG_VEC <= a.C;
    if (a.out) {
        float *o = a.out + row * a.ldo + c0;
        if (whole) {
            vec16 w;
#pragma unroll
            for (int e = 0; e < PG_VEC; ++e) w[e] = __float_as_uint(r[e]);
            *reinterpret_cast<vec16 *>(o) = w;
        } else {
#pragma unroll
            for (int e = 0; e < PG_VEC; ++e)
                if (c0 + e < a.C) o[e] = r[e];
        }
    }
    if (a.yout) {
        float *o = a.yout + row * a.ldyo + c0;
        if (whole) {
            vec16 w;
#pragma unroll
            for (int e = 0; e < PG_VEC; ++e) w[e] = __float_as_uint(bv * r[e]);
            *reinterpret_cast<vec16 *>(o) = w;
        } else {
#pragma unroll
            for (int e = 0; e < PG_VEC; ++e)
                if (c0 + e < a.C) o[e] = bv * r[e];
        }
    }
}

// launch 1: one team per short row or slice
__global__ __launch_bounds__(PG_THREADS) void k_propagate(PgArgs a)
{
    const int team = a.team;
    const int lane = threadIdx.x & (team - 1);
    const int64_t item = (int64_t)blockIdx.x * (PG_THREADS / team) + threadIdx.x / team;
    if (item >= a.n_short + a.n_slices) return;
    int64_t row, beg, cnt;
    const bool is_slice = item >= a.n_short;
    if (!is_slice) {
        row = a.order[item];
        beg = a.rowptr[row];
        cnt = a.rowptr[row + 1] - beg;
    } else {
        const int64_t s = item - a.n_short;
        row = a.slices[2 * s];
        beg = a.slices[2 * s + 1];
        cnt = min((int64_t)a.slice_len, a.rowptr[row + 1] - beg);
    }
    const int32_t chunks = a.Cp / PG_VEC;
    for (int32_t g = lane; g < chunks; g += team) {
        const int32_t c0 = g * PG_VEC;
        float s[PG_VEC];
#pragma unroll
        for (int e = 0; e < PG_VEC; ++e) s[e] = 0.f;
        if (cnt > 0) pg_walk(a, beg, cnt, c0, s);
        if (is_slice) {
            vec16 w;
#pragma unroll
            for (int e = 0; e < PG_VEC; ++e) w[e] = __float_as_uint(s[e]);
            *reinterpret_cast<vec16 *>(a.partials + (item - a.n_short) * a.ldp + c0) = w;
        } else {
            pg_finish(a, row, c0, s);
        }
    }
}

// launch 2: one team per long row, its slices added in slice order
__global__ __launch_bounds__(PG_THREADS) void k_propagate_merge(PgArgs a)
{
    const int team = a.team;
    const int lane = threadIdx.x & (team - 1);
    const int64_t lr = (int64_t)blockIdx.x * (PG_THREADS / team) + threadIdx.x / team;
    if (lr >= a.n_long) return;
    const int64_t row = a.long_rows[2 * lr], s0 = a.long_rows[2 * lr + 1];
    const int64_t deg = a.rowptr[row + 1] - a.rowptr[row];
    const int64_t ns = (deg + a.slice_len - 1) / a.slice_len;
    const int32_t chunks = a.Cp / PG_VEC;
    for (int32_t g = lane; g < chunks; g += team) {
        const int32_t c0 = g * PG_VEC;
        float s[PG_VEC];
#pragma unroll
        for (int e = 0; e < PG_VEC; ++e) s[e] = 0.f;
        for (int64_t k = 0; k < ns; ++k) {
            const vec16 w = *reinterpret_cast<const vec16 *>(a.partials + (s0 + k) * a.ldp + c0);
#pragma unroll
            for (int e = 0; e < PG_VEC; ++e) s[e] += __uint_as_float(w[e]);
        }
        pg_finish(a, row, c0, s);
    }
}

// a, b of gsage_propagate from the row degrees
__global__ __launch_bounds__(PG_THREADS) void k_propagate_scales(const int64_t *rowptr, int64_t n_rows, int norm,
                                                                 float *a, float *b)
{
    const int64_t v = (int64_t)blockIdx.x * PG_THREADS + threadIdx.x;
    if (v >= n_rows) return;
    const int64_t deg = rowptr[v + 1] - rowptr[v];
    const float d = (float)deg;
    float av = 1.f, bv = 1.f;
    if (norm == GSAGE_PROP_SYM) av = bv = deg > 0 ? 1.f / sqrtf(d) : 0.f;
    else if (norm == GSAGE_PROP_ROW) av = deg > 0 ? 1.f / d : 0.f;
    else bv = deg > 0 ? 1.f / d : 0.f;
    a[v] = av;
    b[v] = bv;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

}  // namespace gsage

using namespace gsage;

extern "C" {

int gsage_propagate_scales(const int64_t *rowptr, int64_t n_rows, int norm, float *a, float *b, void *stream)
{
    GSAGE_REQUIRE(norm == GSAGE_PROP_SYM || norm == GSAGE_PROP_ROW || norm == GSAGE_PROP_COL,
                  "propagate_scales: norm must be 0 (sym), 1 (row) or 2 (col), not %d", norm);
    GSAGE_REQUIRE(n_rows > 0 && n_rows < ((int64_t)1 << 31), "propagate_scales: bad n_rows");
    GSAGE_REQUIRE(rowptr && a && b, "propagate_scales: null pointer");
    launch(k_propagate_scales, dim3((uint32_t)ceil_div(n_rows, PG_THREADS)), dim3(PG_THREADS), 0, (hipStream_t)stream,
           rowptr, n_rows, norm, a, b);
    return check_launch("propagate_scales");
}

int gsage_propagate(const float *y, int64_t ldy, const float *base, int64_t ldb, const float *a, const float *b,
                    float alpha, float beta, float lo, float hi, int64_t C,
                    const int64_t *rowptr, const int32_t *col, int64_t n_rows,
                    const int32_t *order, int64_t n_short, const int64_t *slices, int64_t n_slices,
                    const int64_t *long_rows, int64_t n_long, int32_t slice_len, float *partials, int64_t ldp,
                    float *out, int64_t ldo, float *yout, int64_t ldyo, int32_t *err_flag, void *stream)
{
    GSAGE_REQUIRE(C >= 1 && C <= 1024, "propagate: the width C must lie in [1, 1024], not %lld", (long long)C);
    const int64_t Cp = ceil_div(C, PG_VEC) * PG_VEC;
    GSAGE_REQUIRE(ldy % PG_VEC == 0 && ldy >= Cp, "propagate: ldy must be a multiple of 4 floats holding C, not %lld",
                  (long long)ldy);
    GSAGE_REQUIRE(out || yout, "propagate: out and yout are both null");
    GSAGE_REQUIRE(base || beta == 0.f, "propagate: base is null and beta is not 0");
    GSAGE_REQUIRE(!base || (ldb % PG_VEC == 0 && ldb >= Cp), "propagate: ldb must be a multiple of 4 floats holding C");
    GSAGE_REQUIRE(!out || (ldo % PG_VEC == 0 && ldo >= Cp), "propagate: ldo must be a multiple of 4 floats holding C");
    GSAGE_REQUIRE(!yout || (ldyo % PG_VEC == 0 && ldyo >= Cp), "propagate: ldyo must be a multiple of 4 floats holding C");
    GSAGE_REQUIRE(!(lo > hi), "propagate: the clamp needs lo <= hi");
    GSAGE_REQUIRE(n_rows > 0 && n_rows < ((int64_t)1 << 31), "propagate: bad n_rows");
    GSAGE_REQUIRE(n_short >= 0 && n_slices >= 0 && n_long >= 0 && n_short + n_long <= n_rows && n_long <= n_slices,
                  "propagate: bad plan sizes");
    GSAGE_REQUIRE(slice_len >= 8 && slice_len % 8 == 0, "propagate: slice_len must be a positive multiple of 8");
    if (n_slices > 0)
        GSAGE_REQUIRE(partials && ldp >= gsage_segment_reduce_ldp(C) && ldp % 4 == 0 && aligned16(partials),
                      "propagate: partials need [n_slices, ldp >= gsage_segment_reduce_ldp(C)] fp32, 16-byte aligned");
    GSAGE_REQUIRE(y && rowptr && col, "propagate: null pointer");
    GSAGE_REQUIRE(aligned16(y) && aligned16(base) && aligned16(out) && aligned16(yout),
                  "propagate: rows must be 16-byte aligned");
    GSAGE_REQUIRE((const float *)out != y && (const float *)yout != y, "propagate: y must not alias out or yout");
    GSAGE_REQUIRE(n_short == 0 || order, "propagate: null order");
    GSAGE_REQUIRE(n_slices == 0 || (slices && long_rows), "propagate: null slice plan");

    PgArgs p;
    p.y = y; p.ldy = ldy; p.base = base; p.ldb = ldb; p.a = a; p.b = b;
    p.alpha = alpha; p.beta = beta; p.lo = lo; p.hi = hi; p.C = (int32_t)C; p.Cp = (int32_t)Cp;
    p.rowptr = rowptr; p.col = col; p.n_rows = n_rows;
    p.order = order; p.n_short = n_short;
    p.slices = slices; p.n_slices = n_slices; p.long_rows = long_rows; p.n_long = n_long;
    p.slice_len = slice_len; p.partials = partials; p.ldp = ldp;
    p.out = out; p.ldo = ldo; p.yout = yout; p.ldyo = ldyo; p.err = err_flag;
    int team = 8;
    while (team < 64 && team * PG_VEC < Cp) team *= 2;
    p.team = team;
    hipStream_t s = (hipStream_t)stream;
    const int per_wg = PG_THREADS / team;
    launch(k_propagate, dim3((uint32_t)std::max<int64_t>(1, ceil_div(n_short + n_slices, per_wg))), dim3(PG_THREADS), 0,
           s, p);
    int rc = check_launch("propagate");
    if (rc != GSAGE_OK) return rc;
    // always launched (an empty grid exits at once): two launches per step, whatever the graph
    launch(k_propagate_merge, dim3((uint32_t)std::max<int64_t>(1, ceil_div(n_long, per_wg))), dim3(PG_THREADS), 0, s, p);
    return check_launch("propagate_merge");
}

}  // extern "C"
