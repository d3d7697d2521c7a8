// gsage_weighted.hip -- weighted adjacencies (gfx950): the per-edge integer CDF and the edge-weight neighbour sampler.
//
// No reference counterpart: the reference's adjacencies are unweighted.  A weighted adjacency is a device CSR plus one
// uint64 per stored edge, the inclusive running sum of the row's weights in integer QUANTA (include/gsage.h, "Weighted
// adjacency"): with m the row's largest weight and (f, E) = frexp(m), q_e = floor(w_e * 2^(24 - E)) < 2^24.  Scaling by
// a power of two and the floor are done on the bit pattern of w_e (a 24-bit significand shifted), so q_e is the
// mathematical value for denormal weights and for maxima near FLT_MAX alike, integer sums are exact in any order, and
// the table a scan builds does not depend on how the scan was cut.
//
//   gsage_edge_cdf_build       set-up, once per adjacency.  A WAVE per row of degree <= CDF_LONG (64-edge chunks, the
//                              carry in a register), a WORKGROUP per longer row (256-edge chunks, the waves' totals
//                              through LDS): the shipped graphs have a median degree well under 64 and a few rows of
//                              tens of thousands of edges, which a single wave would walk alone long after the rest
//                              of the launch has finished.
//   gsage_sample_csr_weighted  the hot path, one launch per hop: one lane per draw, a Philox word pair scaled to
//                              [0, T) by a 64 x 64 -> high 64 multiplication, then the plain binary search for the
//                              first entry of the row above it.  The n draws of a parent sit in consecutive lanes: the
//                              first probes of their searches read the same words.
//   gsage_sample_hops_weighted every hop of a frontier in ONE launch: frontier_walk
//                              (gsage_sample_dev.h: a workgroup per seed sub-tree, the previous hop in LDS), each
//                              sample the draw above.  The search probes seven evenly spaced entries per round, issued
//                              together (cdf_first_above_k8): three dependent rounds on a row of 420 edges where the
//                              binary search takes nine (GSAGE_WEIGHTED_SEARCH=binary: that search; same frontier).
#include <string.h>
#include "gsage_common.h"
#include "gsage_sample_dev.h"
#include "gsage_weighted_dev.h"

namespace gsage {

namespace {

constexpr int CDF_THREADS = 256;
constexpr int CDF_LONG = 256;              // rows of more edges get a workgroup
constexpr uint32_t WEIGHTED_TAG = 0x57000000u;   // xored into the key's high word: not the uniform sampler's stream
constexpr bool WEIGHTED_HOPS_KARY = true;  // gsage_sample_hops_weighted's search unless GSAGE_WEIGHTED_SEARCH says otherwise

// frexp exponent E of a finite fp32 m > 0 given by its bits: m = f * 2^E, f in [0.5, 1)
__device__ __forceinline__ int frexp_exp_bits(uint32_t b)
{
    const int e = (int)(b >> 23);
    if (e) return e - 126;
    return (31 - __clz((int)(b & 0x7fffffu))) - 148;          // denormal: top set bit p of the fraction, m in [2^(p-149), 2^(p-148))
}

// floor(w * 2^(24 - E)) for a finite fp32 0 <= w < 2^E given by its bits (a sign bit -- the caller has refused such
// weights -- is dropped: every shift below stays in range whatever the bits are)
__device__ __forceinline__ uint32_t quantum_bits(uint32_t b, int E)
{
    b &= 0x7fffffffu;
    const int e = (int)(b >> 23);
    const uint32_t sig = (b & 0x7fffffu) | (e ? 0x800000u : 0u);      // w = sig * 2^(max(e, 1) - 150)
    const int sh = (e ? e : 1) - 126 - E;                             // q = floor(sig * 2^sh); sh <= 23 (denormal maximum)
    if (sh >= 0) return sig << min(sh, 23);
    return sh <= -32 ? 0u : sig >> (-sh);
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
    return v;
}

// inclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ uint64_t wave_scan_u64(uint64_t v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t u = (uint64_t)__shfl_up((unsigned long long)v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// rows of degree <= CDF_LONG: one wave each
__global__ void __launch_bounds__(CDF_THREADS)
k_edge_cdf_wave(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ wbits, int64_t n_rows,
                uint64_t *__restrict__ cdf)
{
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (CDF_THREADS / 64);
    for (int64_t row = (int64_t)blockIdx.x * (CDF_THREADS / 64) + (threadIdx.x >> 6); row < n_rows; row += waves) {
        const int64_t beg = rowptr[row];
        const int64_t deg = rowptr[row + 1] - beg;
        if (deg <= 0 || deg > CDF_LONG) continue;
        uint32_t m = 0;                                   // weights are >= 0: the order of the bits is the order of the values
        for (int64_t j = lane; j < deg; j += 64) m = max(m, wbits[beg + j] & 0x7fffffffu);
        m = wave_max_u32(m);
        const int E = m ? frexp_exp_bits(m) : 0;
        uint64_t carry = 0;
        for (int64_t j0 = 0; j0 < deg; j0 += 64) {
            const int64_t j = j0 + lane;
            const uint64_t q = (m && j < deg) ? (uint64_t)quantum_bits(wbits[beg + j], E) : 0ull;
            const uint64_t s = carry + wave_scan_u64(q, lane);
            if (j < deg) cdf[beg + j] = s;
            carry = (uint64_t)__shfl((unsigned long long)s, 63, 64);
        }
    }
}

// rows of degree > CDF_LONG: one workgroup each
__global__ void __launch_bounds__(CDF_THREADS)
k_edge_cdf_block(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ wbits, int64_t n_rows,
                 uint64_t *__restrict__ cdf)
{
    __shared__ uint32_t s_max[CDF_THREADS / 64];
    __shared__ uint64_t s_tot[CDF_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const int64_t beg = rowptr[row];
        const int64_t deg = rowptr[row + 1] - beg;
        if (deg <= CDF_LONG) continue;                    // (uniform over the workgroup: no barrier is skipped by a part of it)
        uint32_t m = 0;
        for (int64_t j = threadIdx.x; j < deg; j += CDF_THREADS) m = max(m, wbits[beg + j] & 0x7fffffffu);
        m = wave_max_u32(m);
        if (lane == 0) s_max[wave] = m;
        __syncthreads();
        m = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
        const int E = m ? frexp_exp_bits(m) : 0;
        uint64_t carry = 0;
        for (int64_t j0 = 0; j0 < deg; j0 += CDF_THREADS) {
            const int64_t j = j0 + threadIdx.x;
            const uint64_t q = (m && j < deg) ? (uint64_t)quantum_bits(wbits[beg + j], E) : 0ull;
            uint64_t s = wave_scan_u64(q, lane);
            __syncthreads();                              // the previous chunk's (and the maxima's) readers are done
            if (lane == 63) s_tot[wave] = s;
            __syncthreads();
            uint64_t before = carry;
#pragma unroll
            for (int w = 0; w < CDF_THREADS / 64; ++w) {
                if (w < wave) before += s_tot[w];
                carry += s_tot[w];
            }
            if (j < deg) cdf[beg + j] = before + s;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256)
k_sample_weighted(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const uint64_t *__restrict__ cdf,
                  int64_t n_rows, const int64_t *__restrict__ ids, int64_t total, uint32_t n, uint32_t seed_lo,
                  uint32_t seed_hi, const uint64_t *__restrict__ call_ctr, uint64_t call_base, uint64_t g0,
                  int64_t *__restrict__ out, int32_t *err_flag)
{
    const uint64_t call = call_base + (call_ctr ? *call_ctr : 0ull);
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
        const int64_t i = (total <= 0xffffffffLL) ? (int64_t)((uint32_t)t / n) : t / (int64_t)n;
        const int64_t id = ids[i];
        if ((uint64_t)id >= (uint64_t)n_rows) {           // as pick_neighbor: the reference raises IndexError here
            if (err_flag) *err_flag = 1;
            out[t] = 0;
            continue;
        }
        const int64_t beg = rowptr[id], end = rowptr[id + 1];
        const uint64_t T = end > beg ? cdf[end - 1] : 0ull;
        if (T == 0) {                                     // no drawable edge: the dummy node, as a row of degree 0
            out[t] = 0;
            continue;
        }
        const uint64_t x = __umul64hi(philox_word64(g0 + (uint64_t)t, call, seed_lo, seed_hi ^ WEIGHTED_TAG), T);    // < T
        out[t] = (int64_t)col[cdf_first_above(cdf, beg, end, x)];
    }
}

// All hops of a weighted frontier: the frontier walk of gsage_sample_dev.h with gsage_sample_csr_weighted's draw per
// sample, a lane each.  The n children of a parent sit in consecutive lanes: their loads of rowptr and of the row's
// total are the same words.
template <bool KARY>
__global__ void __launch_bounds__(256)
k_sample_hops_weighted(const HopsParams p, const uint64_t *__restrict__ cdf)
{
    extern __shared__ int64_t frontier[];
    Frontier f;
    if (!frontier_setup<256>(p, (int)blockIdx.x, frontier, f)) return;
    frontier_walk(p, f, [&](const Hop &h) {
        for (int64_t t = threadIdx.x; t < h.count; t += 256) {
            const int64_t id = f.cur[(uint32_t)t / h.n];
            int64_t v = 0;                           // the dummy: no drawable edge, or an id outside the graph
            if ((uint64_t)id >= (uint64_t)p.n_rows) {
                if (p.err_flag) *p.err_flag = 1;
            } else {
                const int64_t beg = p.rowptr[id], end = p.rowptr[id + 1];
                const uint64_t T = end > beg ? cdf[end - 1] : 0ull;
                if (T != 0) {
                    const uint64_t r64 = philox_word64(hop_sample(p, h, t), h.call, p.seed_lo, p.seed_hi ^ WEIGHTED_TAG);
                    const uint64_t x = __umul64hi(r64, T);                                 // < T
                    v = (int64_t)p.col[KARY ? cdf_first_above_k8(cdf, beg, end, x) : cdf_first_above(cdf, beg, end, x)];
                }
            }
            hop_store(p, f, h, t, v);
        }
    });
}

inline int weighted_grid(int64_t items, int per_block, int cap)
{
    int64_t b = ceil_div(items, per_block);
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

}  // namespace

}  // namespace gsage

using namespace gsage;

extern "C" {

int gsage_edge_cdf_build(const int64_t *rowptr, const float *weight, int64_t n_rows, uint64_t *cdf, void *stream)
{
    GSAGE_REQUIRE(n_rows >= 0, "edge_cdf_build: negative size");
    if (n_rows == 0) return GSAGE_OK;
    GSAGE_REQUIRE(rowptr && weight && cdf, "edge_cdf_build: null pointer");
    launch(k_edge_cdf_wave, dim3(weighted_grid(n_rows, CDF_THREADS / 64, 16384)), dim3(CDF_THREADS), 0,
           (hipStream_t)stream, rowptr, (const uint32_t *)weight, n_rows, cdf);
    int rc = check_launch("edge_cdf_build");
    if (rc != GSAGE_OK) return rc;
    // always launched (a workgroup that finds no long row among its rows exits after reading their degrees)
    launch(k_edge_cdf_block, dim3(weighted_grid(n_rows, 1, 2048)), dim3(CDF_THREADS), 0, (hipStream_t)stream, rowptr,
           (const uint32_t *)weight, n_rows, cdf);
    return check_launch("edge_cdf_build_long");
}

int gsage_sample_csr_weighted(const int64_t *rowptr, const int32_t *col, const uint64_t *cdf, int64_t n_rows,
                              const int64_t *ids, int64_t M, int32_t n, uint64_t seed, const uint64_t *call_ctr,
                              uint64_t call_base, uint64_t g0, int64_t *out, int32_t *err_flag, void *stream)
{
    GSAGE_REQUIRE(n > 0, "sample_csr_weighted: n_samples must be > 0");
    GSAGE_REQUIRE(M >= 0 && n_rows >= 0, "sample_csr_weighted: negative size");
    if (M == 0) return GSAGE_OK;
    GSAGE_REQUIRE(rowptr && col && cdf && ids && out, "sample_csr_weighted: null pointer");
    const int64_t total = M * (int64_t)n;
    launch(k_sample_weighted, dim3(weighted_grid(total, 256, 8192)), dim3(256), 0, (hipStream_t)stream, rowptr, col,
           cdf, n_rows, ids, total, (uint32_t)n, (uint32_t)seed, (uint32_t)(seed >> 32), call_ctr, call_base, g0, out,
           err_flag);
    return check_launch("sample_csr_weighted");
}

int gsage_sample_hops_weighted(const gsage_hops_desc *hops, const uint64_t *cdf, void *stream)
{
    GSAGE_REQUIRE(hops, "sample_hops_weighted: null descriptor");
    GSAGE_REQUIRE(cdf, "sample_hops_weighted: null cdf (the adjacency carries no edge weights)");
    GSAGE_REQUIRE(!hops->sel && !hops->dense_adj,
                  "sample_hops_weighted: the weighted sampler draws from Philox over a CSR (no sel, no dense adjacency)");
    gsage_hops_desc d = *hops;
    d.max_deg = 1;                                        // ignored: a draw is scaled by its row's total
    HopsParams p;
    size_t lds = 0;
    int rc = fill_hops(p, lds, d);
    if (rc != GSAGE_OK || d.B == 0) return rc;
    // GSAGE_WEIGHTED_SEARCH=kary / binary (read per call, not once: a recorded list keeps the form it was recorded with)
    const char *e = getenv("GSAGE_WEIGHTED_SEARCH");
    const bool kary = e && strcmp(e, "kary") == 0 ? true : e && strcmp(e, "binary") == 0 ? false : WEIGHTED_HOPS_KARY;
    launch(kary ? k_sample_hops_weighted<true> : k_sample_hops_weighted<false>, dim3((unsigned)ceil_div(d.B, p.spw)),
           dim3(256), lds, (hipStream_t)stream, p, cdf);
    return check_launch("sample_hops_weighted");
}

}  // extern "C"
