// gsage_distinct.hip -- neighbour sampling WITHOUT replacement over a CSR (gfx950): the distinct-draw sampler.
//
// No reference counterpart: the reference's sparse sampler computes row[sel % deg], with replacement.  Here a parent of
// degree deg sampled n times gets (include/gsage.h, "Distinct neighbours")
//     deg <= n   every stored edge, floor(n / deg) or ceil(n / deg) times: the row rotated by a uniform r
//     deg >  n   n distinct stored edges, uniformly random as an ordered tuple: n steps of a Fisher-Yates shuffle
// so the plain mean over the n slots is the row's mean whenever deg divides n and an unbiased estimate of it always.
//
//   gsage_sample_csr_distinct   one launch per hop: a workgroup takes whole parents, 256 / n per trip
//   gsage_sample_hops_distinct  every hop of a frontier in ONE launch: frontier_walk
//                               (gsage_sample_dev.h: a workgroup per seed sub-tree, the previous hop in LDS), each hop
//                               walked in the same trips of whole parents
// Both run the body of gsage_distinct_dev.h: one lane per sample, the shuffle's t_j exchanged through LDS.
#include "gsage_common.h"
#include "gsage_sample_dev.h"
#include "gsage_distinct_dev.h"

namespace gsage {

namespace {

constexpr int DISTINCT_N_MAX = 256;                 // a parent's slots fit one trip of a 256-lane workgroup
constexpr size_t DISTINCT_TBUF = 2 * 256 * sizeof(uint32_t);      // two trips' t words

__global__ void __launch_bounds__(256)
k_sample_distinct(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t n_rows,
                  const int64_t *__restrict__ ids, int64_t M, uint32_t n, uint32_t seed_lo, uint32_t seed_hi,
                  const uint64_t *__restrict__ call_ctr, uint64_t call_base, uint64_t g0, int64_t *__restrict__ out,
                  int32_t *err_flag)
{
    __shared__ uint32_t tbuf[2 * 256];
    const uint64_t call = call_base + (call_ctr ? *call_ctr : 0ull);
    const uint32_t P = 256u / n;                        // parents per trip
    const uint32_t q = threadIdx.x / n, j = threadIdx.x - q * n;
    const int64_t groups = (M + P - 1) / P;
    int par = 0;
    for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x, par ^= 1) {       // (uniform over the workgroup)
        const int64_t i = grp * P + q;
        const bool active = q < P && i < M;
        const int64_t t = i * (int64_t)n + j;
        const int64_t v = distinct_trip(rowptr, col, n_rows, active, active ? ids[i] : 0, j, n, g0 + (uint64_t)t, call,
                                        seed_lo, seed_hi, err_flag, tbuf + 256 * par);
        if (active) out[t] = v;
    }
}

// All hops of a frontier: the frontier walk of gsage_sample_dev.h, each hop in trips of whole parents.  The two trip
// buffers sit behind the frontier's two LDS buffers; their parity runs on across the hops.
__global__ void __launch_bounds__(256)
k_sample_hops_distinct(const HopsParams p)
{
    extern __shared__ int64_t frontier[];
    Frontier f;
    if (!frontier_setup<256>(p, (int)blockIdx.x, frontier, f)) return;
    uint32_t *tbuf = (uint32_t *)(frontier + 2 * f.cap);
    int par = 0;
    frontier_walk(p, f, [&](const Hop &h) {
        const uint32_t n = h.n, P = 256u / n;
        const uint32_t q = threadIdx.x / n, j = threadIdx.x - q * n;
        for (int64_t i0 = 0; i0 < h.parents; i0 += P, par ^= 1) {     // (uniform over the workgroup)
            const int64_t i = i0 + q;
            const bool active = q < P && i < h.parents;
            const int64_t t = i * (int64_t)n + j;
            const int64_t v = distinct_trip(p.rowptr, p.col, p.n_rows, active, active ? f.cur[i] : 0, j, n,
                                            hop_sample(p, h, t), h.call, p.seed_lo, p.seed_hi, p.err_flag,
                                            tbuf + 256 * par);
            if (active) hop_store(p, f, h, t, v);
        }
    });
}

}  // namespace

}  // namespace gsage

using namespace gsage;

extern "C" {

int gsage_sample_csr_distinct(const int64_t *rowptr, const int32_t *col, int64_t n_rows, const int64_t *ids, int64_t M,
                              int32_t n, uint64_t seed, const uint64_t *call_ctr, uint64_t call_base, uint64_t g0,
                              int64_t *out, int32_t *err_flag, void *stream)
{
    GSAGE_REQUIRE(n >= 1 && n <= DISTINCT_N_MAX, "sample_csr_distinct: n (samples per parent) must be in 1..256");
    GSAGE_REQUIRE(M >= 0 && n_rows >= 0, "sample_csr_distinct: negative size (M, n_rows)");
    if (M == 0) return GSAGE_OK;
    GSAGE_REQUIRE(rowptr && col && ids && out, "sample_csr_distinct: null pointer (rowptr, col, ids, out)");
    int64_t grid = ceil_div(M, 256 / n);
    if (grid > 8192) grid = 8192;
    launch(k_sample_distinct, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, rowptr, col, n_rows, ids, M,
           (uint32_t)n, (uint32_t)seed, (uint32_t)(seed >> 32), call_ctr, call_base, g0, out, err_flag);
    return check_launch("sample_csr_distinct");
}

int gsage_sample_hops_distinct(const gsage_hops_desc *hops, void *stream)
{
    GSAGE_REQUIRE(hops, "sample_hops_distinct: null descriptor (hops)");
    GSAGE_REQUIRE(!hops->sel, "sample_hops_distinct: sel must be NULL (the distinct sampler draws from Philox)");
    GSAGE_REQUIRE(!hops->dense_adj, "sample_hops_distinct: dense_adj must be NULL (the distinct sampler walks a CSR)");
    GSAGE_REQUIRE(hops->n_hops >= 1 && hops->n_hops <= 5, "sample_hops_distinct: n_hops must be in 1..5");
    for (int k = 0; k < hops->n_hops; ++k)
        GSAGE_REQUIRE(hops->fan[k] >= 1 && hops->fan[k] <= DISTINCT_N_MAX,
                      "sample_hops_distinct: fan[%d] must be in 1..256", k);
    GSAGE_REQUIRE(hops->rowptr && hops->col && hops->ids, "sample_hops_distinct: null pointer (rowptr, col, ids)");
    gsage_hops_desc d = *hops;
    d.max_deg = 1;                                        // ignored: a draw is scaled by its row's degree
    const int64_t widest = hops_widest(d, d.n_hops);
    GSAGE_REQUIRE(hops_lds_bytes(widest, 2 * sizeof(int64_t), DISTINCT_TBUF) <= HOPS_LDS_MAX,
                  "sample_hops_distinct: the product of fan[] is too large: the widest hop of a workgroup's seeds "
                  "(%lld ids) does not fit the LDS", (long long)(widest * hops_spw()));
    HopsParams p;
    size_t lds = 0;
    int rc = fill_hops(p, lds, d, 2 * sizeof(int64_t), DISTINCT_TBUF);
    if (rc != GSAGE_OK || d.B == 0) return rc;
    launch(k_sample_hops_distinct, dim3((unsigned)ceil_div(d.B, p.spw)), dim3(256), lds, (hipStream_t)stream, p);
    return check_launch("sample_hops_distinct");
}

}  // extern "C"
