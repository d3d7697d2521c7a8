// gsage_distinct.hip -- neighbour sampling WITHOUT replacement over a CSR (gfx950): the distinct-draw sampler.
//
// No reference counterpart: the reference's sparse sampler computes row[sel % deg], with replacement.  Here a parent of
// degree deg sampled n times gets (include/gsage.h, "Distinct neighbours")
//     deg <= n   every stored edge, floor(n / deg) or ceil(n / deg) times: the row rotated by a uniform r
//     deg >  n   n distinct stored edges, uniformly random as an ordered tuple: n steps of a Fisher-Yates shuffle
// so the plain mean over the n slots is the row's mean whenever deg divides n and an unbiased estimate of it always.
//
//   gsage_sample_csr_distinct   one launch per hop: a workgroup takes whole parents, 256 / n per trip
//   gsage_sample_hops_distinct  every hop of a frontier in ONE launch: the geometry of sample_hops_workgroup
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

// All hops of a frontier: sample_hops_workgroup's walk (same seeds per workgroup, same ping-pong LDS buffers, same ids
// layout, the LDS barrier between hops), each hop in trips of whole parents.
__global__ void __launch_bounds__(256)
k_sample_hops_distinct(const HopsParams p)
{
    extern __shared__ int64_t frontier[];
    const int seed0 = (int)blockIdx.x * p.spw;
    const int nseed = min(p.spw, p.B - seed0);
    if (nseed <= 0) return;
    int width = 1, widest = 1;
    for (int k = 1; k <= p.n_hops; ++k) { width *= p.fan[k]; widest = max(widest, width); }
    int64_t *cur = frontier, *nxt = frontier + (int64_t)p.spw * widest;
    uint32_t *tbuf = (uint32_t *)(frontier + 2 * (int64_t)p.spw * widest);
    if (p.seed_queue) {           // take the seeds from the queue (and publish them as hop 0)
        const int64_t b = (int64_t)((uint64_t)(*p.batch_idx + p.batch_base) % (uint64_t)p.n_batches);
        for (int t = threadIdx.x; t < nseed; t += 256) {
            const int64_t v = p.seed_queue[b * p.B + seed0 + t];
            cur[t] = v;
            p.ids[p.off[0] + seed0 + t] = v;
        }
    } else {
        for (int t = threadIdx.x; t < nseed; t += 256) cur[t] = p.ids[p.off[0] + seed0 + t];
    }
    lds_barrier();              // LDS only: the ids stored to HBM are not read back in this launch
    const uint64_t ctr = p.call_ctr ? *p.call_ctr : 0ull;
    int64_t per_seed = 1;                            // nodes of hop k per seed
    int par = 0;
    for (int k = 1; k <= p.n_hops; ++k) {
        const uint32_t n = (uint32_t)p.fan[k];
        const int64_t parents = per_seed * nseed;    // <= spw * widest: fits the LDS buffer (fill_hops)
        per_seed *= n;
        const uint64_t call = p.call_base + ctr + (uint64_t)(k - 1);
        const int64_t local0 = (int64_t)seed0 * per_seed;             // first sample of this WG in hop k
        const uint32_t P = 256u / n;
        const uint32_t q = threadIdx.x / n, j = threadIdx.x - q * n;
        for (int64_t i0 = 0; i0 < parents; i0 += P, par ^= 1) {       // (uniform over the workgroup)
            const int64_t i = i0 + q;
            const bool active = q < P && i < parents;
            const int64_t t = i * (int64_t)n + j;
            const int64_t v = distinct_trip(p.rowptr, p.col, p.n_rows, active, active ? cur[i] : 0, j, n,
                                            p.g0[k] + (uint64_t)(local0 + t), call, p.seed_lo, p.seed_hi, p.err_flag,
                                            tbuf + 256 * par);
            if (active) {
                nxt[t] = v;
                p.ids[p.off[k] + local0 + t] = v;
            }
        }
        lds_barrier();
        int64_t *tmp = cur; cur = nxt; nxt = tmp;
    }
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
    {
        int64_t width = 1, widest = 1;                    // (before fill_hops: its message names another entry)
        for (int k = 0; k < d.n_hops; ++k) { width *= d.fan[k]; if (width > widest) widest = width; }
        GSAGE_REQUIRE(sizeof(int64_t) * 2 * (size_t)hops_spw() * (size_t)widest + DISTINCT_TBUF <= 160 * 1024,
                      "sample_hops_distinct: the product of fan[] is too large: the widest hop of a workgroup's seeds "
                      "(%lld ids) does not fit the LDS", (long long)(widest * hops_spw()));
    }
    HopsParams p;
    size_t lds = 0;
    int rc = fill_hops(p, lds, d);
    if (rc != GSAGE_OK || d.B == 0) return rc;
    launch(k_sample_hops_distinct, dim3((unsigned)ceil_div(d.B, p.spw)), dim3(256), lds + DISTINCT_TBUF,
           (hipStream_t)stream, p);
    return check_launch("sample_hops_distinct");
}

}  // extern "C"
