// gsage_sample_dev.h -- device body of the fused multi-hop sampler (K1), shared by the stand-alone
// kernel (gsage_sample.hip) and by k_gather_multi_adam (gsage_gather.hip), which samples a LATER
// batch's frontier inside the launch that gathers the next batch's rows.
//
// Every all-hops sampler is ONE frontier walk (frontier_setup, frontier_walk: a workgroup's seeds, the ping-pong LDS
// buffers, the per-hop bookkeeping, the barrier and the swap) plus its own hop body: the uniform bodies below
// (sample_hops_workgroup, sample_hops_wide) and the weighted, distinct and temporal kernels of their own files.
#pragma once
#include "gsage_common.h"

namespace gsage {

__device__ __forceinline__ int64_t pick_neighbor(const int64_t *__restrict__ rowptr,
                                                 const int32_t *__restrict__ col, int64_t n_rows,
                                                 int64_t id, uint32_t s, int32_t *err_flag)
{
    if ((uint64_t)id >= (uint64_t)n_rows) {          // the reference raises IndexError here
        if (err_flag) *err_flag = 1;
        return 0;
    }
    const int64_t beg = rowptr[id];
    const int64_t deg = rowptr[id + 1] - beg;
    if (deg <= 0) return 0;                          // numpy: x % 0 == 0 -> column 0 of an empty row
    const uint64_t off = (deg <= 0xffffffffLL) ? (uint64_t)(s % (uint32_t)deg) : (uint64_t)s;
    return (int64_t)col[beg + (int64_t)off];
}

// Dense adjacency (reference nn_modules.py:19-49: UniformNeighborSampler over an int64 [n_rows, K] table whose
// rows were pre-sampled to exactly K neighbours): neighbour `column` of node id
__device__ __forceinline__ int64_t pick_dense(const int64_t *__restrict__ adj, int64_t ld, int64_t n_rows,
                                              int64_t id, uint32_t column, int32_t *err_flag)
{
    if ((uint64_t)id >= (uint64_t)n_rows || (int64_t)column >= ld) {     // torch indexing raises IndexError here
        if (err_flag) *err_flag = 1;
        return 0;
    }
    return adj[id * ld + (int64_t)column];
}


// Either of the two inside the fused multi-hop kernel: a dense row is a CSR row with beg = id * ld, deg = ld
// (one code path, two selects: the kernel shares its registers with the HBM-bound gather role, gsage_gather.hip)
__device__ __forceinline__ int64_t pick_any(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                            const int64_t *__restrict__ dense, int64_t dense_ld, int64_t n_rows,
                                            int64_t id, uint32_t s, int32_t *err_flag)
{
    if ((uint64_t)id >= (uint64_t)n_rows) {
        if (err_flag) *err_flag = 1;
        return 0;
    }
    const int64_t beg = dense ? id * dense_ld : rowptr[id];
    const int64_t deg = dense ? dense_ld : rowptr[id + 1] - beg;
    if (deg <= 0) return 0;
    const uint64_t off = (deg <= 0xffffffffLL) ? (uint64_t)(s % (uint32_t)deg) : (uint64_t)s;
    return dense ? dense[beg + (int64_t)off] : (int64_t)col[beg + (int64_t)off];
}

// All hops of a frontier in ONE launch.  A workgroup owns SPW consecutive seeds and walks their
// whole sub-tree: the children of hop k are produced by the same workgroup that consumes them at
// hop k+1, so the only synchronisation is __syncthreads() and the previous hop's ids sit in LDS.
// Sample (hop k, global index g) uses exactly the Philox word the per-hop kernel would use
// (call index call_base + k - 1, counter g), so results are identical to L separate launches.
struct HopsParams {
    const int64_t *rowptr;
    const int32_t *col;
    int64_t *ids;                 // [hop 0 | hop 1 | ... | hop L], hop 0 filled by the caller
    const uint64_t *call_ctr;
    int32_t *err_flag;
    const int64_t *seed_queue;    // optional [n_batches, B] device-resident seed batches ...
    const int64_t *batch_idx;     // ... and the device word selecting the current one
    int64_t n_batches;
    int64_t batch_base;           // added to *batch_idx (sampling AHEAD of the counters, see k_gather_multi_adam)
    const int32_t *sel;           // optional: caller-supplied sel [hop 1 | hop 2 | ...] instead of Philox
    int64_t sel_stride;           // with a seed queue: sel of batch b starts at sel + b * sel_stride
    const int64_t *dense_adj;     // optional: dense [n_rows, dense_ld] adjacency instead of the CSR; sel then holds the
    int64_t dense_ld;             // columns every parent of a hop keeps: [fan[1] of hop 1 | fan[2] of hop 2 | ...]
    int64_t n_rows;
    int64_t off[6];               // first element of hop k in ids
    uint64_t g0[6];               // global sample index of this rank's first sample of hop k
    uint64_t call_base;
    int32_t fan[6];               // fan[k]: samples per parent at hop k (k >= 1)
    int32_t n_hops, B;
    uint32_t max_deg, seed_lo, seed_hi;
    int32_t spw;                  // seeds per workgroup (hops_spw())
};

// Seeds per workgroup of the fused multi-hop sampler.  1 (default): hop 2 of a 25x10 frontier is one pass of 250
// lanes, so a seed's whole sub-tree costs two dependent (rowptr -> col) round trips.  GSAGE_HOPS_SPW=2 / 4 (read once):
// fewer, fatter workgroups -- as a ROLE of k_gather_multi_adam the sampler's B workgroups hold B of the launch's 1 792
// resident slots while their chains run (what the finalisation role ran into).
inline int hops_spw()
{
    static const int v = [] { const char *e = getenv("GSAGE_HOPS_SPW"); const int x = e ? atoi(e) : 1;
                              return x >= 1 && x <= 16 ? x : 1; }();
    return v;
}

// ---- the frontier walk every all-hops sampler shares ------------------------------------------------------------------
// A workgroup's frontier: its seeds, the two ping-pong LDS buffers of cap = spw * widest ids each, sel of its batch.
struct Frontier {
    int seed0, nseed;             // this workgroup's seeds: [seed0, seed0 + nseed) of the batch
    int64_t cap;
    int64_t *cur, *nxt;           // hop k - 1 (read) and hop k (written)
    const int32_t *sel;
};

// Hop 0: the workgroup's seeds into f.cur, from ids or from the seed queue (then published as hop 0 of ids).
// hook(t, src) runs once per seed beside its load: t its slot in f.cur, src its index in a per-seed array of the batch
// (with a seed queue: in the queue).  false: no seed for this workgroup (uniform over it), nothing was touched.
template <int THREADS, typename SeedHook>
__device__ __forceinline__ bool frontier_setup(const HopsParams &p, int wg, int64_t *lds, Frontier &f, SeedHook hook)
{
    f.seed0 = wg * p.spw;
    f.nseed = min(p.spw, p.B - f.seed0);
    if (f.nseed <= 0) return false;
    int width = 1, widest = 1;
    for (int k = 1; k <= p.n_hops; ++k) { width *= p.fan[k]; widest = max(widest, width); }
    f.cap = (int64_t)p.spw * widest;
    f.cur = lds;
    f.nxt = lds + f.cap;
    f.sel = p.sel;
    if (p.seed_queue) {
        const int64_t b = (int64_t)((uint64_t)(*p.batch_idx + p.batch_base) % (uint64_t)p.n_batches);
        if (f.sel) f.sel += b * p.sel_stride;
        for (int t = threadIdx.x; t < f.nseed; t += THREADS) {
            const int64_t v = p.seed_queue[b * p.B + f.seed0 + t];
            f.cur[t] = v;
            p.ids[p.off[0] + f.seed0 + t] = v;
            hook(t, b * p.B + f.seed0 + t);
        }
    } else {
        for (int t = threadIdx.x; t < f.nseed; t += THREADS) {
            f.cur[t] = p.ids[p.off[0] + f.seed0 + t];
            hook(t, (int64_t)f.seed0 + t);
        }
    }
    lds_barrier();              // LDS only: the ids stored to HBM are not read back in this launch
    return true;
}

// ... for a sampler whose seeds carry nothing else
template <int THREADS>
__device__ __forceinline__ bool frontier_setup(const HopsParams &p, int wg, int64_t *lds, Frontier &f)
{
    return frontier_setup<THREADS>(p, wg, lds, f, [](int, int64_t) {});
}

// One hop of one workgroup: sample t in [0, count) is child t % n of parent f.cur[t / n]
struct Hop {
    int k;
    uint32_t n;                   // fan[k]
    int64_t parents, count;       // nodes of hop k - 1 and of hop k under this workgroup's seeds (both <= f.cap)
    int64_t local0;               // first sample of this workgroup in hop k of the batch
    uint64_t call;                // Philox call index of hop k
};

// global sample index of sample t: the counter of its Philox word
__device__ __forceinline__ uint64_t hop_sample(const HopsParams &p, const Hop &h, int64_t t)
{
    return p.g0[h.k] + (uint64_t)(h.local0 + t);
}

__device__ __forceinline__ void hop_store(const HopsParams &p, const Frontier &f, const Hop &h, int64_t t, int64_t v)
{
    f.nxt[t] = v;
    p.ids[p.off[h.k] + h.local0 + t] = v;
}

// Hops 1 .. n_hops: body(h) fills f.nxt and ids for hop h (hop_store), reading f.cur; then the barrier and the swap.
template <typename Body>
__device__ __forceinline__ void frontier_walk(const HopsParams &p, Frontier &f, Body body)
{
    const uint64_t ctr = p.call_ctr ? *p.call_ctr : 0ull;
    int64_t per_seed = 1;                            // nodes of hop k per seed
    for (int k = 1; k <= p.n_hops; ++k) {
        Hop h;
        h.k = k;
        h.n = (uint32_t)p.fan[k];
        h.parents = per_seed * f.nseed;
        per_seed *= h.n;
        h.count = per_seed * f.nseed;
        h.call = p.call_base + ctr + (uint64_t)(k - 1);
        h.local0 = (int64_t)f.seed0 * per_seed;
        body(h);
        lds_barrier();
        int64_t *tmp = f.cur; f.cur = f.nxt; f.nxt = tmp;
    }
}

// The uniform sampler: a lane per sample.  wg: which group of p.spw seeds; frontier: 2 * cap ids of LDS.
// DENSE_OK = false compiles the dense-adjacency mode out: k_gather_multi_adam (gsage_gather.hip) runs this body
// beside the HBM-bound gather role under a 72-VGPR cap it already sits on -- two more live values spill.
template <bool DENSE_OK = true>
__device__ __forceinline__ void sample_hops_workgroup(const HopsParams &p, int wg, int64_t *frontier)
{
    Frontier f;
    if (!frontier_setup<256>(p, wg, frontier, f)) return;
    frontier_walk(p, f, [&](const Hop &h) {
        // dense sampler: ONE column permutation per sampler call, shared by every parent of the hop
        // (nn_modules.py:44-48): sample j of a parent reads column keep_k[j], keep_k = sel[kbase ..]
        int64_t kbase = 0;
        if (DENSE_OK)
            for (int q = 1; q < h.k; ++q) kbase += p.fan[q];
        const bool dense = DENSE_OK && p.dense_adj != nullptr;
        for (int64_t t = threadIdx.x; t < h.count; t += 256) {
            uint32_t s;
            if (f.sel)               // parity level 1: the reference's own draws (nn_modules.py:88), replayed
                s = (uint32_t)f.sel[dense ? kbase + (int64_t)((uint32_t)t % h.n) : p.off[h.k] - p.off[1] + h.local0 + t];
            else
                s = philox_below(philox_word(hop_sample(p, h, t), h.call, p.seed_lo, p.seed_hi), p.max_deg);
            const int64_t parent = f.cur[(uint32_t)t / h.n];
            hop_store(p, f, h, t, DENSE_OK
                ? pick_any(p.rowptr, p.col, p.dense_adj, p.dense_ld, p.n_rows, parent, s, p.err_flag)
                : pick_neighbor(p.rowptr, p.col, p.n_rows, parent, s, p.err_flag));
        }
    });
}


// The same sub-trees walked by a WIDE workgroup (THREADS lanes, U samples per lane and trip, CSR only): the role of a
// launch whose workgroups own a whole CU each (k_mean_tail_mfma, gsage_tail_mfma.hip) -- few workgroups, many seeds
// each, so a hop is several trips of dependent (rowptr -> col) loads; the U samples of a trip have their loads issued
// together instead of one chain after the other.  Same Philox words, same ids as sample_hops_workgroup.
template <int THREADS, int U>
__device__ __forceinline__ void sample_hops_wide(const HopsParams &p, int wg, int64_t *frontier)
{
    Frontier f;
    if (!frontier_setup<THREADS>(p, wg, frontier, f)) return;
    frontier_walk(p, f, [&](const Hop &h) {
        for (int64_t t0 = threadIdx.x; t0 < h.count; t0 += (int64_t)THREADS * U) {
            uint32_t s[U];
            int64_t parent[U], beg[U], deg[U], v[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t t = t0 + (int64_t)u * THREADS;
                ok[u] = t < h.count;
                const int64_t tt = ok[u] ? t : h.count - 1;
                if (f.sel)
                    s[u] = (uint32_t)f.sel[p.off[h.k] - p.off[1] + h.local0 + tt];
                else
                    s[u] = philox_below(philox_word(hop_sample(p, h, tt), h.call, p.seed_lo, p.seed_hi), p.max_deg);
                parent[u] = f.cur[(uint32_t)tt / h.n];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool in = (uint64_t)parent[u] < (uint64_t)p.n_rows;
                if (!in && ok[u] && p.err_flag) *p.err_flag = 1;              // the reference raises IndexError here
                const int64_t id = in ? parent[u] : 0;
                beg[u] = p.rowptr[id];
                deg[u] = in ? p.rowptr[id + 1] - beg[u] : 0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint64_t o = (deg[u] <= 0xffffffffLL) ? (uint64_t)(s[u] % (uint32_t)(deg[u] > 0 ? deg[u] : 1))
                                                            : (uint64_t)s[u];
                v[u] = deg[u] > 0 ? (int64_t)p.col[beg[u] + (int64_t)o] : 0;      // (numpy: x % 0 == 0 -> column 0)
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (ok[u]) hop_store(p, f, h, t0 + (int64_t)u * THREADS, v[u]);
        }
    });
}

// [host] The LDS bound of every all-hops entry: per_id bytes for every id of the widest hop of a workgroup's seeds (the
// two ping-pong buffers: 16) plus `extra`, within HOPS_LDS_MAX.  hops_widest: the widest of the first n_hops hops of one
// seed (an entry that refuses under its own name asks before fill_hops, whose refusal names the uniform sampler).
constexpr size_t HOPS_LDS_MAX = 160 * 1024;

inline int64_t hops_widest(const gsage_hops_desc &d, int n_hops)
{
    int64_t width = 1, widest = 1;
    for (int k = 0; k < n_hops; ++k) { width *= d.fan[k]; if (width > widest) widest = width; }
    return widest;
}

inline size_t hops_lds_bytes(int64_t widest, size_t per_id, size_t extra)
{
    return per_id * (size_t)hops_spw() * (size_t)widest + extra;
}

// [host] validate a gsage_hops_desc and turn it into kernel parameters + dynamic LDS bytes
inline int fill_hops(HopsParams &p, size_t &lds, const gsage_hops_desc &d, size_t per_id = 2 * sizeof(int64_t),
                     size_t extra = 0)
{
    GSAGE_REQUIRE(d.ids && ((d.rowptr && d.col) || d.dense_adj), "sample_hops_philox: null pointer");
    GSAGE_REQUIRE(!d.dense_adj || (d.sel && d.dense_ld > 0),
                  "sample_hops: a dense adjacency needs the kept columns in `sel` and its leading dimension");
    GSAGE_REQUIRE(!d.seed_queue || (d.batch_idx && d.n_batches > 0), "sample_hops_philox: bad seed queue");
    GSAGE_REQUIRE(d.n_hops >= 1 && d.n_hops <= 5, "sample_hops_philox: 1..5 hops");
    GSAGE_REQUIRE(d.B >= 0 && d.B < (1LL << 31) && d.max_deg > 0, "sample_hops_philox: bad sizes");
    p.rowptr = d.rowptr; p.col = d.col; p.ids = d.ids; p.call_ctr = d.call_ctr; p.err_flag = d.err_flag;
    p.seed_queue = d.seed_queue; p.batch_idx = d.batch_idx; p.n_batches = d.n_batches;
    p.batch_base = d.batch_base;
    p.sel = d.sel; p.sel_stride = d.sel ? d.sel_stride : 0;
    p.dense_adj = d.dense_adj; p.dense_ld = d.dense_adj ? d.dense_ld : 0;
    GSAGE_REQUIRE(!d.sel || d.sel_stride >= 0, "sample_hops: bad sel stride");
    p.n_rows = d.n_rows; p.call_base = d.call_base; p.n_hops = d.n_hops; p.B = (int32_t)d.B;
    p.max_deg = d.max_deg;
    p.seed_lo = (uint32_t)d.seed; p.seed_hi = (uint32_t)(d.seed >> 32);
    int64_t size = d.B, off = 0, widest = 1, width = 1;
    p.fan[0] = 1;
    for (int k = 0; k <= 5; ++k) {
        if (k >= 1 && k <= d.n_hops) {
            GSAGE_REQUIRE(d.fan[k - 1] > 0, "sample_hops_philox: n_samples must be > 0");
            p.fan[k] = d.fan[k - 1];
            size *= d.fan[k - 1];
            width *= d.fan[k - 1];
            if (width > widest) widest = width;
        } else if (k > d.n_hops) {
            p.fan[k] = 1;
        }
        p.off[k] = off;
        p.g0[k] = d.rank * (uint64_t)size;
        if (k <= d.n_hops) off += size;
    }
    p.spw = hops_spw();
    lds = hops_lds_bytes(widest, per_id, extra);
    GSAGE_REQUIRE(lds <= HOPS_LDS_MAX, "sample_hops_philox: fan-out product too large for the fused kernel");
    return GSAGE_OK;
}

}  // namespace gsage
