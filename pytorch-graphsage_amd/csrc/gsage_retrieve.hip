// gsage_retrieve.hip -- top-k nearest rows by inner product over a table of embeddings (gsage_topk_ip).
//
//   s(q, j) = sum_d Qm[q, d] * E[j, d];  per query the k best ALLOWED rows under the total order
//   (score descending, row id ascending), best first.  No Q x N buffer exists: a score lives in an MFMA
//   accumulator register until it is either dropped by one compare or inserted into a k-entry list in LDS.
//
// k_topk_scan, grid (query tiles) x (splits), 1 / 2 / 4 waves per workgroup (as many as the LDS holds lists for):
//   * the workgroup's 32 queries are staged once in LDS as [k tile][32 rows][8 x 16 B] in the lds_slot image
//     (conflict-free ds_read_b128 of the B operand), zero-filled past D;
//   * the split's 32-row table tiles are dealt round-robin to the waves.  A wave reads its tile's A fragments
//     straight from global memory (lane l: row l & 31, 16-byte chunk 2 * kk + (l >> 5); the four chunks of a
//     128-byte line are consumed by four consecutive k steps, so three of four reads hit the vector L1),
//     and runs the whole D through one accumulator: table rows are the A operand, queries the B operand, so
//     the 32x32 result has THE QUERY ON THE LANE and 16 table rows in the lane's registers
//     (col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5));
//   * every wave keeps, per query, a sorted list of its best k (score, id) pairs in LDS and the list's k-th entry
//     (the threshold) in registers.  The common path is one compare per score against the threshold.  Only a
//     score that beats it takes the insertion path: exclusion test (id compare for "self", a scan of the
//     query's CSR row for "neighbours"), then an insertion from the list's tail.  The two lanes that share a
//     query (lane, lane + 32) insert one after the other and hand the new threshold across by a shuffle;
//   * at the end one thread per query merges the waves' lists into the split's k entries of the workspace
//     [Q, splits, k].
// k_topk_merge, one wave per query: k rounds of (best head of my lists, wave arg-max, advance) over the split
//   lists, written as ids int64 / scores fp32; an unused slot is id -1, score -inf.
//
// Grid independence: a score is ONE accumulator chain over kk = 0 .. in a fixed order, whatever tile, wave or
// split its row falls in, so its bits do not depend on the grid; every list and both merges keep the exact best k of
// what they saw under a TOTAL order, and the best k of a union is the best k of the parts' best k.  Hence the
// result is bit-identical for every split count (tests/test_gpu_retrieve.py).  NaN compares false both ways and
// never enters a list.
#include "gsage_retrieve_dev.h"

namespace gsage {

constexpr int RT_K_MAX = 128;
constexpr int RT_SENT = 0x7fffffff;               // id of an empty slot inside the kernels (score -inf)

struct RetrieveParams {
    const void *table;
    const void *queries;
    const int64_t *query_ids;
    const int64_t *rowptr;
    const int32_t *col;
    uint2 *ws;                                    // [Q][splits][k] (score bits, id)
    int64_t ldt, ldq, N, Q;
    int64_t tiles_per_split;
    int32_t D, k, exclude, splits;
    int32_t t_vec, q_vec;                         // rows are 16-byte aligned: whole chunks move as one load
};

template <typename T>
__global__ void __launch_bounds__(256)
k_topk_scan(const RetrieveParams p)
{
    extern __shared__ vec16 rt_smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int W = (int)blockDim.x >> 6;
    const int h = lane >> 5;
    const int ql = lane & 31;
    const int k = p.k;
    const rt_shape<T> sh(p.D, p.t_vec);
    vec16 *sQ = rt_smem;
    uint2 *lists = reinterpret_cast<uint2 *>(rt_smem + (size_t)sh.nkt * RT_QT * CH);
    const int64_t q0 = (int64_t)blockIdx.x * RT_QT;

    // ---- the query tile, once ---------------------------------------------------------------------
    rt_stage_queries<T>(sQ, p.queries, p.ldq, q0, p.Q, p.D, p.q_vec, sh.nkt);
    // this wave's lists: entry `pos` of query `ql` at my[pos * 32 + ql]
    uint2 *my = lists + (size_t)wave * RT_QT * k;
    for (int i = lane; i < RT_QT * k; i += 64) my[i] = make_uint2(RT_NEG_INF, (uint32_t)RT_SENT);
    __syncthreads();

    const int64_t q = q0 + ql;
    const bool q_ok = q < p.Q;
    int64_t qid = -1, nb0 = 0, nb1 = 0;
    if (q_ok && p.exclude != RT_EXCLUDE_NONE) {
        qid = p.query_ids[q];
        if (p.exclude == RT_EXCLUDE_NEIGHBOURS && qid >= 0 && qid < p.N) {
            nb0 = p.rowptr[qid];
            nb1 = p.rowptr[qid + 1];
        }
    }
    float ts = __uint_as_float(RT_NEG_INF);       // threshold = the list's k-th entry (an empty slot until it fills)
    int tidx = RT_SENT;
    int cnt = 0;                                  // live entries of the list; the same in both lanes of a query

    const int64_t tiles = (p.N + 31) / 32;
    const int64_t t_begin = (int64_t)blockIdx.y * p.tiles_per_split;
    const int64_t t_end = t_begin + p.tiles_per_split < tiles ? t_begin + p.tiles_per_split : tiles;
    const uint32_t n_u = (uint32_t)p.N;
    for (int64_t t = t_begin + wave; t < t_end; t += W) {
        const int64_t row0 = t * 32;
        int64_t ar = row0 + ql;
        if (ar >= p.N) ar = p.N - 1;              // a valid address; the row is dropped below
        const T *arow = (const T *)p.table + ar * p.ldt;
        f32x16_t acc;
        rt_tile_scores<T>(arow, sQ, ql, h, p.D, p.t_vec, sh, acc);

        // ---- selection: one compare per score ----------------------------------------------------------
        const uint32_t rbase = (uint32_t)row0 + 4u * (uint32_t)h;
        uint32_t mask = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t id = rbase + (uint32_t)rt_frag_row(r);
            if (id < n_u && rt_beats(acc[r], (int)id, ts, tidx)) mask |= 1u << r;
        }
        if (!q_ok) mask = 0;
        if (__any(mask != 0)) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                if (h == half && mask != 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        if (!((mask >> r) & 1u)) continue;
                        const int id = (int)(rbase + (uint32_t)rt_frag_row(r));
                        const float s = acc[r];
                        if (!rt_beats(s, id, ts, tidx)) continue;       // the threshold moved meanwhile
                        bool allowed = true;
                        if (p.exclude != RT_EXCLUDE_NONE) {
                            allowed = (int64_t)id != qid;
                            for (int64_t e = nb0; allowed && e < nb1; ++e) allowed = p.col[e] != id;
                        }
                        if (!allowed) continue;
                        int pos = cnt < k ? cnt : k - 1;
                        while (pos > 0) {
                            const uint2 e = my[(pos - 1) * 32 + ql];
                            if (!rt_beats(s, id, __uint_as_float(e.x), (int)e.y)) break;
                            my[pos * 32 + ql] = e;
                            --pos;
                        }
                        my[pos * 32 + ql] = make_uint2(__float_as_uint(s), (uint32_t)id);
                        if (cnt < k) ++cnt;
                        if (cnt == k) {
                            const uint2 e = my[(k - 1) * 32 + ql];
                            ts = __uint_as_float(e.x);
                            tidx = (int)e.y;
                        }
                    }
                }
                // the other lane of the query sees this half's list and threshold
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                const int src = ql + 32 * half;
                ts = __shfl(ts, src);
                tidx = __shfl(tidx, src);
                cnt = __shfl(cnt, src);
            }
        }
    }

    // ---- the waves' lists -> the split's k entries ------------------------------------------------------
    __syncthreads();
    if (tid < RT_QT && q0 + tid < p.Q) {
        uint2 *out = p.ws + ((q0 + tid) * p.splits + blockIdx.y) * (int64_t)k;
        int hp[4] = {0, 0, 0, 0};
        for (int j = 0; j < k; ++j) {
            uint2 best = make_uint2(RT_NEG_INF, (uint32_t)RT_SENT);
            int bw = -1;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                if (w < W && hp[w] < k) {
                    const uint2 e = lists[(size_t)w * RT_QT * k + hp[w] * 32 + tid];
                    if (bw < 0 || rt_beats(__uint_as_float(e.x), (int)e.y, __uint_as_float(best.x), (int)best.y)) {
                        best = e;
                        bw = w;
                    }
                }
            }
            out[j] = best;
#pragma unroll
            for (int w = 0; w < 4; ++w) hp[w] += (w == bw) ? 1 : 0;
        }
    }
}

// one wave per query: lane l owns the split lists l, l + 64, ...; k rounds of arg-max over the lists' heads
__global__ void __launch_bounds__(256)
k_topk_merge(const uint2 *ws, int64_t Q, int32_t splits, int32_t k, int64_t *out_ids, float *out_scores)
{
    __shared__ uint8_t heads[4][RT_SPLITS_MAX];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * 4 + wave;
    if (q >= Q) return;                                         // wave-uniform
    uint8_t *head = heads[wave];
    for (int l = lane; l < splits; l += 64) head[l] = 0;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const uint2 *base = ws + q * splits * (int64_t)k;
    for (int j = 0; j < k; ++j) {
        float s = __uint_as_float(RT_NEG_INF);
        int id = RT_SENT, li = RT_SENT;
        for (int l = lane; l < splits; l += 64) {
            const int pos = head[l];
            if (pos >= k) continue;
            const uint2 e = base[(int64_t)l * k + pos];
            if (li == RT_SENT || rt_beats(__uint_as_float(e.x), (int)e.y, s, id)) {
                s = __uint_as_float(e.x);
                id = (int)e.y;
                li = l;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float os = __shfl_xor(s, off);
            const int oid = __shfl_xor(id, off);
            const int oli = __shfl_xor(li, off);
            if (rt_beats(os, oid, s, id) || (os == s && oid == id && oli < li)) {
                s = os;
                id = oid;
                li = oli;
            }
        }
        if (lane == 0) {
            out_ids[q * k + j] = id == RT_SENT ? (int64_t)-1 : (int64_t)id;
            out_scores[q * k + j] = s;
        }
        if (li < splits && (li & 63) == lane) head[li] = (uint8_t)(head[li] + 1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

static size_t rt_scan_lds(int64_t D, int esz, int32_t k, int waves)
{
    return rt_query_lds(D, esz) + (size_t)waves * RT_QT * k * sizeof(uint2);
}

template <typename T>
static int rt_launch_scan(const RetrieveParams &p, int waves, size_t lds, hipStream_t stream)
{
    static bool raised = false;
    if (!raised && lds > 64 * 1024) {
        if (hipFuncSetAttribute((const void *)k_topk_scan<T>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)RT_LDS_MAX) != hipSuccess) {
            (void)hipGetLastError();
            set_error("topk_ip: cannot raise the dynamic LDS limit");
            return GSAGE_ELAUNCH;
        }
        raised = true;
    }
    launch(k_topk_scan<T>, dim3((unsigned)ceil_div(p.Q, RT_QT), (unsigned)p.splits), dim3(64 * waves), lds, stream, p);
    return check_launch("topk_ip scan");
}

}  // namespace gsage

using namespace gsage;

extern "C" {

int64_t gsage_topk_ip_workspace(int64_t Q, int64_t N, int64_t k, int64_t splits, int64_t *splits_used)
{
    if (Q < 1 || N < 1 || N >= (1LL << 31) || k < 1 || k > RT_K_MAX || splits < 0 || splits > RT_SPLITS_MAX) return -1;
    const int64_t s = splits > 0 ? splits : rt_auto_splits(Q, N);
    if (splits_used) *splits_used = s;
    return Q * s * k * (int64_t)sizeof(uint2);
}

int gsage_topk_ip(const void *table, int table_dtype, int64_t ldt, int64_t N, const void *queries, int query_dtype,
                  int64_t ldq, int64_t Q, int64_t D, const int64_t *query_ids, const int64_t *rowptr,
                  const int32_t *col, int exclude, int32_t k, int32_t splits, void *workspace, int64_t workspace_bytes,
                  int64_t *out_ids, float *out_scores, void *stream)
{
    GSAGE_REQUIRE(k >= 1 && k <= RT_K_MAX, "topk_ip: k must be in [1, %d], not %d", RT_K_MAX, (int)k);
    GSAGE_REQUIRE(D >= 1 && D <= RT_D_MAX, "topk_ip: D must be in [1, %d], not %lld", RT_D_MAX, (long long)D);
    GSAGE_REQUIRE(ldt >= D && ldq >= D, "topk_ip: ld (table %lld, queries %lld) must be at least D = %lld",
                  (long long)ldt, (long long)ldq, (long long)D);
    GSAGE_REQUIRE(N >= 1 && N < (1LL << 31), "topk_ip: N must be in [1, 2^31), not %lld", (long long)N);
    GSAGE_REQUIRE(Q >= 1, "topk_ip: Q must be at least 1, not %lld", (long long)Q);
    GSAGE_REQUIRE(splits >= 0 && splits <= RT_SPLITS_MAX, "topk_ip: splits must be in [0, %d] (0 = chosen here), not %d",
                  RT_SPLITS_MAX, (int)splits);
    GSAGE_REQUIRE((table_dtype == GSAGE_F32 || table_dtype == GSAGE_BF16) && query_dtype == table_dtype,
                  "topk_ip: dtype of table and queries must both be fp32 or both bf16 (the compute mode)");
    GSAGE_REQUIRE(exclude >= RT_EXCLUDE_NONE && exclude <= RT_EXCLUDE_NEIGHBOURS, "topk_ip: exclude must be 0, 1 or 2");
    GSAGE_REQUIRE(exclude == RT_EXCLUDE_NONE || query_ids, "topk_ip: exclude needs query_ids");
    GSAGE_REQUIRE(exclude != RT_EXCLUDE_NEIGHBOURS || (rowptr && col), "topk_ip: exclude = neighbours needs rowptr and col");
    GSAGE_REQUIRE(table && queries && out_ids && out_scores, "topk_ip: null pointer");
    const int esz = table_dtype == GSAGE_BF16 ? 2 : 4;
    GSAGE_REQUIRE(((uintptr_t)table % esz) == 0 && ((uintptr_t)queries % esz) == 0, "topk_ip: misaligned table or queries");
    const int64_t s = splits > 0 ? splits : rt_auto_splits(Q, N);
    const int64_t need = Q * s * k * (int64_t)sizeof(uint2);
    GSAGE_REQUIRE(workspace && ((uintptr_t)workspace % 8) == 0 && workspace_bytes >= need,
                  "topk_ip: workspace of %lld bytes (8-byte aligned) needed, %lld given", (long long)need,
                  (long long)workspace_bytes);
    GSAGE_REQUIRE(ceil_div(Q, RT_QT) < (1LL << 31), "topk_ip: Q too large");

    int waves = 4;
    while (waves > 1 && rt_scan_lds(D, esz, k, waves) > RT_LDS_MAX) waves >>= 1;
    const size_t lds = rt_scan_lds(D, esz, k, waves);
    GSAGE_REQUIRE(lds <= RT_LDS_MAX, "topk_ip: D = %lld and k = %d do not fit the LDS", (long long)D, (int)k);

    RetrieveParams p;
    p.table = table; p.queries = queries; p.query_ids = query_ids; p.rowptr = rowptr; p.col = col;
    p.ws = (uint2 *)workspace; p.ldt = ldt; p.ldq = ldq; p.N = N; p.Q = Q;
    p.tiles_per_split = ceil_div(ceil_div(N, 32), s);
    p.D = (int32_t)D; p.k = k; p.exclude = exclude; p.splits = (int32_t)s;
    p.t_vec = ((uintptr_t)table % 16) == 0 && (ldt * esz) % 16 == 0;
    p.q_vec = ((uintptr_t)queries % 16) == 0 && (ldq * esz) % 16 == 0;
    const int rc = table_dtype == GSAGE_BF16 ? rt_launch_scan<uint16_t>(p, waves, lds, (hipStream_t)stream)
                                             : rt_launch_scan<float>(p, waves, lds, (hipStream_t)stream);
    if (rc != GSAGE_OK) return rc;
    launch(k_topk_merge, dim3((unsigned)ceil_div(Q, 4)), dim3(256), 0, (hipStream_t)stream, (const uint2 *)workspace, Q,
           (int32_t)s, k, out_ids, out_scores);
    return check_launch("topk_ip merge");
}

}  // extern "C"
