// gsage_rank.hip -- the exact rank of a target row among all rows of a table of embeddings (gsage_rank_ip).
//
//   rank(q) = 1 + |{ j allowed for q, j != t : (s(q, j), j) beats (s(q, t), t) }|,  t = target_ids[q],
//   s(q, j) = sum_d Qm[q, d] * E[j, d], "beats" = the total order of gsage_retrieve.hip (score descending, row id
//   ascending).  The rank is a COUNT: no Q x N buffer, no lists, one compare per score against a threshold that
//   never moves.
//
// Launches: 2 for exclude = none and self (scan, finish), 3 for exclude = neighbours (scan, filter, finish).
//
// k_rank_scan, grid (query tiles) x (splits), 4 waves:
//   * the workgroup's 32 queries are staged in LDS exactly as k_topk_scan stages them (rt_stage_queries);
//   * wave 0 computes the TARGET TILE once: lane l gathers row target_ids[q0 + (l & 31)] as its A row, runs
//     rt_tile_scores -- the one accumulator chain every score of this file and of gsage_topk_ip comes from -- and the
//     lane that holds the diagonal element (q, q) hands s(q, t) to the workgroup through LDS; split 0 writes it to
//     out_score.  (ts, t) then sit in registers for the whole scan;
//   * the split's 32-row table tiles are dealt round-robin to the waves; per tile 16 compares and an integer add into a
//     per-lane count.  Rows >= N, row t and -- for exclude != 0 -- row query_ids[q] do not count; a NaN compares false;
//   * the two lanes of a query and the waves are folded, and the split's count goes to the workspace [Q, splits].
// k_rank_filter (exclude = neighbours), one workgroup per query tile, query tile staged the same way: the waves take the
//   tile's queries in turn; the query's CSR row is walked in 32-column pieces, each piece a 32-row A tile gathered by
//   those columns and run through rt_tile_scores against the whole query tile, of which only the query's own column is
//   used: one count per column that is in range, is neither t nor query_ids[q] (the scan left that one out already)
//   and beats the target.  The walk compares adjacent columns: a row that is not strictly ascending raises *err_flag
//   (a duplicate would be subtracted twice).  The count goes to the workspace's last [Q] words.
//   Keeping "self" inside the scan (one more integer compare per score) saves exclude = self the third launch.
// k_rank_finish, one thread per query: rank = 1 + sum of the split counts - the filter's count as int64; 0 when the
//   target is outside [0, N) (score -inf) or its score is NaN.
//
// Counts are integers, so neither the split count nor the order of anything changes the result.
#include "gsage_retrieve_dev.h"

namespace gsage {

struct RankParams {
    const void *table;
    const void *queries;
    const int64_t *target_ids;
    const int64_t *query_ids;
    const int64_t *rowptr;
    const int32_t *col;
    int32_t *ws;                                  // [Q][splits] split counts, then [Q] filter counts
    float *out_score;
    int32_t *err_flag;
    int64_t ldt, ldq, N, Q;
    int64_t tiles_per_split;
    int32_t D, exclude, splits;
    int32_t t_vec, q_vec;                         // rows are 16-byte aligned: whole chunks move as one load
};

template <typename T>
__global__ void __launch_bounds__(256)
k_rank_scan(const RankParams p)
{
    extern __shared__ vec16 rk_smem[];
    __shared__ float s_ts[RT_QT];
    __shared__ int32_t s_cnt[4 * RT_QT];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int W = (int)blockDim.x >> 6;
    const int h = lane >> 5;
    const int ql = lane & 31;
    const rt_shape<T> sh(p.D, p.t_vec);
    vec16 *sQ = rk_smem;
    const int64_t q0 = (int64_t)blockIdx.x * RT_QT;
    rt_stage_queries<T>(sQ, p.queries, p.ldq, q0, p.Q, p.D, p.q_vec, sh.nkt);
    __syncthreads();

    const int64_t q = q0 + ql;
    const bool q_ok = q < p.Q;
    const int64_t t64 = q_ok ? p.target_ids[q] : -1;
    const bool t_ok = t64 >= 0 && t64 < p.N;
    const uint32_t t_u = t_ok ? (uint32_t)t64 : 0xffffffffu;
    uint32_t x_u = 0xffffffffu;                   // the query's own row, when it is excluded
    if (q_ok && p.exclude != RT_EXCLUDE_NONE) {
        const int64_t qid = p.query_ids[q];
        if (qid >= 0 && qid < p.N) x_u = (uint32_t)qid;
    }

    // ---- the target tile, once per workgroup --------------------------------------------------------------------
    if (wave == 0) {
        const T *arow = (const T *)p.table + (t_ok ? t64 : 0) * p.ldt;
        f32x16_t acc;
        rt_tile_scores<T>(arow, sQ, ql, h, p.D, p.t_vec, sh, acc);
        // (q, q): tile row ql sits in register (ql & 3) + 4 * (ql >> 3) of the lane with h == (ql >> 2) & 1
        const int rsel = (ql & 3) + 4 * (ql >> 3);
        float d = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) d = r == rsel ? acc[r] : d;
        if (h == ((ql >> 2) & 1)) {
            if (!t_ok) d = __uint_as_float(RT_NEG_INF);
            s_ts[ql] = d;
            if (blockIdx.y == 0 && q_ok) p.out_score[q] = d;
        }
    }
    __syncthreads();
    const float ts = s_ts[ql];
    const int tidx = (int)t_u;                    // (-1 for a target out of range: its query is unranked anyway)

    const int64_t tiles = (p.N + 31) / 32;
    const int64_t t_begin = (int64_t)blockIdx.y * p.tiles_per_split;
    const int64_t t_end = t_begin + p.tiles_per_split < tiles ? t_begin + p.tiles_per_split : tiles;
    const uint32_t n_u = (uint32_t)p.N;
    int32_t cnt = 0;
    for (int64_t t = t_begin + wave; t < t_end; t += W) {
        const int64_t row0 = t * 32;
        int64_t ar = row0 + ql;
        if (ar >= p.N) ar = p.N - 1;              // a valid address; the row is dropped below
        const T *arow = (const T *)p.table + ar * p.ldt;
        f32x16_t acc;
        rt_tile_scores<T>(arow, sQ, ql, h, p.D, p.t_vec, sh, acc);
        const uint32_t rbase = (uint32_t)row0 + 4u * (uint32_t)h;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t id = rbase + (uint32_t)rt_frag_row(r);
            cnt += (id < n_u && id != t_u && id != x_u && rt_beats(acc[r], (int)id, ts, tidx)) ? 1 : 0;
        }
    }

    // ---- the two lanes of a query, then the waves ---------------------------------------------------------------
    cnt += __shfl_xor(cnt, 32);
    if (h == 0) s_cnt[wave * RT_QT + ql] = cnt;
    __syncthreads();
    if (tid < RT_QT && q0 + tid < p.Q) {
        int32_t c = 0;
        for (int w = 0; w < W; ++w) c += s_cnt[w * RT_QT + tid];
        p.ws[(q0 + tid) * p.splits + blockIdx.y] = c;
    }
}

template <typename T>
__global__ void __launch_bounds__(256)
k_rank_filter(const RankParams p)
{
    extern __shared__ vec16 rk_smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int W = (int)blockDim.x >> 6;
    const int h = lane >> 5;
    const int ql = lane & 31;
    const rt_shape<T> sh(p.D, p.t_vec);
    vec16 *sQ = rk_smem;
    const int64_t q0 = (int64_t)blockIdx.x * RT_QT;
    rt_stage_queries<T>(sQ, p.queries, p.ldq, q0, p.Q, p.D, p.q_vec, sh.nkt);
    __syncthreads();

    int32_t *filt = p.ws + p.Q * p.splits;
    for (int qq = wave; qq < RT_QT; qq += W) {    // qq, and everything read for it, is wave-uniform
        const int64_t q = q0 + qq;
        if (q >= p.Q) break;
        const int64_t t64 = p.target_ids[q];
        const int64_t qid = p.query_ids[q];
        const bool t_ok = t64 >= 0 && t64 < p.N;
        const float ts = p.out_score[q];
        const int tidx = t_ok ? (int)t64 : -1;
        int64_t nb0 = 0, nb1 = 0;
        if (qid >= 0 && qid < p.N) {
            nb0 = p.rowptr[qid];
            nb1 = p.rowptr[qid + 1];
        }
        int32_t cnt = 0;
        for (int64_t e0 = nb0; e0 < nb1; e0 += 32) {
            const int64_t e = e0 + ql;
            int32_t cid = -1;                     // this lane's tile row: the column's id, -1 when it does not count
            if (e < nb1) {
                const int32_t c = p.col[e];
                if (h == 0 && e > nb0 && p.col[e - 1] >= c && p.err_flag) *p.err_flag = 1;
                if (c >= 0 && (int64_t)c < p.N && (int64_t)c != t64 && (int64_t)c != qid) cid = c;
            }
            const T *arow = (const T *)p.table + (int64_t)(cid >= 0 ? cid : 0) * p.ldt;
            f32x16_t acc;
            rt_tile_scores<T>(arow, sQ, ql, h, p.D, p.t_vec, sh, acc);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int id = __shfl(cid, rt_frag_row(r) + 4 * h);
                cnt += (id >= 0 && rt_beats(acc[r], id, ts, tidx)) ? 1 : 0;
            }
        }
        // only the query's own column counts: lanes qq and qq + 32
        const int32_t total = __shfl(cnt, qq) + __shfl(cnt, qq + 32);
        if (lane == 0) filt[q] = total;
    }
}

__global__ void __launch_bounds__(256)
k_rank_finish(const int32_t *ws, int has_filter, const int64_t *target_ids, const float *out_score, int64_t N, int64_t Q,
              int32_t splits, int64_t *out_rank)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    const int64_t t = target_ids[q];
    const float s = out_score[q];
    int64_t rank = 0;
    if (t >= 0 && t < N && s == s) {
        rank = 1;
        for (int i = 0; i < splits; ++i) rank += ws[q * splits + i];
        if (has_filter) rank -= ws[Q * splits + q];
    }
    out_rank[q] = rank;
}

template <typename T>
static int rk_launch(const RankParams &p, size_t lds, hipStream_t stream)
{
    static bool raised = false;
    if (!raised && lds > 64 * 1024) {
        if (hipFuncSetAttribute((const void *)k_rank_scan<T>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)RT_LDS_MAX) != hipSuccess ||
            hipFuncSetAttribute((const void *)k_rank_filter<T>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)RT_LDS_MAX) != hipSuccess) {
            (void)hipGetLastError();
            set_error("rank_ip: cannot raise the dynamic LDS limit");
            return GSAGE_ELAUNCH;
        }
        raised = true;
    }
    const unsigned qtiles = (unsigned)ceil_div(p.Q, RT_QT);
    launch(k_rank_scan<T>, dim3(qtiles, (unsigned)p.splits), dim3(256), lds, stream, p);
    int rc = check_launch("rank_ip scan");
    if (rc != GSAGE_OK || p.exclude != RT_EXCLUDE_NEIGHBOURS) return rc;
    launch(k_rank_filter<T>, dim3(qtiles), dim3(256), lds, stream, p);
    return check_launch("rank_ip filter");
}

static bool rk_limits(int64_t Q, int64_t N, int64_t splits)
{
    return Q >= 1 && N >= 1 && N < (1LL << 31) && splits >= 0 && splits <= RT_SPLITS_MAX;
}

}  // namespace gsage

using namespace gsage;

extern "C" {

int64_t gsage_rank_ip_workspace(int64_t Q, int64_t N, int64_t splits, int64_t *splits_used)
{
    if (!rk_limits(Q, N, splits)) return -1;
    const int64_t s = splits > 0 ? splits : rt_auto_splits(Q, N);
    if (splits_used) *splits_used = s;
    return Q * (s + 1) * (int64_t)sizeof(int32_t);
}

int gsage_rank_ip(const void *table, int table_dtype, int64_t ldt, int64_t N, const void *queries, int query_dtype,
                  int64_t ldq, int64_t Q, int64_t D, const int64_t *target_ids, const int64_t *query_ids,
                  const int64_t *rowptr, const int32_t *col, int exclude, int32_t splits, void *workspace,
                  int64_t workspace_bytes, int64_t *out_rank, float *out_score, int32_t *err_flag, void *stream)
{
    GSAGE_REQUIRE(D >= 1 && D <= RT_D_MAX, "rank_ip: D must be in [1, %d], not %lld", RT_D_MAX, (long long)D);
    GSAGE_REQUIRE(ldt >= D && ldq >= D, "rank_ip: ld (table %lld, queries %lld) must be at least D = %lld",
                  (long long)ldt, (long long)ldq, (long long)D);
    GSAGE_REQUIRE(N >= 1 && N < (1LL << 31), "rank_ip: N must be in [1, 2^31), not %lld", (long long)N);
    GSAGE_REQUIRE(Q >= 1, "rank_ip: Q must be at least 1, not %lld", (long long)Q);
    GSAGE_REQUIRE(splits >= 0 && splits <= RT_SPLITS_MAX, "rank_ip: splits must be in [0, %d] (0 = chosen here), not %d",
                  RT_SPLITS_MAX, (int)splits);
    GSAGE_REQUIRE((table_dtype == GSAGE_F32 || table_dtype == GSAGE_BF16) && query_dtype == table_dtype,
                  "rank_ip: dtype of table and queries must both be fp32 or both bf16 (the compute mode)");
    GSAGE_REQUIRE(exclude >= RT_EXCLUDE_NONE && exclude <= RT_EXCLUDE_NEIGHBOURS, "rank_ip: exclude must be 0, 1 or 2");
    GSAGE_REQUIRE(target_ids, "rank_ip: target_ids is null");
    GSAGE_REQUIRE(exclude == RT_EXCLUDE_NONE || query_ids, "rank_ip: exclude needs query_ids");
    GSAGE_REQUIRE(exclude != RT_EXCLUDE_NEIGHBOURS || (rowptr && col), "rank_ip: exclude = neighbours needs rowptr and col");
    GSAGE_REQUIRE(table && queries && out_rank && out_score, "rank_ip: null pointer");
    const int esz = table_dtype == GSAGE_BF16 ? 2 : 4;
    GSAGE_REQUIRE(((uintptr_t)table % esz) == 0 && ((uintptr_t)queries % esz) == 0, "rank_ip: misaligned table or queries");
    const int64_t s = splits > 0 ? splits : rt_auto_splits(Q, N);
    const int64_t need = Q * (s + 1) * (int64_t)sizeof(int32_t);
    GSAGE_REQUIRE(workspace && ((uintptr_t)workspace % 4) == 0 && workspace_bytes >= need,
                  "rank_ip: workspace of %lld bytes (4-byte aligned) needed, %lld given", (long long)need,
                  (long long)workspace_bytes);
    GSAGE_REQUIRE(ceil_div(Q, RT_QT) < (1LL << 31), "rank_ip: Q too large");
    const size_t lds = rt_query_lds(D, esz);
    GSAGE_REQUIRE(lds <= RT_LDS_MAX, "rank_ip: D = %lld does not fit the LDS", (long long)D);

    RankParams p;
    p.table = table; p.queries = queries; p.target_ids = target_ids; p.query_ids = query_ids; p.rowptr = rowptr;
    p.col = col; p.ws = (int32_t *)workspace; p.out_score = out_score; p.err_flag = err_flag;
    p.ldt = ldt; p.ldq = ldq; p.N = N; p.Q = Q;
    p.tiles_per_split = ceil_div(ceil_div(N, 32), s);
    p.D = (int32_t)D; p.exclude = exclude; p.splits = (int32_t)s;
    p.t_vec = ((uintptr_t)table % 16) == 0 && (ldt * esz) % 16 == 0;
    p.q_vec = ((uintptr_t)queries % 16) == 0 && (ldq * esz) % 16 == 0;
    const int rc = table_dtype == GSAGE_BF16 ? rk_launch<uint16_t>(p, lds, (hipStream_t)stream)
                                             : rk_launch<float>(p, lds, (hipStream_t)stream);
    if (rc != GSAGE_OK) return rc;
    launch(k_rank_finish, dim3((unsigned)ceil_div(Q, 256)), dim3(256), 0, (hipStream_t)stream, (const int32_t *)workspace,
           exclude == RT_EXCLUDE_NEIGHBOURS ? 1 : 0, target_ids, (const float *)out_score, N, Q, (int32_t)s, out_rank);
    return check_launch("rank_ip finish");
}

}  // extern "C"
