// gsage_retrieve_dev.h -- pieces shared by the kernels that score a table of embeddings against a tile of queries
// (gsage_retrieve.hip: top-k; gsage_rank.hip: exact rank): the limits, the total order, the bounded chunk load, the
// query tile's LDS image and THE accumulator chain.  A score's bits are a function of its two rows alone only because
// every launch of both files runs rt_tile_scores() and nothing else.
#pragma once
#include "gsage_common.h"
#include "gsage_mma_dev.h"

namespace gsage {

constexpr int RT_QT = 32;                         // queries per workgroup (the MFMA's 32 columns)
constexpr int RT_D_MAX = 1024;
constexpr int RT_SPLITS_MAX = 1024;               // the top-k merge keeps one head byte per split in LDS
constexpr uint32_t RT_NEG_INF = 0xff800000u;
constexpr size_t RT_LDS_MAX = 160 * 1024;
enum { RT_EXCLUDE_NONE = 0, RT_EXCLUDE_SELF = 1, RT_EXCLUDE_NEIGHBOURS = 2 };

// the total order: (score descending, id ascending).  false for a NaN score on either side.
__device__ __forceinline__ bool rt_beats(float s, int id, float ts, int tid)
{
    return s > ts || (s == ts && id < tid);
}

// 16-byte chunk c of a row of D elements, zero past D; never reads past the row's D columns
template <typename T>
__device__ __forceinline__ vec16 rt_load_chunk(const T *row, int c, int D, int vec_ok)
{
    constexpr int EPC = 16 / (int)sizeof(T);
    const int d0 = c * EPC;
    if (vec_ok && d0 + EPC <= D) return *reinterpret_cast<const vec16 *>(row + d0);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (d0 < D) {
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            if (d0 + e < D) {
                if (sizeof(T) == 2)
                    w[e >> 1] |= (uint32_t)((const uint16_t *)row)[d0 + e] << (16 * (e & 1));
                else
                    w[e & 3] = ((const uint32_t *)row)[d0 + e];
            }
        }
    }
    const vec16 v = {w[0], w[1], w[2], w[3]};
    return v;
}

// how a row of D elements of T is cut: 16-byte chunks, k tiles of CH chunks (the LDS image), MFMA k steps of two
// chunks, and the leading k steps whose two chunks are whole vector loads of the table
template <typename T>
struct rt_shape {
    int chunks, nkt, nkk, nkk_full;
    __device__ __forceinline__ rt_shape(int D, int t_vec)
    {
        constexpr int EPC = 16 / (int)sizeof(T);
        chunks = (D + EPC - 1) / EPC;
        nkt = (chunks + CH - 1) / CH;
        nkk = (chunks + 1) / 2;
        nkk_full = t_vec ? (D / EPC) / 2 : 0;
    }
};

// the workgroup's 32 queries q0 .. q0 + 31 -> LDS as [k tile][32 rows][8 x 16 B] in the lds_slot image, zero past D and Q
template <typename T>
__device__ __forceinline__ void rt_stage_queries(vec16 *sQ, const void *queries, int64_t ldq, int64_t q0, int64_t Q, int D,
                                                 int q_vec, int nkt)
{
    for (int i = threadIdx.x; i < nkt * RT_QT * CH; i += (int)blockDim.x) {
        const int kt = i >> 8, row = (i >> 3) & 31, ch = i & 7;
        const int64_t q = q0 + row;
        vec16 v = {0u, 0u, 0u, 0u};
        if (q < Q) v = rt_load_chunk<T>((const T *)queries + q * ldq, kt * CH + ch, D, q_vec);
        sQ[kt * (RT_QT * CH) + lds_slot(row, ch)] = v;
    }
}

// THE accumulator chain: the 32 table rows whose lane-`ql` row starts at `arow` (A operand, read from global memory:
// lane l takes chunk 2 * kk + (l >> 5) of row l & 31) against the staged query tile (B operand), the whole D through
// one accumulator in the order kk = 0 ..  Result: query on the lane (col = lane & 31), 16 table rows in the lane's
// registers (rt_frag_row(reg) + 4 * (lane >> 5)).
template <typename T>
__device__ __forceinline__ void rt_tile_scores(const T *arow, const vec16 *sQ, int ql, int h, int D, int t_vec,
                                               const rt_shape<T> &sh, f32x16_t &acc)
{
    constexpr int EPC = 16 / (int)sizeof(T);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    int kk = 0;
    for (; kk < sh.nkk_full; ++kk) {
        const vec16 a = *reinterpret_cast<const vec16 *>(arow + (2 * kk + h) * EPC);
        const vec16 b = sQ[(kk >> 2) * (RT_QT * CH) + lds_slot(ql, (kk & 3) * 2 + h)];
        mma_chunk<T>::run(a, b, acc);
    }
    for (; kk < sh.nkk; ++kk) {
        const vec16 a = rt_load_chunk<T>(arow, 2 * kk + h, D, t_vec);
        const vec16 b = sQ[(kk >> 2) * (RT_QT * CH) + lds_slot(ql, (kk & 3) * 2 + h)];
        mma_chunk<T>::run(a, b, acc);
    }
}

// tile row of accumulator register r in the lanes 0..31; the lanes 32..63 hold the rows 4 further
__device__ __forceinline__ constexpr int rt_frag_row(int r) { return (r & 3) + 8 * (r >> 2); }

// bytes of the staged query tile
static inline size_t rt_query_lds(int64_t D, int esz)
{
    return (size_t)ceil_div(ceil_div(D * esz, 16), CH) * RT_QT * CH * 16;
}

static inline int64_t rt_auto_splits(int64_t Q, int64_t N)
{
    // about four workgroups per CU of a 256-CU part, but no split thinner than 16 table tiles (4 per wave)
    const int64_t qtiles = ceil_div(Q, RT_QT), tiles = ceil_div(N, 32);
    int64_t s = ceil_div(1024, qtiles);
    const int64_t cap = tiles / 16 > 1 ? tiles / 16 : 1;
    if (s > cap) s = cap;
    if (s > RT_SPLITS_MAX) s = RT_SPLITS_MAX;
    return s < 1 ? 1 : s;
}

}  // namespace gsage
