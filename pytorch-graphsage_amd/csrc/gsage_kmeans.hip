// gsage_kmeans.hip -- Lloyd's k-means over selected rows of a table of embeddings: one assignment-and-accumulate pass
// (gsage_kmeans_pass) and the centroid update (gsage_kmeans_update), the two launches of an iteration of infer.kmeans.
//
//   s[i, c] = sum_d X[ids[i], d] * C~[c, d] + bias[c]   for c < k_live     (C~: the fp32 centroids as the compute mode sees them)
//   a[i]    = the c < k_live with the largest s[i, c]; among equal scores the SMALLEST c
//   d2[i]   = max(0, |x_i|^2 - 2 s[i, a[i]])                               (bias[c] = -1/2 |C~[c]|^2 makes it the squared distance)
//   sums[c] = sum over {i : a[i] == c} of X[ids[i], :],   counts[c] = |{i : a[i] == c}|
//   inertia = sum_i d2[i],   changed = |{i : labels_in[i] != a[i]}|
//
// No n x K buffer exists: scores, the arg-max and its one-hot live in MFMA accumulator registers.
//
// k_kmeans_pass<T, CT> is k_probe_pass (gsage_probe.hip) with another middle step: grid (row ranges S) x (D slabs of 256
// columns; 128 for CT = 4 in fp32), 4 waves; CT = 1, 2 or 4 cluster tiles of 32:
//   * C~ (zero past K and D) is staged once per workgroup in LDS, per cluster tile in the lds_slot image; where it does
//     not fit beside the row tile (w_lds == 0) its fragments are read from global memory instead (the same bits).
//   * a workgroup walks a contiguous range of 32-row tiles.  Per tile the gathered rows land in LDS ONCE (zero past D and
//     past n); both products and |x_i|^2 read them from there.  |x_i|^2: eight threads per row, thread q adding the squares
//     of the 16-byte chunks q, q + 8, .. in ascending order (fmaf), then a butterfly over the eight.
//   * wave w owns cluster tile w % CT.  First product, over the whole D in ONE accumulator chain (k step 0, 1, ..): THE
//     CLUSTER ON THE LANE, 16 rows in the lane's registers.  A score's bits depend on its row and its centroid alone.
//   * arg-max: per register a butterfly of (score, index) over the 32 lanes of the half -- larger score, then smaller
//     index; the CT tiles' pairs meet in LDS (one barrier) and every wave folds them in tile order, a later tile winning
//     only with a STRICTLY larger score: the tie rule.
//   * the one-hot of the arg-max replaces the scores and is the B operand of the second product sums^T[d][c] +=
//     sum_i X[i][d] G[i][c] with no lane movement.  bf16: registers 8 s .. 8 s + 7 become k step s as ONE bf16 each (0 and
//     1 are exact: no hi + lo pair); X^T by the probe's transposed LDS reads.  fp32: mfma_f32_32x32x2f32 per register.
//   * the accumulators stay in registers across the workgroup's whole row range and are written once, unscaled, as row
//     blockIdx.x of partial [S][K D + K + 2] = [sums | counts | inertia | changed].  Slab 0 writes counts, inertia,
//     changed, labels and dist.  partial == NULL: labels / dist only, no second product.
// k_kmeans_update: one workgroup per cluster sums the S partial rows in buffer order, divides, normalises (spherical) and
// refreshes the bias; workgroup 0 also writes the iteration's history slot and ticks the index.
//
// No atomics: for fixed (n, K, D, splits) every sum has one order, so the result is bit-identical call to call; labels do
// not depend on the grid at all.
#include "gsage_retrieve_dev.h"

namespace gsage {

constexpr int KM_K_MAX = 128;
constexpr int KM_SPLITS_MAX = 1024;
constexpr int KM_AUTO_SPLITS = 256;               // one persistent workgroup per CU
constexpr int KM_WAVES = 4;
constexpr int64_t KM_RANGE_ROWS_MAX = 1LL << 24;  // counts and `changed` of a workgroup travel as fp32 integers
// columns of the sums a workgroup accumulates (grid.y slabs beyond): the probe's rule
constexpr int km_slab(int ct, int esz) { return ct == 4 && esz == 4 ? 128 : 256; }
constexpr size_t KM_LDS_DYN_MAX = RT_LDS_MAX - 2048;     // beside the static exchange buffers
constexpr int KM_UPD_THREADS = 256;

struct KMeansParams {
    const void *table;
    const int64_t *ids;
    const float *Cn;
    const float *bias;
    const int32_t *labels_in;
    float *partial;
    int32_t *labels_out;
    float *dist_out;
    int64_t ldx, N, n;
    int64_t tiles_per_split;
    int32_t K, D, k_live, x_vec, w_lds;
};

typedef short km_s16x4 __attribute__((ext_vector_type(4)));

// 16-byte chunk ch of centroid c of the fp32 centroids Cn [K][D] as the compute mode sees it; zero past K and D
template <typename T>
__device__ __forceinline__ vec16 km_c_chunk(const float *Cn, int c, int ch, int K, int D)
{
    constexpr int EPC = 16 / (int)sizeof(T);
    const int d0 = ch * EPC;
    float f[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) f[e] = (c < K && d0 + e < D) ? Cn[(int64_t)c * D + d0 + e] : 0.f;
    vec16 v;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = pack_bf16x2(f[2 * e], f[2 * e + 1]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = __float_as_uint(f[e]);
    }
    return v;
}

// sum of the squares of a chunk's elements, in element order, on top of `acc`
template <typename T>
__device__ __forceinline__ float km_chunk_sq(const vec16 &v, float acc)
{
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if constexpr (sizeof(T) == 2) {
            const float lo = __uint_as_float(v[e] << 16), hi = __uint_as_float(v[e] & 0xffff0000u);
            acc = fmaf(lo, lo, acc);
            acc = fmaf(hi, hi, acc);
        } else {
            const float x = __uint_as_float(v[e]);
            acc = fmaf(x, x, acc);
        }
    }
    return acc;
}

template <typename T, int CT>
__global__ void __launch_bounds__(64 * KM_WAVES)
k_kmeans_pass(const KMeansParams p)
{
    extern __shared__ vec16 km_smem[];
    constexpr int WPC = KM_WAVES / CT;                                       // waves that share a cluster tile
    constexpr int NDT = km_slab(CT, (int)sizeof(T)) / 32 / WPC;              // d tiles of a wave
    __shared__ float sS[KM_WAVES][32];                                       // per wave and row: the tile's best score
    __shared__ int sI[KM_WAVES][32];                                         //                   and its cluster
    __shared__ float sN[32];                                                 // |x_i|^2 of the tile's rows
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ct = wave % CT, dg = wave / CT;
    const int h = lane >> 5;
    const int ql = lane & 31;
    const int K = p.K, D = p.D;
    const rt_shape<T> sh(D, p.x_vec);
    const int nkt = sh.nkt;
    vec16 *sX = km_smem;
    vec16 *sW = sX + (size_t)nkt * RT_QT * CH;
    const bool accumulate = p.partial != nullptr;                            // uniform over the launch

    // ---- C~, once ------------------------------------------------------------------------------------------------
    if (p.w_lds) {
        for (int i = tid; i < CT * nkt * RT_QT * CH; i += 64 * KM_WAVES) {
            const int tile = i >> 8, row = (i >> 3) & 31, ch = i & 7;        // tile = cluster tile * nkt + k tile
            const int wt = tile / nkt, kt = tile - wt * nkt;
            sW[tile * (RT_QT * CH) + lds_slot(row, ch)] = km_c_chunk<T>(p.Cn, wt * 32 + row, kt * CH + ch, K, D);
        }
    }
    const int cls = ct * 32 + ql;                                            // this lane's cluster
    const bool cls_ok = cls < K;
    const bool cls_live = cls < p.k_live;
    const float bc = cls_live ? p.bias[cls] : 0.f;

    f32x16_t acc[NDT];
#pragma unroll
    for (int j = 0; j < NDT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    float cntacc = 0.f, inacc = 0.f, chacc = 0.f;

    const int dt0 = ((int)blockIdx.y * WPC + dg) * NDT;                      // this wave's first d tile
    // byte offsets of this lane's X^T reads in the row tile's image (gsage_probe.hip has the derivation)
    uint32_t xt_off[2][2][sizeof(T) == 2 ? 2 : 8];
    if constexpr (sizeof(T) == 2) {
        const int q = (lane >> 2) & 3, pp = lane & 3, cg = ((lane >> 4) & 1) * 16 + 4 * pp;
#pragma unroll
        for (int par = 0; par < 2; ++par)
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const int col = (dt0 + par) * 32 + cg, chunk = col >> 3, row = 16 * s + 8 * jj + 4 * h + q;
                    xt_off[par][s][jj] = (uint32_t)(((chunk >> 3) * (RT_QT * CH) + lds_slot(row, chunk & 7)) * 16 + (col & 7) * 2);
                }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int col = dt0 * 32 + ql, chunk = col >> 2, row = rt_frag_row(r) + 4 * h;
            xt_off[0][r >> 3][r & 7] = (uint32_t)(((chunk >> 3) * (RT_QT * CH) + lds_slot(row, chunk & 7)) * 16 + (col & 3) * 4);
        }
    }
    const bool scribe = blockIdx.y == 0 && wave == 0 && ql == 0;             // writes labels and dist, counts inertia
    const int64_t tiles = (p.n + 31) / 32;
    const int64_t t_begin = (int64_t)blockIdx.x * p.tiles_per_split;
    const int64_t t_end = t_begin + p.tiles_per_split < tiles ? t_begin + p.tiles_per_split : tiles;
    for (int64_t t = t_begin; t < t_end; ++t) {
        const int64_t row0 = t * 32;
        if (t != t_begin) __syncthreads();                                   // everybody is done with the last tile
        // ---- the tile's rows -> LDS -----------------------------------------------------------------------------
        for (int i = tid; i < nkt * RT_QT * CH; i += 64 * KM_WAVES) {
            const int row = i / (nkt * CH), c = i - row * (nkt * CH);        // consecutive threads: one row's chunks
            vec16 v = {0u, 0u, 0u, 0u};
            if (row0 + row < p.n && c < sh.chunks) {
                const int64_t id = p.ids[row0 + row];
                if ((uint64_t)id < (uint64_t)p.N) v = rt_load_chunk<T>((const T *)p.table + id * p.ldx, c, D, p.x_vec);
            }
            sX[(c >> 3) * (RT_QT * CH) + lds_slot(row, c & 7)] = v;
        }
        __syncthreads();

        // ---- |x_i|^2: eight threads per row ---------------------------------------------------------------------------
        {
            const int row = tid >> 3, q = tid & 7;
            float s = 0.f;
            for (int kt = 0; kt < nkt; ++kt) s = km_chunk_sq<T>(sX[kt * (RT_QT * CH) + lds_slot(row, q)], s);
#pragma unroll
            for (int off = 4; off > 0; off >>= 1) s += __shfl_xor(s, off);
            if (q == 0) sN[row] = s;
        }

        // ---- scores of this wave's cluster tile: cluster on the lane, rows in the registers ---------------------------
        f32x16_t z;
#pragma unroll
        for (int r = 0; r < 16; ++r) z[r] = 0.f;
        if (p.w_lds) {
            const vec16 *sWt = sW + ct * nkt * (RT_QT * CH);
            for (int kk = 0; kk < sh.nkk; ++kk) {
                const int slot = (kk >> 2) * (RT_QT * CH) + lds_slot(ql, (kk & 3) * 2 + h);
                mma_chunk<T>::run(sX[slot], sWt[slot], z);
            }
        } else {
            for (int kk = 0; kk < sh.nkk; ++kk) {
                const vec16 a = sX[(kk >> 2) * (RT_QT * CH) + lds_slot(ql, (kk & 3) * 2 + h)];
                mma_chunk<T>::run(a, km_c_chunk<T>(p.Cn, cls, 2 * kk + h, K, D), z);
            }
        }

        // ---- the tile's arg-max per row -------------------------------------------------------------------------------
        // (hh: the lane half, opaque to the compiler, as in k_probe_pass)
        int hh = h;
        asm volatile("" : "+v"(hh));
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = rt_frag_row(r) + 4 * hh;
            float bs = cls_live ? z[r] + bc : -INFINITY;
            int bi = cls;
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) {
                const float os = __shfl_xor(bs, off);
                const int oi = __shfl_xor(bi, off);
                if (os > bs || (os == bs && oi < bi)) { bs = os; bi = oi; }
            }
            if (ql == 0) { sS[wave][row] = bs; sI[wave][row] = bi; }
            __builtin_amdgcn_sched_barrier(0);                   // one row at a time
        }
        __syncthreads();

        // ---- fold the CT tiles in order; the one-hot in place of the scores -------------------------------------------
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = rt_frag_row(r) + 4 * hh;
            float bs = sS[0][row];
            int bi = sI[0][row];
#pragma unroll
            for (int w = 1; w < CT; ++w) {
                const float os = sS[w][row];
                if (os > bs) { bs = os; bi = sI[w][row]; }
            }
            const bool live = row0 + row < p.n;
            z[r] = live && bi == cls ? 1.f : 0.f;
            if (scribe && live) {
                const float d2 = fmaxf(0.f, sN[row] - 2.f * bs);
                inacc += d2;
                if (p.labels_in) chacc += p.labels_in[row0 + row] != bi ? 1.f : 0.f;
                if (p.labels_out) p.labels_out[row0 + row] = bi;
                if (p.dist_out) p.dist_out[row0 + row] = d2;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (!accumulate) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) cntacc += z[r];

        // ---- sums^T tiles of this wave += X^T G ------------------------------------------------------------------------
        if constexpr (sizeof(T) == 2) {
            vec16 g[2];
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int e = 0; e < 4; ++e)                                  // 1.0 as bf16 is 0x3f80
                    g[s][e] = (z[8 * s + 2 * e] != 0.f ? 0x3f80u : 0u) | (z[8 * s + 2 * e + 1] != 0.f ? 0x3f800000u : 0u);
#pragma unroll
            for (int j = 0; j < NDT; ++j) {
                if ((dt0 + j) * 32 < D) {                                    // wave-uniform: EXEC stays whole
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        km_s16x4 x[2];
#pragma unroll
                        for (int jj = 0; jj < 2; ++jj)
                            x[jj] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) km_s16x4 *)(
                                (reinterpret_cast<const char *>(sX) + xt_off[j & 1][s][jj]) + (j >> 1) * (RT_QT * CH * 16)));
                        vec16 a;
                        a[0] = __builtin_bit_cast(uint2, x[0]).x; a[1] = __builtin_bit_cast(uint2, x[0]).y;
                        a[2] = __builtin_bit_cast(uint2, x[1]).x; a[3] = __builtin_bit_cast(uint2, x[1]).y;
                        mma_chunk<T>::run(a, g[s], acc[j]);
                    }
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < NDT; ++j) {
                if ((dt0 + j) * 32 < D) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const char *src = reinterpret_cast<const char *>(sX) + xt_off[0][r >> 3][r & 7];
                        const float a = *reinterpret_cast<const float *>(src + j * (RT_QT * CH * 16));
                        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, z[r], acc[j], 0, 0, 0);
                    }
                }
            }
        }
    }
    if (!accumulate) return;

    // ---- the workgroup's partial row [sums | counts | inertia | changed], unscaled ------------------------------------
    float *out = p.partial + (int64_t)blockIdx.x * ((int64_t)K * D + K + 2);
#pragma unroll
    for (int j = 0; j < NDT; ++j) {
        const int dbase = (dt0 + j) * 32 + 4 * h;
        float *o = out + (int64_t)cls * D + dbase;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (dbase + rt_frag_row(r) < D && cls_ok) o[rt_frag_row(r)] = acc[j][r];
    }
    // counts: by the first wave of each cluster tile, in slab 0; inertia and changed: the two scribe lanes of wave 0
    const float cnt = cntacc + __shfl_xor(cntacc, 32);
    const float inertia = inacc + __shfl_xor(inacc, 32);
    const float changed = chacc + __shfl_xor(chacc, 32);
    if (blockIdx.y == 0 && dg == 0 && h == 0 && cls_ok) out[(int64_t)K * D + cls] = cnt;
    if (blockIdx.y == 0 && wave == 0 && lane == 0) {
        out[(int64_t)K * D + K] = inertia;
        out[(int64_t)K * D + K + 1] = changed;
    }
}

// sum of `v` over the workgroup's KM_UPD_THREADS threads, the same value in all of them (exact: any order)
__device__ __forceinline__ long long km_block_sum_ll(long long v, long long *s)
{
    __syncthreads();
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = KM_UPD_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
        __syncthreads();
    }
    return s[0];
}

// the same by halving in fp32: thread t += thread t + 128, then + 64, .. + 1 -- one fixed order
__device__ __forceinline__ float km_block_sum_f(float v, float *s)
{
    __syncthreads();
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = KM_UPD_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
        __syncthreads();
    }
    return s[0];
}

// workgroup c: centroid c and its bias; workgroup 0 also: the history slot *index and the tick.  S == 0: bias only.
__global__ void __launch_bounds__(KM_UPD_THREADS)
k_kmeans_update(const float *partial, int32_t S, int32_t K, int32_t D, int32_t as_bf16, int32_t spherical, float *Cn,
                float *bias, float *inertia_hist, int64_t *changed_hist, int32_t *empty_hist, int64_t *index,
                int64_t capacity)
{
    __shared__ long long sLL[KM_UPD_THREADS];
    __shared__ float sF[KM_UPD_THREADS];
    __shared__ float sSlot[KM_SPLITS_MAX];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int64_t stride = (int64_t)K * D + K + 2;
    const float *counts = partial + (int64_t)K * D;

    long long mine = 0;
    for (int s = tid; s < S; s += KM_UPD_THREADS) mine += (long long)counts[(int64_t)s * stride + c];
    const long long count = km_block_sum_ll(mine, sLL);

    // this thread's columns d = tid, tid + 256, ..: the sum over the S partial rows in buffer order, divided
    float v[RT_D_MAX / KM_UPD_THREADS];
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < RT_D_MAX / KM_UPD_THREADS; ++i) {
        const int d = tid + i * KM_UPD_THREADS;
        v[i] = 0.f;
        if (d < D) {
            if (count > 0) {
                float sum = 0.f;
                for (int s = 0; s < S; ++s) sum += partial[(int64_t)s * stride + (int64_t)c * D + d];
                v[i] = sum / (float)count;
            } else {
                v[i] = Cn[(int64_t)c * D + d];
            }
        }
        sq = fmaf(v[i], v[i], sq);
    }
    if (spherical && count > 0) {
        const float n2 = km_block_sum_f(sq, sF);
        const float scale = n2 > 0.f ? 1.f / sqrtf(n2) : 1.f;
#pragma unroll
        for (int i = 0; i < RT_D_MAX / KM_UPD_THREADS; ++i) v[i] *= scale;
    }
    float sq2 = 0.f;
#pragma unroll
    for (int i = 0; i < RT_D_MAX / KM_UPD_THREADS; ++i) {
        const int d = tid + i * KM_UPD_THREADS;
        if (d < D && count > 0) Cn[(int64_t)c * D + d] = v[i];
        const float r = as_bf16 ? bf16_to_f32(f32_to_bf16(v[i])) : v[i];
        sq2 = fmaf(r, r, sq2);
    }
    const float n2 = km_block_sum_f(sq2, sF);
    if (tid == 0) bias[c] = spherical ? 0.f : -0.5f * n2;

    if (c != 0 || S == 0) return;
    // ---- the iteration's history ------------------------------------------------------------------------------------
    long long ch = 0, empty = 0;
    for (int s = tid; s < S; s += KM_UPD_THREADS) {
        sSlot[s] = partial[(int64_t)s * stride + stride - 2];
        ch += (long long)partial[(int64_t)s * stride + stride - 1];
    }
    for (int cc = tid; cc < K; cc += KM_UPD_THREADS) {
        long long n_cc = 0;
        for (int s = 0; s < S; ++s) n_cc += (long long)counts[(int64_t)s * stride + cc];
        empty += n_cc == 0 ? 1 : 0;
    }
    const long long changed = km_block_sum_ll(ch, sLL);
    const long long empties = km_block_sum_ll(empty, sLL);
    if (tid == 0) {
        float inertia = 0.f;
        for (int s = 0; s < S; ++s) inertia += sSlot[s];
        const int64_t at = *index;
        if (at >= 0 && at < capacity) {
            inertia_hist[at] = inertia;
            changed_hist[at] = (int64_t)changed;
            empty_hist[at] = (int32_t)empties;
        }
        *index = at + 1;
    }
}

static int64_t km_splits(int64_t n, int64_t splits)
{
    const int64_t tiles = ceil_div(n, 32);
    if (splits > 0) return splits;
    return tiles < KM_AUTO_SPLITS ? tiles : KM_AUTO_SPLITS;
}

static size_t km_lds(int64_t D, int esz, int ct, bool w_lds)
{
    const size_t x = rt_query_lds(D, esz);
    return x + (w_lds ? (size_t)ct * x : 0);
}

template <typename T, int CT>
static int km_launch(const KMeansParams &p, int64_t S, int slabs, size_t lds, hipStream_t stream)
{
    static bool raised = false;
    if (!raised && lds > 60 * 1024) {
        if (hipFuncSetAttribute((const void *)k_kmeans_pass<T, CT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)KM_LDS_DYN_MAX) != hipSuccess) {
            (void)hipGetLastError();
            set_error("kmeans_pass: cannot raise the dynamic LDS limit");
            return GSAGE_ELAUNCH;
        }
        raised = true;
    }
    launch(k_kmeans_pass<T, CT>, dim3((unsigned)S, (unsigned)slabs), dim3(64 * KM_WAVES), lds, stream, p);
    return check_launch("kmeans_pass");
}

template <typename T>
static int km_dispatch(const KMeansParams &p, int ct, int64_t S, int slabs, size_t lds, hipStream_t stream)
{
    if (ct == 1) return km_launch<T, 1>(p, S, slabs, lds, stream);
    if (ct == 2) return km_launch<T, 2>(p, S, slabs, lds, stream);
    return km_launch<T, 4>(p, S, slabs, lds, stream);
}

}  // namespace gsage

using namespace gsage;

extern "C" {

int64_t gsage_kmeans_pass_scratch(int64_t n, int32_t K, int32_t D, int32_t splits)
{
    if (n < 1 || n >= (1LL << 31) || K < 1 || K > KM_K_MAX || D < 1 || D > RT_D_MAX || splits < 0 || splits > KM_SPLITS_MAX)
        return -1;
    const int64_t S = km_splits(n, splits);
    if (ceil_div(ceil_div(n, 32), S) * 32 >= KM_RANGE_ROWS_MAX) return -1;
    return S * ((int64_t)K * D + K + 2);
}

int gsage_kmeans_pass(const void *table, int dtype, int64_t ldx, int64_t N, const int64_t *ids, int64_t n,
                      const float *Cn, const float *bias, int32_t K, int32_t D, int32_t k_live,
                      const int32_t *labels_in, int32_t splits, float *partial, int32_t *labels_out, float *dist_out,
                      void *stream)
{
    GSAGE_REQUIRE(K >= 1 && K <= KM_K_MAX, "kmeans_pass: K must be in [1, %d], not %d", KM_K_MAX, (int)K);
    GSAGE_REQUIRE(D >= 1 && D <= RT_D_MAX, "kmeans_pass: D must be in [1, %d], not %d", RT_D_MAX, (int)D);
    GSAGE_REQUIRE(n >= 1 && n < (1LL << 31), "kmeans_pass: n must be in [1, 2^31), not %lld", (long long)n);
    GSAGE_REQUIRE(N >= 1, "kmeans_pass: N must be at least 1, not %lld", (long long)N);
    GSAGE_REQUIRE(ldx >= D, "kmeans_pass: ldx = %lld must be at least D = %d", (long long)ldx, (int)D);
    GSAGE_REQUIRE(dtype == GSAGE_F32 || dtype == GSAGE_BF16, "kmeans_pass: dtype must be fp32 or bf16 (the compute mode)");
    GSAGE_REQUIRE(k_live >= 1 && k_live <= K, "kmeans_pass: k_live must be in [1, K = %d], not %d", (int)K, (int)k_live);
    GSAGE_REQUIRE(splits >= 0 && splits <= KM_SPLITS_MAX, "kmeans_pass: splits must be in [0, %d] (0 = chosen here), not %d",
                  KM_SPLITS_MAX, (int)splits);
    GSAGE_REQUIRE(table && ids && Cn && bias, "kmeans_pass: null pointer");
    GSAGE_REQUIRE(partial || labels_out || dist_out, "kmeans_pass: null pointer (partial, labels_out and dist_out: no output)");
    const int esz = dtype == GSAGE_BF16 ? 2 : 4;
    GSAGE_REQUIRE(((uintptr_t)table % esz) == 0, "kmeans_pass: misaligned table");
    const int64_t S = km_splits(n, splits);
    const int64_t tiles_per_split = ceil_div(ceil_div(n, 32), S);
    GSAGE_REQUIRE(!partial || tiles_per_split * 32 < KM_RANGE_ROWS_MAX,
                  "kmeans_pass: splits = %d leaves a workgroup %lld rows; its counts are exact below 2^24 only",
                  (int)splits, (long long)(tiles_per_split * 32));

    const int ct = K <= 32 ? 1 : K <= 64 ? 2 : 4;
    const int slabs = partial ? (int)ceil_div(D, km_slab(ct, esz)) : 1;
    const bool w_lds = km_lds(D, esz, ct, true) <= KM_LDS_DYN_MAX;
    const size_t lds = km_lds(D, esz, ct, w_lds);
    GSAGE_REQUIRE(lds <= KM_LDS_DYN_MAX, "kmeans_pass: D = %d does not fit the LDS", (int)D);

    KMeansParams p;
    p.table = table; p.ids = ids; p.Cn = Cn; p.bias = bias; p.labels_in = labels_in; p.partial = partial;
    p.labels_out = labels_out; p.dist_out = dist_out;
    p.ldx = ldx; p.N = N; p.n = n;
    p.tiles_per_split = tiles_per_split;
    p.K = K; p.D = D; p.k_live = k_live;
    p.x_vec = ((uintptr_t)table % 16) == 0 && (ldx * esz) % 16 == 0;
    p.w_lds = w_lds ? 1 : 0;
    return dtype == GSAGE_BF16 ? km_dispatch<uint16_t>(p, ct, S, slabs, lds, (hipStream_t)stream)
                               : km_dispatch<float>(p, ct, S, slabs, lds, (hipStream_t)stream);
}

int gsage_kmeans_update(const float *partial, int32_t S, int32_t K, int32_t D, int dtype, int spherical, float *Cn,
                        float *bias, float *inertia_hist, int64_t *changed_hist, int32_t *empty_hist, int64_t *index,
                        int64_t capacity, void *stream)
{
    GSAGE_REQUIRE(K >= 1 && K <= KM_K_MAX, "kmeans_update: K must be in [1, %d], not %d", KM_K_MAX, (int)K);
    GSAGE_REQUIRE(D >= 1 && D <= RT_D_MAX, "kmeans_update: D must be in [1, %d], not %d", RT_D_MAX, (int)D);
    GSAGE_REQUIRE(S >= 0 && S <= KM_SPLITS_MAX, "kmeans_update: S must be in [0, %d] (0 = the bias only), not %d",
                  KM_SPLITS_MAX, (int)S);
    GSAGE_REQUIRE(dtype == GSAGE_F32 || dtype == GSAGE_BF16, "kmeans_update: dtype must be fp32 or bf16 (the compute mode)");
    GSAGE_REQUIRE(spherical == 0 || spherical == 1, "kmeans_update: spherical must be 0 or 1, not %d", spherical);
    GSAGE_REQUIRE(Cn && bias, "kmeans_update: null pointer");
    GSAGE_REQUIRE(S == 0 || (partial && inertia_hist && changed_hist && empty_hist && index),
                  "kmeans_update: null pointer (partial, the histories and index are needed for S > 0)");
    GSAGE_REQUIRE(S == 0 || capacity >= 1, "kmeans_update: capacity must be at least 1, not %lld", (long long)capacity);
    launch(k_kmeans_update, dim3((unsigned)K), dim3(KM_UPD_THREADS), 0, (hipStream_t)stream, partial, S, K, D,
           (int32_t)(dtype == GSAGE_BF16), (int32_t)spherical, Cn, bias, inertia_hist, changed_hist, empty_hist, index,
           capacity);
    return check_launch("kmeans_update");
}

}  // extern "C"
