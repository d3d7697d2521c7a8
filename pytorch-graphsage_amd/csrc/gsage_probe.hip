// gsage_probe.hip -- one full-batch loss-and-gradient pass of a linear classifier over selected rows of a table of
// embeddings (gsage_probe_pass): the inner step of the linear probe (infer.LinearProbe).
//
//   z[i, c] = sum_d X[ids[i], d] * W~[c, d] + b[c]          (W~: the fp32 master as the compute mode sees it)
//   classification:  l_i = logsumexp_c z[i, .] - z[i, y_i],               G[i, c] = softmax(z_i)[c] - [c == y_i]
//   multilabel:      l_i = (1/C) sum_c (softplus(z[i, c]) - y[i, c] z[i, c]),  G[i, c] = (sigmoid(z[i, c]) - y[i, c]) / C
//   loss = (1/n) sum_i l_i,   dW = (1/n) G^T X[ids],   db = (1/n) sum_i G[i, .]
//
// No n x C buffer exists: logits, probabilities and G live in MFMA accumulator registers.
//
// k_probe_pass<T, CT>, grid (row ranges S) x (D slabs of 256 columns; 128 for CT = 4 in fp32), 4 waves; CT = 1, 2 or 4 class tiles of 32:
//   * W~ (zero past C and D) is staged once per workgroup in LDS, per class tile in the lds_slot image
//     rt_stage_queries uses.  Where it does not fit beside the row tile (w_lds == 0) its fragments are read from
//     global memory instead (the same bits, from the L2).
//   * a workgroup walks a contiguous range of 32-row tiles.  Per tile the gathered rows land in LDS ONCE, in the
//     same image (zero past D and past n); both products read them from there.
//   * wave w owns class tile w % CT; the 4 / CT waves of a class tile share the slab's d tiles.  First product, over
//     the whole D: X rows are the A operand and the tile's classes the B operand, so the 32 x 32 result has THE
//     CLASS ON THE LANE and 16 rows in the lane's registers (class = 32 ct + (lane & 31), row = rt_frag_row(reg)
//     + 4 (lane >> 5)).  Softmax: per register a reduction over the 32 lanes of the half gives the tile's (max, sum
//     of exp); the CT tiles' pairs meet in LDS (one barrier) and every wave folds them in the same order.
//   * second product dW^T[d][c] += sum_i X[i][d] G[i][c] sums over the first product's REGISTER (row) index, so G is
//     the B fragment with no lane movement.  bf16: registers 8 s .. 8 s + 7 become k step s as a hi + lo pair of
//     bf16 (two MFMAs; G as one bf16 would put 2^-9 into every gradient element), element j of lane half h being
//     row 16 s + 8 (j >> 2) + 4 h + (j & 3); X^T comes from the row tile by transposed LDS reads
//     (ds_read_b64_tr_b16) of exactly those rows.  fp32: mfma_f32_32x32x2f32 per register, lane half h supplying
//     row rt_frag_row(reg) + 4 h of X^T by a plain LDS read.
//   * the dW accumulators (up to 2 CT tiles per wave) stay in registers across the workgroup's whole row range and are
//     written once, scaled by 1 / n, as row `blockIdx.x` of partial [S][C D + C + 1] = [dW | db | loss] (the
//     gsage_head_ce convention).  A wider D adds slabs (grid.y), each recomputing the logits over the whole D; slab 0
//     writes db and the loss.
// k_probe_loss: the sum over S of the loss slots in buffer order -> loss_out[*index].
//
// No atomics: for fixed (n, C, D, splits) every sum has one order, so the result is bit-identical call to call.
#include "gsage_retrieve_dev.h"

namespace gsage {

constexpr int PB_C_MAX = 128;
constexpr int PB_SPLITS_MAX = 1024;
constexpr int PB_AUTO_SPLITS = 256;               // one persistent workgroup per CU: a partial row is C D + C + 1 floats
constexpr int PB_WAVES = 4;
// columns of dW a workgroup accumulates (grid.y slabs beyond): 256, but 128 for four class tiles in fp32, whose 8 d tiles
// per wave the compiler does not hold without spilling
constexpr int pb_slab(int ct, int esz) { return ct == 4 && esz == 4 ? 128 : 256; }
constexpr size_t PB_LDS_DYN_MAX = RT_LDS_MAX - 2048;     // beside the static exchange buffers
enum { PB_CLASSIFICATION = 0, PB_MULTILABEL = 1 };

thread_local const int64_t *t_probe_loss_index = nullptr;

struct ProbeParams {
    const void *table;
    const int64_t *ids;
    const void *targets;
    const float *W;
    const float *bias;
    float *partial;
    int64_t ldx, N, n, ldy;
    int64_t tiles_per_split;
    int32_t C, D, task, x_vec, w_lds;
    float inv_n;
};

typedef short pb_s16x4 __attribute__((ext_vector_type(4)));

// 16-byte chunk ch of class c of the fp32 master W [C][D] as the compute mode sees it; zero past C and D
template <typename T>
__device__ __forceinline__ vec16 pb_w_chunk(const float *W, int c, int ch, int C, int D)
{
    constexpr int EPC = 16 / (int)sizeof(T);
    const int d0 = ch * EPC;
    float f[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) f[e] = (c < C && d0 + e < D) ? W[(int64_t)c * D + d0 + e] : 0.f;
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

// sum / max over the 32 lanes of a lane half (the classes of one tile), the same value in all of them
__device__ __forceinline__ float pb_half_sum(float v)
{
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ float pb_half_max(float v)
{
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

template <typename T, int CT>
__global__ void __launch_bounds__(64 * PB_WAVES)
k_probe_pass(const ProbeParams p)
{
    extern __shared__ vec16 pb_smem[];
    constexpr int WPC = PB_WAVES / CT;                                       // waves that share a class tile
    constexpr int NDT = pb_slab(CT, (int)sizeof(T)) / 32 / WPC;              // d tiles of a wave
    __shared__ float2 sE[PB_WAVES][32];                                      // per wave and row: (max, sum of exp)
    __shared__ float sL[PB_WAVES];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ct = wave % CT, dg = wave / CT;
    const int h = lane >> 5;
    const int ql = lane & 31;
    const int C = p.C, D = p.D;
    const rt_shape<T> sh(D, p.x_vec);
    const int nkt = sh.nkt;
    vec16 *sX = pb_smem;
    vec16 *sW = sX + (size_t)nkt * RT_QT * CH;
    float *sY = reinterpret_cast<float *>(sW + (p.w_lds ? (size_t)CT * nkt * RT_QT * CH : 0));
    int *sYi = reinterpret_cast<int *>(sY);

    // ---- W~, once ------------------------------------------------------------------------------------------------
    if (p.w_lds) {
        for (int i = tid; i < CT * nkt * RT_QT * CH; i += 64 * PB_WAVES) {
            const int tile = i >> 8, row = (i >> 3) & 31, ch = i & 7;        // tile = class tile * nkt + k tile
            const int wt = tile / nkt, kt = tile - wt * nkt;
            sW[tile * (RT_QT * CH) + lds_slot(row, ch)] = pb_w_chunk<T>(p.W, wt * 32 + row, kt * CH + ch, C, D);
        }
    }
    const int cls = ct * 32 + ql;                                            // this lane's class
    const bool cls_ok = cls < C;
    const float bc = cls_ok ? p.bias[cls] : 0.f;
    const float inv_c = 1.f / (float)C;

    f32x16_t acc[NDT];
#pragma unroll
    for (int j = 0; j < NDT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    float dbacc = 0.f, lossacc = 0.f;

    const int dt0 = ((int)blockIdx.y * WPC + dg) * NDT;                      // this wave's first d tile
    // byte offsets of this lane's X^T reads in the row tile's image, for the wave's first d tile (bf16: and the next);
    // d tile dt0 + j lies a whole number of k tiles further (dt0 is even), which the reads add as a constant.
    //   bf16: [d tile parity][k step s][jj]: lane 4 q + pp of a 16-lane group addresses row 16 s + 8 jj + 4 h + q,
    //         columns c0 + 4 pp .. + 3 of a 4 x 16 block and receives column (lane & 15) of its 4 rows
    //   fp32: [0][reg >> 3][reg & 7]: row rt_frag_row(reg) + 4 h, column lane & 31
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
    const int64_t tiles = (p.n + 31) / 32;
    const int64_t t_begin = (int64_t)blockIdx.x * p.tiles_per_split;
    const int64_t t_end = t_begin + p.tiles_per_split < tiles ? t_begin + p.tiles_per_split : tiles;
    for (int64_t t = t_begin; t < t_end; ++t) {
        const int64_t row0 = t * 32;
        if (t != t_begin) __syncthreads();                                   // everybody is done with the last tile
        // ---- the tile's rows and targets -> LDS -----------------------------------------------------------------
        for (int i = tid; i < nkt * RT_QT * CH; i += 64 * PB_WAVES) {
            const int row = i / (nkt * CH), c = i - row * (nkt * CH);        // consecutive threads: one row's chunks
            vec16 v = {0u, 0u, 0u, 0u};
            if (row0 + row < p.n && c < sh.chunks) {
                const int64_t id = p.ids[row0 + row];
                if ((uint64_t)id < (uint64_t)p.N) v = rt_load_chunk<T>((const T *)p.table + id * p.ldx, c, D, p.x_vec);
            }
            sX[(c >> 3) * (RT_QT * CH) + lds_slot(row, c & 7)] = v;
        }
        if (p.task == PB_CLASSIFICATION) {
            if (tid < 32) sYi[tid] = row0 + tid < p.n ? (int)((const int64_t *)p.targets)[row0 + tid] : -1;
        } else {
            for (int i = tid; i < 32 * CT * 32; i += 64 * PB_WAVES) {
                const int row = i / (CT * 32), c = i - row * (CT * 32);
                sY[i] = (row0 + row < p.n && c < C) ? ((const float *)p.targets)[(row0 + row) * p.ldy + c] : 0.f;
            }
        }
        __syncthreads();

        // ---- logits of this wave's class tile: class on the lane, rows in the registers ------------------------------
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
                mma_chunk<T>::run(a, pb_w_chunk<T>(p.W, cls, 2 * kk + h, C, D), z);
            }
        }

        // ---- G in place of the logits ---------------------------------------------------------------------------
        // (hh: the lane half, opaque to the compiler -- it otherwise keeps every row's LDS addresses and bounds, a
        // hundred registers that depend on the lane alone, live across the whole tile loop, and spills)
        int hh = h;
        asm volatile("" : "+v"(hh));
        if (p.task == PB_CLASSIFICATION) {
            // softmax over the CT class tiles: per wave (max, sum of exp) over its 32 classes, met in LDS
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rt_frag_row(r) + 4 * hh;
                const float v = z[r] + bc;
                const bool hit = cls == sYi[row];
                if (hit) lossacc -= v;                       // l_i = m + log s - z[i, y_i]; a padding row has y = -1
                const float mw = pb_half_max(cls_ok ? v : -INFINITY);
                const float e = cls_ok ? expf(v - mw) : 0.f;
                const float sw = pb_half_sum(e);
                if (CT > 1) {
                    if (ql == 0) sE[wave][row] = make_float2(mw, sw);
                    z[r] = v;
                } else {
                    const bool live = row0 + row < p.n;
                    if (live && ql == 0) lossacc += mw + logf(sw);
                    z[r] = live ? e / sw - (hit ? 1.f : 0.f) : 0.f;
                }
                __builtin_amdgcn_sched_barrier(0);           // one row at a time: the rows' chains interleaved cost registers
            }
            if (CT > 1) {
                __syncthreads();
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = rt_frag_row(r) + 4 * hh;
                    float2 ms[CT];
                    float m = -INFINITY, s = 0.f;
#pragma unroll
                    for (int w = 0; w < CT; ++w) {
                        ms[w] = sE[w][row];
                        m = fmaxf(m, ms[w].x);
                    }
#pragma unroll
                    for (int w = 0; w < CT; ++w) s += ms[w].y * expf(ms[w].x - m);
                    const bool live = row0 + row < p.n;
                    if (live && wave == 0 && ql == 0) lossacc += m + logf(s);
                    z[r] = live && cls_ok ? expf(z[r] - m) / s - (cls == sYi[row] ? 1.f : 0.f) : 0.f;
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rt_frag_row(r) + 4 * hh;
                const float v = z[r] + bc;
                const float y = sY[row * (CT * 32) + cls];
                const float tt = expf(-fabsf(v));
                const float sig = (v >= 0.f ? 1.f : tt) / (1.f + tt);
                const bool on = row0 + row < p.n && cls_ok;
                if (on) lossacc += (fmaxf(v, 0.f) + log1pf(tt) - y * v) * inv_c;
                z[r] = on ? (sig - y) * inv_c : 0.f;
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) dbacc += z[r];

        // ---- dW^T tiles of this wave += X^T G -----------------------------------------------------------------------
        if constexpr (sizeof(T) == 2) {
            vec16 ghi[2], glo[2];
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float g0 = z[8 * s + 2 * e], g1 = z[8 * s + 2 * e + 1];
                    const uint16_t h0 = f32_to_bf16(g0), h1 = f32_to_bf16(g1);
                    ghi[s][e] = (uint32_t)h0 | ((uint32_t)h1 << 16);
                    glo[s][e] = pack_bf16x2(g0 - bf16_to_f32(h0), g1 - bf16_to_f32(h1));
                }
#pragma unroll
            for (int j = 0; j < NDT; ++j) {
                if ((dt0 + j) * 32 < D) {                                    // wave-uniform: EXEC stays whole
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        pb_s16x4 x[2];
#pragma unroll
                        for (int jj = 0; jj < 2; ++jj)
                            x[jj] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) pb_s16x4 *)(
                                (reinterpret_cast<const char *>(sX) + xt_off[j & 1][s][jj]) + (j >> 1) * (RT_QT * CH * 16)));
                        vec16 a;
                        a[0] = __builtin_bit_cast(uint2, x[0]).x; a[1] = __builtin_bit_cast(uint2, x[0]).y;
                        a[2] = __builtin_bit_cast(uint2, x[1]).x; a[3] = __builtin_bit_cast(uint2, x[1]).y;
                        mma_chunk<T>::run(a, ghi[s], acc[j]);
                        mma_chunk<T>::run(a, glo[s], acc[j]);
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

    // ---- the workgroup's partial row [dW | db | loss], scaled by 1 / n ----------------------------------------------
    float *out = p.partial + (int64_t)blockIdx.x * ((int64_t)C * D + C + 1);
#pragma unroll
    for (int j = 0; j < NDT; ++j) {
        const int dbase = (dt0 + j) * 32 + 4 * h;
        float *o = out + cls * D + dbase;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (dbase + rt_frag_row(r) < D && cls_ok) o[rt_frag_row(r)] = acc[j][r] * p.inv_n;
    }
    // db and the loss are counted once: by the first wave of each class tile, in slab 0
    const float dbv = dbacc + __shfl_xor(dbacc, 32);
    float l = pb_half_sum(lossacc);
    l += __shfl_xor(l, 32);
    if (lane == 0) sL[wave] = l;
    __syncthreads();
    if (blockIdx.y == 0 && dg == 0) {
        if (h == 0 && cls_ok) out[(int64_t)C * D + cls] = dbv * p.inv_n;
        if (wave == 0 && lane == 0) {
            float tot = 0.f;
#pragma unroll
            for (int w = 0; w < CT; ++w) tot += sL[w];
            out[(int64_t)C * D + C] = tot * p.inv_n;
        }
    }
}

// loss_out[*index] = sum over the S partial rows of their loss slot, in buffer order
__global__ void __launch_bounds__(64)
k_probe_loss(const float *partial, int32_t S, int64_t stride, float *loss_out, const int64_t *index)
{
    __shared__ float slot[PB_SPLITS_MAX];
    for (int s = threadIdx.x; s < S; s += 64) slot[s] = partial[(int64_t)s * stride + stride - 1];
    __syncthreads();
    if (threadIdx.x == 0) {
        float l = 0.f;
        for (int s = 0; s < S; ++s) l += slot[s];
        loss_out[index ? *index : 0] = l;
    }
}

static int64_t pb_splits(int64_t n, int64_t splits)
{
    const int64_t tiles = ceil_div(n, 32);
    if (splits > 0) return splits;
    return tiles < PB_AUTO_SPLITS ? tiles : PB_AUTO_SPLITS;
}

static size_t pb_lds(int64_t D, int esz, int ct, int task, bool w_lds)
{
    const size_t x = rt_query_lds(D, esz);
    return x + (w_lds ? (size_t)ct * x : 0) + (task == PB_MULTILABEL ? (size_t)32 * ct * 32 * 4 : 128);
}

template <typename T, int CT>
static int pb_launch(const ProbeParams &p, int64_t S, int slabs, size_t lds, hipStream_t stream)
{
    static bool raised = false;
    if (!raised && lds > 60 * 1024) {
        if (hipFuncSetAttribute((const void *)k_probe_pass<T, CT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)PB_LDS_DYN_MAX) != hipSuccess) {
            (void)hipGetLastError();
            set_error("probe_pass: cannot raise the dynamic LDS limit");
            return GSAGE_ELAUNCH;
        }
        raised = true;
    }
    launch(k_probe_pass<T, CT>, dim3((unsigned)S, (unsigned)slabs), dim3(64 * PB_WAVES), lds, stream, p);
    return check_launch("probe_pass");
}

template <typename T>
static int pb_dispatch(const ProbeParams &p, int ct, int64_t S, int slabs, size_t lds, hipStream_t stream)
{
    if (ct == 1) return pb_launch<T, 1>(p, S, slabs, lds, stream);
    if (ct == 2) return pb_launch<T, 2>(p, S, slabs, lds, stream);
    return pb_launch<T, 4>(p, S, slabs, lds, stream);
}

}  // namespace gsage

using namespace gsage;

extern "C" {

int gsage_probe_loss_index_next(const int64_t *index)
{
    t_probe_loss_index = index;
    return GSAGE_OK;
}

int64_t gsage_probe_pass_scratch(int64_t n, int32_t C, int32_t D, int32_t splits)
{
    if (n < 1 || n >= (1LL << 31) || C < 1 || C > PB_C_MAX || D < 1 || D > RT_D_MAX || splits < 0 || splits > PB_SPLITS_MAX)
        return -1;
    return pb_splits(n, splits) * ((int64_t)C * D + C + 1);
}

int gsage_probe_pass(const void *table, int dtype, int64_t ldx, int64_t N, const int64_t *ids, int64_t n,
                     const void *targets, int task, int64_t ldy, const float *W, const float *bias, int32_t C,
                     int32_t D, int32_t splits, float *partial, float *loss_out, void *stream)
{
    const int64_t *index = t_probe_loss_index;
    t_probe_loss_index = nullptr;
    GSAGE_REQUIRE(C >= 1 && C <= PB_C_MAX, "probe_pass: C must be in [1, %d], not %d", PB_C_MAX, (int)C);
    GSAGE_REQUIRE(D >= 1 && D <= RT_D_MAX, "probe_pass: D must be in [1, %d], not %d", RT_D_MAX, (int)D);
    GSAGE_REQUIRE(n >= 1 && n < (1LL << 31), "probe_pass: n must be in [1, 2^31), not %lld", (long long)n);
    GSAGE_REQUIRE(N >= 1, "probe_pass: N must be at least 1, not %lld", (long long)N);
    GSAGE_REQUIRE(ldx >= D, "probe_pass: ldx = %lld must be at least D = %d", (long long)ldx, (int)D);
    GSAGE_REQUIRE(dtype == GSAGE_F32 || dtype == GSAGE_BF16, "probe_pass: dtype must be fp32 or bf16 (the compute mode)");
    GSAGE_REQUIRE(task == PB_CLASSIFICATION || task == PB_MULTILABEL,
                  "probe_pass: task must be 0 (classification) or 1 (multilabel_classification), not %d", task);
    GSAGE_REQUIRE(task != PB_MULTILABEL || ldy >= C, "probe_pass: ldy = %lld must be at least C = %d", (long long)ldy, (int)C);
    GSAGE_REQUIRE(splits >= 0 && splits <= PB_SPLITS_MAX, "probe_pass: splits must be in [0, %d] (0 = chosen here), not %d",
                  PB_SPLITS_MAX, (int)splits);
    GSAGE_REQUIRE(table && ids && targets && W && bias && partial && loss_out, "probe_pass: null pointer");
    const int esz = dtype == GSAGE_BF16 ? 2 : 4;
    GSAGE_REQUIRE(((uintptr_t)table % esz) == 0, "probe_pass: misaligned table");

    const int ct = C <= 32 ? 1 : C <= 64 ? 2 : 4;
    const int slabs = (int)ceil_div(D, pb_slab(ct, esz));
    const bool w_lds = pb_lds(D, esz, ct, task, true) <= PB_LDS_DYN_MAX;
    const size_t lds = pb_lds(D, esz, ct, task, w_lds);
    GSAGE_REQUIRE(lds <= PB_LDS_DYN_MAX, "probe_pass: D = %d does not fit the LDS", (int)D);
    const int64_t S = pb_splits(n, splits);

    ProbeParams p;
    p.table = table; p.ids = ids; p.targets = targets; p.W = W; p.bias = bias; p.partial = partial;
    p.ldx = ldx; p.N = N; p.n = n; p.ldy = ldy;
    p.tiles_per_split = ceil_div(ceil_div(n, 32), S);
    p.C = C; p.D = D; p.task = task;
    p.x_vec = ((uintptr_t)table % 16) == 0 && (ldx * esz) % 16 == 0;
    p.w_lds = w_lds ? 1 : 0;
    p.inv_n = 1.f / (float)n;
    const int rc = dtype == GSAGE_BF16 ? pb_dispatch<uint16_t>(p, ct, S, slabs, lds, (hipStream_t)stream)
                                       : pb_dispatch<float>(p, ct, S, slabs, lds, (hipStream_t)stream);
    if (rc != GSAGE_OK) return rc;
    launch(k_probe_loss, dim3(1), dim3(64), 0, (hipStream_t)stream, (const float *)partial, (int32_t)S,
           (int64_t)C * D + C + 1, loss_out, index);
    return check_launch("probe_pass loss");
}

}  // extern "C"
