// gsage_head_wide.hip -- the head of GSSupervised for a WIDE class dimension (up to 128 outputs), forward and
// backward in one launch, for softmax cross-entropy and for the multilabel soft-margin loss:
//
//     z      = E / max(||E||_2, 1e-12)                        F.normalize, per row
//     logits = z W^T + b                                       nn.Linear(D, C)               -> preds
//     task 0:  l_i = logsumexp(logits_i) - logits_i[y_i]       F.cross_entropy (targets int64 [B])
//     task 1:  l_i = (1/C) sum_c softplus(logits_ic) - y_ic logits_ic     F.multilabel_soft_margin_loss (fp32 [B, ldy])
//     loss = (1/Bv) sum_{i < Bv} l_i;  G = d loss / d logits;  dz = G W;  dE_i = (dz_i - z_i <z_i, dz_i>) / max(||E_i||, 1e-12)
//     dW = G^T z,  db = column sums of G
//
// gsage_head_ce keeps a class per lane of ONE wave (<= 64) and walks the columns on the VALU.  Here the three
// products are exact fp32 MFMAs (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain, the numerics of the other heads).
//
// k_head_wide: one workgroup (4 waves) per tile of 16 rows.
//   * the tile's rows are normalised into LDS (zs [16][ld], zero past D and past B); fc.weight is staged once beside
//     them (Ws [C][ld], zero past D) where both fit the LDS, else its fragments are read from global memory / the L2.
//   * logits: A = z (row on lane & 15, k on lane >> 4), B = W^T (class on lane & 15), so the 16 x 16 result has THE
//     CLASS ON THE LANE and rows 4 (lane >> 4) + r in the lane's four registers.  Wave w owns class tiles w and w + 4.
//     Softmax: (max, sum of exp) per tile over its 16 lanes, the tiles' pairs meet in LDS and are folded in one order;
//     sigmoid / softplus need no exchange.  G replaces the logits in the registers.
//   * <z_i, dz_i> = sum_c G_ic (logits_ic - b_c): formed from the registers (no second pass over D).
//   * dW^T [d][c] = sum_i z[i][d] G[i][c] sums over the REGISTER (row) index of the first product: register r of G is
//     the B operand of k step r as it stands (rows r, 4 + r, 8 + r, 12 + r), z^T comes from LDS.  Four MFMAs per
//     (class tile, d tile), written straight to the workgroup's partial row: no accumulator outlives a d tile.
//   * dz = G W sums over the class, which is on the lane: G crosses the workgroup through LDS (Gs [16][132]) and comes
//     back as the A operand; wave w owns d tiles w, w + 4, ...; d E is written from the accumulators.
//   * output: row blockIdx.x of partial [n_wg][C D + C + 1] = [dW | db | sum of l_i] (gsage_head_ce's convention: the
//     gradients carry the 1 / Bv, the loss slot does not).
// k_head_wide_reduce: the optional dW | db | loss = sums of the partial rows in buffer order (k_head_reduce with the
//   live-row count read on the device).
//
// No atomics; for fixed (B, C, D) every sum has one order, so the result is bit-identical from launch to launch.
#include "gsage_common.h"

namespace gsage {

constexpr int HW_CMAX = 128;
constexpr int HW_DMAX = 1024;
constexpr int HW_ROWS = 16;                        // rows of a workgroup (one MFMA tile)
constexpr int HW_LDG = HW_CMAX + 4;                // row stride of Gs: 4 mod 64, conflict-free A-operand reads
constexpr size_t HW_LDS_DYN_MAX = 160 * 1024 - 2048;      // beside the static exchange buffers
enum { HW_CLASSIFICATION = 0, HW_MULTILABEL = 1 };

typedef float hw_f32x4 __attribute__((ext_vector_type(4)));

struct HeadWideParams {
    const float *E;          // [B, lde]
    const float *W;          // [C, D]
    const float *bias;       // [C]
    const void *targets;     // int64 [n_batches, B] or fp32 [n_batches, B, ldy]; NULL: forward only
    const int64_t *batch_idx;
    int64_t n_batches;
    const int32_t *n_valid;
    float *preds;            // [B, C]
    void *dE;                // [B, ldd] bf16 or fp32
    float *partial;          // [n_wg, C*D + C + 1]
    int64_t lde, ldd, ldy;
    int32_t B, C, D, task, dE_dtype, w_lds, ld;
};

__device__ __forceinline__ float hw_sum16(float v)      // over the 16 lanes that share lane >> 4
{
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float hw_max16(float v)
{
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ hw_f32x4 hw_mma(float a, float b, hw_f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__global__ void __launch_bounds__(256)
k_head_wide(const HeadWideParams p)
{
    extern __shared__ __attribute__((aligned(16))) float hw_lds[];
    __shared__ float2 sE[HW_CMAX / 16][HW_ROWS];   // per class tile and row: (max, sum of exp)
    __shared__ float sZ[4][HW_ROWS];               // per wave and row: its classes' share of <z, dz>
    __shared__ float sN[HW_ROWS];                  // max(||E_i||, 1e-12)
    __shared__ float sL[4];
    const int C = p.C, D = p.D, ld = p.ld;
    float *zs = hw_lds;                            // [16][ld]
    float *Gs = zs + HW_ROWS * ld;                 // [16][HW_LDG]
    float *Ws = Gs + HW_ROWS * HW_LDG;             // [C][ld] (w_lds)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, kq = lane >> 4;
    const int row0 = blockIdx.x * HW_ROWS;
    const int CT = (C + 15) >> 4, D4 = (D + 3) & ~3, C4 = (C + 3) & ~3;
    const int64_t bq = p.batch_idx ? (int64_t)((uint64_t)*p.batch_idx % (uint64_t)p.n_batches) : 0;
    // rows past Bv are padding (the reference's chunks are not all of one size): no loss, no gradient
    const int Bv = p.n_valid ? min(max(p.n_valid[bq], 1), p.B) : p.B;
    const bool backward = p.targets != nullptr;

    // this wave's class tiles, this lane's classes
    const bool tile_on[2] = {wave < CT, wave + 4 < CT};                 // wave-uniform
    const int cls[2] = {wave * 16 + j, (wave + 4) * 16 + j};
    const bool ok[2] = {cls[0] < C, cls[1] < C};

    // ---- targets and bias of this lane's (row, class) pairs: requested before anything waits -----------------------
    int yi[4];
    float yf[2][4], bc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) bc[t] = ok[t] ? p.bias[cls[t]] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = row0 + 4 * kq + r;
        yi[r] = -1;
        yf[0][r] = yf[1][r] = 0.f;
        if (backward && i < p.B) {
            if (p.task == HW_CLASSIFICATION) {
                yi[r] = (int)((const int64_t *)p.targets)[bq * p.B + i];
            } else {
                const float *y = (const float *)p.targets + (bq * p.B + i) * p.ldy;
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    if (ok[t]) yf[t][r] = y[cls[t]];
            }
        }
    }

    // ---- 1. the tile's rows, normalised, -> LDS (wave w: rows 4 w .. 4 w + 3) --------------------------------------
    {
        float ss[4] = {0.f, 0.f, 0.f, 0.f}, nrm[4];
        for (int k = lane; k < D; k += 64)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = row0 + 4 * wave + r;
                const float e = i < p.B ? p.E[(int64_t)i * p.lde + k] : 0.f;
                ss[r] += e * e;
            }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) ss[r] += __shfl_xor(ss[r], o, 64);
            nrm[r] = fmaxf(sqrtf(ss[r]), 1e-12f);          // F.normalize's eps
            if (lane == 0) sN[4 * wave + r] = nrm[r];
        }
        for (int k = lane; k < ld; k += 64)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = row0 + 4 * wave + r;
                const float e = (k < D && i < p.B) ? p.E[(int64_t)i * p.lde + k] : 0.f;
                zs[(4 * wave + r) * ld + k] = e / nrm[r];
            }
    }
    // ---- fc.weight -> LDS, once: 8 rows x 4 column groups = 32 independent loads in flight per lane ----------------
    if (p.w_lds) {
        for (int c0 = wave * 8; c0 < C; c0 += 32)
            for (int kk = 0; kk < D; kk += 256) {
                float w[8][4];
                // (addresses clamped into the matrix: no predicate outlives its use)
#pragma unroll
                for (int u = 0; u < 8; ++u)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        w[u][q] = p.W[(int64_t)min(c0 + u, C - 1) * D + min(kk + 64 * q + lane, D - 1)];
#pragma unroll
                for (int u = 0; u < 8; ++u)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int k = kk + 64 * q + lane;
                        if (c0 + u < C && k < D) Ws[(c0 + u) * ld + k] = w[u][q];
                    }
            }
        const int pad = ld - D;                                 // 4 .. 7 zero columns behind every row
        for (int i = tid; i < C * pad; i += 256) Ws[(i / pad) * ld + D + i % pad] = 0.f;
    }
    __syncthreads();

    // ---- 2. logits of this wave's class tiles: class on the lane, rows 4 kq + r in the registers -------------------
    hw_f32x4 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) acc[t] = hw_f32x4{0.f, 0.f, 0.f, 0.f};
    {
        const float *za = zs + j * ld + kq;
        if (p.w_lds) {
            const float *w0 = Ws + min(cls[0], C - 1) * ld + kq;
            const float *w1 = Ws + min(cls[1], C - 1) * ld + kq;
            // four k steps to a trip: their twelve LDS reads are in flight together (one wave per SIMD hides nothing)
            for (int k0 = 0; k0 < D4; k0 += 16) {
                float a[4], b0[4], b1[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const bool in = k0 + 4 * s < D4;
                    a[s] = in ? za[k0 + 4 * s] : 0.f;
                    b0[s] = (in && tile_on[0] && ok[0]) ? w0[k0 + 4 * s] : 0.f;
                    b1[s] = (in && tile_on[1] && ok[1]) ? w1[k0 + 4 * s] : 0.f;
                }
                if (tile_on[0])
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc[0] = hw_mma(a[s], b0[s], acc[0]);
                if (tile_on[1])
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc[1] = hw_mma(a[s], b1[s], acc[1]);
            }
        } else {
            const float *w0 = p.W + (int64_t)min(cls[0], C - 1) * D;
            const float *w1 = p.W + (int64_t)min(cls[1], C - 1) * D;
            // four k steps to a trip: their fragments are requested together
            for (int k0 = 0; k0 < D4; k0 += 16) {
                float a[4], b0[4], b1[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int k = k0 + 4 * s + kq;
                    a[s] = k0 + 4 * s < D4 ? za[k0 + 4 * s] : 0.f;
                    b0[s] = (tile_on[0] && ok[0] && k < D) ? w0[k] : 0.f;
                    b1[s] = (tile_on[1] && ok[1] && k < D) ? w1[k] : 0.f;
                }
                if (tile_on[0])
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc[0] = hw_mma(a[s], b0[s], acc[0]);
                if (tile_on[1])
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc[1] = hw_mma(a[s], b1[s], acc[1]);
            }
        }
    }
    float u[2][4], v[2][4];                        // z . W_c, and the logit
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            u[t][r] = acc[t][r];
            v[t][r] = u[t][r] + bc[t];
            const int i = row0 + 4 * kq + r;
            if (tile_on[t] && ok[t] && i < p.B) p.preds[(int64_t)i * C + cls[t]] = v[t][r];
        }
    if (!backward) return;                         // (block-uniform) evaluation: predictions only

    // ---- 3. G in place of the logits -------------------------------------------------------------------------------
    const float invB = 1.f / (float)Bv;
    float G[2][4], lossacc = 0.f;
    if (p.task == HW_CLASSIFICATION) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (tile_on[t]) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float m = hw_max16(ok[t] ? v[t][r] : -INFINITY);
                    const float s = hw_sum16(ok[t] ? expf(v[t][r] - m) : 0.f);
                    if (j == 0) sE[wave + 4 * t][4 * kq + r] = make_float2(m, s);
                }
            }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * kq + r;
            float M = -INFINITY, S = 0.f;
            for (int w = 0; w < CT; ++w) M = fmaxf(M, sE[w][row].x);
            for (int w = 0; w < CT; ++w) S += sE[w][row].y * expf(sE[w][row].x - M);
            const float lse = M + logf(S);
            const bool live = row0 + row < Bv;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const bool hit = ok[t] && tile_on[t] && cls[t] == yi[r];
                const float pr = expf(v[t][r] - M) / S;
                G[t][r] = (live && ok[t] && tile_on[t]) ? (pr - (hit ? 1.f : 0.f)) * invB : 0.f;
                if (hit && live) lossacc += lse - v[t][r];
            }
        }
    } else {
        const float inv_c = 1.f / (float)C;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float x = v[t][r], y = yf[t][r];
                const float tt = expf(-fabsf(x));
                const float sig = (x >= 0.f ? 1.f : tt) / (1.f + tt);
                const bool on = row0 + 4 * kq + r < Bv && ok[t] && tile_on[t];
                if (on) lossacc += (fmaxf(x, 0.f) + log1pf(tt) - y * x) * inv_c;
                G[t][r] = on ? ((sig - y) * inv_c) * invB : 0.f;
            }
    }
    // <z_i, dz_i> = sum_c G_ic (z_i . W_c): this wave's classes; G -> LDS for the product over the class
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float zp = hw_sum16(G[0][r] * u[0][r] + G[1][r] * u[1][r]);
        if (j == 0) sZ[wave][4 * kq + r] = zp;
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (tile_on[t]) Gs[(4 * kq + r) * HW_LDG + cls[t]] = G[t][r];
    }
    __syncthreads();

    // ---- 4. dz = G W (wave w: d tiles w, w + 4, ..., two at a time), d E from the accumulators ---------------------
    {
        const int n_dt = (D + 15) >> 4;
        float zdz[4], nr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * kq + r;
            zdz[r] = (sZ[0][row] + sZ[1][row]) + (sZ[2][row] + sZ[3][row]);
            nr[r] = sN[row];
        }
        const float *ga = Gs + j * HW_LDG + kq;
        for (int dt = wave; dt < n_dt; dt += 8) {
            const bool two = dt + 4 < n_dt;                            // wave-uniform
            const int d0 = dt * 16 + j, d1 = (dt + 4) * 16 + j;
            const bool in0 = d0 < D, in1 = two && d1 < D;
            hw_f32x4 a0 = hw_f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0;
            if (p.w_lds) {
                for (int k0 = 0; k0 < C4; k0 += 16) {
                    float g[4], b0[4], b1[4];
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int c = k0 + 4 * s + kq;
                        g[s] = k0 + 4 * s < C4 ? ga[k0 + 4 * s] : 0.f;
                        b0[s] = (c < C && in0) ? Ws[c * ld + d0] : 0.f;
                        b1[s] = (c < C && in1) ? Ws[c * ld + d1] : 0.f;
                    }
#pragma unroll
                    for (int s = 0; s < 4; ++s) a0 = hw_mma(g[s], b0[s], a0);
                    if (two)
#pragma unroll
                        for (int s = 0; s < 4; ++s) a1 = hw_mma(g[s], b1[s], a1);
                }
            } else {
                for (int k0 = 0; k0 < C4; k0 += 16) {
                    float g[4], b0[4], b1[4];
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int c = k0 + 4 * s + kq;
                        g[s] = k0 + 4 * s < C4 ? ga[k0 + 4 * s] : 0.f;
                        b0[s] = (c < C && in0) ? p.W[(int64_t)c * D + d0] : 0.f;
                        b1[s] = (c < C && in1) ? p.W[(int64_t)c * D + d1] : 0.f;
                    }
#pragma unroll
                    for (int s = 0; s < 4; ++s) a0 = hw_mma(g[s], b0[s], a0);
                    if (two)
#pragma unroll
                        for (int s = 0; s < 4; ++s) a1 = hw_mma(g[s], b1[s], a1);
                }
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int d = h ? d1 : d0;
                if (!(h ? in1 : in0)) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 4 * kq + r, i = row0 + row;
                    if (i >= p.B) continue;
                    const float dz = h ? a1[r] : a0[r];
                    // padding rows: an explicit zero gradient
                    const float g = i < Bv ? (dz - zs[row * ld + d] * zdz[r]) / nr[r] : 0.f;
                    if (p.dE_dtype == GSAGE_BF16)
                        ((uint16_t *)p.dE)[(int64_t)i * p.ldd + d] = f32_to_bf16(g);
                    else
                        ((float *)p.dE)[(int64_t)i * p.ldd + d] = g;
                }
            }
        }
    }

    // ---- 5. the workgroup's partial row: dW^T tiles = z^T G (K = the 16 rows), db, loss ----------------------------
    float *out = p.partial + (int64_t)blockIdx.x * ((int64_t)C * D + C + 1);
    {
        const int n_dt = (D + 15) >> 4;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if (!tile_on[t]) continue;
            for (int dt = 0; dt < n_dt; dt += 2) {                  // two d tiles to a trip: two independent chains
                float za[2][4];
#pragma unroll
                for (int e = 0; e < 2; ++e)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int d = (dt + e) * 16 + j;
                        za[e][r] = d < D ? zs[(4 * kq + r) * ld + d] : 0.f;
                    }
                hw_f32x4 a[2] = {hw_f32x4{0.f, 0.f, 0.f, 0.f}, hw_f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int e = 0; e < 2; ++e) a[e] = hw_mma(za[e][r], G[t][r], a[e]);
                // lane: class cls[t], columns (dt + e) * 16 + 4 kq + r
                if (ok[t]) {
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        float *o = out + (int64_t)cls[t] * D + (dt + e) * 16 + 4 * kq;
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if ((dt + e) * 16 + 4 * kq + r < D) o[r] = a[e][r];
                    }
                }
            }
            float dbv = (G[t][0] + G[t][1]) + (G[t][2] + G[t][3]);
            dbv += __shfl_xor(dbv, 16, 64);
            dbv += __shfl_xor(dbv, 32, 64);
            if (kq == 0 && ok[t]) out[(int64_t)C * D + cls[t]] = dbv;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lossacc += __shfl_xor(lossacc, o, 64);
    if (lane == 0) sL[wave] = lossacc;
    __syncthreads();
    if (tid == 0) out[(int64_t)C * D + C] = (sL[0] + sL[1]) + (sL[2] + sL[3]);
}

// dW | db | loss = sums over the workgroups' partial rows, in buffer order per quarter (k_head_reduce of gsage_head.hip,
// with loss = (sum of the loss slots) / Bv and Bv read here, as the head reads it)
__global__ void __launch_bounds__(256)
k_head_wide_reduce(const float *__restrict__ partial, int32_t n_wg, int64_t width, int64_t cd, int32_t C,
                   float *__restrict__ dW, float *__restrict__ db, float *__restrict__ loss,
                   const int32_t *__restrict__ n_valid, const int64_t *__restrict__ batch_idx, int64_t n_batches, int32_t B)
{
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * 64 + lane;
    const int per = (n_wg + 3) / 4;
    const int g0 = q * per, g1 = min(n_wg, g0 + per);
    float s = 0.f;
    if (t < width) {
        int g = g0;
        for (; g + 8 <= g1; g += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = partial[(int64_t)(g + u) * width + t];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; g < g1; ++g) s += partial[(int64_t)g * width + t];
    }
    red[q][lane] = s;
    __syncthreads();
    if (q == 0 && t < width) {
        s = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
        if (t < cd) dW[t] = s;
        else if (t < cd + C) db[t - cd] = s;
        else if (loss) {
            const int64_t bq = batch_idx ? (int64_t)((uint64_t)*batch_idx % (uint64_t)n_batches) : 0;
            const int Bv = n_valid ? min(max(n_valid[bq], 1), B) : B;
            *loss = s / (float)Bv;
        }
    }
}

static size_t hw_lds_bytes(int C, int D, bool w_lds)
{
    const size_t ld = (size_t)((D + 3) & ~3) + 4;
    return sizeof(float) * (HW_ROWS * ld + HW_ROWS * HW_LDG + (w_lds ? (size_t)C * ld : 0));
}

}  // namespace gsage

using namespace gsage;

extern "C" {

int64_t gsage_head_wide_scratch(int32_t B, int32_t C, int32_t D)
{
    if (B < 1 || C < 1 || C > HW_CMAX || D < 1 || D > HW_DMAX) return -1;
    return ceil_div(B, HW_ROWS) * ((int64_t)C * D + C + 1);
}

int gsage_head_wide(const float *E, int64_t lde, const float *W, const float *bias, const void *targets, int task,
                    int64_t ldy, int32_t B, int32_t C, int32_t D, float *preds, void *dE, int dE_dtype, int64_t ldd,
                    float *dW, float *db, float *loss, float *scratch, const int64_t *batch_idx, int64_t n_batches,
                    void *stream)
{
    const int32_t *n_valid = take_head_n_valid();     // (consumed before any return path: never left for a later launch)
    GSAGE_REQUIRE(C >= 1 && C <= HW_CMAX, "head_wide: n_classes must be in [1, %d], not %d", HW_CMAX, (int)C);
    GSAGE_REQUIRE(D >= 1 && D <= HW_DMAX, "head_wide: the width must be in [1, %d], not %d", HW_DMAX, (int)D);
    GSAGE_REQUIRE(B >= 1, "head_wide: B must be at least 1, not %d", (int)B);
    GSAGE_REQUIRE(task == HW_CLASSIFICATION || task == HW_MULTILABEL,
                  "head_wide: task must be 0 (classification) or 1 (multilabel_classification), not %d", task);
    GSAGE_REQUIRE(lde >= D, "head_wide: lde = %lld must be at least D = %d", (long long)lde, (int)D);
    GSAGE_REQUIRE(!batch_idx || n_batches > 0, "head_wide: bad target queue");
    GSAGE_REQUIRE(E && W && bias && preds, "head_wide: null pointer");
    const bool forward_only = targets == nullptr && dE == nullptr;
    if (!forward_only) {
        GSAGE_REQUIRE(targets && dE, "head_wide: targets and dE go together (both NULL: forward only)");
        GSAGE_REQUIRE(scratch, "head_wide: a backward call needs scratch (gsage_head_wide_scratch floats)");
        GSAGE_REQUIRE(ldd >= D, "head_wide: ldd = %lld must be at least D = %d", (long long)ldd, (int)D);
        GSAGE_REQUIRE(task != HW_MULTILABEL || ldy >= C, "head_wide: ldy = %lld must be at least C = %d",
                      (long long)ldy, (int)C);
        GSAGE_REQUIRE(dE_dtype == GSAGE_BF16 || dE_dtype == GSAGE_F32, "head_wide: bad dE dtype");
        GSAGE_REQUIRE((dW == nullptr) == (db == nullptr), "head_wide: dW and db go together");
    }
    const bool w_lds = hw_lds_bytes(C, D, true) <= HW_LDS_DYN_MAX;
    const size_t lds = hw_lds_bytes(C, D, w_lds);
    GSAGE_REQUIRE(lds <= HW_LDS_DYN_MAX, "head_wide: the row tile does not fit the LDS (D = %d)", (int)D);

    HeadWideParams p;
    p.E = E; p.W = W; p.bias = bias; p.targets = targets; p.batch_idx = batch_idx; p.n_batches = n_batches;
    p.n_valid = n_valid; p.preds = preds; p.dE = dE; p.partial = scratch;
    p.lde = lde; p.ldd = ldd; p.ldy = ldy; p.B = B; p.C = C; p.D = D; p.task = task; p.dE_dtype = dE_dtype;
    p.w_lds = w_lds ? 1 : 0;
    p.ld = ((D + 3) & ~3) + 4;
    static bool raised = false;
    if (!raised && lds > 48 * 1024) {
        if (hipFuncSetAttribute((const void *)k_head_wide, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)HW_LDS_DYN_MAX) != hipSuccess) {
            (void)hipGetLastError();
            set_error("head_wide: cannot raise the dynamic LDS limit");
            return GSAGE_ELAUNCH;
        }
        raised = true;
    }
    const int n_wg = (int)ceil_div(B, HW_ROWS);
    launch(k_head_wide, dim3(n_wg), dim3(256), lds, (hipStream_t)stream, p);
    int rc = check_launch("head_wide");
    if (rc != GSAGE_OK || forward_only || dW == nullptr) return rc;    // caller reduces the partials
    const int64_t width = (int64_t)C * D + C + 1;
    launch(k_head_wide_reduce, dim3((unsigned)ceil_div(width, 64)), dim3(256), 0, (hipStream_t)stream,
           (const float *)scratch, n_wg, width, (int64_t)C * D, C, dW, db, loss, n_valid, batch_idx, n_batches, B);
    return check_launch("head_wide_reduce");
}

}  // extern "C"
