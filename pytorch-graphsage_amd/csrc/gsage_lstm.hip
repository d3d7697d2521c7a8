// gsage_lstm.hip -- the recurrence of the LSTM aggregator (reference nn_modules.py:259-286) and its backward.
//
// The aggregator keeps ONE time step of a batch_first LSTM over each node's n neighbour rows (the last position), so
// only the sequential part is new here; the input projection GX = rows W_ih^T + (b_ih + b_hh) is one K5 launch and the
// weight / input gradients are K5b / K5 launches on the dG this file writes (ops.py, _LSTMLast).
//
//   k_lstm_fwd   one workgroup (8 waves) owns a tile of TM sequences for all n steps: per step
//                gates_t = GX_t + h_{t-1} W_hh^T on the matrix cores, then the cell update in fp32.  h_{t-1} lives in
//                LDS (two buffers: the step's A operand and the one being written), c_{t-1} is read back from the
//                fp32 reserve.  W_hh is read from L2 in fragment order (k_lstm_pack): a wave's four 32 x 32 accumulators are the i, f, g, o gates of
//                the SAME 32 hidden units, so the cell update needs no exchange.  The activated gates overwrite GX
//                (the backward's reserve), c_t goes to cseq, h_t to row t + 1 of hprev (row t of hprev = the step's
//                INPUT state: dW_hh = dG^T hprev needs no shifted view) and h_{n-1} to the result.
//   k_lstm_bwd   t = n-1 .. 0: dh_t = [t == n-1] dh_last + dgates_{t+1} W_hh (matrix cores, dgates_{t+1} in LDS),
//                then dgates_t from the saved gates and c in fp32, written to dG and to LDS; dc_{t-1} = dc_t f_t.
// Hidden units are padded to whole 32-unit blocks with zero weights: a padded unit has c = h = 0 and a zero gradient.
// TM = 16 keeps half of each 32-row MFMA tile empty: twice the workgroups when M is small (gsage_lstm.hip:lstm_tile).
#include "gsage_mma_dev.h"

namespace gsage {

constexpr int LSTM_WAVES = 8;
constexpr int LSTM_THREADS = LSTM_WAVES * 64;
constexpr int LSTM_NMAX = 128;
constexpr int64_t LSTM_LDS_MAX = 160 * 1024;

template <typename T>
struct lstm_el;
template <>
struct lstm_el<uint16_t> {
    static constexpr int E = 8;            // elements per 16-byte lane chunk
    static constexpr bool FAST = true;     // bf16 mode: hardware exp / rcp (errors far below a bf16 ulp)
    __device__ static __forceinline__ float ld(uint16_t v) { return bf16_to_f32(v); }
    __device__ static __forceinline__ uint16_t cvt(float v) { return f32_to_bf16(v); }
};
template <>
struct lstm_el<float> {
    static constexpr int E = 4;
    static constexpr bool FAST = false;    // exact-fp32 mode: accurate expf
    __device__ static __forceinline__ float ld(float v) { return v; }
    __device__ static __forceinline__ float cvt(float v) { return v; }
};

template <bool FAST>
__device__ __forceinline__ float lstm_sigmoid(float x)
{
    if (FAST) return __builtin_amdgcn_rcpf(1.f + __expf(-x));
    return 1.f / (1.f + expf(-x));
}

template <bool FAST>
__device__ __forceinline__ float lstm_tanh(float x)
{
    // tanh(x) = sign(x) (1 - 2 / (exp(2|x|) + 1)); exp overflow gives exactly 1
    const float ax = fabsf(x);
    float t;
    if (FAST) t = 1.f - 2.f * __builtin_amdgcn_rcpf(__expf(2.f * ax) + 1.f);
    else t = 1.f - 2.f / (expf(2.f * ax) + 1.f);
    return x < 0.f ? -t : t;
}

// ---- W_hh in fragment order ----------------------------------------------------------------------------------------
// forward copy   F[ub][kc][g][lane][e] = W_hh[g H + ub 32 + (lane & 31)][kc 2E + (lane >> 5) E + e]
// backward copy  B[cb][kc][lane][e]    = W_hh[row(kc 2E + (lane >> 5) E + e)][cb 32 + (lane & 31)],
//                row(j) = (j / Hp) H + j % Hp: the reduction index of dh = dgates W_hh runs over (gate, padded unit)
// zero outside H x H.  One thread per 16-byte chunk of each copy.
template <typename T>
__global__ __launch_bounds__(256) void k_lstm_pack(const float *__restrict__ W, int64_t ldw, int H, int Hp,
                                                   T *__restrict__ F, T *__restrict__ B)
{
    constexpr int E = lstm_el<T>::E;
    const int64_t chunks = 4 * (int64_t)Hp * Hp / E;
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= chunks) return;
    const int lane = (int)(c & 63);
    const int lr = lane & 31, lh = lane >> 5;
    {
        const int KC = Hp / (2 * E);
        int64_t r = c >> 6;
        const int g = (int)(r & 3);
        r >>= 2;
        const int kc = (int)(r % KC);
        const int ub = (int)(r / KC);
        const int unit = ub * 32 + lr;
        const int k0 = kc * 2 * E + lh * E;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const bool in = unit < H && k0 + e < H;
            F[c * E + e] = lstm_el<T>::cvt(in ? W[((int64_t)g * H + unit) * ldw + k0 + e] : 0.f);
        }
    }
    {
        const int KCB = 4 * Hp / (2 * E);
        const int64_t r = c >> 6;
        const int kc = (int)(r % KCB);
        const int cb = (int)(r / KCB);
        const int col = cb * 32 + lr;
        const int j0 = kc * 2 * E + lh * E;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int j = j0 + e;
            const int g = j / Hp, u = j % Hp;
            const bool in = u < H && col < H;
            B[c * E + e] = lstm_el<T>::cvt(in ? W[((int64_t)g * H + u) * ldw + col] : 0.f);
        }
    }
}

// ---- forward -------------------------------------------------------------------------------------------------------
template <typename T>
struct LstmFwd {
    T *gates;             // [M n, ldg]: GX in, activated gates out (columns g H + u)
    int64_t ldg;
    const vec16 *Wp;      // forward copy of k_lstm_pack (unused when n == 1)
    int64_t M;
    int32_t n, H, Hp, tm;   // tm: sequences per workgroup, 16 or 32
    float *cseq;          // [M n, H]
    T *hprev;             // [M n, ldh]: row (m, t + 1) = h_t; row (m, 0) is left to the caller (zero)
    int64_t ldh;
    T *out;               // [M, ldo]: h_{n-1}
    int64_t ldo;
};

// accumulator register q of a 32 x 32 MFMA tile: row (q / 4) 8 + (lane / 32) 4 + q % 4, column lane % 32.  Every global
// address below is a wave-uniform base (tile, step, unit block, q's row) plus ONE 32-bit lane offset per array.
__device__ __forceinline__ constexpr int lstm_qrow(int q) { return (q >> 2) * 8 + (q & 3); }

template <typename T>
__global__ __launch_bounds__(LSTM_THREADS) void k_lstm_fwd(LstmFwd<T> p)
{
    using el = lstm_el<T>;
    constexpr int E = el::E;
    constexpr bool FAST = el::FAST;
    extern __shared__ vec16 lstm_smem[];
    T *hbuf = reinterpret_cast<T *>(lstm_smem);
    const int Hp = p.Hp, H = p.H, n = p.n, TM = p.tm;
    const int ldl = Hp + E;                       // row pitch: 16 bytes past a multiple of 64
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 31, lh = lane >> 5;
    const int nb = Hp >> 5, KC = Hp / (2 * E);
    const int64_t m0 = (int64_t)blockIdx.x * TM;
    const int left = (int)(p.M - m0 < TM ? p.M - m0 : TM);          // live rows of this tile
    const int64_t rs_g = (int64_t)n * p.ldg, rs_c = (int64_t)n * H, rs_h = (int64_t)n * p.ldh;
    const uint32_t vo_g = (uint32_t)(lh * 4 * rs_g + lr), vo_c = (uint32_t)(lh * 4 * rs_c + lr);
    const uint32_t vo_h = (uint32_t)(lh * 4 * rs_h + lr), vo_o = (uint32_t)(lh * 4 * p.ldo + lr);

    for (int t = 0; t < n; ++t) {
        const T *hin = hbuf + (size_t)(t & 1) * TM * ldl;
        T *hout = hbuf + (size_t)((t + 1) & 1) * TM * ldl;
#pragma unroll 1
        for (int ub = wave; ub < nb; ub += LSTM_WAVES) {        // (wave-uniform)
            const bool ulive = ub * 32 + lr < H;
            T *g_t = p.gates + (m0 * n + t) * p.ldg + ub * 32;
            float *c_t = p.cseq + (m0 * n + t) * H + ub * 32;
            f32x16_t acc[4];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const bool valid = lstm_qrow(q) + lh * 4 < left && ulive;
                const T *src = g_t + lstm_qrow(q) * rs_g;
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g][q] = valid ? el::ld(src[(size_t)(vo_g + (uint32_t)(g * H))]) : 0.f;
            }
            if (t > 0) {                          // (h_{-1} = 0: no recurrent term in the first step)
                const T *arow = hin + (size_t)(lr & (TM - 1)) * ldl + lh * E;
                const vec16 *wp = p.Wp + (size_t)ub * KC * 4 * 64 + lane;
                for (int kc = 0; kc < KC; ++kc) {
                    const vec16 a = *reinterpret_cast<const vec16 *>(arow + kc * 2 * E);
#pragma unroll
                    for (int g = 0; g < 4; ++g) mma_chunk<T>::run(a, wp[(size_t)(kc * 4 + g) * 64], acc[g]);
                }
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                if ((q >> 2) * 8 >= TM) continue; // (wave-uniform: the empty half of a 16-row tile)
                const int row = lstm_qrow(q) + lh * 4;
                const bool valid = row < left && ulive;
                const float ig = lstm_sigmoid<FAST>(acc[0][q]);
                const float fg = lstm_sigmoid<FAST>(acc[1][q]);
                const float gg = lstm_tanh<FAST>(acc[2][q]);
                const float og = lstm_sigmoid<FAST>(acc[3][q]);
                // c_{t-1} comes back from the fp32 reserve this lane wrote a step ago (exact: no rounding on the way)
                float *cq = c_t + lstm_qrow(q) * rs_c;
                const float cprev = valid && t > 0 ? (cq - H)[(size_t)vo_c] : 0.f;
                const float cv = fg * cprev + ig * gg;
                const T hv = el::cvt(og * lstm_tanh<FAST>(cv));
                hout[(size_t)row * ldl + ub * 32 + lr] = hv;
                if (valid) {
                    T *dst = g_t + lstm_qrow(q) * rs_g;
                    dst[(size_t)vo_g] = el::cvt(ig);
                    dst[(size_t)(vo_g + (uint32_t)H)] = el::cvt(fg);
                    dst[(size_t)(vo_g + (uint32_t)(2 * H))] = el::cvt(gg);
                    dst[(size_t)(vo_g + (uint32_t)(3 * H))] = el::cvt(og);
                    cq[(size_t)vo_c] = cv;
                    if (t + 1 < n) (p.hprev + (m0 * n + t + 1) * p.ldh + ub * 32 + lstm_qrow(q) * rs_h)[(size_t)vo_h] = hv;
                    else (p.out + (m0 + lstm_qrow(q)) * p.ldo + ub * 32)[(size_t)vo_o] = hv;
                }
            }
        }
        __syncthreads();
    }
}

// ---- backward ------------------------------------------------------------------------------------------------------
template <typename T>
struct LstmBwd {
    const T *gates;       // [M n, ldg] activated gates (forward reserve)
    int64_t ldg;
    const vec16 *Wp;      // backward copy of k_lstm_pack (unused when n == 1)
    int64_t M;
    int32_t n, H, Hp, tm;   // tm: sequences per workgroup, 16 or 32
    const float *cseq;    // [M n, H]
    const float *dh;      // [M, lddh] gradient of h_{n-1}
    int64_t lddh;
    T *dG;                // [M n, lddg] gradient of the pre-activation gates
    int64_t lddg;
    float *carry;         // [M, 2 H] scratch: dh_t | dc_t f_t between two steps (each element stays with one lane)
};

template <typename T>
__global__ __launch_bounds__(LSTM_THREADS) void k_lstm_bwd(LstmBwd<T> p)
{
    using el = lstm_el<T>;
    constexpr int E = el::E;
    constexpr bool FAST = el::FAST;
    extern __shared__ vec16 lstm_smem[];
    T *dgl = reinterpret_cast<T *>(lstm_smem);    // [TM][4 Hp + E]: dgates of the step just done, column g Hp + u
    const int Hp = p.Hp, H = p.H, n = p.n, TM = p.tm;
    const int ldl = 4 * Hp + E;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 31, lh = lane >> 5;
    const int nb = Hp >> 5, KCB = 4 * Hp / (2 * E);
    const int64_t m0 = (int64_t)blockIdx.x * TM;
    const int left = (int)(p.M - m0 < TM ? p.M - m0 : TM);
    const int64_t rs_g = (int64_t)n * p.ldg, rs_c = (int64_t)n * H, rs_d = (int64_t)n * p.lddg;
    const uint32_t vo_g = (uint32_t)(lh * 4 * rs_g + lr), vo_c = (uint32_t)(lh * 4 * rs_c + lr);
    const uint32_t vo_d = (uint32_t)(lh * 4 * rs_d + lr), vo_h = (uint32_t)(lh * 4 * p.lddh + lr);
    const uint32_t vo_r = (uint32_t)(lh * 4 * 2 * H + lr);

    for (int t = n - 1; t >= 0; --t) {
        const bool last = t == n - 1;
        if (!last) {
#pragma unroll 1
            for (int ub = wave; ub < nb; ub += LSTM_WAVES) {
                const bool ulive = ub * 32 + lr < H;
                f32x16_t acc;
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[q] = 0.f;
                const T *arow = dgl + (size_t)(lr & (TM - 1)) * ldl + lh * E;
                const vec16 *wp = p.Wp + (size_t)ub * KCB * 64 + lane;
                for (int kc = 0; kc < KCB; ++kc) {
                    const vec16 a = *reinterpret_cast<const vec16 *>(arow + kc * 2 * E);
                    mma_chunk<T>::run(a, wp[(size_t)kc * 64], acc);
                }
                float *cr = p.carry + m0 * 2 * H + ub * 32;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    if ((q >> 2) * 8 >= TM) continue;
                    if (lstm_qrow(q) + lh * 4 < left && ulive) (cr + lstm_qrow(q) * 2 * H)[(size_t)vo_r] = acc[q];
                }
            }
            __syncthreads();                      // every wave has read dgates_{t+1}
        }
#pragma unroll 1
        for (int ub = wave; ub < nb; ub += LSTM_WAVES) {
            const bool ulive = ub * 32 + lr < H;
            const T *g_t = p.gates + (m0 * n + t) * p.ldg + ub * 32;
            const float *c_t = p.cseq + (m0 * n + t) * H + ub * 32;
            T *d_t = p.dG + (m0 * n + t) * p.lddg + ub * 32;
            float *cr = p.carry + m0 * 2 * H + ub * 32;
            const float *dh = p.dh + m0 * p.lddh + ub * 32;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                if ((q >> 2) * 8 >= TM) continue;
                const int row = lstm_qrow(q) + lh * 4;
                const bool valid = row < left && ulive;
                float di = 0.f, df = 0.f, dg = 0.f, dO = 0.f;
                if (valid) {
                    const T *src = g_t + lstm_qrow(q) * rs_g;
                    const float ig = el::ld(src[(size_t)vo_g]), fg = el::ld(src[(size_t)(vo_g + (uint32_t)H)]);
                    const float gg = el::ld(src[(size_t)(vo_g + (uint32_t)(2 * H))]);
                    const float og = el::ld(src[(size_t)(vo_g + (uint32_t)(3 * H))]);
                    const float *cq = c_t + lstm_qrow(q) * rs_c;
                    const float cv = cq[(size_t)vo_c];
                    const float cprev = t > 0 ? (cq - H)[(size_t)vo_c] : 0.f;
                    const float tc = lstm_tanh<FAST>(cv);
                    float *crq = cr + lstm_qrow(q) * 2 * H;
                    const float dhv = last ? (dh + lstm_qrow(q) * p.lddh)[(size_t)vo_h] : crq[(size_t)vo_r];
                    const float dc = (last ? 0.f : (crq + H)[(size_t)vo_r]) + dhv * og * (1.f - tc * tc);
                    dO = dhv * tc * og * (1.f - og);
                    di = dc * gg * ig * (1.f - ig);
                    df = dc * cprev * fg * (1.f - fg);
                    dg = dc * ig * (1.f - gg * gg);
                    if (t > 0) (crq + H)[(size_t)vo_r] = dc * fg;
                    T *dst = d_t + lstm_qrow(q) * rs_d;
                    dst[(size_t)vo_d] = el::cvt(di);
                    dst[(size_t)(vo_d + (uint32_t)H)] = el::cvt(df);
                    dst[(size_t)(vo_d + (uint32_t)(2 * H))] = el::cvt(dg);
                    dst[(size_t)(vo_d + (uint32_t)(3 * H))] = el::cvt(dO);
                }
                if (t > 0) {
                    T *l = dgl + (size_t)row * ldl + ub * 32 + lr;
                    l[0] = el::cvt(di);
                    l[Hp] = el::cvt(df);
                    l[2 * Hp] = el::cvt(dg);
                    l[3 * Hp] = el::cvt(dO);
                }
            }
        }
        __syncthreads();
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------
static inline int64_t lstm_hp(int64_t H) { return (H + 31) / 32 * 32; }
static inline int64_t lstm_hmax(int dtype) { return dtype == GSAGE_BF16 ? 1024 : 512; }
static inline int64_t lstm_lds(int dtype, int64_t Hp, int tm, bool bwd)
{
    const int64_t sz = dtype == GSAGE_BF16 ? 2 : 4, E = 16 / sz;
    return bwd ? tm * (4 * Hp + E) * sz : 2 * tm * (Hp + E) * sz;
}

// Sequence-tile height.  32 rows fill the MFMA tile and halve the W_hh traffic per sequence, but a workgroup is
// sequential over n steps: below one 32-row tile per CU the 16-row tile doubles the CUs at work (seed level, M = 512:
// 32 workgroups instead of 16), and it is the only one whose LDS image fits for the widest hidden sizes.
static int lstm_tile(int dtype, int64_t M, int64_t Hp, bool bwd)
{
    if (lstm_lds(dtype, Hp, 32, bwd) > LSTM_LDS_MAX) return 16;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
        else (void)hipGetLastError();
    } else (void)hipGetLastError();
    return ceil_div(M, 32) >= cus ? 32 : 16;
}

template <typename K>
static int lstm_raise_lds(K kernel, bool &done)
{
    if (done) return GSAGE_OK;
    if (hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LSTM_LDS_MAX) !=
        hipSuccess) {
        (void)hipGetLastError();
        set_error("lstm: cannot raise the dynamic LDS limit");
        return GSAGE_ELAUNCH;
    }
    done = true;
    return GSAGE_OK;
}

template <typename T>
static int lstm_launch_fwd(const LstmFwd<T> &p, size_t lds, hipStream_t stream)
{
    static bool raised = false;
    const int rc = lstm_raise_lds(k_lstm_fwd<T>, raised);
    if (rc != GSAGE_OK) return rc;
    launch(k_lstm_fwd<T>, dim3((unsigned)ceil_div(p.M, p.tm)), dim3(LSTM_THREADS), lds, stream, p);
    return GSAGE_OK;
}

template <typename T>
static int lstm_launch_bwd(const LstmBwd<T> &p, size_t lds, hipStream_t stream)
{
    static bool raised = false;
    const int rc = lstm_raise_lds(k_lstm_bwd<T>, raised);
    if (rc != GSAGE_OK) return rc;
    launch(k_lstm_bwd<T>, dim3((unsigned)ceil_div(p.M, p.tm)), dim3(LSTM_THREADS), lds, stream, p);
    return GSAGE_OK;
}

}  // namespace gsage

using namespace gsage;

extern "C" int gsage_lstm_ok(int dtype, int64_t H, int32_t n)
{
    if (dtype != GSAGE_BF16 && dtype != GSAGE_F32) return 0;
    return H >= 1 && H <= lstm_hmax(dtype) && n >= 1 && n <= LSTM_NMAX ? 1 : 0;
}

extern "C" int gsage_lstm_tile(int dtype, int64_t M, int64_t H, int backward)
{
    if (!gsage_lstm_ok(dtype, H, 1) || M < 0) return 0;
    return lstm_tile(dtype, M, lstm_hp(H), backward != 0);
}

extern "C" int64_t gsage_lstm_packed_elems(int64_t H)
{
    const int64_t Hp = lstm_hp(H);
    return H >= 1 ? 8 * Hp * Hp : 0;
}

extern "C" int gsage_lstm_pack_whh(const float *W_hh, int64_t ldw, int64_t H, int dtype, void *Wp, void *stream)
{
    GSAGE_REQUIRE(gsage_lstm_ok(dtype, H, 1), "lstm_pack_whh: H must be in [1, %d] for this dtype (1024 bf16, 512 fp32)",
                  (int)lstm_hmax(dtype == GSAGE_BF16 ? GSAGE_BF16 : GSAGE_F32));
    GSAGE_REQUIRE(ldw >= H, "lstm_pack_whh: ldw < H");
    GSAGE_REQUIRE(W_hh && Wp, "lstm_pack_whh: null pointer");
    GSAGE_REQUIRE(((uintptr_t)Wp & 15) == 0, "lstm_pack_whh: Wp must be 16-byte aligned");
    const int64_t Hp = lstm_hp(H);
    const int64_t half = 4 * Hp * Hp;
    const int64_t chunks = half / (dtype == GSAGE_BF16 ? 8 : 4);
    if (dtype == GSAGE_BF16)
        launch(k_lstm_pack<uint16_t>, dim3((unsigned)ceil_div(chunks, 256)), dim3(256), 0, (hipStream_t)stream, W_hh, ldw,
               (int)H, (int)Hp, (uint16_t *)Wp, (uint16_t *)Wp + half);
    else
        launch(k_lstm_pack<float>, dim3((unsigned)ceil_div(chunks, 256)), dim3(256), 0, (hipStream_t)stream, W_hh, ldw,
               (int)H, (int)Hp, (float *)Wp, (float *)Wp + half);
    return check_launch("lstm_pack_whh");
}

extern "C" int gsage_lstm_fwd(void *gates, int dtype, int64_t ldg, const void *Wp, int64_t M, int32_t n, int64_t H,
                              float *cseq, void *hprev, int64_t ldh, void *out, int64_t ldo, void *stream)
{
    GSAGE_REQUIRE(dtype == GSAGE_BF16 || dtype == GSAGE_F32, "lstm_fwd: bad dtype %d", dtype);
    GSAGE_REQUIRE(n >= 1 && n <= LSTM_NMAX, "lstm_fwd: n = %d outside [1, %d]", (int)n, LSTM_NMAX);
    GSAGE_REQUIRE(H >= 1 && H <= lstm_hmax(dtype), "lstm_fwd: H = %lld outside [1, %d] (1024 bf16, 512 fp32)",
                  (long long)H, (int)lstm_hmax(dtype));
    GSAGE_REQUIRE(M >= 0 && M * n < ((int64_t)1 << 40), "lstm_fwd: bad M");
    GSAGE_REQUIRE(ldg >= 4 * H && ldg <= (1 << 20), "lstm_fwd: ldg outside [4 H, 2^20]");
    GSAGE_REQUIRE(ldo >= H && ldo <= (1 << 20), "lstm_fwd: ldo outside [H, 2^20]");
    GSAGE_REQUIRE(n == 1 || (ldh >= H && ldh <= (1 << 20)), "lstm_fwd: ldh outside [H, 2^20]");
    if (M == 0) return GSAGE_OK;
    GSAGE_REQUIRE(gates && cseq && out && (n == 1 || (Wp && hprev)), "lstm_fwd: null pointer");
    GSAGE_REQUIRE(((uintptr_t)Wp & 15) == 0, "lstm_fwd: Wp must be 16-byte aligned");
    const int64_t Hp = lstm_hp(H);
    const int tm = lstm_tile(dtype, M, Hp, false);
    const size_t lds = (size_t)lstm_lds(dtype, Hp, tm, false);
    int rc;
    if (dtype == GSAGE_BF16) {
        LstmFwd<uint16_t> p = {(uint16_t *)gates, ldg, (const vec16 *)Wp, M, n, (int32_t)H, (int32_t)Hp, tm, cseq,
                               (uint16_t *)hprev, ldh, (uint16_t *)out, ldo};
        rc = lstm_launch_fwd<uint16_t>(p, lds, (hipStream_t)stream);
    } else {
        LstmFwd<float> p = {(float *)gates, ldg, (const vec16 *)Wp, M, n, (int32_t)H, (int32_t)Hp, tm, cseq,
                            (float *)hprev, ldh, (float *)out, ldo};
        rc = lstm_launch_fwd<float>(p, lds, (hipStream_t)stream);
    }
    if (rc != GSAGE_OK) return rc;
    return check_launch("lstm_fwd");
}

extern "C" int gsage_lstm_bwd(const void *gates, int dtype, int64_t ldg, const void *Wp, int64_t M, int32_t n, int64_t H,
                              const float *cseq, const float *dh, int64_t lddh, void *dG, int64_t lddg, float *carry,
                              void *stream)
{
    GSAGE_REQUIRE(dtype == GSAGE_BF16 || dtype == GSAGE_F32, "lstm_bwd: bad dtype %d", dtype);
    GSAGE_REQUIRE(n >= 1 && n <= LSTM_NMAX, "lstm_bwd: n = %d outside [1, %d]", (int)n, LSTM_NMAX);
    GSAGE_REQUIRE(H >= 1 && H <= lstm_hmax(dtype), "lstm_bwd: H = %lld outside [1, %d] (1024 bf16, 512 fp32)",
                  (long long)H, (int)lstm_hmax(dtype));
    GSAGE_REQUIRE(M >= 0 && M * n < ((int64_t)1 << 40), "lstm_bwd: bad M");
    GSAGE_REQUIRE(ldg >= 4 * H && lddg >= 4 * H && ldg <= (1 << 20) && lddg <= (1 << 20),
                  "lstm_bwd: ldg / lddg outside [4 H, 2^20]");
    GSAGE_REQUIRE(lddh >= H && lddh <= (1 << 20), "lstm_bwd: lddh outside [H, 2^20]");
    if (M == 0) return GSAGE_OK;
    GSAGE_REQUIRE(gates && cseq && dh && dG && (n == 1 || (Wp && carry)), "lstm_bwd: null pointer");
    GSAGE_REQUIRE(((uintptr_t)Wp & 15) == 0, "lstm_bwd: Wp must be 16-byte aligned");
    const int64_t Hp = lstm_hp(H);
    const int tm = lstm_tile(dtype, M, Hp, true);
    const size_t lds = (size_t)lstm_lds(dtype, Hp, tm, true);
    int rc;
    if (dtype == GSAGE_BF16) {
        LstmBwd<uint16_t> p = {(const uint16_t *)gates, ldg, (const vec16 *)Wp, M, n, (int32_t)H, (int32_t)Hp, tm, cseq, dh,
                               lddh, (uint16_t *)dG, lddg, carry};
        rc = lstm_launch_bwd<uint16_t>(p, lds, (hipStream_t)stream);
    } else {
        LstmBwd<float> p = {(const float *)gates, ldg, (const vec16 *)Wp, M, n, (int32_t)H, (int32_t)Hp, tm, cseq, dh, lddh,
                            (float *)dG, lddg, carry};
        rc = lstm_launch_bwd<float>(p, lds, (hipStream_t)stream);
    }
    if (rc != GSAGE_OK) return rc;
    return check_launch("lstm_bwd");
}
