// gsage_fp8.hip -- the quantiser of the FP8 feature table (gfx950; format: include/gsage.h, "FP8 feature table").
//
// An fp32 / bf16 table becomes one OCP e4m3fn byte per element plus one power-of-two fp32 scale per column, in two
// passes over the table: the column maxima, then the encoding.  A one-off (tables are fixed inputs): both passes are
// plain streaming kernels, element loads coalesced across a wave's lanes, no LDS.  The gathers that READ the result
// are in gsage_gather.hip.
#include "gsage_common.h"

namespace gsage {

template <typename T> __device__ __forceinline__ float load_f32(const T *p);
template <> __device__ __forceinline__ float load_f32<float>(const float *p) { return *p; }
template <> __device__ __forceinline__ float load_f32<uint16_t>(const uint16_t *p) { return bf16_to_f32(*p); }

// what the quantiser sees of an input: NaN counts as 0, anything beyond +-2^127 (the infinities too) as +-2^127 --
// the largest magnitude whose decoded value e4m3 * 2^k is still a finite fp32 / bf16 number for every code
__device__ __forceinline__ float fp8_sanitize(float x)
{
    if (x != x) return 0.f;
    return fminf(fmaxf(x, -0x1p127f), 0x1p127f);
}

// pass 1: amax_bits[c] = max_r bits(|x[r, c]|) -- non-negative floats order like their bit patterns, and an integer
// max does not depend on the order of its operands: deterministic.  Workgroup = 64 columns x 4 row lanes; grid.y
// row slabs.
template <typename T>
__global__ void __launch_bounds__(256)
k_fp8_colmax(const T *__restrict__ x, int64_t ld, int64_t n_rows, int32_t D, uint32_t *__restrict__ amax_bits)
{
    const int32_t c = (int32_t)blockIdx.x * 64 + (threadIdx.x & 63);
    if (c >= D) return;
    const int64_t step = (int64_t)gridDim.y * 4;
    int64_t r = (int64_t)blockIdx.y * 4 + (threadIdx.x >> 6);
    float m = 0.f;
    for (; r + 3 * step < n_rows; r += 4 * step) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = load_f32(x + (r + u * step) * ld + c);
#pragma unroll
        for (int u = 0; u < 4; ++u) m = fmaxf(m, fabsf(fp8_sanitize(v[u])));
    }
    for (; r < n_rows; r += step) m = fmaxf(m, fabsf(fp8_sanitize(load_f32(x + r * ld + c))));
    if (m > 0.f) atomicMax(amax_bits + c, __float_as_uint(m));
}

// between the passes: amax bits -> scale, in place.  amax = 1.m x 2^e: s = 2^(e-8) when 1.m <= 1.75 (448 = 1.75 x 2^8),
// else 2^(e-7); never below 2^-126 (s and 1/s both stay normal numbers); 1.0 for an all-zero or padding column.
__global__ void __launch_bounds__(256)
k_fp8_scale(float *__restrict__ scale, int32_t D, int32_t ld_q)
{
    const int32_t c = (int32_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ld_q) return;
    const uint32_t b = c < D ? __float_as_uint(scale[c]) : 0u;
    float s = 1.f;
    if (b != 0u) {
        int k = (int)(b >> 23) - 127 - ((b & 0x7fffffu) <= 0x600000u ? 8 : 7);
        k = k < -126 ? -126 : k;
        s = __uint_as_float((uint32_t)(k + 127) << 23);
    }
    scale[c] = s;
}

// pass 2: one work item = the four bytes of columns 4g .. 4g+3 of one row (pad columns: zero bytes).  x / s is
// exact (s a power of two), the hardware conversion rounds to nearest even; the clamp keeps it away from the NaN
// encodings whatever the hardware does above 448.
template <typename T>
__global__ void __launch_bounds__(256)
k_fp8_encode(const T *__restrict__ x, int64_t ld, int64_t n_rows, int32_t D, const float *__restrict__ scale,
             uint32_t *__restrict__ q, int32_t words)
{
    const int64_t total = n_rows * (int64_t)words;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
        const int64_t r = t / words;
        const int32_t c0 = (int32_t)(t - r * words) * 4;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[e] = 0.f;
            if (c0 + e < D) {
                const float inv = 1.f / scale[c0 + e];            // exact: a power of two in [2^-126, 2^119]
                v[e] = fminf(fmaxf(fp8_sanitize(load_f32(x + r * ld + c0 + e)) * inv, -448.f), 448.f);
            }
        }
        int w = 0;
        w = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], w, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], w, true);
        q[t] = (uint32_t)w;
    }
}

template <typename T>
static int quantize(const void *table, int64_t ld, int64_t n_rows, int64_t D, void *table_q, int64_t ld_q,
                    float *scale, hipStream_t s)
{
    if (hipMemsetAsync(scale, 0, (size_t)ld_q * sizeof(float), s) != hipSuccess) {
        set_error("quantize_fp8: memset failed: %s", hipGetErrorString(hipGetLastError()));
        return GSAGE_ELAUNCH;
    }
    if (n_rows > 0) {
        int64_t slabs = ceil_div(n_rows, 4 * 16);                  // >= 16 rows per lane before another slab
        slabs = slabs > 1024 ? 1024 : slabs;
        launch(k_fp8_colmax<T>, dim3((unsigned)ceil_div(D, 64), (unsigned)slabs), dim3(256), 0, s,
               (const T *)table, ld, n_rows, (int32_t)D, (uint32_t *)scale);
        int rc = check_launch("quantize_fp8 (column maxima)");
        if (rc != GSAGE_OK) return rc;
    }
    launch(k_fp8_scale, dim3((unsigned)ceil_div(ld_q, 256)), dim3(256), 0, s, scale, (int32_t)D, (int32_t)ld_q);
    int rc = check_launch("quantize_fp8 (scales)");
    if (rc != GSAGE_OK || n_rows == 0) return rc;
    const int32_t words = (int32_t)(ld_q / 4);
    int64_t blocks = ceil_div(n_rows * words, 256);
    blocks = blocks > 65536 ? 65536 : blocks;
    launch(k_fp8_encode<T>, dim3((unsigned)blocks), dim3(256), 0, s, (const T *)table, ld, n_rows, (int32_t)D,
           (const float *)scale, (uint32_t *)table_q, words);
    return check_launch("quantize_fp8 (encode)");
}

}  // namespace gsage

using namespace gsage;

extern "C" int gsage_quantize_fp8(const void *table, int dtype, int64_t ld, int64_t n_rows, int64_t D, void *table_q,
                                  int64_t ld_q, float *scale, void *stream)
{
    GSAGE_REQUIRE(dtype == GSAGE_F32 || dtype == GSAGE_BF16, "quantize_fp8: the input table is fp32 or bf16 (got %d)", dtype);
    GSAGE_REQUIRE(n_rows >= 0 && D > 0 && D <= 0x7fffffff && ld >= D, "quantize_fp8: bad sizes");
    GSAGE_REQUIRE(ld_q % 16 == 0 && ld_q >= D && ld_q <= 0x7fffffff, "quantize_fp8: ld_q is a multiple of 16 bytes, >= D");
    GSAGE_REQUIRE(scale && ((uintptr_t)scale % 16) == 0, "quantize_fp8: scale must be 16-byte aligned");
    GSAGE_REQUIRE(n_rows == 0 || (table && table_q && ((uintptr_t)table_q % 16) == 0), "quantize_fp8: bad table pointers");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == GSAGE_F32) return quantize<float>(table, ld, n_rows, D, table_q, ld_q, scale, s);
    return quantize<uint16_t>(table, ld, n_rows, D, table_q, ld_q, scale, s);
}
