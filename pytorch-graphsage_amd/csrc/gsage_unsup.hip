// gsage_unsup.hip -- unsupervised GraphSAGE: the batch builder (random-walk positives, degree^0.75 negatives) in one
// launch and the skip-gram head, forward AND backward, in two.  Definitions: include/gsage.h, "Unsupervised GraphSAGE".
//
// The builder is latency, not bandwidth: a lane per seed walks a chain of at most 16 dependent (rowptr -> col) loads,
// a lane per negative walks a binary search of log2(n_rows) dependent loads; both roles share the launch.
//
// The weighted builder (steps drawn from a weighted adjacency's per-edge table) gives a walk to a WAVE: a step has to
// find the first table entry above its draw, and the 64 lanes probe 64 entries of the row per round trip -- one round
// for a row of at most 64 edges, ceil(log64(deg)) for a longer one -- instead of a lane's log2(deg) dependent probes.
//
// The temporal builder (include/gsage.h, "Temporal walks": every step among the edges before the walk's time) gives a
// walk to a TEAM of 16 lanes, the unit the temporal sampler's search is written for (gsage_temporal_dev.h): a step is the
// row's extent, two to three dependent search rounds and the col load.
//
// The head is k_head_ce (gsage_head.hip) with the normalised negatives in the role of fc.weight and the loss
// exchanged: B x Q x D = 512 x 20 x 256 is 2.6 MFLOP, so the cost is launches and dependent phases, not flops.  A
// workgroup keeps its 16 normalised seed rows in LDS, streams the negatives' rows from L2 (64 x 1024 floats do not fit
// beside them), and leaves one partial of d z_neg per workgroup for the second launch to sum in a fixed order.
#include "gsage_common.h"
#include "gsage_temporal_dev.h"
#include "gsage_walk_dev.h"
#include "gsage_weighted_dev.h"

namespace gsage {

constexpr uint32_t UNSUP_TAG_LEN = 0x4C000000u;     // walk length
constexpr uint32_t UNSUP_TAG_STEP = 0x53000000u;    // | (step >> 2): walk steps, four to a Philox block
constexpr uint32_t UNSUP_TAG_NEG = 0x4E000000u;     // negatives
constexpr uint32_t UNSUP_TAG_WSTEP = 0x5A000000u;   // | (step >> 1): weighted walk steps, two to a Philox block
constexpr uint32_t UNSUP_TAG_BIAS = 0x42000000u;    // | (step << 8) | round: a biased step's rounds, a block each
constexpr uint32_t UNSUP_TAG_TSTEP = 0x56000000u;   // | (step >> 2): temporal walk steps, four to a Philox block
constexpr int UNSUP_WALK_MAX = 16;

struct UnsupParams {
    const int64_t *rowptr;
    const int32_t *col;
    const int64_t *seeds;
    const double *cdf;
    const uint64_t *edge_cdf;                           // the weighted builder's per-edge table (else unused)
    const uint64_t *call_ctr;
    int64_t *ids;
    float *pair_w;
    int32_t *err_flag;
    int64_t n_rows, B, Q;
    uint64_t call_base, g0;
    double cdf_total;
    uint32_t seed_lo, seed_hi;
    int32_t walk_len, walk_blocks;
};

__device__ __forceinline__ philox4 unsup_philox(const UnsupParams &p, uint64_t c, uint64_t call, uint32_t tag)
{
    return philox_block(c, call, p.seed_lo, p.seed_hi ^ tag);
}

// the negatives' role of both builders: the workgroups behind the walk workgroups, a lane per negative
__device__ __forceinline__ void unsup_negative(const UnsupParams &p, uint64_t call)
{
    const int64_t q = (int64_t)((int)blockIdx.x - p.walk_blocks) * 256 + threadIdx.x;
    if (q >= p.Q) return;
    const philox4 r = unsup_philox(p, (uint64_t)q, call, UNSUP_TAG_NEG);
    const uint64_t u53 = ((uint64_t)r.v[0] << 21) | (uint64_t)(r.v[1] >> 11);
    const double x = ((double)u53 * 0x1p-53) * p.cdf_total;
    int64_t lo = 0, hi = p.n_rows - 1;                          // first i with cdf[i] > x, clamped to the last row
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (p.cdf[mid] > x) hi = mid; else lo = mid + 1;
    }
    p.ids[2 * p.B + q] = lo;
}

// ---- the frame of the four batch builders: the role split, the walk's length, the walk's record ------------------
// Blocks [0, walk_blocks) build walks, the rest draw negatives.  true: this workgroup walks; false: its lanes were
// the negatives' and are done.
__device__ __forceinline__ bool unsup_walk_role(const UnsupParams &p, uint64_t call)
{
    if ((int)blockIdx.x < p.walk_blocks) return true;
    unsup_negative(p, call);
    return false;
}

// steps of walk g: uniform in 1 .. walk_len
__device__ __forceinline__ int unsup_walk_steps(const UnsupParams &p, uint64_t g, uint64_t call)
{
    return 1 + (int)philox_below(unsup_philox(p, g, call, UNSUP_TAG_LEN).v[0], (uint32_t)p.walk_len);
}

// the three words of walk i: seed s, positive v (a walk that ends on its seed is no pair)
__device__ __forceinline__ void unsup_store(const UnsupParams &p, int64_t i, int64_t s, int64_t v)
{
    p.ids[i] = s;
    p.ids[p.B + i] = v;
    p.pair_w[i] = v == s ? 0.f : 1.f;
}

// ... of a seed outside the graph: the flag, and 0, 0, 0.f
__device__ __forceinline__ void unsup_store_bad(const UnsupParams &p, int64_t i)
{
    if (p.err_flag) *p.err_flag = 1;
    unsup_store(p, i, 0, 0);
}

// walk blocks: a lane per seed
__global__ void __launch_bounds__(256)
k_unsup_batch(const UnsupParams p)
{
    const uint64_t call = p.call_base + (p.call_ctr ? *p.call_ctr : 0ull);
    if (!unsup_walk_role(p, call)) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.B) return;
    const int64_t s = p.seeds[i];
    const uint64_t g = p.g0 + (uint64_t)i;
    if ((uint64_t)s >= (uint64_t)p.n_rows) {
        unsup_store_bad(p, i);
        return;
    }
    const int t = unsup_walk_steps(p, g, call);
    int64_t v = s;
    philox4 r = {};
    for (int j = 0; j < t; ++j) {
        const int64_t beg = p.rowptr[v];
        const int64_t deg = p.rowptr[v + 1] - beg;
        if (deg <= 0) break;
        if ((j & 3) == 0) r = unsup_philox(p, g, call, UNSUP_TAG_STEP | (uint32_t)(j >> 2));
        v = (int64_t)p.col[beg + (int64_t)philox_below_deg(philox_pick(r, j & 3), deg)];
        if ((uint64_t)v >= (uint64_t)p.n_rows) {
            if (p.err_flag) *p.err_flag = 1;
            v = 0;
            break;
        }
    }
    unsup_store(p, i, s, v);
}


// ---- weighted walks: a wave per walk ---------------------------------------------------------------------------------
__device__ __forceinline__ int64_t wave_uniform(int64_t x)             // a value every lane holds, made provably so
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)x >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ uint64_t wave_lane_u64(uint64_t x, int src)   // lane src's x
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)x, src, 64);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(x >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}

// One weighted step by the whole wave (beg, end, r64 wave-uniform, end > beg): T = cdf[end - 1]; T == 0 -> -1 (no
// drawable edge); else the first edge e of the row with cdf[e] > x, x = (r64 * T) >> 64.  cdf is non-decreasing inside
// a row and cdf[end - 1] = T > x, so the answer exists.  A range of at most 64 entries: a lane per entry, one ballot.
// A longer range [lo, hi] with cdf[hi] > x: lane l probes lo + floor((hi - lo)(l + 1) / 64) -- ascending, lane 63 is hi
// itself, which in the first round is the row's last entry and yields T -- and the first probe above x bounds the
// sixty-fourth of the range that holds the answer.
__device__ __forceinline__ int64_t wave_cdf_step(const uint64_t *__restrict__ cdf, int64_t beg, int64_t end, uint64_t r64,
                                                 int lane)
{
    int64_t lo = beg, hi = end - 1;
    uint64_t x = 0;
    bool have_x = false;
    while (hi - lo >= 64) {
        const int64_t span = hi - lo;
        const uint64_t c = cdf[lo + ((span * (int64_t)(lane + 1)) >> 6)];
        if (!have_x) {
            const uint64_t T = wave_lane_u64(c, 63);
            if (T == 0) return -1;
            x = __umul64hi(r64, T);
            have_x = true;
        }
        const int k = __ffsll((unsigned long long)__ballot(c > x)) - 1;       // (lane 63's probe is above x: k >= 0)
        hi = lo + ((span * (int64_t)(k + 1)) >> 6);
        if (k > 0) lo = lo + ((span * (int64_t)k) >> 6) + 1;
    }
    const int n = (int)(hi - lo) + 1;                                          // 1 .. 64 entries left
    const uint64_t c = lane < n ? cdf[lo + lane] : 0ull;
    if (!have_x) {
        const uint64_t T = wave_lane_u64(c, n - 1);
        if (T == 0) return -1;
        x = __umul64hi(r64, T);
    }
    return lo + (__ffsll((unsigned long long)__ballot(lane < n && c > x)) - 1);
}

// walk blocks: a wave per seed (four to a workgroup), every branch wave-uniform.  Lane 0 writes the walk's three words.
__global__ void __launch_bounds__(256)
k_unsup_batch_weighted(const UnsupParams p)
{
    const uint64_t call = p.call_base + (p.call_ctr ? *p.call_ctr : 0ull);
    if (!unsup_walk_role(p, call)) return;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (i >= p.B) return;
    const int64_t s = wave_uniform(p.seeds[i]);
    const uint64_t g = p.g0 + (uint64_t)i;
    if ((uint64_t)s >= (uint64_t)p.n_rows) {
        if (lane == 0) unsup_store_bad(p, i);
        return;
    }
    const int t = unsup_walk_steps(p, g, call);
    int64_t v = s;
    philox4 r = {};
    bool bad = false;
    for (int j = 0; j < t; ++j) {
        const int64_t beg = wave_uniform(p.rowptr[v]), end = wave_uniform(p.rowptr[v + 1]);
        if (end <= beg) break;
        if ((j & 1) == 0) r = unsup_philox(p, g, call, UNSUP_TAG_WSTEP | (uint32_t)(j >> 1));
        const int64_t e = wave_uniform(wave_cdf_step(p.edge_cdf, beg, end, philox_r64(r, (j & 1) != 0), lane));
        if (e < 0) break;
        v = wave_uniform((int64_t)p.col[e]);
        if ((uint64_t)v >= (uint64_t)p.n_rows) {
            bad = true;
            v = 0;
            break;
        }
    }
    if (lane == 0) {
        if (bad && p.err_flag) *p.err_flag = 1;
        unsup_store(p, i, s, v);
    }
}

// ---- biased walks: second-order steps by rejection, a wave per walk -------------------------------------------------------
struct UnsupBiasedParams {
    UnsupParams u;
    WalkBias b;
};

// include/gsage.h, "Biased walks".  blocks [0, walk_blocks): a wave per seed (four to a workgroup), every value that
// steers a branch made wave-uniform;  the rest: a lane per negative.  edge_cdf == NULL: uniform proposals.  Round 0
// proposes with the word the first-order builder would use; the acceptance word is looked at before the row of the
// previous node is, and most rounds never need that row.  Lane 0 writes the walk's three words.
__global__ void __launch_bounds__(256)
k_unsup_batch_biased(const UnsupBiasedParams bp)
{
    const UnsupParams &p = bp.u;
    const WalkBias &b = bp.b;
    const uint64_t call = p.call_base + (p.call_ctr ? *p.call_ctr : 0ull);
    if (!unsup_walk_role(p, call)) return;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (i >= p.B) return;
    const int64_t s = wave_uniform(p.seeds[i]);
    const uint64_t g = p.g0 + (uint64_t)i;
    if ((uint64_t)s >= (uint64_t)p.n_rows) {
        if (lane == 0) unsup_store_bad(p, i);
        return;
    }
    const int t = unsup_walk_steps(p, g, call);
    const bool weighted = p.edge_cdf != nullptr;
    int64_t v = s, prev = -1;
    philox4 r = {};
    bool bad = false;
    for (int j = 0; j < t; ++j) {
        const int64_t beg = wave_uniform(p.rowptr[v]), end = wave_uniform(p.rowptr[v + 1]);
        if (end <= beg) break;
        const int64_t deg = end - beg;
        if (weighted) {
            if ((j & 1) == 0) r = unsup_philox(p, g, call, UNSUP_TAG_WSTEP | (uint32_t)(j >> 1));
        } else {
            if ((j & 3) == 0) r = unsup_philox(p, g, call, UNSUP_TAG_STEP | (uint32_t)(j >> 2));
        }
        const bool second = j > 0 && !b.neutral;               // a previous node, and thresholds that can reject
        int64_t x = -1;
        bool dead = false;
        for (int k = 0; k < WALK_ROUNDS; ++k) {
            philox4 nb = {};
            if (second) nb = unsup_philox(p, g, call, UNSUP_TAG_BIAS | ((uint32_t)j << 8) | (uint32_t)k);
            int64_t e;
            if (weighted) {
                const uint64_t r64 = k == 0 ? philox_r64(r, (j & 1) != 0) : ((uint64_t)nb.v[0] << 32) | nb.v[1];
                e = wave_uniform(wave_cdf_step(p.edge_cdf, beg, end, r64, lane));
                if (e < 0) {                                   // T_v == 0: the walk ends at v
                    dead = true;
                    break;
                }
            } else {
                e = beg + (int64_t)philox_below_deg(k == 0 ? philox_pick(r, j & 3) : nb.v[0], deg);
            }
            x = wave_uniform((int64_t)p.col[e]);
            if ((uint64_t)x >= (uint64_t)p.n_rows) {
                bad = true;
                break;
            }
            if (!second) break;
            const uint32_t aw = __builtin_amdgcn_readfirstlane(nb.v[2]);
            int a = walk_accept_early(b, aw, x == prev);
            if (a < 0) {
                const int64_t tb = wave_uniform(p.rowptr[prev]), te = wave_uniform(p.rowptr[prev + 1]);
                a = walk_accept_scanned(b, aw, wave_row_contains(p.col, tb, te, (int32_t)x, lane)) ? 1 : 0;
            }
            if (a) break;                                      // (no round accepts: x is round 31's proposal)
        }
        if (dead) break;
        if (bad) {
            v = 0;
            break;
        }
        prev = v;
        v = x;
    }
    if (lane == 0) {
        if (bad && p.err_flag) *p.err_flag = 1;
        unsup_store(p, i, s, v);
    }
}

// ---- temporal walks: a team of 16 lanes per walk ---------------------------------------------------------------------
// include/gsage.h, "Temporal walks".  blocks [0, walk_blocks): a team per seed (sixteen to a workgroup, four to a wave);
// the rest: a lane per negative.  A step's eligible edges are the first cnt of the row, cnt found by the team with
// temporal_count (gsage_temporal_dev.h).  That search is WAVE-uniform around __ballot and the four walks of a wave have
// different lengths and end early at different steps, so the step loop runs until no team of the wave walks any more
// and a team that has finished passes deg = 0.  Every value a team steers by (v, tau, cnt, the Philox words) is
// computed by all of its 16 lanes from team-uniform inputs; lane 0 of the team writes the walk's five words.
struct UnsupTemporalParams {
    UnsupParams u;
    const int64_t *etime;
    const int64_t *times;
    const int32_t *n_valid;                             // live seeds (device word) or NULL: the negatives' times
    int64_t *out_times;
};

template <int INHERIT>
__global__ void __launch_bounds__(256)
k_unsup_batch_temporal(const UnsupTemporalParams tp)
{
    const UnsupParams &p = tp.u;
    const uint64_t call = p.call_base + (p.call_ctr ? *p.call_ctr : 0ull);
    if (!unsup_walk_role(p, call)) {                            // the negatives' times beside their ids
        const int64_t q = (int64_t)((int)blockIdx.x - p.walk_blocks) * 256 + threadIdx.x;
        if (q < p.Q) {
            const int64_t b = tp.n_valid ? (int64_t)min(max((int64_t)*tp.n_valid, (int64_t)1), p.B) : p.B;
            tp.out_times[2 * p.B + q] = tp.times[q % b];
        }
        return;
    }
    const uint32_t team = threadIdx.x / TEAM, l = threadIdx.x & (TEAM - 1);
    const int64_t i = (int64_t)blockIdx.x * (256 / TEAM) + team;
    const bool live = i < p.B;
    const int64_t s = live ? p.seeds[i] : 0;
    const int64_t t0 = live ? tp.times[i] : 0;
    const bool seed_ok = live && (uint64_t)s < (uint64_t)p.n_rows;
    const uint64_t g = p.g0 + (uint64_t)i;
    const int steps = seed_ok ? unsup_walk_steps(p, g, call) : 0;
    int64_t v = s, tau = t0;
    bool walking = seed_ok, bad = false;
    philox4 r = {};
    for (int j = 0; j < UNSUP_WALK_MAX; ++j) {
        const bool act = walking && j < steps;
        if (!__any(act)) break;                                 // (uniform over the wave: its longest live walk is done)
        int64_t beg;
        const uint32_t deg = temporal_row(p.rowptr, p.n_rows, act, v, beg, p.err_flag);
        const uint32_t cnt = temporal_count(tp.etime, beg, deg, tau);            // every lane of the wave
        if (act && cnt == 0) walking = false;                   // no edge before tau: the walk ends at v
        if (act && cnt != 0) {
            if ((j & 3) == 0) r = unsup_philox(p, g, call, UNSUP_TAG_TSTEP | (uint32_t)(j >> 2));
            const int64_t e = beg + (int64_t)philox_below(philox_pick(r, j & 3), cnt);  // < beg + cnt <= the row's end
            const int64_t x = (int64_t)p.col[e];
            if (INHERIT == GSAGE_TEMPORAL_INHERIT_EDGE) tau = tp.etime[e];
            if ((uint64_t)x >= (uint64_t)p.n_rows) {
                bad = true;
                walking = false;
                v = 0;
            } else {
                v = x;
            }
        }
    }
    if (!live || l != 0) return;
    if (!seed_ok) {
        unsup_store_bad(p, i);
    } else {
        if (bad && p.err_flag) *p.err_flag = 1;
        unsup_store(p, i, s, v);
    }
    tp.out_times[i] = t0;
    tp.out_times[p.B + i] = t0;
}

// ---- skip-gram head ------------------------------------------------------------------------------------------------
constexpr int SG_QMAX = 64;        // negatives
constexpr int SG_DMAX = 1024;      // embedding width
constexpr int SG_ROWS = 16;        // seeds per workgroup

struct SkipgramParams {
    const float *E;          // [2B + Q, lde]
    const float *pair_w;     // [B]
    void *dE;                // [2B + Q, ldd]
    float *aff;              // [B, 1 + Q] or NULL
    float *partial;          // [n_wg][Q * D + 1]: d z_neg | loss
    float *loss;
    const int32_t *n_valid;  // live seeds (device word) or NULL: seeds [b, B) are padding, b = clamp(*n_valid, 1, B)
    int64_t lde, ldd;
    int32_t B, Q, D, dE_dtype, n_wg;
    float neg_weight;
};

__device__ __forceinline__ float sg_wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float sg_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float sg_sigmoid(float x)
{
    const float e = expf(-fabsf(x));
    return (x >= 0.f ? 1.f : e) / (1.f + e);
}

// live seeds of the batch, as k_head_ce reads them (gsage_head.hip): a padded seed has no loss and no gradient
__device__ __forceinline__ int sg_live(const SkipgramParams &p)
{
    return p.n_valid ? min(max(*p.n_valid, 1), p.B) : p.B;
}

__device__ __forceinline__ void sg_store(const SkipgramParams &p, int64_t row, int k, float g)
{
    if (p.dE_dtype == GSAGE_BF16)
        ((uint16_t *)p.dE)[row * p.ldd + k] = f32_to_bf16(g);
    else
        ((float *)p.dE)[row * p.ldd + k] = g;
}

// 16 per-lane partial sums -> 16 wave sums with 17 shuffles instead of 96: every exchange step halves the values a
// lane carries.  Afterwards v[0] of lane l is the whole wave's sum of value (l >> 2) & 15.
__device__ __forceinline__ float sg_reduce16(float (&v)[SG_ROWS], int lane)
{
#pragma unroll
    for (int half = 8, o = 32; half >= 1; half >>= 1, o >>= 1) {
        const bool up = (lane & o) != 0;
#pragma unroll
        for (int j = 0; j < half; ++j) {
            const float send = up ? v[j] : v[j + half];
            const float keep = up ? v[j + half] : v[j];
            v[j] = keep + __shfl_xor(send, o, 64);
        }
    }
    float s = v[0];
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 1, 64);
    return s;
}

// NJ = ceil(D / 64): columns a lane holds of one row (4, 8 or 16).  Thread t of the column phase owns columns t + 256 j.
template <int NJ>
__global__ void __launch_bounds__(256)
k_head_skipgram(const SkipgramParams p)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int D = p.D, Q = p.Q, B = p.B, b = sg_live(p);
    float *nT = lds;                                  // [SG_QMAX][16] n_iq           (16-byte rows: ds_read_b128)
    float *dT = nT + SG_QMAX * SG_ROWS;               // [SG_QMAX][16] d n_iq
    float *sinv = dT + SG_QMAX * SG_ROWS;             // [16] 1 / norm of the seed rows
    float *pinv = sinv + SG_ROWS;                     // [16] ... of the positives' rows
    float *av = pinv + SG_ROWS;                       // [16] a_i
    float *dav = av + SG_ROWS;                        // [16] d a_i
    float *zdz = dav + SG_ROWS;                       // [16] <z_i, d z_i>
    float *ninv = zdz + SG_ROWS;                      // [SG_QMAX] 1 / norm of the negatives' rows
    float *red = ninv + SG_QMAX;                      // [4] (+ 12 of padding)
    float *zs = red + 16;                             // [16][D] normalised seed rows (zero rows past b)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * SG_ROWS;
    const float *__restrict__ E = p.E;
    const float *__restrict__ En = E + (int64_t)2 * B * p.lde;     // the negatives' rows

    // 1. norms of the 16 seed rows and of their positives, a_i, the normalised seed rows -> LDS (wave w: rows w + 4 m)
#pragma unroll
    for (int m = 0; m < SG_ROWS / 4; ++m) {
        const int r = wave + 4 * m, i = row0 + r;
        float es[NJ], ep[NJ], ss = 0.f, sp = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k = lane + 64 * j;
            const bool ok = k < D && i < b;
            es[j] = ok ? E[(int64_t)i * p.lde + k] : 0.f;
            ep[j] = ok ? E[((int64_t)B + i) * p.lde + k] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) { ss += es[j] * es[j]; sp += ep[j] * ep[j]; }
        const float ns = fmaxf(sqrtf(sg_wave_sum(ss)), 1e-12f), np = fmaxf(sqrtf(sg_wave_sum(sp)), 1e-12f);
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k = lane + 64 * j;
            const float z = es[j] / ns;
            a += z * (ep[j] / np);
            if (k < D) zs[r * D + k] = z;
        }
        a = sg_wave_sum(a);
        if (lane == 0) { sinv[r] = 1.f / ns; pinv[r] = 1.f / np; av[r] = a; }
    }
    __syncthreads();

    // 2. n_iq for the 16 rows: wave w takes negatives w, w + 4, ...; the next negative's row is in flight meanwhile
    {
        float cur[NJ], nxt[NJ];
        auto fetch = [&](int q, float (&buf)[NJ]) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int k = lane + 64 * j;
                buf[j] = (k < D && q < Q) ? En[(int64_t)q * p.lde + k] : 0.f;
            }
        };
        fetch(wave, cur);
        for (int q = wave; q < Q; q += 4) {
            fetch(q + 4, nxt);
            float acc[SG_ROWS], ss = 0.f;
#pragma unroll
            for (int r = 0; r < SG_ROWS; ++r) acc[r] = 0.f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int k = lane + 64 * j;
                if (k < D) {                                   // (keeps the LDS reads inside zs)
                    const float e = cur[j];
                    ss += e * e;
#pragma unroll
                    for (int r = 0; r < SG_ROWS; ++r) acc[r] += zs[r * D + k] * e;
                }
            }
            const float inv = 1.f / fmaxf(sqrtf(sg_wave_sum(ss)), 1e-12f);
            const float dot = sg_reduce16(acc, lane);
            if ((lane & 3) == 0) nT[q * SG_ROWS + ((lane >> 2) & 15)] = dot * inv;
            if (lane == 0) ninv[q] = inv;
#pragma unroll
            for (int j = 0; j < NJ; ++j) cur[j] = nxt[j];
        }
    }
    __syncthreads();

    // 3. loss, aff, d n_iq; then (a lane per row) d a_i and <z_i, d z_i> = d a_i a_i + sum_q d n_iq n_iq
    const float invB = 1.f / (float)b;
    float my_loss = 0.f;
    for (int e = tid; e < Q * SG_ROWS; e += 256) {
        const int q = e >> 4, i = row0 + (e & 15);
        float dn = 0.f;
        if (i < b) {
            const float n = nT[e];
            if (p.aff) p.aff[(int64_t)i * (1 + Q) + 1 + q] = n;
            my_loss += p.neg_weight * sg_softplus(n);
            dn = p.neg_weight * invB * sg_sigmoid(n);
        }
        dT[e] = dn;
    }
    __syncthreads();
    if (tid < SG_ROWS) {
        const int r = tid, i = row0 + r;
        float da = 0.f, s = 0.f;
        if (i < b) {
            const float a = av[r], w = p.pair_w[i];
            if (p.aff) p.aff[(int64_t)i * (1 + Q)] = a;
            my_loss += w * sg_softplus(-a);
            da = -w * invB * sg_sigmoid(-a);
            s = da * a;
            for (int q = 0; q < Q; ++q) s += dT[q * SG_ROWS + r] * nT[q * SG_ROWS + r];
        }
        dav[r] = da;
        zdz[r] = s;
    }
    my_loss = sg_wave_sum(my_loss);
    if (lane == 0) red[wave] = my_loss;
    __syncthreads();

    // 4. thread <-> column: d z_i = d a_i z_pos + sum_q d n_iq z_neg_q, this workgroup's partial of
    //    d z_neg_q = sum_i d n_iq z_i, then the two gradient rows of every seed through their normalisations
    float *__restrict__ out = p.partial + (int64_t)blockIdx.x * ((int64_t)Q * D + 1);
    if (tid == 0) out[(int64_t)Q * D] = (red[0] + red[1]) + (red[2] + red[3]);
    for (int k = tid; k < D; k += 256) {
        float z[SG_ROWS], dz[SG_ROWS], zp[SG_ROWS];
#pragma unroll
        for (int r = 0; r < SG_ROWS; ++r) {
            z[r] = zs[r * D + k];
            dz[r] = 0.f;
            zp[r] = (row0 + r < b) ? E[((int64_t)B + row0 + r) * p.lde + k] : 0.f;
        }
        for (int q0 = 0; q0 < Q; q0 += 4) {
            float en[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) en[u] = (q0 + u < Q) ? En[(int64_t)(q0 + u) * p.lde + k] : 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (q0 + u < Q) {                              // block-uniform
                    const float zn = en[u] * ninv[q0 + u];
                    const float4 *dn4 = (const float4 *)(dT + (q0 + u) * SG_ROWS);
                    float dzn = 0.f;
#pragma unroll
                    for (int h = 0; h < SG_ROWS / 4; ++h) {
                        const float4 d = dn4[h];
                        dz[4 * h + 0] += d.x * zn; dzn += d.x * z[4 * h + 0];
                        dz[4 * h + 1] += d.y * zn; dzn += d.y * z[4 * h + 1];
                        dz[4 * h + 2] += d.z * zn; dzn += d.z * z[4 * h + 2];
                        dz[4 * h + 3] += d.w * zn; dzn += d.w * z[4 * h + 3];
                    }
                    out[(int64_t)(q0 + u) * D + k] = dzn;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < SG_ROWS; ++r) {
            const int i = row0 + r;
            if (i >= b) {                                      // block-uniform; padding: exact zeros (K5b reads them)
                if (i < B) { sg_store(p, i, k, 0.f); sg_store(p, (int64_t)B + i, k, 0.f); }
            } else {
                const float da = dav[r], zpos = zp[r] * pinv[r];
                sg_store(p, i, k, (da * zpos + dz[r] - z[r] * zdz[r]) * sinv[r]);
                sg_store(p, (int64_t)B + i, k, da * (z[r] - zpos * av[r]) * pinv[r]);     // <z_pos, d z_pos> = d a_i a_i
            }
        }
    }
}

// A workgroup per negative q: d z_neg_q = the partials summed in workgroup order, then that row's normalisation
// backward.  Workgroup 0 also sums the loss.  Thread t owns columns t + 256 j.
__global__ void __launch_bounds__(256)
k_head_skipgram_neg(const SkipgramParams p)
{
    __shared__ float red[4];
    const int D = p.D, q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t width = (int64_t)p.Q * D + 1;
    const int64_t row = (int64_t)2 * p.B + q;
    auto block_sum = [&](float v) {
        v = sg_wave_sum(v);
        __syncthreads();
        if (lane == 0) red[wave] = v;
        __syncthreads();
        return (red[0] + red[1]) + (red[2] + red[3]);
    };
    float e[SG_DMAX / 256], dz[SG_DMAX / 256], ss = 0.f;
#pragma unroll
    for (int j = 0; j < SG_DMAX / 256; ++j) {
        const int k = tid + 256 * j;
        e[j] = k < D ? p.E[row * p.lde + k] : 0.f;
        float s = 0.f;
        if (k < D) {
            const float *col = p.partial + (int64_t)q * D + k;
            int g = 0;
            for (; g + 8 <= p.n_wg; g += 8) {                  // 8 loads in flight, summed in order
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = col[(int64_t)(g + u) * width];
#pragma unroll
                for (int u = 0; u < 8; ++u) s += v[u];
            }
            for (; g < p.n_wg; ++g) s += col[(int64_t)g * width];
        }
        dz[j] = s;
        ss += e[j] * e[j];
    }
    const float nrm = fmaxf(sqrtf(block_sum(ss)), 1e-12f);
    float zd = 0.f;
#pragma unroll
    for (int j = 0; j < SG_DMAX / 256; ++j) { e[j] = e[j] / nrm; zd += e[j] * dz[j]; }
    zd = block_sum(zd);
#pragma unroll
    for (int j = 0; j < SG_DMAX / 256; ++j) {
        const int k = tid + 256 * j;
        if (k < D) sg_store(p, row, k, (dz[j] - e[j] * zd) / nrm);
    }
    if (q == 0 && wave == 0) {                                 // the loss: lanes over the workgroups, a fixed tree
        float l = 0.f;
        for (int g = lane; g < p.n_wg; g += 64) l += p.partial[(int64_t)g * width + width - 1];
        l = sg_wave_sum(l);
        if (lane == 0) *p.loss = l / (float)sg_live(p);
    }
}

// ---- [host] what the batch builders' entry points share ---------------------------------------------------------------
// the checks of the plain, weighted and biased entries on their filled parameters (the temporal entry words its own);
// needs_edge_cdf: the entry draws its steps from the per-edge table
static int unsup_check(const char *entry, const UnsupParams &u, bool needs_edge_cdf)
{
    GSAGE_REQUIRE(u.rowptr && u.col && u.seeds && u.cdf && u.ids && u.pair_w, "%s: null pointer", entry);
    GSAGE_REQUIRE(!needs_edge_cdf || u.edge_cdf, "%s: the adjacency carries no edge weights (edge_cdf is NULL)", entry);
    GSAGE_REQUIRE(u.n_rows > 0 && u.B > 0 && u.B < (1LL << 31) && u.Q > 0 && u.Q < (1LL << 31), "%s: bad sizes", entry);
    GSAGE_REQUIRE(u.walk_len >= 1 && u.walk_len <= UNSUP_WALK_MAX, "%s: needs 1 <= walk_len <= %d", entry, UNSUP_WALK_MAX);
    GSAGE_REQUIRE(u.cdf_total > 0.0 && u.cdf_total <= 1.7976931348623157e308,
                  "%s: the negatives' weights sum to %g (every row has weight 0?)", entry, u.cdf_total);
    return GSAGE_OK;
}

// per_block: walks a workgroup of the builder's kernel takes
static void unsup_fill(UnsupParams &u, const int64_t *rowptr, const int32_t *col, const uint64_t *edge_cdf, int64_t n_rows,
                       const int64_t *seeds, int64_t B, int per_block, int32_t walk_len, int64_t Q, const double *cdf,
                       double cdf_total, uint64_t seed, const uint64_t *call_ctr, uint64_t call_base, uint64_t g0,
                       int64_t *ids, float *pair_w, int32_t *err_flag)
{
    u.rowptr = rowptr; u.col = col; u.seeds = seeds; u.cdf = cdf; u.edge_cdf = edge_cdf; u.call_ctr = call_ctr;
    u.ids = ids; u.pair_w = pair_w; u.err_flag = err_flag; u.n_rows = n_rows; u.B = B; u.Q = Q; u.call_base = call_base;
    u.g0 = g0; u.cdf_total = cdf_total; u.seed_lo = (uint32_t)seed; u.seed_hi = (uint32_t)(seed >> 32);
    u.walk_len = walk_len; u.walk_blocks = (int32_t)ceil_div(B, per_block);
}

// the walk workgroups, then a lane per negative
static dim3 unsup_grid(const UnsupParams &u) { return dim3((unsigned)(u.walk_blocks + ceil_div(u.Q, 256))); }

template <typename K>
static int sg_raise_lds(K kernel, size_t lds, bool &done)
{
    if (done || lds <= 64 * 1024) return GSAGE_OK;
    if (hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) != hipSuccess) {
        (void)hipGetLastError();
        set_error("head_skipgram: cannot raise the dynamic LDS limit");
        return GSAGE_ELAUNCH;
    }
    done = true;
    return GSAGE_OK;
}

}  // namespace gsage

using namespace gsage;

extern "C" {

int gsage_unsup_batch(const int64_t *rowptr, const int32_t *col, int64_t n_rows, const int64_t *seeds, int64_t B,
                      int32_t walk_len, int64_t Q, const double *cdf, double cdf_total, uint64_t seed,
                      const uint64_t *call_ctr, uint64_t call_base, uint64_t g0, int64_t *ids, float *pair_w,
                      int32_t *err_flag, void *stream)
{
    UnsupParams p;
    unsup_fill(p, rowptr, col, nullptr, n_rows, seeds, B, 256, walk_len, Q, cdf, cdf_total, seed, call_ctr, call_base, g0,
               ids, pair_w, err_flag);                                            // a lane per walk
    int rc = unsup_check("unsup_batch", p, false);
    if (rc != GSAGE_OK) return rc;
    launch(k_unsup_batch, unsup_grid(p), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch("unsup_batch");
}

int gsage_unsup_batch_weighted(const int64_t *rowptr, const int32_t *col, const uint64_t *edge_cdf, int64_t n_rows,
                               const int64_t *seeds, int64_t B, int32_t walk_len, int64_t Q, const double *cdf,
                               double cdf_total, uint64_t seed, const uint64_t *call_ctr, uint64_t call_base, uint64_t g0,
                               int64_t *ids, float *pair_w, int32_t *err_flag, void *stream)
{
    UnsupParams p;
    unsup_fill(p, rowptr, col, edge_cdf, n_rows, seeds, B, 4, walk_len, Q, cdf, cdf_total, seed, call_ctr, call_base, g0,
               ids, pair_w, err_flag);                                            // a wave per walk, four to a workgroup
    int rc = unsup_check("unsup_batch_weighted", p, true);
    if (rc != GSAGE_OK) return rc;
    launch(k_unsup_batch_weighted, unsup_grid(p), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch("unsup_batch_weighted");
}

int gsage_unsup_batch_biased(const int64_t *rowptr, const int32_t *col, const uint64_t *edge_cdf, int64_t n_rows,
                             const int64_t *seeds, int64_t B, int32_t walk_len, int64_t Q, const double *cdf,
                             double cdf_total, uint64_t seed, const uint64_t *call_ctr, uint64_t call_base, uint64_t g0,
                             double p, double q, int64_t *ids, float *pair_w, int32_t *err_flag, void *stream)
{
    GSAGE_REQUIRE(p >= 0.125 && p <= 8.0, "unsup_batch_biased: p must be in [1/8, 8] (got %g)", p);
    GSAGE_REQUIRE(q >= 0.125 && q <= 8.0, "unsup_batch_biased: q must be in [1/8, 8] (got %g)", q);
    UnsupBiasedParams bp;
    (void)walk_bias_make(p, q, 0.0, bp.b);                                        // (the limits were checked above)
    unsup_fill(bp.u, rowptr, col, edge_cdf, n_rows, seeds, B, 4, walk_len, Q, cdf, cdf_total, seed, call_ctr, call_base,
               g0, ids, pair_w, err_flag);                                        // a wave per walk, four to a workgroup
    int rc = unsup_check("unsup_batch_biased", bp.u, false);
    if (rc != GSAGE_OK) return rc;
    launch(k_unsup_batch_biased, unsup_grid(bp.u), dim3(256), 0, (hipStream_t)stream, bp);
    return check_launch("unsup_batch_biased");
}

int gsage_unsup_batch_temporal(const int64_t *rowptr, const int32_t *col, const int64_t *etime, int64_t n_rows,
                               const int64_t *seeds, const int64_t *times, int64_t B, int32_t walk_len, int64_t Q,
                               const double *cdf, double cdf_total, uint64_t seed, const uint64_t *call_ctr,
                               uint64_t call_base, uint64_t g0, int32_t inherit, const int32_t *n_valid, int64_t *ids,
                               int64_t *out_times, float *pair_w, int32_t *err_flag, void *stream)
{
    GSAGE_REQUIRE(rowptr && col && etime, "unsup_batch_temporal: null pointer (rowptr, col, etime)");
    GSAGE_REQUIRE(seeds && times, "unsup_batch_temporal: null pointer (seeds, times)");
    GSAGE_REQUIRE(cdf, "unsup_batch_temporal: null pointer (cdf)");
    GSAGE_REQUIRE(ids && out_times && pair_w, "unsup_batch_temporal: null pointer (ids, out_times, pair_w)");
    GSAGE_REQUIRE(n_rows > 0, "unsup_batch_temporal: n_rows must be >= 1");
    GSAGE_REQUIRE(B >= 1 && B < (1LL << 31), "unsup_batch_temporal: B must be in [1, 2^31)");
    GSAGE_REQUIRE(Q >= 1 && Q < (1LL << 31), "unsup_batch_temporal: Q must be in [1, 2^31)");
    GSAGE_REQUIRE(walk_len >= 1 && walk_len <= UNSUP_WALK_MAX, "unsup_batch_temporal: walk_len must be in 1..%d",
                  UNSUP_WALK_MAX);
    GSAGE_REQUIRE(inherit == GSAGE_TEMPORAL_INHERIT_SEED || inherit == GSAGE_TEMPORAL_INHERIT_EDGE,
                  "unsup_batch_temporal: unknown inherit rule %d (0: seed, 1: edge)", (int)inherit);
    GSAGE_REQUIRE(cdf_total > 0.0 && cdf_total <= 1.7976931348623157e308,
                  "unsup_batch_temporal: cdf_total, the sum of the negatives' weights, is %g (every row has weight 0?)",
                  cdf_total);
    UnsupTemporalParams tp;
    unsup_fill(tp.u, rowptr, col, nullptr, n_rows, seeds, B, 256 / TEAM, walk_len, Q, cdf, cdf_total, seed, call_ctr,
               call_base, g0, ids, pair_w, err_flag);                             // a team per walk, sixteen to a workgroup
    tp.etime = etime; tp.times = times; tp.n_valid = n_valid; tp.out_times = out_times;
    auto kernel = inherit == GSAGE_TEMPORAL_INHERIT_EDGE ? k_unsup_batch_temporal<GSAGE_TEMPORAL_INHERIT_EDGE>
                                                         : k_unsup_batch_temporal<GSAGE_TEMPORAL_INHERIT_SEED>;
    launch(kernel, unsup_grid(tp.u), dim3(256), 0, (hipStream_t)stream, tp);
    return check_launch("unsup_batch_temporal");
}

int64_t gsage_head_skipgram_scratch(int32_t B, int32_t Q, int32_t D)
{
    if (B <= 0 || Q <= 0 || D <= 0) return -1;
    return ceil_div(B, SG_ROWS) * ((int64_t)Q * D + 1);
}

int gsage_head_skipgram_live(const float *E, int64_t lde, int32_t B, int32_t Q, int32_t D, const float *pair_w,
                             float neg_weight, const int32_t *n_valid, void *dE, int dE_dtype, int64_t ldd, float *loss,
                             float *aff, float *scratch, void *stream)
{
    GSAGE_REQUIRE(E && pair_w && dE && loss && scratch, "head_skipgram: null pointer");
    GSAGE_REQUIRE(B > 0 && Q > 0 && Q <= SG_QMAX && D > 0 && D <= SG_DMAX,
                  "head_skipgram: needs 1 <= n_negatives <= %d and 1 <= width <= %d", SG_QMAX, SG_DMAX);
    GSAGE_REQUIRE(lde >= D && ldd >= D, "head_skipgram: leading dimensions smaller than the width");
    GSAGE_REQUIRE(dE_dtype == GSAGE_BF16 || dE_dtype == GSAGE_F32, "head_skipgram: bad dE dtype");
    SkipgramParams p;
    p.E = E; p.pair_w = pair_w; p.dE = dE; p.aff = aff; p.partial = scratch; p.loss = loss; p.lde = lde; p.ldd = ldd;
    p.B = B; p.Q = Q; p.D = D; p.dE_dtype = dE_dtype; p.n_wg = (int32_t)ceil_div(B, SG_ROWS); p.neg_weight = neg_weight;
    p.n_valid = n_valid;
    const size_t lds = sizeof(float) * (2 * SG_QMAX * SG_ROWS + 5 * SG_ROWS + SG_QMAX + 16 + (size_t)SG_ROWS * D);
    hipStream_t s = (hipStream_t)stream;
    if (D <= 256) {
        launch(k_head_skipgram<4>, dim3(p.n_wg), dim3(256), lds, s, p);
    } else if (D <= 512) {
        launch(k_head_skipgram<8>, dim3(p.n_wg), dim3(256), lds, s, p);
    } else {
        static bool raised = false;
        const int rc = sg_raise_lds(k_head_skipgram<16>, lds, raised);
        if (rc != GSAGE_OK) return rc;
        launch(k_head_skipgram<16>, dim3(p.n_wg), dim3(256), lds, s, p);
    }
    int rc = check_launch("head_skipgram");
    if (rc != GSAGE_OK) return rc;
    launch(k_head_skipgram_neg, dim3(Q), dim3(256), 0, s, p);
    return check_launch("head_skipgram_neg");
}

int gsage_head_skipgram(const float *E, int64_t lde, int32_t B, int32_t Q, int32_t D, const float *pair_w,
                        float neg_weight, void *dE, int dE_dtype, int64_t ldd, float *loss, float *aff, float *scratch,
                        void *stream)
{
    return gsage_head_skipgram_live(E, lde, B, Q, D, pair_w, neg_weight, nullptr, dE, dE_dtype, ldd, loss, aff, scratch,
                                    stream);
}

}  // extern "C"
