/*
 * gsage.h -- C ABI of libgsage_hip.so, the MI355X (gfx950) GraphSAGE hot path.
 *
 * This is the drop-in boundary.  The reference (bkj/pytorch-graphsage) is pure Python with no
 * FFI of its own; its plugin surface is three string->class tables
 * (nn_modules.py:104-107, :169-173, :324-330) plus GSSupervised (models.py:21-104).  The
 * entry points below are what a ctypes binding inside those classes would call -- one per
 * tensor-level operation of the hot path -- and INTEGRATION.md shows that binding.  Each
 * declaration cites the reference lines it replaces.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / C++ types.
 *   - Unless marked [host], every pointer is a DEVICE pointer (HBM) owned by the caller;
 *     nothing is allocated or freed behind the caller's back, outputs are caller-allocated.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Every call only
 *     enqueues work on that stream and returns; no call synchronises.  All kernels are
 *     hipGraph-capturable (no allocation, no sync, no host-side state besides launch counters).
 *   - Return value: 0 on success, a negative GSAGE_E* code otherwise; gsage_last_error()
 *     returns a thread-local message.  Asynchronous data errors (an id outside the graph) are
 *     reported through the caller-supplied `err_flag` device word (0 = ok).
 *   - dtype codes: GSAGE_F32 / GSAGE_BF16 (bf16 = upper 16 bits of an IEEE fp32, RNE).  GSAGE_FP8 names the storage
 *     format of a quantised feature table ("FP8 feature table" below); only the *_fp8 entry points take it.
 *   - Graph layout ("device CSR", built once from the reference's scipy csr_matrix in the
 *     (v,r,c) convention of problem.py:70-72 / utils/convert.py:100-126):
 *         rowptr int64 [n_rows+1]   rowptr[i+1]-rowptr[i] = degree of node i
 *         col    int32 [nnz]        neighbour ids (1-based; 0 is the dummy node), stored in
 *                                   column order 0..deg-1 of the reference matrix
 *   - Feature-table layout: row-major [n_rows, ld] with ld >= D; vectorised paths need
 *     ld % 8 == 0 (bf16) / ld % 4 == 0 (fp32) and columns [D, ld) equal to zero.
 */
#ifndef GSAGE_H
#define GSAGE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSAGE_ABI_VERSION 6

enum { GSAGE_F32 = 0, GSAGE_BF16 = 1, GSAGE_FP8 = 2 };
enum {
    GSAGE_OK = 0,
    GSAGE_EINVAL = -1,   /* bad argument (null pointer, bad size / alignment / dtype) */
    GSAGE_ELAUNCH = -2,  /* hipLaunchKernel / runtime error (message in gsage_last_error) */
    GSAGE_ENODEV = -3    /* no gfx950 device visible */
};
enum { GSAGE_POOL_MAX = 0, GSAGE_POOL_MEAN = 1 };
enum { GSAGE_ACT_NONE = 0, GSAGE_ACT_RELU = 1, GSAGE_ACT_TANH = 2 };

int gsage_abi_version(void);
const char *gsage_last_error(void);
/* Number of kernels this library has launched since load (tests use it to prove the HIP path
 * ran instead of some fallback). */
uint64_t gsage_launch_count(void);
/* [host] debugging aid: from now on a SIGABRT first writes the native backtrace of the aborting thread to the
 * file descriptor `fd` (< 0: stderr), then runs whatever handler was installed before.  The HSA runtime reports a
 * GPU memory fault by calling abort() on a thread of its own, with a message that a test runner capturing fd 2
 * swallows: the backtrace says who aborted (tests/conftest.py installs it for -m gpu sessions). */
int gsage_debug_abort_trace(int fd);
/* [host] device name / CU count of the current device; returns GSAGE_ENODEV without a GPU. */
int gsage_device_info(char *arch, int arch_len, int *cu_count, int *wave_size);

/* ------------------------------------------------------------------------------------------
 * Command lists.  No reference counterpart: the reference dispatches one PyTorch op per tensor
 * expression from Python (models.py:71-104); here a train_step is ~9 kernels of 5-40 us and the
 * way they are issued matters as much as the kernels.
 *
 *   gsage_cmdlist_begin()            [host] every gsage_* kernel call made by THIS thread from now
 *                                    on is validated and recorded (kernel, geometry, by-value
 *                                    arguments) instead of launched; `stream` arguments are ignored.
 *   gsage_cmdlist_end(&list)         [host] stops recording, returns the list.
 *   gsage_cmdlist_replay(list, s)    [host] issues the recorded kernels back to back on stream s
 *                                    (one hipLaunchKernel each, no validation, no Python).  The
 *                                    pointers recorded must still be valid: same rule as a hipGraph.
 *   gsage_cmdlist_size / _destroy
 * Unlike a hipGraph a list has no start-up gap on the device and can be cut anywhere (e.g.
 * around an RCCL collective on another stream) at no cost.  Host-side calls (gsage_mt_*) and the
 * one-time LDS-limit setup of a kernel are not recordable: run one un-recorded step first.
 * ---------------------------------------------------------------------------------------- */
/*   gsage_cmdlist_mark(slot)        [host] while recording: the list records HIP event `slot` (0..15) at
 *                                    this point of every replay (on the replay's stream).
 *   gsage_cmdlist_elapsed(l,a,b,&ms) [host] waits for mark b of the last replay and returns the time
 *                                    between marks a and b: how bench.py times ONE kernel of a step in
 *                                    place, on the stream it runs on (measurement only: a list with
 *                                    marks pays an event record per mark). */
/*   gsage_stream_create_masked      [host] a HIP stream whose kernels run on the compute units set in
 *                                    cu_mask only (bit n = CU n of the device, `words` x 32 bits): how
 *                                    the engines give the weight-independent, HBM-bound gathers of the
 *                                    NEXT batch and the latency-bound forward / backward chain of the
 *                                    current batch disjoint halves of the chip, so that the two really
 *                                    run side by side.  gsage_stream_destroy frees it. */
int gsage_stream_create_masked(const uint32_t *cu_mask, int32_t words, void **stream);
int gsage_stream_destroy(void *stream);
/*   gsage_event_create / _destroy   [host] a HIP event without timing, for ordering between streams.
 *   gsage_cmdlist_replay_pair       [host] one step of a two-stream pipeline in one call: on stream b
 *                                    {wait for event wait_b; replay list_b; record record_b}, then on
 *                                    stream a {wait for wait_a; replay list_a; record record_a}; finally
 *                                    then_wait_stream (may be NULL) is made to wait for record_b
 *                                    (then_wait_on_b != 0) or record_a.  Events / lists may be NULL. */
int gsage_event_create(void **event);
void gsage_event_destroy(void *event);
int gsage_cmdlist_replay_pair(const void *list_a, void *stream_a, void *wait_a, void *record_a,
                              const void *list_b, void *stream_b, void *wait_b, void *record_b,
                              void *then_wait_stream, int then_wait_on_b);
int gsage_cmdlist_begin(void);
int gsage_cmdlist_end(void **list);
int gsage_cmdlist_mark(int slot);
/*   gsage_cmdlist_time_next(a, b)    [host] while recording: the NEXT recorded kernel is dispatched with
 *                                    start event a and stop event b attached to the dispatch itself
 *                                    (hipExtLaunchKernel): gsage_cmdlist_elapsed(l, a, b) is then that
 *                                    kernel's own duration -- no event packets before or after it. */
int gsage_cmdlist_time_next(int slot_a, int slot_b);
int gsage_cmdlist_elapsed(const void *list, int slot_a, int slot_b, float *ms);
int64_t gsage_cmdlist_size(const void *list);
int gsage_cmdlist_replay(const void *list, void *stream);
/* Side sections: launches recorded between _side_begin and _side_end replay on a second stream that belongs to
 * the list, forked from the main stream at the point of the section (the side stream waits for everything the
 * main stream was given before it); _join makes the main stream wait for the end of the last side section.
 * What it is for: a bandwidth-bound job that does not depend on the neighbouring launches (the NEXT batch's
 * level-0 gathers) beside a latency-bound launch whose workgroups leave registers and the memory pipes of
 * their CUs idle (the seed-level kernel: one 384-register wave per SIMD) -- two kernels can share a CU where one
 * kernel's uniform LDS / register footprint cannot.  One section open at a time; the main-stream launches that
 * follow _side_end and precede _join run concurrently with the section. */
int gsage_cmdlist_side_begin(void);
int gsage_cmdlist_side_end(void);
int gsage_cmdlist_join(void);
void gsage_cmdlist_destroy(void *list);
/* Host calls inside a list (ABI 4).  A data-parallel step has ONE exchange and a deterministic
 * row reduction (a vendor sort until round 6): what is not a kernel of this library still belongs INTO the step's list so that a
 * step stays one C call (no Python between the pieces, no second list around the collective).
 *   gsage_host_call(fn, ctx, s)      [host] recording: a node that calls fn(ctx, stream) at this point of every replay
 *                                    (inside a side section: with the side stream); not recording: calls fn(ctx, s)
 *                                    now.  fn enqueues work on the stream it is given and returns 0, or non-zero to
 *                                    make the replay fail (GSAGE_ELAUNCH, message "host call failed").  The engines
 *                                    use it for collectives of backends that have no C entry point (gloo in the
 *                                    CPU-side tests: a ctypes callback); RCCL goes through gsage_comm_* below. */
typedef int (*gsage_host_fn)(void *ctx, void *stream);
int gsage_host_call(gsage_host_fn fn, void *ctx, void *stream);

/* ------------------------------------------------------------------------------------------
 * The step's collectives, issued by the library itself (ABI 4).  No reference counterpart: the reference is one
 * process.  One RCCL communicator per process, created from an id that rank 0 makes and the host
 * language distributes (torch.distributed's store, MPI, a file -- not this library's business):
 *   gsage_comm_load(path)            [host] dlopen of librccl (path NULL: the loader's search order).  The library has
 *                                    no link-time dependency on RCCL: single-GPU processes never load it.
 *   gsage_comm_unique_id(id)         [host] 128 bytes, rank 0 only
 *   gsage_comm_create(id, r, w, &c)  [host] collective over the w ranks (current HIP device = this rank's GPU)
 *   gsage_comm_all_reduce_f32        in place over n floats; average != 0: ncclAvg, else ncclSum
 *   gsage_comm_all_gather            recv[r * bytes : (r + 1) * bytes] = rank r's send[0:bytes]  (bytes % 4 == 0)
 *   gsage_comm_group(begin)          ncclGroupStart (begin != 0) / ncclGroupEnd: several collectives as one
 * The three collective calls follow the library's convention: recorded as a node while a command list is being
 * recorded (side sections included: that is how the exchange overlaps the next batch's gathers), issued on `stream`
 * otherwise.  Every rank must issue the same sequence. */
int gsage_comm_load(const char *path);
int gsage_comm_unique_id(void *id128);
int gsage_comm_create(const void *id128, int32_t rank, int32_t world, void **comm);
int gsage_comm_destroy(void *comm);
int gsage_comm_all_reduce_f32(void *comm, float *buf, int64_t n, int32_t average, void *stream);
int gsage_comm_all_gather(void *comm, const void *send, void *recv, int64_t bytes, void *stream);
int gsage_comm_group(void *comm, int32_t begin, void *stream);

/* ------------------------------------------------------------------------------------------
 * K1  neighbour sampler     replaces SparseUniformNeighborSampler.__call__, nn_modules.py:80-101
 *     (and __init__, :72-78: degrees are rowptr differences, nothing is precomputed)
 *
 *     out[i*n+j] = col[rowptr[ids[i]] + sel[i*n+j] % deg_i]   (deg_i > 0)      nn_modules.py:89-93
 *                = 0 (the dummy node)                          (deg_i == 0)
 * ---------------------------------------------------------------------------------------- */

/* `sel` supplied by the caller (int32 [M*n], each in [0, max_deg)): parity level 1, and the
 * device half of compat mode where sel comes from the legacy MT19937 stream (gsage_mt_*). */
int gsage_sample_csr_sel(const int64_t *rowptr, const int32_t *col, int64_t n_rows,
                         const int64_t *ids, int64_t M, int32_t n, const int32_t *sel,
                         int64_t *out, int32_t *err_flag, void *stream);

/* UniformNeighborSampler.__call__ (reference nn_modules.py:43-49): `adj[ids][:, perm][:, :n]` over the dense
 * int64 [n_rows, ld] adjacency (every row pre-sampled to exactly ld neighbours by the converter), in one launch:
 *     out[i*n + j] = adj[ids[i]*ld + keep[j]]
 * keep: DEVICE int64 [n] = the first n entries of the torch.randperm(ld) the caller drew from torch's global
 * CPU generator (one permutation per call, shared by the whole batch).  An id outside
 * [0, n_rows) or a column outside [0, ld) yields 0 and raises *err_flag (the reference: IndexError). */
int gsage_sample_dense(const int64_t *adj, int64_t ld, int64_t n_rows, const int64_t *ids, int64_t M,
                       const int64_t *keep, int32_t n, int64_t *out, int32_t *err_flag, void *stream);

/* Counter mode (throughput): sel is generated in-kernel by Philox4x32-10,
 *     g    = g0 + i*n + j                      global sample index of the whole job
 *     call = call_base + (call_ctr ? *call_ctr : 0)        (call_ctr: device word, may be NULL;
 *            lets a captured hipGraph advance the stream between replays)
 *     word = philox4x32_10({lo(g>>2), hi(g>>2), lo(call), hi(call)}, {lo(seed), hi(seed)})[g&3]
 *     sel  = (word * max_deg) >> 32
 * `sel_out` (int32 [M*n], may be NULL) receives sel for verification. */
int gsage_sample_csr_philox(const int64_t *rowptr, const int32_t *col, int64_t n_rows,
                            const int64_t *ids, int64_t M, int32_t n, uint32_t max_deg,
                            uint64_t seed, const uint64_t *call_ctr, uint64_t call_base,
                            uint64_t g0, int64_t *out, int32_t *sel_out, int32_t *err_flag,
                            void *stream);

/* Every hop of a frontier in one launch (counter mode).  `ids` is the concatenated frontier
 * [hop 0 (B seeds, filled by the caller) | hop 1 (B*fan[0]) | hop 2 (B*fan[0]*fan[1]) | ...];
 * hop k is sampled exactly as gsage_sample_csr_philox would with call index call_base + k - 1 and
 * g0 = rank * |hop k| -- results are bit-identical to n_hops separate launches.  fan: HOST array
 * of n_hops (<= 5) fan-outs.  seed_queue (may be NULL): device-resident [n_batches, B] seed
 * batches; the batch *batch_idx % n_batches is copied into hop 0 by the kernel itself, so a
 * captured graph can walk an epoch without per-step host copies. */
int gsage_sample_hops_philox(const int64_t *rowptr, const int32_t *col, int64_t n_rows, int64_t *ids,
                             int64_t B, int32_t n_hops, const int32_t *fan, uint32_t max_deg,
                             uint64_t seed, const uint64_t *call_ctr, uint64_t call_base,
                             uint64_t rank, const int64_t *seed_queue, const int64_t *batch_idx,
                             int64_t n_batches, int32_t *err_flag, void *stream);
/* The same arguments as a struct (HOST memory).  batch_base is added to *batch_idx before the modulo:
 * with call_base it addresses a batch AHEAD of the device counters without touching them -- how a
 * later batch's frontier is sampled from inside another launch (gsage_gather_mean_multi_adam). */
typedef struct gsage_hops_desc {
    const int64_t *rowptr;
    const int32_t *col;
    int64_t n_rows;
    int64_t *ids;
    int64_t B;
    int32_t n_hops;
    int32_t fan[5];
    uint32_t max_deg;
    uint64_t seed;
    const uint64_t *call_ctr;
    uint64_t call_base;
    uint64_t rank;
    const int64_t *seed_queue;
    const int64_t *batch_idx;
    int64_t batch_base;
    int64_t n_batches;
    int32_t *err_flag;
    /* sel (may be NULL): caller-supplied draws instead of Philox -- int32, this rank's samples of
     * [hop 1 (B*fan[0]) | hop 2 | ...] back to back, each in [0, max_deg): the fused sampler then
     * computes exactly gsage_sample_csr_sel per hop (parity level 1: replays the `sel` the reference
     * drew at nn_modules.py:88).  With a seed queue the draws of batch b start at sel + b*sel_stride. */
    const int32_t *sel;
    int64_t sel_stride;
    /* dense_adj (may be NULL; ABI 3): the frontier of the reference's DENSE sampler (UniformNeighborSampler,
     * nn_modules.py:19-49) instead of the CSR walk -- int64 [n_rows, dense_ld], every row pre-sampled to exactly
     * dense_ld neighbours.  `sel` is then mandatory and holds, per batch, the columns the sampler keeps:
     * [fan[0] columns for hop 1 | fan[1] columns for hop 2 | ...] (sel_stride = their sum), i.e. the head of the
     * torch.randperm(K) the reference draws ONCE per sampler call and shares between all parents:
     *     ids[hop k][i*fan + j] = dense_adj[ids[hop k-1][i], keep_k[j]].
     * rowptr / col / max_deg / seed / call_* are ignored. */
    const int64_t *dense_adj;
    int64_t dense_ld;
} gsage_hops_desc;
/* gsage_sample_hops_philox from a descriptor (the only way to pass batch_base). */
int gsage_sample_hops(const gsage_hops_desc *hops, void *stream);

/* *ctr += inc on the stream (advances the Philox call counter inside a captured graph). */
int gsage_counter_add(uint64_t *ctr, uint64_t inc, void *stream);
/* Two small device-to-device copies in one launch (4-byte granularity): a step's seed ids and targets into the
 * static buffers a recorded / captured step reads (train.py:141-148 hands over fresh tensors per batch). */
int gsage_copy_pair(void *dst0, const void *src0, int64_t bytes0, void *dst1, const void *src1, int64_t bytes1,
                    void *stream);

/* [host] the numpy legacy MT19937 stream the reference draws from (helpers.py:15,
 * nn_modules.py:88, problem.py:146), for compat mode.  All pointers here are HOST pointers. */
void *gsage_mt_create(uint32_t seed);
void gsage_mt_destroy(void *mt);
void gsage_mt_seed(void *mt, uint32_t seed);
/* np.random.choice(high, count) -> int32 out[count]; returns 32-bit words consumed. */
int64_t gsage_mt_choice_i32(void *mt, int64_t high, int64_t count, int32_t *out);
/* The same np.random.choice(high, count) with the stream ON THE DEVICE: `state` = 625 device words (the
 * 624 MT19937 state words + the position, numpy's np.random.get_state()[1], [2]); the launch consumes
 * exactly the words numpy would, leaves state / position where numpy would, and writes int32 out[count]
 * (device).  One workgroup (the recurrence is sequential; refill, tempering and the order-preserving
 * rejection are parallel inside it).  Not recordable into a graph-free command list restriction: it IS an
 * ordinary kernel launch and can be recorded like any other. */
int gsage_mt_choice_device(uint32_t *state, int64_t high, int64_t count, int32_t *out, void *stream);
/* n_seg requests served back to back from the same device-resident stream in ONE launch: request q writes
 * seg_cnt[q] values to out + seg_off[q] (seg_off / seg_cnt: DEVICE int64 arrays).  Consecutive
 * np.random.choice(high, .) calls consume numpy's stream exactly like this, so a whole training epoch's sampler
 * draws (per batch: hop 1's M * n_1 values, hop 2's M * n_1 * n_2, ... -- nn_modules.py:88 called from
 * models.py:78-80 batch after batch) are produced up front and the fused engines' device-side batch queue replays
 * them (gsage_hops_desc.sel): samples bit-identical to the reference's for the same seed.  high >= 2 (numpy draws
 * nothing for a range of one value). */
int gsage_mt_choice_segments(uint32_t *state, int64_t high, int64_t n_seg, const int64_t *seg_off,
                             const int64_t *seg_cnt, int32_t *out, void *stream);

/* The same requests served by MANY workgroups (ABI 5; csrc/gsage_mtjump.hip): MT19937 is linear over GF(2), so the
 * state n refills ahead is a convolution of a seed-independent polynomial's bits with the stream's raw words -- a
 * workgroup jumps to its chunk with two table look-ups, pass A counts every chunk's accepted words, a scan turns the
 * counts into offsets, pass B regenerates the chunks and stores value #n of the request at its slot; state and
 * position are left exactly where numpy would leave them (same contract as gsage_mt_choice_segments).
 *   seg_cum [n_seg + 1] (DEVICE): prefix sums of the requests' counts; seg_off [n_seg] (DEVICE); n_total = seg_cum[n_seg]
 *   table (DEVICE): gsage_mt_jump_table()'s 128 x 312 words;  scratch: gsage_mt_choice_par_scratch(n_wg) bytes, 16-byte aligned
 *   n_wg chunks of units_per_wg x 64 refills each (n_wg x units_per_wg <= 4096): choose them to cover
 *   n_total / (624 x acceptance rate) refills with a margin; a serial finisher serves what an unlucky stretch left. */
int gsage_mt_choice_par(uint32_t *state, int64_t high, int64_t n_seg, const int64_t *seg_cum, const int64_t *seg_off,
                        int64_t n_total, int32_t *out, const uint64_t *table, void *scratch, int64_t scratch_bytes,
                        int32_t n_wg, int32_t units_per_wg, void *stream);
int64_t gsage_mt_choice_par_scratch(int32_t n_wg);
/* HOST: the jump polynomials x^(b * 64 * 624) and x^(a * 64 * 64 * 624) mod phi(x), a, b < 64 (phi: MT19937's
 * characteristic polynomial, found by Berlekamp-Massey on the generator's own output bits; ~1 s the first time in a
 * process, callers cache the words).  out: gsage_mt_jump_table_words() x 8 bytes: [b = 0..63 | a = 0..63][312]. */
int gsage_mt_jump_table(uint64_t *out, int64_t words);
int64_t gsage_mt_jump_table_words(void);
/* HOST (tests): out[624] = the state `poly` steps ahead of state[624] (word 0's low 31 bits are not part of the state) */
int gsage_mt_jump_host(const uint32_t *state, const uint64_t *poly, uint32_t *out);
/* np.random.permutation(n) -> int64 out[n]. */
void gsage_mt_permutation(void *mt, int64_t n, int64_t *out);

/* ------------------------------------------------------------------------------------------
 * K2  gather + mean         replaces feats[ids] (models.py:76,80) followed by
 *                           neibs.view(M,-1,D).mean(dim=1) (nn_modules.py:197-198)
 *
 *     out[i, c] = (1/n) * sum_j table[rows(i,j), c],   rows(i,j) = ids ? ids[i*n+j] : i*n+j
 *     n == 1 is the plain row gather feats[ids].  fp32 accumulation; `out` has `out_dtype`.
 *     Columns [D, round_up(D, vec)) of out are written as zero.
 *     PRECONDITION: 0 <= ids[.] < 2^31 (the kernels read the low 32-bit word of each int64 id: node ids of a table
 *     with < 2^31 rows; store.FeatureStore / DeviceCSR refuse larger tables) -- also for gsage_gather_mean_multi(_adam).
 * ---------------------------------------------------------------------------------------- */
int gsage_gather_mean(const void *table, int dtype, int64_t ld, const int64_t *ids, int64_t M,
                      int32_t n, int64_t D, void *out, int out_dtype, int64_t out_ld,
                      void *stream);

/* Up to 8 gather+mean problems (e.g. all hops of one level) in one launch; bf16 in / bf16 out (or
 * fp32 in / fp32 out: the exact-arithmetic parity mode).
 * tables / ids / outs / M / n are HOST arrays of n_seg entries holding DEVICE pointers and sizes;
 * segment s computes outs[s][i] = mean_j tables[s][ rows(i, j) ] exactly like gsage_gather_mean
 * (ids[s] == NULL: rows i*n+j of tables[s]).  All segments share ld, D, out_ld. */
int gsage_gather_mean_multi(int32_t n_seg, const void *const *tables, const int64_t *const *ids,
                            void *const *outs, const int64_t *M, const int32_t *n, int dtype,
                            int64_t ld, int64_t D, int out_dtype, int64_t out_ld, void *stream);

/* ------------------------------------------------------------------------------------------
 * FP8 feature table (opt-in storage of a fixed input-feature table; additive, ABI version unchanged)
 *
 *     table_q[r, c]  one OCP e4m3fn byte (gfx950's hardware format, not MI300X's fnuz), rows of ld_q bytes,
 *                    ld_q % 16 == 0 (store.FeatureStore pads rows to 128 bytes), bytes of columns >= D zero
 *     scale[c]       fp32 [ld_q], 16-byte aligned: an exact power of two, 1.0 for an all-zero or padding column
 *     value          e4m3(table_q[r, c]) * scale[c]  -- exactly representable in bf16
 *
 * gsage_quantize_fp8: scale[c] = the smallest power of two s (2^-126 <= s) with max_r |x[r, c]| / s <= 448;
 * table_q[r, c] = x[r, c] / s rounded to e4m3fn, round-to-nearest-even, saturating at +-448 (never a NaN
 * encoding; a NaN input counts as 0, one beyond +-2^127 as +-2^127, so every decoded value is finite).  Two passes over x: the column maxima
 * (integer atomic max of |x| bits: order-independent, hence deterministic), then the encoding.  dtype = type of
 * x (GSAGE_F32 / GSAGE_BF16), ld its leading dimension in elements.  A one-off: `scale` is cleared by a memset on
 * the stream, so the call is not for recording into a command list.
 * ---------------------------------------------------------------------------------------- */
int gsage_quantize_fp8(const void *table, int dtype, int64_t ld, int64_t n_rows, int64_t D, void *table_q,
                       int64_t ld_q, float *scale, void *stream);

/* out[i, :] = decode(table_q[ids[i], :]) as bf16 or fp32: the FP8 form of the n == 1 row gather. */
int gsage_gather_rows_fp8(const void *table_q, int64_t ld, const float *scale, const int64_t *ids, int64_t M,
                          int64_t D, void *out, int out_dtype, int64_t out_ld, void *stream);

/* gsage_gather_mean / gsage_gather_mean_multi on an FP8 table: 16-byte chunks (16 columns) per lane, fp32
 * accumulation of the UNSCALED e4m3 values in neighbour order, scale[c] applied once per output element before
 * the division by n.  Scaling by a power of two commutes with fp32 rounding, so the result equals, bit for bit,
 * gsage_gather_mean on a bf16 table that holds the decoded values.  out_dtype: GSAGE_BF16 or GSAGE_F32; same
 * output layout, columns [D, round_up(D, 16 bytes of out)) written as zero.  The multi form needs 16-byte
 * aligned outputs whose out_ld is a whole number of 16-byte pieces; the single form falls back to element
 * stores (columns < D only) for any other output. */
int gsage_gather_mean_fp8(const void *table_q, int64_t ld, const float *scale, const int64_t *ids, int64_t M,
                          int32_t n, int64_t D, void *out, int out_dtype, int64_t out_ld, void *stream);
int gsage_gather_mean_multi_fp8(int32_t n_seg, const void *const *tables_q, const int64_t *const *ids,
                                void *const *outs, const int64_t *M, const int32_t *n, const float *scale,
                                int64_t ld, int64_t D, int out_dtype, int64_t out_ld, void *stream);

/* Backward of the segment mean w.r.t. contiguous neighbour rows (autograd of nn_modules.py:198):
 *     dneibs[i*n+j, c] = dagg[i, c] / n          (fp32 in, fp32 out) */
int gsage_segment_mean_bwd(const float *dagg, int64_t ld, int64_t M, int32_t n, int64_t D,
                           float *dneibs, int64_t out_ld, void *stream);

/* K6  table_grad[ids[i], c] += scale * rows[i / n, c]   for i in [0, M*n)  (atomic fp32).
 *     Backward of gather_mean w.r.t. a trainable table (the dense nn.Embedding gradient of
 *     NodeEmbeddingPrep, nn_modules.py:134,146-149); n = 1, scale = 1 for a plain gather. */
int gsage_scatter_add_rows(const float *rows, int64_t ld, const int64_t *ids, int64_t M,
                           int32_t n, int64_t D, float scale, float *table_grad,
                           int64_t table_ld, void *stream);

/* ------------------------------------------------------------------------------------------
 * K5  projection GEMM (MFMA) replaces fc_x(x), fc_neib(agg), cat, activation
 *                           (nn_modules.py:200-202) and every other nn.Linear on the path
 *
 *     act in GSAGE_ACT_{NONE,RELU,TANH}.
 *     for g in [0, groups):   C[m, g*c_gstride + j] = act( sum_k A_g[m,k] * W_g[j,k] + bias_g[j] )
 *         A_g row m  = (a_rows ? A + a_rows[m]*lda : A + m*lda) + g*a_gstride      [M, K]
 *         W_g        = W + g*w_gstride                                             [N, K] row-major
 *         bias_g     = bias ? bias + g*N : none                                    fp32
 *     groups = 2 writes both halves of the concat in one launch (x | agg against Wx | Wn).
 *     `a_rows` (int64 [M], may be NULL, group 0 only when `a_rows_group0_only`) fuses the row
 *     gather feats[ids] into the A-operand load.
 *     dtype = type of A and W (bf16: v_mfma_f32_32x32x16_bf16; fp32: v_mfma_f32_32x32x2_f32),
 *     fp32 accumulation, C stored as c_dtype.  Needs lda, ldw % (16/sizeof) == 0 and zero
 *     padding of A and W in columns [K, round_up(K, 16/sizeof)).
 * ---------------------------------------------------------------------------------------- */
int gsage_linear_nt(const void *A, int dtype, int64_t lda, const int64_t *a_rows,
                    int a_rows_group0_only, const void *W, int64_t ldw, const float *bias,
                    void *C, int c_dtype, int64_t ldc, int64_t M, int64_t N, int64_t K, int act,
                    int groups, int64_t a_gstride, int64_t w_gstride, int64_t c_gstride,
                    void *stream);

/* K5 with the weight operand in MFMA fragment order (bf16 only): a wave's B fragment is one coalesced
 * 1 KiB load from L2 straight into registers, so only A goes through LDS and both operand rings run
 * deeper than LDS capacity allows the plain kernel.  Same arithmetic and
 * arguments as gsage_linear_nt with dtype = bf16; Wp from gsage_pack_weight (or kept current by the
 * optimizer through gsage_prep_desc.dst_p), groups laid out back to back.  A rows must be whole
 * 128-byte lines, zero padded up to round_up(K, 64).
 *     Wp[g][jb][kc][lane][e] = W_g[jb*32 + (lane & 31)][kc*16 + (lane >> 5)*8 + e]   (0 outside N x K)
 *     jb < ceil(N/32), kc < 4*ceil(K/64), lane < 64, e < 8;  gsage_packed_weight_elems() bf16 elements. */
int64_t gsage_packed_weight_elems(int64_t N, int64_t K, int32_t groups);
int gsage_pack_weight(const void *W, int dtype, int64_t ldw, int64_t w_gstride, int64_t N, int64_t K,
                      int32_t groups, void *Wp, void *stream);
int gsage_linear_nt_packed(const void *A, int64_t lda, const int64_t *a_rows, int a_rows_group0_only,
                           const void *Wp, const float *bias, void *C, int c_dtype, int64_t ldc,
                           int64_t M, int64_t N, int64_t K, int act, int groups, int64_t a_gstride,
                           int64_t c_gstride, void *stream);

/* K5b weight gradient (MFMA, bf16 in / fp32 out): the backward of the projection above w.r.t. its
 *     weights (autograd of nn_modules.py:189-190,200 under loss.backward(), models.py:100)
 *
 *     out[g*out_gstride + n*K + k] = sum_m dC[m, g*n_per_group + n] * A_g[m, k]
 *         A_g = A + g*a_gstride  ([M, lda] row-major)      dC, A: bf16;  out: fp32 [groups, n_per_group, K]
 *     The reduction over M is split into ceil(M / rows_per_split) slices whose partial tiles are
 *     written to `slabs` (fp32 [slices, Ntot, ldk], caller-allocated) and summed deterministically
 *     into `out` (out == NULL: the slabs are left for gsage_finalize_grads).
 *     Needs ldc, lda % 8 == 0 and 16-byte aligned dC, A (16-byte lane loads), ldk % 4 == 0,
 *     Ntot % 4 == 0, K <= ldk <= lda, rows_per_split % 16 == 0, n_per_group % 128 == 0 unless there
 *     is a single group. */
int gsage_wgrad(const void *dC, int dtype, int64_t ldc, const void *A, int64_t lda, int64_t a_gstride, int64_t M,
                int64_t Ntot, int64_t K,
                int64_t n_per_group, int64_t rows_per_split, float *slabs, int64_t ldk, float *out,
                int64_t out_gstride, void *stream);
/* [host] number of slabs gsage_wgrad writes for (M, rows_per_split). */
int gsage_wgrad_slabs(int64_t M, int64_t rows_per_split);
/* Up to 8 weight-gradient problems (all the levels of one backward pass) in ONE launch; the partial
 * tiles stay in each problem's slabs for gsage_finalize_grads.  Each problem alone fills a fraction
 * of the chip for the length of its M-slice, so side by side they cost the longest, not the sum.
 * `probs` is a HOST array (copied into the kernel arguments).  Field meaning as in gsage_wgrad. */
typedef struct gsage_wgrad_desc {
    const void *dC;
    const void *A;
    float *slabs;
    int64_t ldc, lda, a_gstride;
    int64_t M, Ntot, K, n_per_group, ldk, rows_per_split;
    const int64_t *a_rows;      /* optional (NULL = A's own rows): reduction index m reads row a_rows[m] of A -- a
                                 * frontier's table rows in place, no gathered copy; 16-byte aligned, ids < 2^32.
                                 * With several groups the list belongs to group 0's operand only (the other groups
                                 * read A + g * a_gstride row by row, like gsage_linear_nt's a_rows_group0_only) */
} gsage_wgrad_desc;
int gsage_wgrad_multi(int32_t n_prob, const gsage_wgrad_desc *probs, int dtype, void *stream);
/* [host] 1 when gsage_wgrad_multi gives a problem's workgroups TWO 128-row output tiles each (its waves pair up on the
 * same rows of A: half the readers per A line; long bf16 reductions with whole tile pairs per group) -- the caller then
 * wants slices half as long for the same number of workgroups (ops.wgrad_plan). */
int gsage_wgrad_pair_ok(int dtype, int64_t M, int64_t Ntot, int64_t n_per_group, int64_t rows_per_split);
/* Device counters for the NEXT gsage_wgrad_multi launch of the calling thread to advance when it starts (consumed by
 * it, also while a command list is being recorded): *tick += 1, *tick1 += inc1, *tick2 += inc2 (any may be NULL).
 * For steps without a finalisation launch (gsage_adam_desc.reduce_descs): the Adam step count, the Philox call
 * counter and the batch-queue index must move AFTER the seed level read them and BEFORE the launch that carries the
 * update and the next frontier's sampling -- K5b sits exactly there and reads none of them. */
int gsage_wgrad_ticks_next(int64_t *tick, int64_t *tick1, int64_t inc1, int64_t *tick2, int64_t inc2);
/* dtype (both entry points) = type of dC and A: GSAGE_BF16 (the MFMA kernel described above) or
 * GSAGE_F32 (plain fp32 FMAs, same decomposition and slab layout: the exact-arithmetic parity mode in
 * which the golden fixtures generated from the reference are replayed through the fused engines). */

/* ------------------------------------------------------------------------------------------
 * K3  pooling MLP           replaces mlp(neibs) -> view(M,-1,H) -> max/mean over the fanout
 *                           (nn_modules.py:224-226 with pool_fn of :240 / :252)
 *
 *     pooled[i, j] = pool_{r in [0,n)} relu( sum_k A[i*n+r, k] * W[j,k] + bias[j] )
 *     A rows are gathered through a_rows when given (A row = A + a_rows[i*n+r]*lda).
 *     argmax (int32 [M, H], may be NULL; max pool only) receives the winning r for backward: the FIRST
 *     maximum of the segment (as torch.max / np.argmax; row 0 when every ReLU'd value is 0).
 *     The [M*n, H] hidden activations are never written to HBM.
 * ---------------------------------------------------------------------------------------- */
int gsage_pool_mlp(const void *A, int dtype, int64_t lda, const int64_t *a_rows, const void *W,
                   int64_t ldw, const float *bias, int64_t M, int32_t n, int64_t H, int64_t K,
                   int pool, float *pooled, int64_t pooled_ld, int32_t *argmax, void *pooled_bf16,
                   int64_t pooled_bf16_ld, uint32_t *relu_mask, void *stream);
/* pooled_bf16 (may be NULL): the same result rounded to bf16, [M, pooled_bf16_ld] -- the operand
 * copy the following projection (gsage_linear_nt) and its weight gradient (gsage_wgrad) read.
 * relu_mask (may be NULL; H % 32 == 0): [M*n, H/32] words, bit c%32 of word c/32 of row r = hidden
 * activation (r, c) > 0 -- all the mean pool's backward needs of the hidden layer. */

/* K3 on the packed weight operand (bf16; see gsage_linear_nt_packed): one workgroup covers 64 rows x
 * 256 hidden columns, so A is read once per 256 columns instead of once per 128, and W goes from L2
 * straight into registers.  Same results and arguments as gsage_pool_mlp; Wp = gsage_pack_weight of
 * the [H, K] weight; A rows must be whole 128-byte lines, zero padded up to round_up(K, 64). */
int gsage_pool_mlp_packed(const void *A, int64_t lda, const int64_t *a_rows, const void *Wp,
                          const float *bias, int64_t M, int32_t n, int64_t H, int64_t K, int pool,
                          float *pooled, int64_t pooled_ld, int32_t *argmax, void *pooled_bf16,
                          int64_t pooled_bf16_ld, uint32_t *relu_mask, void *stream);

/* Backward routing of the max pool: the [M*n, ldo] gradient of the hidden activations, bf16 or fp32 (out_dtype),
 *     out[i*n + j, c] = (argmax[i, c] == j && pooled[i, c] > 0) ? T(g[i, c]) : +0
 * (autograd of nn_modules.py:224-226,240: max picks one row per (segment, channel), ReLU passes
 * positive maxima only) -- the dC operand of gsage_wgrad for the MLP's weight gradient.  Selects, not
 * products: a closed gate (pooled +0, -0, negative or NaN) gives all-zero bits whatever g holds, an open
 * one g's bf16 rounding (fp32: g's own bits).  An argmax outside [0, n) routes nothing: its column is
 * zero in all n rows of the segment.  Every element of rows [0, M*n) x columns [0, H) is written.
 * bf16: H, ldo % 8 == 0;  fp32: H, ldo % 4 == 0;  out 16-byte aligned; ldg, ldp, lda >= H (any
 * alignment: 16-byte loads when all three are multiples of 4 and the pointers 16-byte aligned, else
 * 4-byte loads, the same bits).  M == 0 launches nothing. */
int gsage_pool_route_bwd(const float *g, int64_t ldg, const float *pooled, int64_t ldp,
                         const int32_t *argmax, int64_t lda, int64_t M, int32_t n, int32_t H, void *out,
                         int out_dtype, int64_t ldo, void *stream);

/* Same for the mean pool: out[i*n + j, c] = relu_mask(i*n + j, c) ? T(g[i, c] * fl(1 / n)) : +0   (autograd
 * of nn_modules.py:224-226,252; relu_mask as K3 writes it, [M*n, H/32] words).  The quotient is the
 * product with the ROUNDED fp32 reciprocal -- two roundings, within 2^-23 of g / n, exact for n a power of
 * two -- not a division.  Plus -- when bias_part != NULL -- the MLP bias gradient as n_part deterministic
 * partial rows [n_part, H] (a second launch; summed by gsage_finalize_grads): row b holds
 * (sum over segments i = b, b + n_part, ... of g[i, c] * cnt(i, c)) / n, cnt = the segment's set bits
 * at c, a segment without a set bit contributing nothing whatever g holds; rows no segment feeds
 * (n_part > M) are written as zeros.  H % 32 == 0, ldo % 8 == 0 (both output types), out 16-byte
 * aligned, 1 <= n_part <= 1024. */
int gsage_pool_route_mean_bwd(const float *g, int64_t ldg, const uint32_t *relu_mask, int64_t M, int32_t n,
                              int32_t H, void *out, int out_dtype, int64_t ldo, float *bias_part, int32_t n_part,
                              void *stream);

/* Bias gradient of the pooling MLP under the max pool: column sums of g * (pooled > 0) over the M
 * segments, as `n_part` deterministic partial rows part[b, c] (b < n_part; summed by
 * gsage_finalize_grads with S = n_part, stride = H): row b sums the segments b, b + n_part, ...
 * in that order, rows no segment feeds are zeros.  A select: g behind a closed gate (+0, -0, negative,
 * NaN) adds nothing.  n_part <= 1024; H, ldg, ldp % 4 == 0; g, pooled, part 16-byte aligned. */
int gsage_pool_bias_partials(const float *g, int64_t ldg, const float *pooled, int64_t ldp, int64_t M,
                             int32_t H, float *part, int32_t n_part, void *stream);

/* Input gradient of a pool-aggregator level, merged and masked (autograd of nn_modules.py:224-230
 * w.r.t. the previous level's post-ReLU output Hprev [R, ldh] bf16):
 *     dH[m, c] = (Hprev[m, c] > 0) * ( (m < r_x ? DX[m, c] : 0) + (m >= r0 ? DN[m - r0, c] : 0) )
 * DX fp32 [r_x, ldx] = gradient through fc_x of the rows that were "x", DN fp32 [R - r0, ldn] =
 * gradient through the pooling MLP of the rows that were neighbours.  One IEEE fp32 addition where both
 * apply (a row with DX alone keeps DX's bits, a row with DN alone holds 0 + DN, a row with neither --
 * r_x <= m < r0 -- is written as zeros), then the gate (a select: Hprev +0, -0, negative or NaN gives
 * +0), then the rounding to bf16 when dtype is GSAGE_BF16 (Hprev and dH share dtype).  D and the four
 * leading dimensions % 4 == 0; 0 <= r_x, r0 <= R.  The kernel moves four columns per load and store:
 * DX and DN must be 16-byte aligned, Hprev and dH 16-byte aligned in fp32 and 8-byte aligned in bf16
 * (the caller's obligation: the entry point checks the leading dimensions, not the pointers). */
int gsage_pool_merge_bwd(const void *Hprev, int dtype, int64_t ldh, const float *DX, int64_t ldx, int64_t r_x,
                         const float *DN, int64_t ldn, int64_t r0, void *dH, int64_t ldo, int64_t R,
                         int32_t D, void *stream);

/* ------------------------------------------------------------------------------------------
 * K4  attention aggregation  replaces AttentionAggregator.forward's weighting,
 *                            nn_modules.py:307-315 (scores, softmax over the fanout, weighted
 *                            sum of the RAW neighbour rows)
 *
 *     na[i,r,:] given (att(neibs), [M*n, Ha] fp32), xa[i,:] given (att(x), [M, Ha] fp32)
 *     s[i,r] = <na[i,r,:], xa[i,:]>;  w = softmax_r(s);  agg[i,:] = sum_r w[i,r] * neibs[i*n+r,:]
 *     neibs rows are gathered from `table` through ids when ids != NULL.
 *     ws (fp32 [M, n]) is written for backward.
 * ---------------------------------------------------------------------------------------- */
int gsage_attn_aggregate(const float *na, int64_t na_ld, const float *xa, int64_t xa_ld,
                         const void *table, int dtype, int64_t ld, const int64_t *ids, int64_t M,
                         int32_t n, int64_t Ha, int64_t D, float *agg, int64_t agg_ld, float *ws,
                         void *stream);
/* Same, plus (agg_lp != NULL) the result rounded to the table's type, [M, agg_lp_ld] with zero pad columns -- the
 * operand copy the fc_neib projection and its weight gradient read (no cast launch); agg may then be NULL. */
int gsage_attn_aggregate_lp(const float *na, int64_t na_ld, const float *xa, int64_t xa_ld, const void *table,
                            int dtype, int64_t ld, const int64_t *ids, int64_t M, int32_t n, int64_t Ha, int64_t D,
                            float *agg, int64_t agg_ld, float *ws, void *agg_lp, int64_t agg_lp_ld, void *stream);
/* Second layer of the att MLP (nn_modules.py:292-296: Linear(32, 32, bias=False) after the tanh), Ha == 32:
 *   gsage_attn_mlp2_fwd   a[m, :] = hid[m, :] W2^T                       hid, W2: `dtype` (operand copies), a: fp32
 *   gsage_attn_mlp2_bwd   da = T(dan + dax);  dhid = T((da W2) * (1 - hid^2))   -- the cast, the product and the
 *                         tanh backward of the chain d a -> d hid in one pass; W2T = the transposed operand copy */
int gsage_attn_mlp2_fwd(const void *hid, int dtype, int64_t ldh, const void *W2, int64_t ldw, float *a, int64_t lda,
                        int64_t M, int32_t Ha, void *stream);
int gsage_attn_mlp2_bwd(const float *dan, int64_t ldn, const float *dax, int64_t ldx, const void *hid, int dtype,
                        int64_t ldh, const void *W2T, int64_t ldw, void *da, int64_t ldda, void *dhid, int64_t lddh,
                        int64_t M, int32_t Ha, void *stream);
/* Backward of the weighting w.r.t. att(neibs) and att(x), one launch (autograd of the three lines
 * above):  dws[i,r] = <neibs[i*n+r,:], g[i,:]>;  ds = ws * (dws - sum_r dws*ws);
 *          dxa[i,:] = sum_r ds[i,r] * na[i*n+r,:];   dna[i*n+r,:] = ds[i,r] * xa[i,:].
 * g: fp32 [M, g_ld] gradient of agg.  Rows must be whole 16-byte chunks (ld % 8 == 0 bf16 / % 4 == 0
 * fp32, 16-byte aligned table); n <= 32. */
int gsage_attn_bwd(const float *g, int64_t g_ld, const float *ws, const float *na, int64_t na_ld,
                   const float *xa, int64_t xa_ld, const void *table, int dtype, int64_t ld,
                   const int64_t *ids, int64_t M, int32_t n, int64_t Ha, int64_t D, float *dna,
                   int64_t dna_ld, float *dxa, int64_t dxa_ld, void *stream);

/* K4 / K4' with the attention MLP inside (round 6; csrc/gsage_attn_fused.hip): one pass over a hop's child rows per
 * direction instead of three (the att.0 GEMM with its tanh, gsage_attn_mlp2_fwd and gsage_attn_aggregate_lp; backward
 * gsage_attn_bwd and gsage_attn_mlp2_bwd) -- reference nn_modules.py:293-296 + 309-315 and their autograd.  bf16 rows
 * of whole 16-byte chunks, D <= 640, fan-out 2..16, the reference's 32-wide attention MLP: gsage_attn_fused_ok says
 * whether a shape is covered (1 / 0; no GPU needed).  Child `pos` = parent * n + j is row `ids[pos]` of `table` (ids
 * NULL: row `row0 + pos`); every per-child array is indexed by pos, every per-parent array by the parent.
 *   forward   hid = bf16(tanh(row W0^T)) [M n, hid_ld], a = hid W2^T (fp32) [M n, a_ld] for the children;
 *             ws = softmax_j <a_child, xa_parent> [M n]; agg_lp = bf16(sum_j ws row_j) [M, lp_ld], the operand copy
 *             the fc_neib projection and its weight gradient read, with zero pad columns up to the next multiple of 32
 *             W0 / W2: the bf16 operand copies of att.0.weight [32, ldw0 >= 32 ceil(D / 32)] and att.2.weight [32, ldw2]
 *   backward  dws = <row, g_parent>, ds = ws (dws - sum ws dws); dxa[parent] = sum_j ds_j na_j (fp32 [M, dxa_ld]);
 *             da = bf16(ds xa_parent) [M n, da_ld]; dhid = bf16((da W2)(1 - hid^2)) [M n, dhid_ld] -- the rows of a
 *             LAST hop are nobody's parents, so da has no second term.  W2T[k][h] = W2[h][k]: transposed operand copy
 * Pad columns.  The kernels run KS = 1, 2, 4, 8, 19 or 20 steps of 32 columns, the first of these >= ceil(D / 32), and
 * read cols = 32 KS columns of every row whatever D is: ld, ldw0, g_ld and lp_ld must be >= cols (gsage_attn_fused_ok
 * checks ld: D = 129..192 needs ld >= 256, D = 257..608 needs ld >= 608).  The columns [D, cols) of the table rows and
 * of W0 must be ZERO; those of g may hold anything finite (they meet the rows' zeros); agg_lp gets zeros there, and its
 * columns >= cols, like the columns >= 32 of hid, a, da, dhid and dxa, are not written. */
int gsage_attn_fused_ok(int dtype, int64_t ld, int64_t D, int32_t n, int64_t Ha);
int gsage_attn_fused_fwd(const void *table, int dtype, int64_t ld, const int64_t *ids, int64_t row0, const void *W0,
                         int64_t ldw0, const void *W2, int64_t ldw2, const float *xa, int64_t xa_ld, int64_t M,
                         int32_t n, int64_t D, void *hid, int64_t hid_ld, float *a, int64_t a_ld, float *ws, void *agg_lp,
                         int64_t lp_ld, void *stream);
int gsage_attn_fused_bwd(const void *table, int dtype, int64_t ld, const int64_t *ids, int64_t row0, const void *W2T,
                         int64_t ldw2t, const float *g, int64_t g_ld, const float *ws, const float *na, int64_t na_ld,
                         const float *xa, int64_t xa_ld, const void *hid, int64_t hid_ld, int64_t M, int32_t n, int64_t D,
                         void *da, int64_t da_ld, void *dhid, int64_t dhid_ld, float *dxa, int64_t dxa_ld, void *stream);

/* The trainable node-embedding prep as two row pipelines (round 6; csrc/gsage_prep_rows.hip; reference nn_modules.py:126-155
 * and its autograd).  bf16 operands, 64-wide embeddings: gsage_prep_rows_ok says whether a shape is covered (1 / 0).
 * Frontier position pos reads table row (pos < n_seed ? spare : ids[pos]) -- the seeds all read the spare row n_nodes.
 *   forward   eraw[pos] = bf16(table row); out[pos] = bf16(eraw[pos] W^T + bias): the embedding gather and the prep.fc
 *             projection in one launch (W: prep.fc's bf16 operand copy [64, ldw]; `out` points at the prep's columns of
 *             the level-0 rows)
 *   backward  v = (dhid ? dhid W0 : DATT ? DATT : 0) + (pos < r_x ? DX[pos] : 0) + w(pos) DAGG[parent(pos)]  -- the sources
 *             and the hop layout of gsage_attn_merge_bwd2, no ReLU mask (the prep is affine); dhid [R, lddh] bf16 with
 *             W0T = att.0's transposed operand copy [64, ldw0t] saves the GEMM that would have produced DATT;
 *             din0[pos] = bf16(v); bias_part[b] = column sums of v over workgroup b's rows (n_part workgroups: the
 *             prep.fc.bias gradient's partials); d = bf16(v) WpT^T (WpT[e][c] = prep.fc.weight[c][e]); then either
 *             g_table[row(pos)] += d with fp32 atomics -- the seeds' rows summed per 16-row tile first -- or
 *             (deraw != NULL) deraw[pos] = d and no atomics (the sorted, deterministic table gradient of data-parallel runs) */
int gsage_prep_rows_ok(int dtype, int64_t E);
int gsage_prep_rows_fwd(const float *table, int64_t ldt, const int64_t *ids, int64_t n_seed, int64_t spare, const void *W,
                        int64_t ldw, const float *bias, int64_t M, int64_t E, void *eraw, int64_t lde, void *out,
                        int64_t ldo, void *stream);
int gsage_prep_rows_bwd(const void *dhid, int64_t lddh, const void *W0T, int64_t ldw0t, const float *DATT, int64_t ldatt,
                        const float *DX, int64_t ldx, int64_t r_x, const float *DAGG, int64_t ldagg, const float *ws,
                        int32_t n_hops, const int64_t *off, const int32_t *fan, int64_t R, int64_t E, void *din0,
                        int64_t ldd, float *bias_part, int32_t n_part, const void *WpT, int64_t ldwpt, const int64_t *ids,
                        int64_t n_seed, int64_t spare, float *g_table, int64_t ldg, float *deraw, int64_t ldde,
                        void *stream);

/* The recurrence of the LSTM aggregator and its backward (csrc/gsage_lstm.hip; reference nn_modules.py:259-286 keeps the
 * LAST position of a batch_first LSTM over each node's n neighbour rows, and its autograd).  Gate order i, f, g, o;
 * `dtype` is the compute type of the gates, of the packed weights, of h and of dG (bf16: v_mfma_f32_32x32x16_bf16; fp32:
 * v_mfma_f32_32x32x2_f32); c and all gate arithmetic are fp32.  gsage_lstm_ok says whether a shape is covered (1 / 0; no
 * GPU needed): 1 <= n <= 128, 1 <= H <= 1024 (bf16) / 512 (fp32).  Sequence m, step t is row m n + t of every [M n, .] array.
 *   gsage_lstm_pack_whh   W_hh (fp32 [4 H, ldw]) -> both fragment-ordered copies, gsage_lstm_packed_elems(H) elements of
 *                         `dtype` (16-byte aligned): the forward copy first, the backward copy in the second half
 *   gsage_lstm_fwd        gates: GX = rows W_ih^T + b_ih + b_hh on entry (K5), the activated gates on exit (column g H + u);
 *                         cseq[m n + t] = c_t (fp32 [M n, H]); hprev[m n + t + 1] = h_t for t < n - 1 -- row m n + t is
 *                         the step's INPUT state, rows m n + 0 are the caller's (zero); out[m] = h_{n-1}.
 *                         n == 1 (a zero initial state, no recurrent term): Wp and hprev may be NULL
 *   gsage_lstm_bwd        dh: gradient of out (fp32 [M, lddh]); dG[m n + t] = gradient of step t's pre-activation gates,
 *                         from which d W_ih, d W_hh (= dG^T hprev), the biases (column sums) and d rows (= dG W_ih) follow
 *                         on K5b / K5.  Wp: the BACKWARD copy (second half of gsage_lstm_pack_whh's output); carry: fp32 [M, 2 H]
 *                         scratch (dh_t and dc_t f_t between two steps; may be NULL when n == 1)
 *   gsage_lstm_tile       [host] sequences per workgroup (16 or 32) that gsage_lstm_fwd (backward == 0) / gsage_lstm_bwd
 *                         choose for M sequences of H units on the current device; 0 for an H gsage_lstm_ok refuses */
int gsage_lstm_ok(int dtype, int64_t H, int32_t n);
int gsage_lstm_tile(int dtype, int64_t M, int64_t H, int backward);
int64_t gsage_lstm_packed_elems(int64_t H);
int gsage_lstm_pack_whh(const float *W_hh, int64_t ldw, int64_t H, int dtype, void *Wp, void *stream);
int gsage_lstm_fwd(void *gates, int dtype, int64_t ldg, const void *Wp, int64_t M, int32_t n, int64_t H, float *cseq,
                   void *hprev, int64_t ldh, void *out, int64_t ldo, void *stream);
int gsage_lstm_bwd(const void *gates, int dtype, int64_t ldg, const void *Wp, int64_t M, int32_t n, int64_t H,
                   const float *cseq, const float *dh, int64_t lddh, void *dG, int64_t lddg, float *carry, void *stream);

/* Glue of the native attention train step (engine.FusedAttnTrainStep): what autograd ran as separate cast /
 * add / tanh-backward / expand kernels between K4, K5 and K5b.
 *   gsage_add_cast        dst[m, c] = T(a[m, c] + (b ? b[m, c] : 0))             (fp32 in, bf16 / fp32 out)
 *   gsage_tanh_bwd        out[m, c] = T(g[m, c] * (1 - hid[m, c]^2))             (the att MLP's tanh, nn_modules.py:294)
 *   gsage_attn_merge_bwd  input gradient of an attention level (autograd of nn_modules.py:307-317 w.r.t. x and
 *                         neibs), rows = hops concatenated (hop k from off[k], fan[k] children per parent):
 *       dIn[m] = mask(m) * ( DATT[m] + (m < r_x ? DX[m] : 0) + (hop(m) >= 1 ? ws[m - off[1]] * DAGG[parent(m)] : 0) )
 *       DATT: through att(.), every row; DX: through fc_x; ws: the softmax weights of every (parent, child) pair
 *       in hop order (the ws outputs of gsage_attn_aggregate, back to back); mask = (H[m, c] > 0) when H is given
 *       (the ReLU of the level below), else 1.  DATT may be NULL (no such path: a MEAN aggregator level over an
 *       embedding prep), ws may be NULL (uniform weights 1 / fan[hop]: the mean, nn_modules.py:197-198). */
int gsage_add_cast(const float *a, int64_t lda, const float *b, int64_t ldb, void *dst, int dst_dtype, int64_t ldd,
                   int64_t M, int64_t D, void *stream);
int gsage_tanh_bwd(const float *g, int64_t ldg, const void *hid, int dtype, int64_t ldh, void *out, int64_t ldo,
                   int64_t M, int64_t D, void *stream);
int gsage_attn_merge_bwd(const void *H, int h_dtype, int64_t ldh, const float *DATT, int64_t ldatt, const float *DX,
                         int64_t ldx, int64_t r_x, const float *DAGG, int64_t ldagg, const float *ws, void *out,
                         int out_dtype, int64_t ldo, int64_t R, int32_t D, int32_t n_hops, const int64_t *off,
                         const int32_t *fan, void *stream);
/* gsage_attn_merge_bwd2: the same, plus (out2_bf16 != NULL) a second, bf16 copy of the result [R, ldo2] -- the operand
 * the following GEMMs read when `out` has to stay fp32 (a bias gradient's column sums). */
int gsage_attn_merge_bwd2(const void *H, int h_dtype, int64_t ldh, const float *DATT, int64_t ldatt, const float *DX,
                         int64_t ldx, int64_t r_x, const float *DAGG, int64_t ldagg, const float *ws, void *out,
                         int out_dtype, int64_t ldo, int64_t R, int32_t D, int32_t n_hops, const int64_t *off,
                         const int32_t *fan, void *out2_bf16, int64_t ldo2,
                          void *stream);

/* L1 head of the reference's regression problems, forward + backward (Pokec: problem.py:39-42 behind models.py:90-91,100):
 *     z = E / max(||E||_2, 1e-12);  preds[i] = <z_i, W> + bias;  loss = F.l1_loss(preds [B,1], targets [B])
 * The reference passes targets.squeeze(), so [B,1] against [B] broadcasts to [B,B]: loss = mean_ij |p_i - t_j| and
 * d loss / d p_i = (1/B^2) sum_j sign(p_i - t_j) -- reproduced as is.  One output column (n_classes == 1), B <= 2048.
 * scratch: fp32, gsage_head_l1_scratch(B, D) elements; its first ceil(B / 16) rows of D + 2 floats are per-workgroup
 * partials [d fc.weight (D) | d fc.bias | loss] whose sum is the result (gsage_finalize_grads: S = ceil(B / 16),
 * stride D + 2); dE: [B, ldd] in dE_dtype. */
int gsage_head_l1(const float *E, int64_t lde, const float *W, const float *bias, const float *targets, int64_t B,
                  int64_t D, float *preds, void *dE, int dE_dtype, int64_t ldd, float *scratch, void *stream);
int gsage_head_l1_scratch(int64_t B, int64_t D);
/* The same head on ONE SHARD of a data-parallel batch (ABI 4): `targets` holds the T targets of the GLOBAL batch
 * (every rank's, T <= 8192), E / preds / dE the B rows of this rank.  loss_r = 1/(B T) sum_{i in shard} sum_j |p_i - t_j|,
 * d loss_r / d p_i = 1/(B T) sum_j sign(p_i - t_j): the AVERAGE over the ranks of loss_r and of its gradients equals
 * the single-process loss over the global batch, pair for pair (d p_i depends on p_i and the targets only). */
int gsage_head_l1_sharded(const float *E, int64_t lde, const float *W, const float *bias, const float *targets,
                          int64_t T, int64_t B, int64_t D, float *preds, void *dE, int dE_dtype, int64_t ldd,
                          float *scratch, void *stream);

/* ------------------------------------------------------------------------------------------
 * Classification head, forward + backward   replaces F.normalize(dim=1) -> fc -> F.cross_entropy
 *                                            (models.py:90-91, problem.py:34) and their autograd
 *
 *     z = E / max(||E||_2, 1e-12) (row-wise);  preds = z W^T + bias;  loss = mean CE(preds, targets)
 *     dE (bf16 or fp32, [B, ldd]), dW [C, D], db [C] = gradients of loss;  loss may be NULL.
 *     C <= 64, D <= 1024.  scratch: fp32, gsage_head_ce_scratch(B, C, D) elements = per-workgroup
 *     partials [n_wg][C*D + C + 1] (dW | db | loss); dW == NULL leaves them for gsage_finalize_grads.
 *     batch_idx (may be NULL): targets is a queue [n_batches, B], batch *batch_idx % n_batches is used. */
int gsage_head_ce(const float *E, int64_t lde, const float *W, const float *bias,
                  const int64_t *targets, int32_t B, int32_t C, int32_t D, float *preds, void *dE,
                  int dE_dtype, int64_t ldd, float *dW, float *db, float *loss, float *scratch,
                  const int64_t *batch_idx, int64_t n_batches, void *stream);
int64_t gsage_head_ce_scratch(int32_t B, int32_t C, int32_t D);

/* The head for a WIDE class dimension, forward + backward in one launch (csrc/gsage_head_wide.hip), the three
 * products as exact fp32 MFMAs:
 *
 *     z = E / max(||E||_2, 1e-12);  preds = z W^T + bias                                       (fp32 [B, C])
 *     task 0 (targets int64 [B]):            l_i = logsumexp(preds_i) - preds_i[y_i]              F.cross_entropy
 *     task 1 (targets fp32 [B, ldy >= C]):   l_i = (1/C) sum_c softplus(preds_ic) - y_ic preds_ic
 *                                                                               F.multilabel_soft_margin_loss
 *     loss = (1/Bv) sum_{i < Bv} l_i;  dE (bf16 or fp32, [B, ldd]), dW [C, D], db [C] = its gradients.
 *
 * Limits (GSAGE_EINVAL before any launch, also without a GPU): 1 <= C <= 128, 1 <= D <= 1024, lde, ldd >= D,
 * ldy >= C, task 0 or 1.  Bv: the live rows announced by gsage_head_n_valid_next (consumed by this call on every
 * return path, clamped to [1, B]; B without it); rows Bv .. B-1 get predictions, no loss term, and explicit zeros in
 * dE.  batch_idx (may be NULL): targets is a queue [n_batches, B] (task 1: [n_batches, B, ldy]) and n_valid an array
 * [n_batches]; batch *batch_idx % n_batches is used.
 * scratch: fp32, gsage_head_wide_scratch(B, C, D) floats (-1 outside the limits) = one partial row
 * [dW | db | sum of l_i] of C*D + C + 1 floats per 16 rows of the batch -- gsage_head_ce's convention: with dW == NULL
 * (and db == NULL) the rows are left for gsage_finalize_grads (one gsage_reduce_desc, stride = ld = C*D + C + 1,
 * cols = C*D + C); otherwise a second launch sums them in buffer order into dW, db and, when not NULL, loss.
 * targets == NULL and dE == NULL: forward only -- preds is written, scratch and dE are not touched.
 * No atomics: for fixed (B, C, D) the result is bit-identical from launch to launch. */
int gsage_head_wide(const float *E, int64_t lde, const float *W, const float *bias, const void *targets, int task,
                    int64_t ldy, int32_t B, int32_t C, int32_t D, float *preds, void *dE, int dE_dtype, int64_t ldd,
                    float *dW, float *db, float *loss, float *scratch, const int64_t *batch_idx, int64_t n_batches,
                    void *stream);
int64_t gsage_head_wide_scratch(int32_t B, int32_t C, int32_t D);

/* The whole seed level of a mean-aggregator model in one launch: segment mean of the n sampled
 * neighbours (nn_modules.py:197-198), emb = cat[fc_x(x), fc_neib(agg)] (:200-202, identity
 * activation), the classification head above (models.py:90-91, problem.py:34) and the backward down
 * to the previous level's activations.  H: bf16 [B*(1+n), 256] = previous level output (seed rows,
 * then their n neighbours each); w2 / w2t: bf16 operand copies [2,128,ldw2] / [2,256,ldw2t] of
 * (fc_x | fc_neib) and their transposes.  Writes agg (bf16 [B,256]) and dE (bf16 [B,256]) -- the
 * operands of this level's gsage_wgrad --, preds [B,C], dH (bf16 [B*(1+n),256], ReLU mask of H
 * applied) and the fc.weight | fc.bias | loss partials (layout of gsage_head_ce, scratch size
 * gsage_mean_tail_ce_scratch).  Fixed widths: previous level 256, this level 2h = 256; n <= 32;
 * C <= 64.
 * gather (may be NULL): B / 4 workgroups of ~22 us of dependent phases leave half of the chip idle at
 * B = 512, so n_workgroups extra workgroups of the same launch compute rows [0, rows) of a
 * gsage_gather_mean segment (bf16 table and output, fan-out n = 5, 10 or 15) -- part of the NEXT batch's
 * level-0 gather, which that launch then skips.  Results are those of gsage_gather_mean. */
typedef struct gsage_tail_gather_desc {
    const void *table;
    const int64_t *ids;
    void *out;
    int64_t ld, out_ld, D, rows;
    int32_t n, n_workgroups;
} gsage_tail_gather_desc;
int gsage_mean_tail_ce(const void *H, int32_t B, int32_t n, const void *w2, int64_t ldw2,
                       const void *w2t, int64_t ldw2t, const float *Wfc, const float *bfc, int32_t C,
                       const int64_t *targets, const int64_t *batch_idx, int64_t n_batches, void *agg,
                       void *dE, float *preds, void *dH, float *partial,
                       const gsage_tail_gather_desc *gather, int dtype, void *stream);
/* The same role for the NEXT gsage_linear_nt_packed launch of the calling thread (consumed by it; HOST descriptor, read
 * before gsage_gather_role_next's caller continues -- it may live on the stack until that launch call returns): one
 * more z-slice of the projection's grid (as many workgroups as one group has) gathers rows [0, rows) of the segment.
 * Only with act = ReLU and fan-out 5 or 10 (the level-0 projection of the mean engine: 416 workgroups where 768
 * fit, streaming at half of what a CU keeps in flight); n_workgroups is ignored.  NULL: no role. */
int gsage_gather_role_next(const gsage_tail_gather_desc *gather);
/* A SAMPLER role for the NEXT gsage_linear_nt_packed OR gsage_mean_tail_mfma launch of the calling thread (ABI 5;
 * consumed by whichever comes first; HOST descriptor, read before that launch call returns).  In the seed-level launch
 * (which must carry a gather role): gsage_mean_tail_mfma_sampler_wgs(B, widest) workgroups right behind the seed-level ones --
 * every workgroup of that launch owns a CU, so the caller sizes the gather role for the CUs that are left.  In the
 * projection: one more z-slice of the projection's grid runs the fused
 * multi-hop sampler (gsage_sample_hops) for a LATER batch -- address it through call_base / batch_base, the counters
 * are not touched -- ceil(B / slice size) seeds per workgroup.  K1 is ~9 us of dependent loads that move almost
 * nothing: in the projection's free workgroup slots it is off every critical path.  Only with act = ReLU, a CSR
 * adjacency and no gather role; same frontier as gsage_sample_hops (sampling reads no weights).  NULL: no role. */
int gsage_hops_role_next(const gsage_hops_desc *hops);
/* dtype = storage type of H, w2, w2t, agg, dE, dH: GSAGE_BF16, or GSAGE_F32 -- the same kernel source
 * instantiated on fp32 storage (every bf16 rounding point becomes a no-op; no gather role), used to
 * replay the reference-generated golden fixtures through this kernel at fp32 tolerance. */
int64_t gsage_mean_tail_ce_scratch(int32_t B, int32_t C);
/* The same seed level on the matrix cores (ABI 5; bf16 storage only): 16 seeds per 512-thread workgroup -- one MFMA
 * row tile -- instead of 4 per 256-thread workgroup on the VALU.  ceil(B / 16) workgroups stream the projection
 * weights (32 instead of 128 times at B = 512), both projections and the input gradients run on
 * v_mfma_f32_16x16x32_bf16, the head (logits, d z, d fc.weight) on v_mfma_f32_16x16x4_f32 (exact fp32 products, as
 * on the VALU).  Same arguments, same outputs and rounding points as gsage_mean_tail_ce with dtype = GSAGE_BF16
 * (sums run in a different order: results agree to fp32 round-off, agg / dE / dH to one bf16 rounding); the partials
 * are ceil(B / 16) rows (gsage_mean_tail_mfma_scratch).  gather: the role's workgroups are 512 threads here. */
int gsage_mean_tail_mfma(const void *H, int32_t B, int32_t n, const void *w2, int64_t ldw2,
                         const void *w2t, int64_t ldw2t, const float *Wfc, const float *bfc, int32_t C,
                         const int64_t *targets, const int64_t *batch_idx, int64_t n_batches, void *agg,
                         void *dE, float *preds, void *dH, float *partial,
                         const gsage_tail_gather_desc *gather, void *stream);
int64_t gsage_mean_tail_mfma_scratch(int32_t B, int32_t C);
/* workgroups a sampler role (gsage_hops_role_next) adds to that launch for a batch of B seeds whose widest hop holds
 * `widest` ids per seed (the product of the fan-outs so far); 0: the role's frontier does not fit the launch's LDS */
int32_t gsage_mean_tail_mfma_sampler_wgs(int64_t B, int64_t widest);

/* ------------------------------------------------------------------------------------------
 * Fused tail of train_step (models.py:101-102) and inter-layer backward routing (models.py:85-86
 * under autograd), used by the hipGraph engine.
 * ---------------------------------------------------------------------------------------- */

/* clip_grad_norm(params, max_norm) + Adam(betas, eps, L2 weight_decay) over FLAT fp32 buckets of n
 * elements: p (parameters), g (gradients; overwritten with the clipped gradient), m, v (Adam
 * moments).  lr and step are DEVICE scalars (float / int64) so a captured graph follows the LR
 * schedule and counts steps.  step_is_current == 0: this call is update number *step + 1 and
 * increments *step afterwards; != 0: *step was already advanced for this update (by
 * gsage_prep_weights' / gsage_finalize_grads' tick) and is left alone.  partial: fp32 scratch of
 * gsage_adam_partials(n) elements.  norm_out (may be NULL) receives the pre-clip gradient norm.
 * (step_is_current & 2: the caller consumes g in this call and zeroes it next -- a scatter-added
 * embedding-table gradient --, so the clipped values are not written back.  step_is_current & 4: use the
 * arithmetic of the deferred row updates (gsage_rows_*: 1-ulp sqrt and reciprocal) instead of
 * torch.optim.Adam's correctly rounded sqrt and division, so that a table updated densely here and row by
 * row there gets the same bits; every other caller leaves the bit clear and gets torch's roundings.)
 * n_partial_ready > 0: `partial` already holds that many squared-norm partials (written by
 * gsage_finalize_grads) and the norm pass is skipped.  prep_descs (DEVICE array of n_prep
 * gsage_prep_desc whose src point into p; may be NULL): the bf16 operand copies of the updated
 * weights are refreshed in the same launch.
 * beta1, beta2, eps, weight_decay and max_norm are FLOAT arguments: the update is Adam with the float32 roundings of
 * the caller's values, and 1 - beta is formed from those.  1 - float32(0.999) = 0.00099998713 is 1.3e-5 (relative)
 * below 0.001, so against torch.optim.Adam(betas=(0.9, 0.999)), whose 1 - beta2 is a double, the g^2 term of v is
 * smaller by that fraction (|dv| <= 1.3e-8 (g^2 + v)); for beta1 the fraction is 2.4e-7.
 */
int gsage_clip_adam_step(float *p, float *g, float *m, float *v, int64_t n, float *partial,
                         const float *lr, int64_t *step, float beta1, float beta2, float eps,
                         float weight_decay, float max_norm, float *norm_out, int step_is_current,
                         int32_t n_partial_ready, const void *prep_descs, int32_t n_prep,
                         int64_t *tick1, int64_t inc1, int64_t *tick2, int64_t inc2, void *stream);
/* The same arguments as a struct (HOST memory), for gsage_gather_mean_multi_adam. */
typedef struct gsage_adam_desc {
    float *p, *g, *m, *v;
    int64_t n;
    float *partial;
    const float *lr;
    int64_t *step;
    float beta1, beta2, eps, weight_decay, max_norm;
    float *norm_out;
    int32_t step_is_current, n_partial_ready;
    const void *prep_descs;
    int32_t n_prep;
    int64_t *tick1;
    int64_t inc1;
    int64_t *tick2;
    int64_t inc2;
    /* ABI 4, gsage_gather_mean_multi_adam only: the update's workgroups form the squared norm of g THEMSELVES
     * (n_partial_ready == 0 and norm_slots given).  They are few (one per 1 024 elements, <= 1 024 of them, dispatched
     * first, all resident at once).  Each loads the elements it is about to update, publishes their partial as
     * norm_slots[its index] = (update number << 32 | float bits) with ONE device-scope store, and polls the slots of
     * the others until all carry this update's number; every workgroup then adds the same partials in the same order.
     * No counter, no reset between launches (*step must change from launch to launch: it is the update number).  For
     * the data-parallel step: the norm of the AVERAGED gradient exists only after the exchange, and a launch of its
     * own for it sat on the critical path behind the collective.  norm_slots: >= 1 024 x 8 bytes, zero-initialised. */
    uint64_t *norm_slots;
    /* ABI 5 (with norm_slots, n_partial_ready == 0): NO finalisation launch ran -- g does not exist yet.  reduce_descs:
     * DEVICE array of n_reduce (<= 16) gsage_reduce_desc (below) that together cover [0, n): every update workgroup
     * sums the partial buffers of the 1 024 elements it is about to update in buffer order 0 .. S-1, stores them to g
     * (then the clipped values, when the clip is active) and goes on as above.  Those are the bits gsage_finalize_grads
     * produces where it adds in buffer order too -- its 16-byte and scalar paths (S < 32, or descriptors that fill
     * their grid row) --; where it shares the partials of an element among threads (S >= 32 with few elements: per-share
     * sums met in LDS) the two agree within the summation bound S 2^-24 sum |x_s| of a float32 sum, not bit for bit.  Replaces the finalisation launch of the single-GPU step (~6.5 us between K5b and the update,
     * reading the same partial buffers); a data-parallel step keeps it (the exchange needs the flat bucket).  The
     * step's ticks then ride in the K5b launch (gsage_wgrad_ticks_next).  NULL: g holds the gradient. */
    const void *reduce_descs;
    int32_t n_reduce;
} gsage_adam_desc;
/* The update of a gsage_adam_desc with norm_slots as a launch of its own (per-call steps: nothing to ride with):
 * one workgroup per 1 024 elements, all resident (<= 1 024 and <= gsage_gather_adam_capacity of an LDS-free launch). */
int gsage_clip_adam_meet(const gsage_adam_desc *adam, void *stream);
/* Workgroups of gsage_gather_mean_multi_adam's launch that are resident at once on the current device when the
 * sampler role needs lds_bytes of dynamic LDS (one per CU kept as margin): the in-launch norm is admitted only when
 * the update's workgroups -- ceil(n / 1024) -- all fit; callers fall back to norm partials otherwise.  dtype: of the
 * gathered table.  0 on failure. */
int gsage_gather_adam_capacity(int dtype, int64_t lds_bytes);
/* tick1 / tick2 (may be NULL): *tick1 += inc1, *tick2 += inc2 when the kernel starts (e.g. the
 * Philox call index and batch-queue index, when nothing in the same launch reads them). */
/* Live rows for the NEXT head launch of the calling thread (gsage_head_ce, gsage_mean_tail_ce, gsage_head_l1),
 * consumed by it -- also while a command list is being recorded, the pointer then belongs to the recorded
 * launch.  n_valid: DEVICE int32, one word (or [n_batches], indexed like the target queue when the head is given
 * a batch_idx).  Rows past n_valid are padding: they get predictions, but no loss term and a zero gradient,
 * and the loss / gradient means run over n_valid rows.  Why: the reference's `iterate` (problem.py:141-153) cuts
 * an epoch into near-equal chunks that are never all of one size, while a recorded step has one geometry -- short
 * chunks are padded to it.  NULL (the default): every row is live. */
int gsage_head_n_valid_next(const int32_t *n_valid);
/* 1 while a count announced by gsage_head_n_valid_next waits for the calling thread's next head launch, else 0 (a peek:
 * nothing is consumed).  Every head entry point takes the count before its first return path, refusals included. */
int gsage_head_n_valid_pending(void);

/* gsage_gather_mean_multi (the NEXT batch's level-0 gathers: they read features and ids only) with up
 * to two short latency-bound jobs riding in the same launch, each a few hundred workgroups that are
 * free next to the HBM-bound gather:
 *   adam (may be NULL)  the clip + Adam update of the CURRENT batch (~8 us alone).  n_partial_ready
 *                       must be > 0 (norm partials from gsage_finalize_grads) -- or 0 with norm_slots given
 *                       (the norm is formed inside the launch) -- and step_is_current != 0.
 *   hops (may be NULL)  gsage_sample_hops_philox of the batch AFTER the next one (~9 us alone) into
 *                       its own frontier buffer (hops->ids must not alias the ids being gathered).
 *                       adam's ticks must then not touch hops->call_ctr / hops->batch_idx: address the
 *                       future batch through call_base / batch_base instead.
 * At least one of the two must be given. */
int gsage_gather_mean_multi_adam(int32_t n_seg, const void *const *tables, const int64_t *const *ids,
                                 void *const *outs, const int64_t *M, const int32_t *n, int dtype,
                                 int64_t ld, int64_t D, int out_dtype, int64_t out_ld,
                                 const gsage_adam_desc *adam, const gsage_hops_desc *hops, void *stream);

/* Sums partial gradient buffers into the flat bucket and emits the squared-norm partials the
 * clip needs, in one launch: for descriptor d, flat_g[out_off + r*cols + c] =
 * sum_{s<S} src[s*stride + r*ld + c].  Covers the K5b slabs (call gsage_wgrad with out == NULL)
 * and the head partials (gsage_head_ce with dW == NULL: one row of C*D + C columns, ld = stride
 * = C*D + C + 1).  descs: DEVICE array.  partial_sq: gsage_finalize_partials(n_desc, max_elems)
 * floats.  tick (may be NULL): *tick += 1 (the Adam step counter); tick1 / tick2 (may be NULL):
 * *tick1 += inc1, *tick2 += inc2 (Philox call index, batch-queue index). */
typedef struct {
    const float *src;
    int64_t stride;
    int64_t out_off;
    int32_t S, rows, cols, ld;
} gsage_reduce_desc;
int gsage_finalize_grads(const void *descs, int32_t n_desc, int64_t max_elems, float *flat_g,
                         float *partial_sq, int64_t *tick, int64_t *tick1, int64_t inc1,
                         int64_t *tick2, int64_t inc2, void *stream);
int gsage_finalize_partials(int32_t n_desc, int64_t max_elems);
/* Pieces of the same tail for a bucket that holds a trainable embedding table (NodeEmbeddingPrep, config 4:
 * a dense 418 MB gradient by the reference's semantics):
 *   gsage_grad_sqnorm      partial[b] = sum of g[i]^2 over block b's slice (n_partial <= 1024 blocks): squared-norm
 *                          partials of a bucket slice, to sit next to gsage_finalize_grads' in one `partial` array
 *   gsage_zero_rows        table[ids[r], 0:D] = 0: undoes a gsage_scatter_add_rows once the optimizer has consumed
 *                          it -- the gradient table is zeroed by touching the rows that were written, not all of it
 *   gsage_colsum_partials  part[b, c] = sum_{i = b, b + n_part, ...} src[i, c]: a Linear's bias gradient as
 *                          deterministic partial rows (summed by gsage_finalize_grads, S = n_part, stride = D) */
int gsage_grad_sqnorm(const float *g, int64_t n, float *partial, int32_t n_partial, void *stream);
int gsage_zero_rows(float *table, int64_t ld, const int64_t *ids, int64_t M, int64_t D, void *stream);
int gsage_colsum_partials(const float *src, int64_t ld, int64_t M, int32_t D, float *part, int32_t n_part, void *stream);
int gsage_adam_partials(int64_t n);

/* Deferred ("lazy") Adam over the rows of a trainable embedding table: the reference's dense update
 * (torch.optim.Adam over nn.Embedding.weight, nn_modules.py:131-155 + models.py:44-46), applied row by row
 * and bit-identical to gsage_clip_adam_step over the whole table.  The update of a row whose gradient is zero
 * (m, v decay; p moves by -step_size * m / (sqrt(v) / sqrt(bc2) + eps); weight decay adds wd * p) depends on that
 * row alone, so it is replayed when the row is next needed instead of streaming the table every step:
 *   last[r]   number of the last update applied to row r (initialise to the optimizer's step count)
 *   seen[r]   stamp used to count every row once in the norm (initialise to 0)
 *   hist      2 * hist_cap floats: (step_size, 1/sqrt(bc2)) of update t at slot t % hist_cap, written by
 *             gsage_rows_adam (hist_cap: a power of two) -- every row must be caught up at least once every
 *             hist_cap - 1 updates
 * The update number of a call is *step + step_off (device counter, like gsage_clip_adam_step).
 *   gsage_rows_catch_up      rows ids0[0:n0] ++ ids1[0:n1] (duplicates allowed) brought up to that update --
 *                            BEFORE the forward reads them
 *   gsage_rows_catch_up_all  every row -- before anything else reads the table, m or v
 *   gsage_rows_sqnorm        partial[0:n_partial] = squared-norm partials of the listed gradient rows, each row
 *                            once (to sit beside gsage_finalize_grads' partials)
 *   gsage_rows_adam          clip (total norm from partial[0:n_partial_ready]) + update of the listed rows, each
 *                            once, and their gradient rows zeroed; records the update's constants in hist.
 *                            Must run for EVERY update (also with empty lists). */
typedef struct gsage_row_adam {
    float *p, *g, *m, *v;           /* [n_rows, E] fp32, dense rows, 16-byte aligned */
    int32_t *last, *seen;           /* [n_rows] */
    float *hist;
    const float *lr;                /* device scalar */
    const int64_t *step;            /* device counter */
    int64_t n_rows;
    int32_t E, hist_cap;            /* E % 4 == 0, E <= 256 */
    float beta1, beta2, eps, weight_decay, max_norm;
    int32_t sorted_ids;             /* ABI 4: != 0: ids0[0:n0] is sorted ascending and n1 == 0 -- the first entry of a run of
                                       equal ids does the row's work, the others are skipped by comparing neighbours:
                                       no atomics, `seen` unused, and the order in which gsage_rows_sqnorm adds its
                                       terms depends on the list alone (data-parallel replicas stay bit-identical) */
} gsage_row_adam;
int gsage_rows_catch_up(const gsage_row_adam *d, const int64_t *ids0, int64_t n0, const int64_t *ids1, int64_t n1,
                        int32_t step_off, void *stream);
int gsage_rows_catch_up_all(const gsage_row_adam *d, int32_t step_off, void *stream);
int gsage_rows_sqnorm(const gsage_row_adam *d, const int64_t *ids0, int64_t n0, const int64_t *ids1, int64_t n1,
                      int32_t step_off, float *partial, int32_t n_partial, void *stream);
int gsage_rows_adam(const gsage_row_adam *d, const int64_t *ids0, int64_t n0, const int64_t *ids1, int64_t n1,
                    int32_t step_off, const float *partial, int32_t n_partial_ready, void *stream);

/* Deterministic gradient of a trainable table (ABI 4): the reference's dense `nn.Embedding` gradient
 * (nn_modules.py:131-155 under autograd) is the sum of the gradient rows of every occurrence of a node in the frontier.
 * gsage_scatter_add_rows forms it with fp32 atomics -- an order of additions that changes from run to run and, in a
 * data-parallel run, from rank to rank (the replicas' tables would drift apart bit by bit).  Here instead:
 *   gsage_sort_rows      keys[i] = i < n0 ? ids0[i] : tail_id  (i < n0 + n_tail: a frontier's ids followed by n_tail
 *                        entries of one spare row, e.g. the row every seed reads, nn_modules.py:147-149) sorted
 *                        ascending, STABLE: ids_sorted[0:n], pos_sorted[0:n] = original positions, ascending within
 *                        equal ids.  Only the low key_bits bits are compared (ids < 2^key_bits).  The library's own
 *                        radix sort (round 6: 8 bits per pass, three launches per pass; rocPRIM's until then);
 *                        temp: gsage_sort_rows_temp_bytes(n, key_bits) bytes of 16-byte-aligned device scratch.
 *                        Recordable like any kernel of the library.
 *   gsage_segment_sum_rows   for the first entry i of every run of equal ids:
 *                        table[ids_sorted[i], 0:E] = scale * sum_{j in run, in order} rows(pos_sorted[j]),
 *                        rows(p) = p < n0 ? rows0[p * ld0 : ] : rows1[(p - n0) * ld1 : ]     (fp32, E % 4 == 0, E <= 256)
 *                        -- stores, not atomics: rows of the table that are in no run are not touched.
 * Then gsage_rows_sqnorm / gsage_rows_adam over ids_sorted with sorted_ids = 1. */
int64_t gsage_sort_rows_temp_bytes(int64_t n, int32_t key_bits);
int gsage_sort_rows(const int64_t *ids0, int64_t n0, int64_t tail_id, int64_t n_tail, int32_t key_bits,
                    int64_t *ids_sorted, int32_t *pos_sorted, void *temp, int64_t temp_bytes, void *stream);
int gsage_segment_sum_rows(const int64_t *ids_sorted, const int32_t *pos_sorted, int64_t n, const float *rows0,
                           int64_t ld0, int64_t n0, const float *rows1, int64_t ld1, int32_t E, float scale,
                           float *table, int64_t ldt, void *stream);

/* One launch converting fp32 parameters into the bf16 operand copies K5 / K5b read:
 * dst[r, c] = bf16(src[r, c]) with leading dimension dst_ld, and/or the transposed copy
 * dst_t[c, r] (leading dimension dst_t_ld), and/or the fragment-ordered copy dst_p (see
 * gsage_linear_nt_packed).  `descs` is a DEVICE array of n_desc descriptors; padding of dst / dst_t /
 * dst_p is not written (allocate them zeroed).
 * max_elems = max rows*cols over the descriptors.  Being the first launch of a step it can also
 * advance two device counters: *tick0 += inc0, *tick1 += inc1 (either pointer may be NULL). */
typedef struct {
    const float *src;
    uint16_t *dst;
    uint16_t *dst_t;
    int32_t rows, cols, dst_ld, dst_t_ld;
    uint16_t *dst_p;       /* optional: the gsage_linear_nt_packed operand of THIS matrix (one group) */
    int64_t kc_p;          /* its k chunks per column block: 4 * ceil(cols / 64) */
    int32_t dst_f32;       /* != 0: dst / dst_t are fp32 copies of the same layout (parity mode); dst_p unused */
    int32_t reserved;
} gsage_prep_desc;
int gsage_prep_weights(const void *descs, int32_t n_desc, int64_t max_elems, int64_t *tick0,
                       int64_t inc0, int64_t *tick1, int64_t inc1, void *stream);

/* Gradient of a level's ReLU output H (bf16 [R, ldh], rows = hops concatenated, hop k starting at
 * row off[k] with fan-out fan[k] relative to hop k-1):
 *     dH[m] = (H[m] > 0) * ( (m < r_x ? DG[m, 0:D] : 0)
 *                          + (hop(m) >= 1 ? DG[parent(m), dagg_off : dagg_off + D] / fan[hop(m)] : 0) )
 *     parent(m) = off[k-1] + (m - off[k]) / fan[k]
 * DG: fp32 [r_x, ldg] = the level above's (dX | dAgg); dH: bf16 [R, ldo].  off / fan: HOST arrays
 * of n_hops (<= 6) entries. */
int gsage_bwd_merge(const void *H, int dtype, int64_t ldh, const float *DG, int64_t ldg, int64_t dagg_off,
                    void *dH, int64_t ldo, int64_t R, int64_t r_x, int32_t D, int32_t n_hops,
                    const int64_t *off, const int32_t *fan, void *stream);

/* ------------------------------------------------------------------------------------------
 * Metrics of the train / eval log     replaces ProblemMetrics, problem.py:44-64 (sklearn f1_score on
 *                                     host copies of predictions and targets, called per batch at
 *                                     train.py:150)
 *
 *   gsage_metric_f1: out[0] = micro-F1, out[1] = macro-F1 of
 *       classification (multilabel == 0): argmax_c logits[i, c] against targets int64 [B]; the macro
 *                      mean runs over the classes that occur in targets or predictions (sklearn's label set)
 *       multilabel     (multilabel != 0): logits[i, c] > 0 against targets [B, ldy] (float32 when
 *                      targets_f32, else int64; non-zero = positive); macro over all C labels
 *     counts: int32 scratch [3 * C + 1] (tp | fp | fn per class, integer atomics: exact; + the number of
 *     classification targets outside [0, C)).  out: DOUBLE [3] -- micro, macro, that number: sklearn would
 *     add such a label to its label set, so a caller that sees out[2] != 0 must score the batch on the host
 *     (problem.DeviceMetrics does).  argmax: first maximum wins and a NaN logit wins over numbers (np.argmax).
 *   gsage_metric_mae: out[0] (DOUBLE) = mean |y_true[i] - y_pred[i]| over n elements (problem.py:62-64).
 * ---------------------------------------------------------------------------------------- */
int gsage_metric_f1(const float *logits, int64_t ld, const void *targets, int multilabel, int targets_f32,
                    int64_t ldy, int64_t B, int32_t C, int32_t *counts, double *out, void *stream);
int gsage_metric_mae(const float *y_true, const float *y_pred, int64_t n, double *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Full-neighbourhood segment reduce (layer-wise inference, infer.py)
 *
 *     out[v, c] = reduce_{u in N(v)} table[u, c]   for every row v of a CSR adjacency, c < D
 *     N(v) = col[rowptr[v] .. rowptr[v+1]); a row of degree 0 has the single neighbour 0 (the dummy).
 *   mode GSAGE_SEG_MEAN:              (1/|N(v)|) sum
 *   mode GSAGE_SEG_MAX:               max
 *   mode GSAGE_SEG_SOFTMAX_WEIGHTED:  sum_u softmax_u(keys[u, :32] . keys[v, :32]) table[u, c]
 *     (keys: fp32 [n_rows, ldk], ldk >= 32, 16-byte aligned rows; online softmax, fp32).
 *   table: bf16 or fp32 (dtype), ld a multiple of 16 bytes with round_up(D, 16 bytes) <= ld; fp32 accumulation.
 *   out: bf16 or fp32 (out_dtype) [n_rows, out_ld] -- may point into the middle of a wider row (the right half
 *   of a concat); only columns < D are stored.  act: GSAGE_ACT_NONE or GSAGE_ACT_RELU (epilogue).
 *   Plan (built by the caller once per adjacency):
 *     order     int32 [n_short]         rows of degree <= slice_len (their order is the schedule: degree-descending)
 *     slices    int64 [n_slices, 2]     (row, first edge) of the slice_len-edge slices of every longer row
 *     long_rows int64 [n_long, 2]       (row, index of its first slice); the slices of a row are consecutive
 *   partials: fp32 [n_slices, ldp], ldp >= gsage_segment_reduce_ldp(D), 16-byte aligned (unused if n_slices == 0).
 *   Two launches (short rows + slices, then the per-row merge in slice order); no floating-point atomics: the same
 *   inputs give the same bits.  err_flag (int32, may be NULL) is set to 1 when a neighbour id is outside
 *   [0, n_rows); such an id reads row 0.
 * ---------------------------------------------------------------------------------------- */
enum { GSAGE_SEG_MEAN = 0, GSAGE_SEG_MAX = 1, GSAGE_SEG_SOFTMAX_WEIGHTED = 2, GSAGE_SEG_WEIGHTED_MEAN = 3 };
/* HOST: the smallest row length of the partials buffer for width D (-1 when D <= 0) */
int64_t gsage_segment_reduce_ldp(int64_t D);
int gsage_segment_reduce(int mode, const void *table, int dtype, int64_t ld, int64_t D, const float *keys,
                         int64_t ldk, const int64_t *rowptr, const int32_t *col, int64_t n_rows,
                         const int32_t *order, int64_t n_short, const int64_t *slices, int64_t n_slices,
                         const int64_t *long_rows, int64_t n_long, int32_t slice_len, float *partials,
                         int64_t ldp, void *out, int out_dtype, int64_t out_ld, int act, int32_t *err_flag,
                         void *stream);

/* ------------------------------------------------------------------------------------------
 * Unsupervised GraphSAGE (csrc/gsage_unsup.hip): random-walk positives, degree^0.75 negatives, skip-gram head
 *
 * gsage_unsup_batch -- one launch.  From B seed ids it writes the encoder's id batch
 *     ids    int64 [2B + Q] = [seeds (B) | positives (B) | negatives (Q)]        pair_w  fp32 [B]
 * Every draw is a word of Philox4x32-10 (the sampler's generator) under a ROLE TAG xored into the key's high word:
 *     call       = call_base + (call_ctr ? *call_ctr : 0)           (call_ctr: device word, may be NULL)
 *     P(c, tag)  = philox4x32_10({lo(c), hi(c), lo(call), hi(call)}, {lo(seed), hi(seed) ^ tag})     (four words)
 *   Positive of seed i (global index g = g0 + i; a shard [g0, g0 + B) of a larger batch draws what the whole draws):
 *     t_i  = 1 + ((P(g, 0x4C000000)[0] * walk_len) >> 32)                        (64-bit product; 1 <= walk_len <= 16)
 *     v    = seeds[i];  for j = 0 .. t_i - 1:
 *              beg = rowptr[v], deg = rowptr[v + 1] - beg;   deg <= 0: the walk ends at v
 *              word = P(g, 0x53000000 | (j >> 2))[j & 3]
 *              off  = deg <= 2^32 - 1 ? (word * deg) >> 32 : word                (64-bit product)
 *              v    = col[beg + off]
 *     ids[B + i] = v;  pair_w[i] = (v == seeds[i]) ? 0 : 1;  ids[i] = seeds[i]
 *     An id outside [0, n_rows) -- a seed, or a node the walk reaches -- raises *err_flag (int32, may be NULL) and
 *     ends the walk at node 0: ids[B + i] = 0; such a seed is also written as ids[i] = 0 with pair_w[i] = 0.
 *   Negative q (the same Q ids for every seed and every shard: g0 does not enter):
 *     r = P(q, 0x4E000000);  u = ((uint64)r[0] << 21 | r[1] >> 11) * 2^-53      (53 bits, exact in a double)
 *     x = u * cdf_total                                                           (one double multiplication)
 *     ids[2B + q] = min(first i with cdf[i] > x, n_rows - 1)                      (binary search)
 *   cdf: DOUBLE [n_rows], the inclusive running sum of non-negative row weights (the model: degree^0.75), so a row of
 *   weight 0 is never drawn; cdf_total: the HOST's copy of cdf[n_rows - 1], read once when the table is built --
 *   cdf_total <= 0 (or not finite) is GSAGE_EINVAL before anything is launched.  Q >= 1, 1 <= B < 2^31.
 * ---------------------------------------------------------------------------------------- */
int gsage_unsup_batch(const int64_t *rowptr, const int32_t *col, int64_t n_rows, const int64_t *seeds, int64_t B,
                      int32_t walk_len, int64_t Q, const double *cdf, double cdf_total, uint64_t seed,
                      const uint64_t *call_ctr, uint64_t call_base, uint64_t g0, int64_t *ids, float *pair_w,
                      int32_t *err_flag, void *stream);

/* gsage_head_skipgram -- forward + backward in two launches.  E: fp32 [2B + Q, lde], the encoder's un-normalised rows
 * in the order of gsage_unsup_batch;  z = E / max(||E||_2, 1e-12) row-wise (F.normalize, inside the head):
 *     a_i  = <z_i, z_{B+i}>          n_iq = <z_i, z_{2B+q}>          softplus(x) = max(x, 0) + log1p(exp(-|x|))
 *     loss = (1/B) sum_i [ pair_w[i] softplus(-a_i) + neg_weight sum_q softplus(n_iq) ]
 *   loss: one float.  aff (may be NULL): fp32 [B, 1 + Q] = [a_i | n_i0 .. n_i,Q-1].  dE: [2B + Q, ldd], bf16 or fp32
 *   (dE_dtype) = d loss / d E, i.e. through the normalisation.  1 <= Q <= 64, 1 <= D <= 1024, lde >= D, ldd >= D.
 *   Launch 1: a workgroup per 16 seeds writes their rows and their positives' rows of dE, aff, and its partial of
 *   d z of the negatives and of the loss into scratch (fp32, gsage_head_skipgram_scratch(B, Q, D) elements =
 *   [ceil(B / 16)][Q * D + 1]).  Launch 2: a workgroup per negative sums the partials in workgroup order and applies
 *   that row's normalisation backward; it also sums the loss.  No floating-point atomics: same inputs, same bits. */
int gsage_head_skipgram(const float *E, int64_t lde, int32_t B, int32_t Q, int32_t D, const float *pair_w,
                        float neg_weight, void *dE, int dE_dtype, int64_t ldd, float *loss, float *aff, float *scratch,
                        void *stream);
int64_t gsage_head_skipgram_scratch(int32_t B, int32_t Q, int32_t D);

/* gsage_head_skipgram_live -- the same two launches for a batch of fixed geometry whose last seeds are padding (the
 * fused unsupervised engine: the reference's array_split chunks are never all of one size).  n_valid: device int32
 * word, read by the kernels as gsage_head_ce reads its own; b = clamp(*n_valid, 1, B) seeds are live:
 *     loss = (1/b) sum_{i < b} [ pair_w[i] softplus(-a_i) + neg_weight sum_q softplus(n_iq) ]
 *   Seeds i >= b add nothing to the loss or to d z of the negatives, their rows of aff are left as they were, and rows
 *   i and B + i of dE are written as zeros (the weight-gradient launch reads every row).  Every workgroup still
 *   writes its partial and launch 2 sums all of them in workgroup order.  n_valid == NULL, or *n_valid >= B: the bits
 *   of gsage_head_skipgram.  Same scratch, same limits, same errors.  Additive; the ABI version is unchanged. */
int gsage_head_skipgram_live(const float *E, int64_t lde, int32_t B, int32_t Q, int32_t D, const float *pair_w,
                             float neg_weight, const int32_t *n_valid, void *dE, int dE_dtype, int64_t ldd, float *loss,
                             float *aff, float *scratch, void *stream);

/* gsage_unsup_batch_weighted -- gsage_unsup_batch over a weighted adjacency ("Weighted adjacency" below): one launch,
 * the same outputs (ids, pair_w), the same call / g / err_flag conventions, shards concatenate to the one-rank draw.
 * edge_cdf: the adjacency's table from gsage_edge_cdf_build (uint64 [nnz], aligned with col).  Only the walk's steps
 * differ: each is drawn in proportion to the edge quanta, under a role tag of its own.
 *   Positive of seed i (g = g0 + i):
 *     t_i  = 1 + ((P(g, 0x4C000000)[0] * walk_len) >> 32)                        (the lengths of the unweighted batch)
 *     v    = seeds[i];  for j = 0 .. t_i - 1:
 *              beg = rowptr[v], end = rowptr[v + 1];   T_v = end > beg ? edge_cdf[end - 1] : 0
 *              T_v == 0 (an empty row, or one without a drawable edge): the walk ends at v
 *              w    = P(g, 0x5A000000 | (j >> 1));   r64 = (uint64)w[2 (j & 1)] << 32 | w[2 (j & 1) + 1]
 *              x    = (r64 * T_v) >> 64                                           (128-bit product)
 *              v    = col[first e in [beg, end) with edge_cdf[e] > x]             (never an edge of quantum 0)
 *     ids[B + i] = v;  pair_w[i] = (v == seeds[i]) ? 0 : 1;  ids[i] = seeds[i];  ids outside [0, n_rows) as above.
 *   Negatives: exactly gsage_unsup_batch's (tag 0x4E000000, the double table) -- the same Q ids for the same table,
 *   seed and call.  The model's table gives weight 0 to a row with T_v == 0 (ops.neg_cdf(weighted=True)).
 *   A wave per walk (four to a workgroup): the 64 lanes read a row of at most 64 edges in one round trip and ballot;
 *   a longer row is narrowed to one sixty-fourth per round trip of 64 evenly spaced probes, ceil(log64(deg)) in all.
 *   The table is non-decreasing inside a row, so the entry found does not depend on the probe pattern.
 *   edge_cdf == NULL is GSAGE_EINVAL before anything is launched; walk_len, Q, B, cdf_total as for gsage_unsup_batch.
 *   Additive; the ABI version is unchanged. */
int gsage_unsup_batch_weighted(const int64_t *rowptr, const int32_t *col, const uint64_t *edge_cdf, int64_t n_rows,
                               const int64_t *seeds, int64_t B, int32_t walk_len, int64_t Q, const double *cdf,
                               double cdf_total, uint64_t seed, const uint64_t *call_ctr, uint64_t call_base, uint64_t g0,
                               int64_t *ids, float *pair_w, int32_t *err_flag, void *stream);

/* ------------------------------------------------------------------------------------------
 * Weighted adjacency (csrc/gsage_weighted.hip, csrc/gsage_fullgraph.hip): edge-weight neighbour sampling and the
 * weight-normalised mean of layer-wise inference.  Additive; the ABI version is unchanged.  No reference counterpart.
 *
 * A weighted adjacency is the device CSR plus `cdf`, one uint64 per stored edge (aligned with col): the inclusive
 * running sum, inside each row, of the edge weights in integer quanta.
 *
 * gsage_edge_cdf_build -- set-up, once per adjacency (two launches: a wave per row of degree <= 256, a workgroup per
 * longer row).  weight: fp32 [nnz], finite and >= 0 (the CALLER checks: the kernels do not).  For row v with largest
 * weight m_v:
 *     degree 0 or m_v == 0     no drawable edge: every entry of the row is 0; the row behaves everywhere as a row of
 *                              degree 0 does (the dummy node 0)
 *     otherwise                (f, E) = frexp(m_v), f in [0.5, 1);   q_e = floor(w_e * 2^(24 - E))   in [0, 2^24)
 *                              cdf[e] = sum of q over the row's edges up to and including e        (<= deg * 2^24)
 * The scaling and the floor are done on the bits of w_e: q_e is the mathematical value for denormal weights and for a
 * maximum of 3.4e38 alike, and integer sums are exact, so every scan order gives the same table.  An edge lighter than
 * m_v * 2^-24 has q_e = 0 and is never drawn.
 *
 * gsage_sample_csr_weighted -- one launch per hop, Philox4x32-10 (the uniform sampler's generator, own key):
 *     g    = g0 + i*n + j,    call = call_base + (call_ctr ? *call_ctr : 0)        (as gsage_sample_csr_philox)
 *     w    = philox4x32_10({lo(g>>1), hi(g>>1), lo(call), hi(call)}, {lo(seed), hi(seed) ^ 0x57000000})
 *     r64  = (w[2*(g&1)] << 32) | w[2*(g&1) + 1]                                    (a block holds two draws)
 *     T    = the last cdf entry of row ids[i];   x = (r64 * T) >> 64               (128-bit product, x < T)
 *     out[i*n+j] = col[first e in the row with cdf[e] > x]                          (binary search)
 * T == 0 or degree 0 yields the dummy 0; an id outside [0, n_rows) yields 0 and raises *err_flag (may be NULL).
 *
 * gsage_sample_hops_weighted -- every hop of a frontier in ONE launch: gsage_sample_hops' descriptor, geometry (a
 * 256-lane workgroup walks the sub-tree of its seeds, the previous hop in LDS) and queue fields, with the draw above per
 * sample.  Sample (hop k, global index g = rank * |hop k| + local):
 *     call = call_base + (call_ctr ? *call_ctr : 0) + (k - 1);   w, r64, T, x and the child as above
 * -- the frontier is bit-identical to n_hops launches of gsage_sample_csr_weighted with call indices call_base + k - 1
 * and g0 = rank * |hop k|.  T == 0 or degree 0 yields the dummy 0; a parent outside [0, n_rows) yields 0 and raises
 * *err_flag.  seed_queue / batch_idx / batch_base / n_batches as in gsage_sample_hops: batch
 * (*batch_idx + batch_base) % n_batches is copied into hop 0.  cdf is an argument of its own: gsage_hops_desc is
 * unchanged.  max_deg is ignored.  hops == NULL, cdf == NULL, sel != NULL, dense_adj != NULL, n_hops outside 1..5 and a
 * fan-out product beyond gsage_sample_hops' LDS bound give GSAGE_EINVAL without a launch (and without a GPU); B == 0
 * returns GSAGE_OK without one.  The search probes seven evenly spaced entries of the row per round (cdf is
 * non-decreasing inside a row: the first entry above x is one entry however it is found); the environment variable
 * GSAGE_WEIGHTED_SEARCH=binary, read per call, selects the binary search instead.
 *
 * gsage_segment_reduce_weighted -- gsage_segment_reduce's arguments for a mean (no keys) plus cdf:
 *     out[v, c] = sum_e p_e table[col[e], c],   p_e = (cdf[e] - cdf[e-1]) / T_v    (the row's first edge subtracts 0)
 * -- what the sampled mean estimates under gsage_sample_csr_weighted, from the same quanta (mode
 * GSAGE_SEG_WEIGHTED_MEAN).  q_e < 2^24 is exact as a float and p_e = float(q_e) / float(T_v) is one IEEE division, so
 * a row with a single drawable edge (p_e == 1) returns that neighbour's row bit for bit; short rows and slices
 * accumulate fma(p_e, x, acc) in edge order, the merge adds a long row's partials in slice order.  A row with
 * T_v == 0 reads row 0.  Same plan, partials, alignment rules, activation and err_flag as
 * gsage_segment_reduce; no floating-point atomics.
 * ---------------------------------------------------------------------------------------- */
int gsage_edge_cdf_build(const int64_t *rowptr, const float *weight, int64_t n_rows, uint64_t *cdf, void *stream);
int gsage_sample_csr_weighted(const int64_t *rowptr, const int32_t *col, const uint64_t *cdf, int64_t n_rows,
                              const int64_t *ids, int64_t M, int32_t n, uint64_t seed, const uint64_t *call_ctr,
                              uint64_t call_base, uint64_t g0, int64_t *out, int32_t *err_flag, void *stream);
int gsage_sample_hops_weighted(const gsage_hops_desc *hops, const uint64_t *cdf, void *stream);
int gsage_segment_reduce_weighted(const void *table, int dtype, int64_t ld, int64_t D, const int64_t *rowptr,
                                  const int32_t *col, const uint64_t *cdf, int64_t n_rows, const int32_t *order,
                                  int64_t n_short, const int64_t *slices, int64_t n_slices, const int64_t *long_rows,
                                  int64_t n_long, int32_t slice_len, float *partials, int64_t ldp, void *out,
                                  int out_dtype, int64_t out_ld, int act, int32_t *err_flag, void *stream);

/* ------------------------------------------------------------------------------------------
 * Distinct neighbours (csrc/gsage_distinct.hip): neighbour sampling WITHOUT replacement over a device CSR.  Additive;
 * the ABI version is unchanged.  No reference counterpart (its sparse sampler computes row[sel % deg]).
 *
 * One sampler call with n samples per parent, 1 <= n <= 256.  The global sample index is g = g0 + i*n + j (parent i,
 * slot j in 0..n-1), the call index call = call_base + (call_ctr ? *call_ctr : 0)   (as gsage_sample_csr_philox):
 *     w(g) = philox4x32_10({lo(g>>2), hi(g>>2), lo(call), hi(call)}, {lo(seed), hi(seed) ^ 0x44000000})[g & 3]
 * -- the uniform sampler's addressing under a key tag of its own: neither the uniform nor the weighted stream.
 * For parent v = ids[i] with beg = rowptr[v], deg = rowptr[v+1] - beg and w_j = w(g0 + i*n + j):
 *     v outside [0, n_rows)   all n outputs are 0 and *err_flag (may be NULL) is set to 1
 *     deg <= 0                all n outputs are the dummy 0
 *     deg >= 2^32             the outputs are 0 and *err_flag is set to 1 (so that the arithmetic below is 64-bit exact)
 *     deg <= n                every neighbour, balanced:   r = (w_0 * deg) >> 32;   out[j] = col[beg + (j + r) % deg]
 *                             -- every stored edge appears floor(n/deg) or ceil(n/deg) times, the edges with the extra
 *                             copy a cyclic window with a uniform start: each edge is expected n/deg times, the plain
 *                             mean over the slots is an unbiased estimate of the row's mean and, when deg divides n, IS
 *                             the row's mean
 *     deg >  n                n distinct edges, uniformly random as an ordered tuple: a partial Fisher-Yates shuffle
 *                             over a virtual array a[x] = x,
 *                                 for j in 0..n-1:   t_j = j + ((w_j * (deg - j)) >> 32)          in [j, deg)
 *                                                    off[j] = a[t_j];   a[t_j] = a[j]             (a[j] read first)
 *                                 out[j] = col[beg + off[j]]
 *                             Per slot, from t_0 .. t_j alone: x = t_j, bound = j; repeat { the largest i < bound with
 *                             t_i == x; none: stop; else x = i, bound = i }; off[j] = x.
 * "Distinct" means distinct STORED EDGES: a row that stores a column twice can return it twice.
 *
 * gsage_sample_csr_distinct -- one launch per hop: out int64 [M * n].  n outside 1..256, a negative size or a null
 * pointer give GSAGE_EINVAL without a launch; M == 0 returns GSAGE_OK without one.
 *
 * gsage_sample_hops_distinct -- every hop of a frontier in ONE launch: gsage_sample_hops' descriptor, geometry (a
 * 256-lane workgroup walks the sub-tree of its seeds, the previous hop in LDS) and queue fields.  Hop k uses call index
 * call_base + (call_ctr ? *call_ctr : 0) + (k - 1) and g0 = rank * |hop k|: the frontier is bit-identical to n_hops
 * launches of gsage_sample_csr_distinct.  seed_queue / batch_idx / batch_base / n_batches as in gsage_sample_hops.
 * max_deg is ignored.  hops == NULL, sel != NULL, dense_adj != NULL, n_hops outside 1..5, a fan-out outside 1..256 and a
 * frontier that does not fit the LDS (16 bytes per id of the widest hop of a workgroup's seeds, plus 2 KiB) give
 * GSAGE_EINVAL without a launch (and without a GPU), the message naming the argument; B == 0 returns GSAGE_OK without
 * one.  Both entries can be recorded in a command list.
 * ---------------------------------------------------------------------------------------- */
int gsage_sample_csr_distinct(const int64_t *rowptr, const int32_t *col, int64_t n_rows, const int64_t *ids, int64_t M,
                              int32_t n, uint64_t seed, const uint64_t *call_ctr, uint64_t call_base, uint64_t g0,
                              int64_t *out, int32_t *err_flag, void *stream);
int gsage_sample_hops_distinct(const gsage_hops_desc *hops, void *stream);

/* ------------------------------------------------------------------------------------------
 * Temporal neighbours (csrc/gsage_temporal.hip): neighbour sampling over the edges that happened BEFORE a query
 * time, and the snapshot of a graph "as of T".  Additive; the ABI version is unchanged.  No reference counterpart
 * (its samplers know no time).
 *
 * A temporal CSR is rowptr int64 [n_rows + 1], col int32 [nnz] and etime int64 [nnz]: within every row etime is
 * non-decreasing, every etime is below INT64_MAX, every row is shorter than 2^32 (a longer one yields the dummy and
 * sets *err_flag, as under "Distinct neighbours").
 *
 * One sampler call with n >= 1 samples per parent takes the parents ids[i], their query times times[i] (int64), a
 * strategy and an inheritance rule.  For parent v = ids[i], t = times[i] and beg = rowptr[v]:
 *     cnt  = the number of edges e of row v with etime[e] < t     -- STRICT: an edge that happens at the prediction
 *            time is not visible; the comparison is one of signed 64-bit values.  The eligible edges are positions
 *            0 .. cnt-1 of the row (the row is in time order); t = INT64_MAX sees the whole row.
 *     w(g) = philox4x32_10({lo(g>>2), hi(g>>2), lo(call), hi(call)}, {lo(seed), hi(seed) ^ 0x54000000})[g & 3]
 *            with g = g0 + i*n + j and call = call_base + (call_ctr ? *call_ctr : 0): the uniform sampler's addressing
 *            under a key tag of its own.
 *     GSAGE_TEMPORAL_UNIFORM   off = (w(g) * cnt) >> 32         (not the reference's sel % deg: cnt is typically far
 *                              below max_deg, and the modulo bias would reach a factor of two)
 *     GSAGE_TEMPORAL_RECENT    off = cnt - 1 - (j % cnt)        -- no random word: the min(n, cnt) most recent eligible
 *                              edges, most recent first, cycled; when cnt divides n the plain mean over the slots is
 *                              the exact mean over the eligible edges
 *     out[i*n+j]      = col[beg + off]
 *     out_time[i*n+j] = times[i]            under GSAGE_TEMPORAL_INHERIT_SEED: every hop looks before the seed's time
 *                     = etime[beg + off]    under GSAGE_TEMPORAL_INHERIT_EDGE: the next hop looks before the edge just
 *                                           walked, so times strictly decrease along a path
 *     cnt == 0                 the dummy 0 in all n slots, out_time = times[i]
 *     v outside [0, n_rows)    0 in all n slots, out_time = times[i], and *err_flag (may be NULL) is set to 1
 *
 * gsage_sample_csr_temporal -- one launch per hop: out, out_time int64 [M * n].
 * gsage_temporal_count -- cnt[i] (int64 [M]) for the rows ids[i], or for every row i in [0, M) when ids == NULL
 * (then M <= n_rows), against times[i], or against the one scalar t when times == NULL.  A row outside the graph
 * counts 0 and sets *err_flag.
 * gsage_temporal_compact -- given cnt int64 [n_rows] and its exclusive prefix int64 [n_rows], copy the first
 * min(cnt[v], deg_v) entries of every row's col and etime to out_col / out_etime (out_nnz entries each) from
 * position prefix[v] on: with the prefix as the new rowptr, the CSR of the edges before t.  Nothing is written
 * outside [0, out_nnz).
 *
 * All three: a null pointer, a negative size, n < 1, an unknown strategy or rule give GSAGE_EINVAL without a launch,
 * the message naming the argument; M == 0 (n_rows == 0 for the compaction) returns GSAGE_OK without one.  All three
 * can be recorded in a command list.
 *
 * gsage_sample_hops_temporal -- every hop of a temporal frontier in ONE launch: gsage_sample_hops' descriptor, geometry
 * (a 256-lane workgroup walks the sub-tree of its seeds, the previous hop in LDS) and queue fields, with the times
 * travelling beside the ids.  gsage_hops_desc is unchanged: etime, times, time_queue and out_times are arguments of their
 * own (as cdf is for gsage_sample_hops_weighted).
 *     frontier    hops->ids is the usual buffer [hop 0 (B) | hop 1 (B * fan[0]) | ...]
 *     out_times   may be NULL; when given: int64 of the same layout, receives every entry's query time, hop 0 included
 *     hop 0       without hops->seed_queue its times are times[i] (int64 [B], device): times must not be NULL and
 *                 time_queue must be NULL.  With hops->seed_queue, batch b = (*batch_idx + batch_base) % n_batches supplies
 *                 the seeds (as in gsage_sample_hops: published as hop 0 of ids) and time_queue[b * B + i] (int64
 *                 [n_batches, B]) their times (published as hop 0 of out_times when it is given): time_queue must not be
 *                 NULL, times is ignored
 *     hop k       k = 1 .. n_hops: exactly one gsage_sample_csr_temporal call with ids = hop k-1's ids, times = hop k-1's
 *                 times, n = fan[k-1], the given strategy and inheritance rule, call index
 *                 call_base + (call_ctr ? *call_ctr : 0) + (k - 1) and g0 = rank * |hop k|
 * -- the frontier and its times are bit-identical to n_hops launches of the per-hop entry: the strict signed 64-bit
 * comparison, cnt == 0 giving the dummy 0 with the parent's time, a parent outside [0, n_rows) giving 0 with its time and
 * setting *err_flag, the >= 2^32 row rule, the key tag 0x54 and the word addressing w(g).  max_deg is ignored.
 * A hop runs in two phases: teams of 16 lanes count (one search per parent, however many samples it takes), then one
 * lane per sample draws.  LDS: 44 bytes per id of the widest hop of a workgroup's seeds (ids and times, each in two
 * ping-pong buffers, and a parent's first edge and count), at most 160 KiB.
 * GSAGE_EINVAL without a launch (and without a GPU), the message naming the argument: hops == NULL; etime == NULL;
 * rowptr / col / ids NULL; sel != NULL; dense_adj != NULL; n_hops outside 1..5; a fan-out < 1; an unknown strategy or
 * rule; times / time_queue not matching the presence of seed_queue as above; a frontier that does not fit the LDS.
 * B == 0 returns GSAGE_OK without a launch.  The entry can be recorded in a command list.
 * ---------------------------------------------------------------------------------------- */
#define GSAGE_TEMPORAL_UNIFORM 0
#define GSAGE_TEMPORAL_RECENT 1
#define GSAGE_TEMPORAL_INHERIT_SEED 0
#define GSAGE_TEMPORAL_INHERIT_EDGE 1
int gsage_sample_csr_temporal(const int64_t *rowptr, const int32_t *col, const int64_t *etime, int64_t n_rows,
                              const int64_t *ids, const int64_t *times, int64_t M, int32_t n, int32_t strategy,
                              int32_t inherit, uint64_t seed, const uint64_t *call_ctr, uint64_t call_base, uint64_t g0,
                              int64_t *out, int64_t *out_time, int32_t *err_flag, void *stream);
int gsage_sample_hops_temporal(const gsage_hops_desc *hops, const int64_t *etime, const int64_t *times,
                               const int64_t *time_queue, int32_t strategy, int32_t inherit, int64_t *out_times,
                               void *stream);
int gsage_temporal_count(const int64_t *rowptr, const int64_t *etime, int64_t n_rows, const int64_t *ids, int64_t M,
                         const int64_t *times, int64_t t, int64_t *cnt, int32_t *err_flag, void *stream);
int gsage_temporal_compact(const int64_t *rowptr, const int32_t *col, const int64_t *etime, int64_t n_rows,
                           const int64_t *cnt, const int64_t *prefix, int32_t *out_col, int64_t *out_etime,
                           int64_t out_nnz, void *stream);

/* ------------------------------------------------------------------------------------------
 * Temporal walks (csrc/gsage_unsup.hip): the unsupervised batch builder over a temporal CSR.  Additive; the ABI
 * version is unchanged.  No reference counterpart.
 *
 * gsage_unsup_batch_temporal -- one launch.  The temporal CSR is the one of "Temporal neighbours" (rows in time order,
 * every etime < INT64_MAX, rows shorter than 2^32).  seeds, times: int64 [B] on the device.  It writes
 *     ids        int64 [2B + Q] = [seeds (B) | positives (B) | negatives (Q)]      pair_w  fp32 [B]
 *     out_times  int64 [2B + Q]: the query time every row of ids is to be embedded at
 * call, P(c, tag) and g = g0 + i are exactly those of "Unsupervised GraphSAGE".
 *   Positive of seed i, v = seeds[i], tau = times[i]:
 *     t_i  = 1 + ((P(g, 0x4C000000)[0] * walk_len) >> 32)       (the plain builder's length word: the same seed takes
 *                                                                the same number of steps)
 *     for j = 0 .. t_i - 1:
 *              cnt  = the number of edges e of row v with etime[e] < tau          (strict, signed 64-bit: the sampler's
 *                     count);   cnt == 0: the walk ends at v
 *              word = P(g, 0x56000000 | (j >> 2))[j & 3]                           (a tag no other role uses)
 *              off  = (word * cnt) >> 32;   v = col[beg + off]                     (64-bit product, beg = rowptr[v])
 *              GSAGE_TEMPORAL_INHERIT_EDGE: tau = etime[beg + off] -- a time-respecting walk, the edge times strictly
 *              decrease along it;   GSAGE_TEMPORAL_INHERIT_SEED: tau stays times[i]
 *     ids[i] = seeds[i];  ids[B + i] = v;  pair_w[i] = (v == seeds[i]) ? 0 : 1     (a seed without history before its
 *     time takes no positive loss);   out_times[i] = out_times[B + i] = times[i]   (both ends of a pair are embedded as
 *     of the prediction time, under either rule)
 *     An id outside [0, n_rows) -- a seed, or a node the walk reaches -- is treated as in gsage_unsup_batch:
 *     ids[B + i] = 0, a bad seed also ids[i] = 0 and pair_w[i] = 0, *err_flag (may be NULL) is set; out_times keeps
 *     times[i].  A row of 2^32 edges or more counts as cnt = 0 and sets the flag.
 *   A walk always draws uniformly among the eligible edges: the sampler's strategy does not enter ("recent" would make
 *   every walk the same path).
 *   Negative q:  ids[2B + q] is gsage_unsup_batch's, bit for bit (tag 0x4E000000, the double table; g0 does not enter);
 *     out_times[2B + q] = times[q % b],  b = clamp(*n_valid, 1, B)   (n_valid: device int32 word as in
 *     gsage_head_skipgram_live, NULL: b = B) -- a batch padded to a recorded geometry gives its negatives the times the
 *     unpadded batch gives them.  A stated compromise: the Q negatives are shared by all seeds, so a negative is seen
 *     as of one of the batch's query times, not as of each seed's.
 *   A team of 16 lanes carries a walk and finds cnt together (the sampler's search, csrc/gsage_temporal_dev.h); the
 *   negatives take a lane each.  No LDS.
 *   GSAGE_EINVAL without a launch, the message naming the argument: a null pointer (n_valid, call_ctr and err_flag
 *   may be NULL), B outside [1, 2^31), Q < 1, walk_len outside 1..16, an unknown rule, a cdf_total that is not positive
 *   or not finite.  The entry can be recorded in a command list.
 * ---------------------------------------------------------------------------------------- */
int gsage_unsup_batch_temporal(const int64_t *rowptr, const int32_t *col, const int64_t *etime, int64_t n_rows,
                               const int64_t *seeds, const int64_t *times, int64_t B, int32_t walk_len, int64_t Q,
                               const double *cdf, double cdf_total, uint64_t seed, const uint64_t *call_ctr,
                               uint64_t call_base, uint64_t g0, int32_t inherit, const int32_t *n_valid, int64_t *ids,
                               int64_t *out_times, float *pair_w, int32_t *err_flag, void *stream);

/* ------------------------------------------------------------------------------------------
 * Importance neighbourhoods (csrc/gsage_importance.hip): a node's most-visited nodes under short random walks become
 * its neighbourhood, the visit counts its edge weights (the construction PinSAGE introduced).  What turns ANY
 * adjacency into a weighted one for everything under "Weighted adjacency".  Additive; the ABI version is unchanged.
 * No reference counterpart.
 *
 * Inputs: a device CSR (rowptr int64 [n_rows + 1], col int32 [nnz]; n_rows < 2^31), optionally its per-edge table
 * cdf uint64 [nnz] ("Weighted adjacency"; NULL: the graph is unweighted), sources ids int64 [M], n_walks R >= 1,
 * walk_len L in 1..16, top T in 1..64, R * L <= 4096, a 64-bit seed.
 *
 * Walks.  For source v = ids[i] and walk r in [0, R): u = v, then steps s = 0 .. L - 1:
 *     w    = philox4x32_10({lo(v), r, s >> 1, 0}, {lo(seed), hi(seed) ^ 0x49000000})
 *     r64  = (w[2*(s&1)] << 32) | w[2*(s&1) + 1]                                    (a block holds two steps)
 *   The counter holds the source's ID, not its position in ids: a source's row does not depend on which other sources
 *   share the launch, on their order, or on how the caller cuts them into launches.
 *     uniform step  (cdf == NULL)   deg = rowptr[u+1] - rowptr[u];  deg <= 0: the walk ends;
 *                                   u = col[rowptr[u] + ((r64 * deg) >> 64)]        (128-bit product)
 *     weighted step                 T_u = cdf[rowptr[u+1] - 1] (0 for an empty row);  T_u == 0: the walk ends;
 *                                   x = (r64 * T_u) >> 64;  u = col[first e of the row with cdf[e] > x]
 *                                   (the search of gsage_sample_csr_weighted)
 *   A step that lands on an id outside [0, n_rows) raises *err_flag (int32, may be NULL), ends the walk and is not
 *   counted.  A source outside [0, n_rows) raises the flag and gets an empty row.
 * Counting.  Every landing u != v is one visit of u; landings on the source itself are not counted.  Row 0 is a node
 * like any other here (the reference's convention never stores it as a neighbour).
 * Result row.  The distinct visited nodes in the TOTAL ORDER (count descending, id ascending); k_i = min(T, distinct):
 *     out_deg[i]      = k_i                                   int32 [M]
 *     out_col[i*T+j]  = the j-th node, j < k_i                int32 [M, T]
 *     out_w[i*T+j]    = its count as a float (an exact integer <= 4096, which the quanta of gsage_edge_cdf_build
 *                       represent without loss)                fp32 [M, T]
 *   Entries j >= k_i are written as 0 / 0.f: the padded row is fully defined.
 * The result is a pure function of the graph, the source's id and the seed: no atomics, same bits for every grid.
 * One launch.  GSAGE_EINVAL (without a GPU) for sizes outside the limits; the message names R * L > 4096.
 *
 * gsage_importance_compact -- the padded rows packed into a CSR: for j < out_deg[i],
 *     col_new[rowptr_new[i] + j] = out_col[i*T+j],  w_new[rowptr_new[i] + j] = out_w[i*T+j]
 * rowptr_new int64 [M]: the exclusive scan of out_deg (the caller's: set-up, once per graph).  One launch.
 * ---------------------------------------------------------------------------------------- */
int gsage_importance_walks(const int64_t *rowptr, const int32_t *col, const uint64_t *cdf, int64_t n_rows,
                           const int64_t *ids, int64_t M, int32_t n_walks, int32_t walk_len, int32_t top, uint64_t seed,
                           int32_t *out_col, float *out_w, int32_t *out_deg, int32_t *err_flag, void *stream);
int gsage_importance_compact(const int32_t *out_col, const float *out_w, const int32_t *out_deg,
                             const int64_t *rowptr_new, int64_t M, int32_t top, int32_t *col_new, float *w_new,
                             void *stream);

/* ------------------------------------------------------------------------------------------
 * Biased walks (csrc/gsage_walk_dev.h, csrc/gsage_unsup.hip, csrc/gsage_importance.hip): node2vec's second-order
 * steps -- a return parameter p and an in-out parameter q -- for the positives of "Unsupervised GraphSAGE" and the
 * walks of "Importance neighbourhoods", and a restart probability for the latter.  Additive; the ABI version is
 * unchanged.  No reference counterpart.
 *
 * Parameters.  p, q: doubles, finite, in [1/8, 8];  restart: a double in [0, 1).
 * Thresholds, computed once on the host in double arithmetic (classes c = return, near, far):
 *     a       = (1.0 / p, 1.0, 1.0 / q);   a_max = max(a)
 *     theta_c = a_c == a_max ? 2^32 : (uint64)floor((a_c / a_max) * 4294967296.0)
 *     theta_restart = (uint64)floor(restart * 4294967296.0)
 *   e.g. (p, q) = (4, 0.25): theta = (2^28, 2^30, 2^32).  The kernels receive these integers.
 *
 * A FIRST-ORDER step from node v is the step of the entry being biased, given the draw's random words:
 *     builder, uniform     word (32 bits):  off = deg <= 2^32 - 1 ? (word * deg) >> 32 : word;   x = col[beg + off]
 *     builder, weighted    r64:  x = col[first e of the row with edge_cdf[e] > (r64 * T_v) >> 64]
 *     importance, uniform  r64:  x = col[beg + ((r64 * deg) >> 64)]
 *     importance, weighted r64:  x = col[first e of the row with cdf[e] > (r64 * T_v) >> 64]
 *   A dead end (deg <= 0, or T_v == 0 under a table) ends the walk before any word is looked at, as in those entries.
 *
 * A SECOND-ORDER step from v with the previous node t known: rejection sampling over the first-order step.
 *     for round k = 0 .. 31:
 *         x = the first-order step from v under round k's proposal words
 *         x outside [0, n_rows): the error of the legacy entry (below), whether or not the round would have accepted
 *         class(x) = return  if x == t
 *                    near    else if x occurs among the STORED columns of row t -- col[rowptr[t] .. rowptr[t+1]), at
 *                            any position, under any weight (an edge of quantum 0 counts), however often it repeats
 *                    far     otherwise
 *         accept iff (round k's 32-bit acceptance word) < theta_class(x);   an accepted x is the step
 *     no round accepts: the step is the x of round 31.
 *   The bias of that last rule is the probability that 32 rounds reject, (1 - accept)^32 with accept the mean of
 *   theta_class / 2^32 over the proposal distribution: at most 1.3e-4 on a clique at p = 4, q = 0.25 (accept = 1/4 + O(1/n),
 *   0.75^32 = 1.0e-4 .. 1.3e-4), far less elsewhere.  A node whose only neighbour is t takes it either way.  A dead-end
 *   row proposes nothing: the walk ends.  Steps WITHOUT a previous node -- the first step of a walk, the first step
 *   after a restart -- are first-order steps under round 0's proposal words, with no acceptance test.
 *
 * Words.  Round 0's PROPOSAL words are the words the legacy entry uses for that step; everything else comes from
 * Philox blocks no other role addresses.
 *   builder, step j (0-based) of seed g, with P(c, tag) of "Unsupervised GraphSAGE":
 *     round 0 proposal     uniform:  P(g, 0x53000000 | (j >> 2))[j & 3];   weighted:  r64 of P(g, 0x5A000000 | (j >> 1)), half j & 1
 *     Bk = P(g, 0x42000000 | (j << 8) | k)             (j <= 15, k <= 31: tags 0x42000000 .. 0x42000F1F, used by nothing else)
 *     round k >= 1 proposal   uniform:  Bk[0];   weighted:  r64 = (uint64)Bk[0] << 32 | Bk[1]
 *     round k acceptance word Bk[2]    (k = 0 included; Bk[3], and B0[0..1], are unused)
 *   importance, step s of walk r of source v, key {lo(seed), hi(seed) ^ 0x49000000}:
 *     round 0 proposal     r64 of philox4x32_10({lo(v), r, s >> 1, 0}, key), half s & 1            (the legacy block)
 *     Nk = philox4x32_10({lo(v), r, s, 1 + k}, key)    (the legacy blocks have 0 in the fourth counter word)
 *     round k >= 1 proposal   r64 = (uint64)Nk[0] << 32 | Nk[1]
 *     round k acceptance word Nk[2];   the restart word of step s is N0[3]
 *
 * gsage_unsup_batch_biased -- gsage_unsup_batch (edge_cdf == NULL: uniform proposals) or gsage_unsup_batch_weighted
 * (edge_cdf != NULL) with second-order steps: walk lengths t_i, dead ends, pair_w, negatives, call / g0 / err_flag and
 * the outputs are those entries'; step 0 of every walk is first-order, steps j >= 1 are second-order with t the node
 * the walk stood on before v.  A seed outside [0, n_rows) is handled as there; a PROPOSAL outside [0, n_rows) raises
 * *err_flag and ends the walk at node 0.  One launch: a wave per walk, four to a workgroup, the negatives' workgroups
 * behind them.  The acceptance word is looked at first: below min(theta_near, theta_far) it accepts any x != t, at or
 * above their maximum it rejects it, and only between the two are the stored columns of row t read (64 per load, by
 * the wave); with q = 1 no row is ever read.
 *
 * gsage_importance_walks_biased -- gsage_importance_walks with second-order steps and restarts; counting, the total
 * order, the outputs, the limits and the size classes are that entry's.  Walk r of source v: u = v, no previous node;
 *     for s = 0 .. L - 1 (the walk not ended):
 *         s >= 1 and N0[3] < theta_restart:  u = v, the previous node is forgotten, nothing is counted, the step is
 *                                            consumed -- the walk goes on with step s + 1
 *         else  row u is a dead end: the walk ends
 *               x = a first-order step (no previous node) or a second-order step (t = the previous node) from u
 *               x outside [0, n_rows): *err_flag is raised, the walk ends, nothing is counted
 *               the previous node becomes u;  u = x;  u != v: one visit of u
 *   One launch, a walk per lane; the lanes step together, and the membership queries of a round are answered by the
 *   whole wave one after another (64 stored columns of row t per load).
 *
 * CONSEQUENCE.  With p = q = 1 every class threshold is 2^32, round 0 always accepts and its proposal is the legacy
 * word: the results are gsage_unsup_batch's / gsage_unsup_batch_weighted's / gsage_importance_walks', bit for bit.
 * With restart = 0, theta_restart = 0 and no walk restarts.
 *
 * p or q outside [1/8, 8] (NaN included), restart outside [0, 1), null pointers and the legacy entries' size checks
 * give GSAGE_EINVAL without a launch and without a GPU; the message names the argument.  Both entries can be recorded
 * in a command list.
 * ---------------------------------------------------------------------------------------- */
int gsage_unsup_batch_biased(const int64_t *rowptr, const int32_t *col, const uint64_t *edge_cdf, int64_t n_rows,
                             const int64_t *seeds, int64_t B, int32_t walk_len, int64_t Q, const double *cdf,
                             double cdf_total, uint64_t seed, const uint64_t *call_ctr, uint64_t call_base, uint64_t g0,
                             double p, double q, int64_t *ids, float *pair_w, int32_t *err_flag, void *stream);
int gsage_importance_walks_biased(const int64_t *rowptr, const int32_t *col, const uint64_t *cdf, int64_t n_rows,
                                  const int64_t *ids, int64_t M, int32_t n_walks, int32_t walk_len, int32_t top,
                                  uint64_t seed, double p, double q, double restart, int32_t *out_col, float *out_w,
                                  int32_t *out_deg, int32_t *err_flag, void *stream);

/* ------------------------------------------------------------------------------------------
 * k-hop closure blocks (csrc/gsage_block.hip, csrc/gsage_fullgraph.hip): full-neighbourhood inference for a query
 * set (infer.closure / infer.query).  Additive; the ABI version is unchanged.  No reference counterpart.
 *
 * Node sets S_L c ... c S_0 of a query vector over a CSR (rowptr int64, col int32, optional cdf):
 *     S_L     = the queries, duplicates removed, in order of first appearance
 *     S_{l-1} = S_l unchanged as a prefix, then the nodes of N(S_l) u {0} not yet present, in ascending id
 * Row 0 (the dummy) is a member of every source set.  A node's position in its set is its local index, the same in
 * every larger set.  Block l (destinations S_l, sources S_{l-1}): rowptr int64 [n_dst + 1]; col int32 = the stored
 * rows of S_l, whole, in stored order, duplicates kept, each id replaced by its local index; cdf = the rows' segments
 * verbatim.  An id outside [0, n_rows) raises *err_flag (int32, may be NULL) and is dropped from the sets; in a block's
 * col it is the dummy's local index.
 *
 * State the caller keeps per adjacency and hands to every call:
 *     local   int32 [n_rows]               -1 everywhere between queries
 *     bitmap  uint32 [ceil(n_rows / 32)]   0 everywhere between queries
 * Scratch: sums int64 [ceil(n / gsage_closure_span()) + 1] per scan over n items; the scans are three-phase (per-
 * workgroup sums over spans of gsage_closure_span() items, scan of the sums, apply): no workgroup waits for another.
 *
 * gsage_closure_seed_count (3 launches)   counts[0] = |S_L|.  The caller reads it back and allocates set.
 * gsage_closure_seed_write (3 launches)   set[0 .. n_set) = S_L, local[] of its members, pos[i] = the local index of
 *                                         queries[i] (-1 for an id outside the graph).  1 <= nq < 2^31.
 * gsage_closure_expand_count (4 launches) marks N(set[lo .. hi)) -- the members the previous hop added -- and the
 *                                         dummy; counts[0] = new members, counts[1] = edges of block (rows set[0 .. hi)),
 *                                         counts[2] = the dummy's local index in the grown set.  One readback.
 * gsage_closure_expand_write (3 launches) set[n_dst .. n_dst + counts[0]) = the new members, ascending (the caller has
 *                                         copied the prefix), their local[], the bitmap cleared; blk_rowptr [n_dst + 1],
 *                                         blk_col / blk_cdf [counts[1]] (blk_cdf NULL when cdf is).
 * gsage_closure_restore (1 launch)        local[set[i]] = -1, i < n: over S_0 it puts the state back.
 *
 * gsage_segment_reduce_block -- gsage_segment_reduce / _weighted over a block: n_dst output rows; table (and keys) of
 * n_src >= n_dst rows, a neighbour id is bounded by n_src; a row of degree 0, a weighted row without a drawable edge
 * and an id outside the table read row `dummy`.  cdf non-NULL exactly for GSAGE_SEG_WEIGHTED_MEAN.  The plan is built
 * over the block's rowptr with the same slice_len, so a block's row has the whole graph's edges, order and slices:
 * its output equals the whole-graph call's row bit for bit.  The whole-graph entry points are n_src = n_rows, dummy = 0.
 * ---------------------------------------------------------------------------------------- */
/* HOST: items per workgroup of the closure's scans (bitmap words, set members, queries) */
int64_t gsage_closure_span(void);
int gsage_closure_seed_count(const int64_t *queries, int64_t nq, int64_t n_rows, int32_t *local, int64_t *sums,
                             int64_t *counts, int32_t *err_flag, void *stream);
int gsage_closure_seed_write(const int64_t *queries, int64_t nq, int64_t n_rows, int32_t *local, const int64_t *sums,
                             int64_t *set, int64_t n_set, int64_t *pos, void *stream);
int gsage_closure_expand_count(const int64_t *rowptr, const int32_t *col, int64_t n_rows, const int64_t *set, int64_t lo,
                               int64_t hi, const int32_t *local, uint32_t *bitmap, int64_t *sums_words,
                               int64_t *sums_rows, int64_t *counts, int32_t *err_flag, void *stream);
int gsage_closure_expand_write(const int64_t *rowptr, const int32_t *col, const uint64_t *cdf, int64_t n_rows,
                               int64_t *set, int64_t n_dst, int32_t *local, uint32_t *bitmap, const int64_t *sums_words,
                               const int64_t *sums_rows, int64_t *blk_rowptr, int32_t *blk_col, uint64_t *blk_cdf,
                               int32_t *err_flag, void *stream);
int gsage_closure_restore(const int64_t *set, int64_t n, int32_t *local, void *stream);
int gsage_segment_reduce_block(int mode, const void *table, int dtype, int64_t ld, int64_t D, const float *keys,
                               int64_t ldk, const int64_t *rowptr, const int32_t *col, const uint64_t *cdf,
                               int64_t n_dst, int64_t n_src, int64_t dummy, const int32_t *order, int64_t n_short,
                               const int64_t *slices, int64_t n_slices, const int64_t *long_rows, int64_t n_long,
                               int32_t slice_len, float *partials, int64_t ldp, void *out, int out_dtype,
                               int64_t out_ld, int act, int32_t *err_flag, void *stream);

/* ------------------------------------------------------------------------------------------
 * Retrieval over embeddings (csrc/gsage_retrieve.hip): the k nearest rows of a table by inner product
 * (ops.topk_ip / infer.nearest).  Additive; the ABI version is unchanged.  No reference counterpart.
 *
 * Given a table E [N, D], queries Qm [Q, D] and k, the score of row j for query q is
 *     s(q, j) = sum_d Qm[q, d] * E[j, d]
 * over every ALLOWED row j, and the result is the k best under the TOTAL ORDER (score descending, row id
 * ascending), best first: out_ids int64 [Q, k], out_scores fp32 [Q, k].
 *     exclude = 0 (none)        every row is allowed
 *     exclude = 1 (self)        every row except query_ids[q]
 *     exclude = 2 (neighbours)  every row except query_ids[q] and the columns stored in row query_ids[q] of the
 *                               CSR (rowptr int64 [N + 1], col int32; columns in any order, duplicates allowed)
 * Fewer than k allowed rows: the tail is id -1, score -inf.  A NaN score is never selected.
 * Compute mode = the operands' dtype, the same for both: GSAGE_BF16 operands are multiplied by
 * mfma_f32_32x32x16_bf16 (fp32 accumulate; the caller rounds fp32 data to bf16 once), GSAGE_F32 operands by the
 * exact mfma_f32_32x32x2f32.  A score is one accumulator chain over d in an order that does not depend on where the
 * row falls in the grid, and the order above is total, so the result is bit-identical for every split count and run.
 *
 * Limits (GSAGE_EINVAL, the message names the argument): 1 <= k <= 128; 1 <= D <= 1024; ldt, ldq >= D (elements;
 * nothing past a row's D columns is read, a D that is no multiple of the MFMA's K step is zero-filled in LDS);
 * 1 <= N < 2^31; Q >= 1; 0 <= splits <= 1024 (0 = chosen by the library); exclude != 0 needs query_ids,
 * exclude = 2 needs rowptr and col.  No Q x N buffer exists; the only scratch is
 *     workspace  [Q, splits, k] pairs of (score, id), 8 bytes each, 8-byte aligned.
 * Two launches (scan, merge); recordable in a command list.
 *
 * gsage_topk_ip_workspace (HOST arithmetic, no GPU): the workspace's bytes for (Q, k, splits), -1 for arguments
 * outside the limits; *splits_used (may be NULL) = splits, or for splits = 0 the count the library chooses for (Q, N).
 * ---------------------------------------------------------------------------------------- */
int64_t gsage_topk_ip_workspace(int64_t Q, int64_t N, int64_t k, int64_t splits, int64_t *splits_used);
int gsage_topk_ip(const void *table, int table_dtype, int64_t ldt, int64_t N, const void *queries, int query_dtype,
                  int64_t ldq, int64_t Q, int64_t D, const int64_t *query_ids, const int64_t *rowptr,
                  const int32_t *col, int exclude, int32_t k, int32_t splits, void *workspace, int64_t workspace_bytes,
                  int64_t *out_ids, float *out_scores, void *stream);

/* ------------------------------------------------------------------------------------------
 * Exact link ranking over embeddings (csrc/gsage_rank.hip): the rank of one target row among ALL rows of a table by
 * inner product (ops.rank_ip / infer.link_rank).  Additive; the ABI version is unchanged.  No reference counterpart.
 *
 * Given a table E [N, D], queries Qm [Q, D], target_ids int64 [Q] and optionally query_ids int64 [Q] and a filter
 * CSR, with s(q, j) = sum_d Qm[q, d] * E[j, d] as in gsage_topk_ip and t = target_ids[q]:
 *     rank(q) = 1 + |{ j allowed for q, j != t : (s(q, j), j) beats (s(q, t), t) }|
 * "beats" is gsage_topk_ip's TOTAL ORDER (score descending, row id ascending); a row whose score is NaN beats nothing.
 * Outputs: out_rank int64 [Q]; out_score fp32 [Q] = s(q, t).
 *     exclude = 0 (none)        every row is allowed
 *     exclude = 1 (self)        every row except query_ids[q]
 *     exclude = 2 (neighbours)  every row except query_ids[q] and the columns of row query_ids[q] of the CSR: the
 *                               "filtered" setting -- known edges of the source do not count against the target
 * In both excluding modes the target itself is never excluded (a held-out edge's target is normally in the full
 * adjacency, and src == dst is legal): the excluded set is ({query_ids[q]} u cols) \ {t}.
 * Unranked: a target outside [0, N) gives rank 0 and score -inf; a target whose own score is NaN gives rank 0 and
 * score NaN.
 * Filter CSR (rowptr int64 [N + 1], col int32): in THIS entry point every row's columns must be STRICTLY ASCENDING
 * (sorted, no duplicates -- stricter than gsage_topk_ip, because a subtraction must not count a duplicate twice).  A
 * row that is read and violates it raises *err_flag (int32 device word, may be NULL; 0 = ok); the ranks of that call
 * are then not to be used.  The check is an adjacent-column compare where the row is walked anyway.  Columns outside
 * [0, N) are ignored.
 *
 * Compute mode = the operands' dtype, as in gsage_topk_ip, and every score -- the target's and the excluded rows'
 * included -- is the SAME accumulator chain as there: its bits are a function of the two rows alone, identical in
 * every launch of both entry points.  Counts are integers, so the result is bit-identical for every split count.
 *
 * Limits (GSAGE_EINVAL, the message names the argument; checked on the host before anything touches the GPU):
 * 1 <= D <= 1024; ldt, ldq >= D (elements; nothing past a row's D columns is read); 1 <= N < 2^31; Q >= 1;
 * 0 <= splits <= 1024 (0 = chosen by the library, gsage_topk_ip's rule); exclude != 0 needs query_ids, exclude = 2
 * needs rowptr and col.  The only scratch is
 *     workspace  [Q, splits] int32 split counts, then [Q] int32 filter counts: 4 * Q * (splits + 1) bytes, 4-byte aligned.
 * Launches: 2 for exclude = 0 and 1 (scan, finish), 3 for exclude = 2 (scan, filter, finish); recordable in a command
 * list.
 *
 * gsage_rank_ip_workspace (HOST arithmetic, no GPU): the workspace's bytes for (Q, splits), -1 for arguments outside
 * the limits; *splits_used (may be NULL) = splits, or for splits = 0 the count the library chooses for (Q, N).
 * ---------------------------------------------------------------------------------------- */
int64_t gsage_rank_ip_workspace(int64_t Q, int64_t N, int64_t splits, int64_t *splits_used);
int gsage_rank_ip(const void *table, int table_dtype, int64_t ldt, int64_t N, const void *queries, int query_dtype,
                  int64_t ldq, int64_t Q, int64_t D, const int64_t *target_ids, const int64_t *query_ids,
                  const int64_t *rowptr, const int32_t *col, int exclude, int32_t splits, void *workspace,
                  int64_t workspace_bytes, int64_t *out_rank, float *out_score, int32_t *err_flag, void *stream);

/* ------------------------------------------------------------------------------------------
 * Linear probe over embeddings (csrc/gsage_probe.hip): one full-batch loss-and-gradient evaluation of a linear
 * classifier on selected rows of a table (ops.probe_pass / infer.LinearProbe).  Additive; the ABI version is
 * unchanged.  The losses are the reference's ProblemLosses.classification (F.cross_entropy) and
 * ProblemLosses.multilabel_classification (F.multilabel_soft_margin_loss).
 *
 * Given a table X [N, ldx], ids int64 [n], an fp32 master W [C, D] (dense), bias fp32 [C] and targets:
 *     z[i, c] = sum_d X[ids[i], d] * W~[c, d] + bias[c]
 *     task = 0 (classification)            targets int64 [n], class ids in [0, C):
 *         l_i = logsumexp_c z[i, .] - z[i, y_i],                      G[i, c] = softmax(z_i)[c] - [c == y_i]
 *     task = 1 (multilabel_classification) targets fp32 [n, ldy], values in [0, 1]:
 *         l_i = (1/C) sum_c (softplus(z[i, c]) - y[i, c] z[i, c]),    G[i, c] = (sigmoid(z[i, c]) - y[i, c]) / C
 *     loss = (1/n) sum_i l_i,   dW = (1/n) G^T X[ids]  [C, D],   db = (1/n) sum_i G[i, .]
 * Compute mode = the table's dtype: GSAGE_BF16 rows meet W~ = W rounded to bf16 (RNE, when it is staged) on
 * mfma_f32_32x32x16_bf16; GSAGE_F32 rows meet W~ = W on the exact mfma_f32_32x32x2f32.  Logits, probabilities and G
 * never leave the registers (no n x C buffer); in bf16 mode G enters the gradient product as a hi + lo pair of bf16
 * (relative error 2^-17, not 2^-9).
 *
 * Outputs:
 *     partial   fp32 [S][C*D + C + 1]: one row [dW | db | loss] per workgroup (a contiguous range of 32-row tiles),
 *               already scaled by 1/n -- gsage_head_ce's convention, so ONE gsage_reduce_desc (src = partial, S,
 *               rows = 1, cols = C*D + C, stride = ld = C*D + C + 1) hands it to gsage_finalize_grads unchanged.
 *               S = splits, or for splits = 0 the count the library chooses: min(ceil(n / 32), 256).  A range
 *               that holds no tile (splits > tiles) writes zeros.
 *     loss_out  device float: the sum over S of the loss slots in buffer order (a second, one-workgroup launch).
 *               After gsage_probe_loss_index_next(index) the NEXT gsage_probe_pass of the calling thread writes
 *               loss_out[*index] instead (index: DEVICE int64, read when the launch runs; consumed by that call,
 *               also while a command list is being recorded) -- e.g. the step counter gsage_finalize_grads ticks
 *               AFTER the pass, so a replayed list fills a loss history.
 * No atomics: for fixed (n, C, D, splits) every sum has one order and the result is bit-identical from call to call;
 * different splits agree to fp32 round-off.
 *
 * Limits (GSAGE_EINVAL, the message names the argument; checked on the host before anything touches the GPU):
 * 1 <= C <= 128; 1 <= D <= 1024; 1 <= n < 2^31; N >= 1; ldx >= D (elements; nothing past a row's D columns is
 * read); ldy >= C for task 1; 0 <= splits <= 1024.  ids must lie in [0, N) and class ids in [0, C) (the callers
 * check once; an id outside [0, N) reads as a zero row, a class outside [0, C) as no class).  Two launches;
 * recordable in a command list.
 *
 * gsage_probe_pass_scratch (HOST arithmetic, no GPU): the number of FLOATS of `partial` for (n, C, D, splits), -1 for
 * arguments outside the limits; divided by C*D + C + 1 it is S.
 * ---------------------------------------------------------------------------------------- */
int64_t gsage_probe_pass_scratch(int64_t n, int32_t C, int32_t D, int32_t splits);
int gsage_probe_loss_index_next(const int64_t *index);
int gsage_probe_pass(const void *table, int dtype, int64_t ldx, int64_t N, const int64_t *ids, int64_t n,
                     const void *targets, int task, int64_t ldy, const float *W, const float *bias, int32_t C,
                     int32_t D, int32_t splits, float *partial, float *loss_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Graph propagation (csrc/gsage_propagate.hip): one step of label / residual propagation over a CSR adjacency
 * (propagate.py: label propagation, Correct and Smooth, SGC / APPNP-style feature smoothing).  Additive; the ABI
 * version is unchanged.  All values are fp32.
 *
 *     acc[v, c]  = sum over e in [rowptr[v], rowptr[v+1]) of y[col[e], c]
 *                  in stored-edge order within a slice and slice order within a row;
 *                  an empty row gives 0, NOT the dummy;
 *                  an id outside [0, n_rows) contributes 0 and raises *err_flag (int32, may be NULL)
 *     out[v, c]  = min(max(beta * base[v, c] + alpha * (a[v] * acc[v, c]), lo), hi)
 *                  for c < C;  lo = -inf and hi = +inf switch the clamp off
 *     yout[v, c] = b[v] * out[v, c]      (b == NULL: yout = out; a == NULL: a[v] = 1)
 *
 * y is the PRE-SCALED iterate b (.) x: the neighbour loop is a plain sum of 16-byte row chunks with no per-neighbour
 * scale fetch, and the kernel produces the next iteration's y in its own epilogue.  out or yout may be NULL, not both.
 * y must not alias out or yout (the caller ping-pongs two buffers).  base may be NULL only with beta == 0.
 *
 * gsage_propagate_scales fills a and b (fp32 [n_rows] each) from the row degrees deg[v] = rowptr[v+1] - rowptr[v]:
 *     norm = GSAGE_PROP_SYM:  a = b = deg^-1/2, and 0 where deg == 0
 *     norm = GSAGE_PROP_ROW:  a = 1 / deg (0 where deg == 0), b = 1
 *     norm = GSAGE_PROP_COL:  a = 1, b = 1 / deg (0 where deg == 0)
 * On an adjacency that stores both directions of every edge, "sym" is D^-1/2 A D^-1/2.  On any other adjacency it is
 * the definition above applied to the stored rows: the scales are those of the stored rows' degrees, nothing is
 * symmetrised.  One launch.
 *
 * Plan, partials and schedule are gsage_segment_reduce's (order / slices / long_rows over slice_len, partials fp32
 * [n_slices, ldp], unused if n_slices == 0): a team of 8 / 16 / 32 / 64 lanes per short row or slice, one 16-byte chunk
 * (4 columns) per lane, 8 neighbour rows in flight per lane; the merge of a long row's slices applies a, base, alpha,
 * beta, the clamp and b exactly as the short-row path does.  Two launches per call, whatever the graph; no
 * floating-point atomics: the same inputs give the same bits.  Recordable in a command list.
 *
 * Limits (GSAGE_EINVAL, with a message, before anything is launched): 1 <= C <= 1024; y, base, out, yout 16-byte
 * aligned with ldy, ldb, ldo, ldyo multiples of 4 floats and >= round_up(C, 4) (columns >= C are read from y and base
 * but never stored); ldp >= gsage_segment_reduce_ldp(C); lo <= hi; 1 <= n_rows < 2^31; slice_len a positive multiple of 8.
 * ---------------------------------------------------------------------------------------- */
enum { GSAGE_PROP_SYM = 0, GSAGE_PROP_ROW = 1, GSAGE_PROP_COL = 2 };
int gsage_propagate_scales(const int64_t *rowptr, int64_t n_rows, int norm, float *a, float *b, void *stream);
int gsage_propagate(const float *y, int64_t ldy, const float *base, int64_t ldb, const float *a, const float *b,
                    float alpha, float beta, float lo, float hi, int64_t C,
                    const int64_t *rowptr, const int32_t *col, int64_t n_rows,
                    const int32_t *order, int64_t n_short, const int64_t *slices, int64_t n_slices,
                    const int64_t *long_rows, int64_t n_long, int32_t slice_len, float *partials, int64_t ldp,
                    float *out, int64_t ldo, float *yout, int64_t ldyo, int32_t *err_flag, void *stream);

/* ------------------------------------------------------------------------------------------
 * K-means over embeddings (csrc/gsage_kmeans.hip): one assignment-and-accumulate pass of Lloyd's algorithm over
 * selected rows of a table, and the centroid update (ops.kmeans_pass / ops.kmeans_update / infer.kmeans).  Additive;
 * the ABI version is unchanged.
 *
 * gsage_kmeans_pass.  Given a table X [N, ldx], ids int64 [n], fp32 centroids Cn [K, D] (dense), bias fp32 [K] and
 * k_live in [1, K]:
 *     s[i, c]  = sum_d X[ids[i], d] * C~[c, d] + bias[c]                for c < k_live
 *     a[i]     = the c < k_live with the largest s[i, c]; among equal scores the SMALLEST c
 *     d2[i]    = max(0, |x_i|^2 - 2 s[i, a[i]])
 *     sums[c]  = sum over {i : a[i] == c} of X[ids[i], :]  [K, D],     counts[c] = |{i : a[i] == c}|
 *     inertia  = sum_i d2[i],     changed = |{i : labels_in[i] != a[i]}|   (0 if labels_in == NULL)
 * With bias[c] = -1/2 |C~[c]|^2 (gsage_kmeans_update writes it) a[i] is the nearest centroid and d2 the squared
 * distance to it.  Compute mode = the table's dtype: GSAGE_BF16 rows meet C~ = Cn rounded to bf16 (RNE) on
 * mfma_f32_32x32x16_bf16; GSAGE_F32 rows meet C~ = Cn on the exact mfma_f32_32x32x2f32.  A score is ONE accumulator
 * chain over d in ascending 16-byte steps, the same in every launch: a[i] does not depend on splits.  |x_i|^2 is fp32
 * (eight partial sums per row over interleaved 16-byte chunks, then a butterfly).  Scores, the arg-max and its one-hot
 * never leave the registers (no n x K buffer); the one-hot is the second product's operand as it stands (0 and 1 are
 * exact in bf16), so sums are fp32 sums of the table's values.
 *
 * Outputs:
 *     partial     fp32 [S][K*D + K + 2]: one row [sums | counts | inertia | changed] per workgroup (a contiguous
 *                 range of 32-row tiles), unscaled; counts and changed as fp32 integers.  S = splits, or for
 *                 splits = 0 the count the library chooses: min(ceil(n / 32), 256).  A range that holds no tile
 *                 (splits > tiles) writes zeros.  Clusters >= k_live get zeros.  NULL: labels / dist only (the second
 *                 product is skipped) -- then labels_out or dist_out must be given.
 *     labels_out  int32 [n] = a (may be NULL);   dist_out  fp32 [n] = d2 (may be NULL).
 *     labels_in   int32 [n] (may be NULL) must not alias labels_out.
 * No atomics: for fixed (n, K, D, splits) every sum has one order and the result is bit-identical from call to call;
 * different splits give the same labels, counts and changed, and sums / inertia that agree to fp32 round-off.
 *
 * gsage_kmeans_update (one launch; one workgroup of 256 threads per cluster).  With sum_c / count_c the sums over the
 * S partial rows in buffer order (counts and changed summed as integers):
 *     count_c > 0:  Cn[c] = sum_c / (float)count_c;  spherical = 1: then Cn[c] /= |Cn[c]| (left alone if the norm is 0)
 *     count_c == 0: Cn[c] is KEPT
 *     bias[c] = -1/2 sum_d C~[c, d]^2 (C~: Cn[c] rounded as the mode `dtype` sees it);  spherical = 1: bias[c] = 0
 *     slot = *index (DEVICE int64, read when the launch runs):  if 0 <= slot < capacity:  inertia_hist[slot] = inertia
 *     (fp32, the S slots added in buffer order), changed_hist[slot] = changed (int64), empty_hist[slot] = the number of
 *     c with count_c == 0 (int32);  then *index = slot + 1 -- a replayed command list fills the histories.
 * The order of every sum over d: thread t adds d = t, t + 256, t + 512, t + 768 in this order (fmaf), the 256 partial
 * sums are folded by halving (t += t + 128, then t + 64, .. t + 1).
 * S = 0: only bias is computed, from the given Cn; partial, the histories and index may be NULL and are not touched.
 *
 * Limits (GSAGE_EINVAL, the message names the argument; checked on the host before anything touches the GPU):
 * 1 <= K <= 128; 1 <= D <= 1024; 1 <= n < 2^31; N >= 1; ldx >= D (elements; nothing past a row's D columns is read);
 * 1 <= k_live <= K; 0 <= splits <= 1024 (update: 0 <= S <= 1024); with partial != NULL a workgroup's range must hold
 * fewer than 2^24 rows (ceil(ceil(n / 32) / S) * 32 < 2^24: its counts are fp32); capacity >= 1 for S > 0.  ids must
 * lie in [0, N) (the callers check once; an id outside reads as a zero row).  One launch each; recordable in a command
 * list.
 *
 * gsage_kmeans_pass_scratch (HOST arithmetic, no GPU): the number of FLOATS of `partial` for (n, K, D, splits), -1 for
 * arguments outside the limits; divided by K*D + K + 2 it is S.
 * ---------------------------------------------------------------------------------------- */
int64_t gsage_kmeans_pass_scratch(int64_t n, int32_t K, int32_t D, int32_t splits);
int gsage_kmeans_pass(const void *table, int dtype, int64_t ldx, int64_t N, const int64_t *ids, int64_t n,
                      const float *Cn, const float *bias, int32_t K, int32_t D, int32_t k_live,
                      const int32_t *labels_in, int32_t splits, float *partial, int32_t *labels_out, float *dist_out,
                      void *stream);
int gsage_kmeans_update(const float *partial, int32_t S, int32_t K, int32_t D, int dtype, int spherical, float *Cn,
                        float *bias, float *inertia_hist, int64_t *changed_hist, int32_t *empty_hist, int64_t *index,
                        int64_t capacity, void *stream);

/* ------------------------------------------------------------------------------------------
 * Graph construction (csrc/gsage_build.hip): an edge list becomes a device CSR, and a device CSR its transpose or its
 * symmetrised graph, on the GPU in a fixed number of launches.  Additive; the ABI version is unchanged.  Reference:
 * utils/convert.py:100-126 (make_sparse_adjacency over a networkx graph), which the definition below restates; the
 * GPU build, the host mode (numpy) and the tests' serial restatement agree on it bit for bit.
 *
 * Input.  src, dst: int64 [E], node ids in 0 .. n_nodes - 1 (n_nodes is given up front).  sel: optional bool
 * [n_nodes].  weight: optional fp32 [E], finite and >= 0.  time: optional int64 [E], < INT64_MAX.  Weight and time
 * together are refused.
 *
 * Records.  Input edge i makes record 2i = (src_i -> dst_i) and, unless the build is `directed` or src_i == dst_i,
 * record 2i + 1 = (dst_i -> src_i): a self-loop is ONE record (Graph.add_edge(u, u) stores one entry).  With sel a
 * record exists only if both of its ends are selected (make_sparse_adjacency(G, sel): only selected nodes get a row,
 * only selected neighbours count).  A record carries its edge's weight or time.
 *
 * duplicates -- records with the same (row, neighbour):
 *     "first"   (default without time) keep the record with the smallest index, with its payload: the reference
 *     "sum"     (weights only) keep the first record; its weight becomes the fp32 sum of the run's weights, added in
 *               record order, sequentially (s = w_0; s += w_1; ...): no atomics, the same bits every run
 *     "all"     (default with time) keep every record: repeated interactions are distinct events
 * order inside a row:
 *     "insertion"   (default without time) ascending record index: the reference, networkx's neighbour order
 *     "id"          ascending neighbour id, ties by record index
 *     "time"        (default and only choice with time) ascending time, ties by record index: what TemporalAdj's
 *                   stable lexsort gives
 *
 * Output, in the reference's sparse convention: n_rows = n_nodes + 1, row u + 1 holds neighbour + 1 as int32, row 0
 * is the empty dummy.  rowptr int64 [n_rows + 1]; max_deg = max(largest row length, 1) -- for a non-empty graph the
 * shape[1] scipy infers for the reference's matrix (`--rng compat` draws sel ~ U[0, shape[1])).  Weights become the
 * edge table of "Weighted adjacency", times the etime of "Temporal neighbours", unchanged.
 *
 * Limits, checked from the shapes before anything is allocated: the record count (2E, or E when directed) must be
 * below 2^31 (the sort carries int32 positions; a chunked build with a merge does not exist), and
 * 2 * ceil(log2(n_rows)) <= 62.  A temporal build sorts time - min(time): max(time) - min(time) must be below 2^63.
 * An id outside 0 .. n_nodes - 1 sets *err_flag (the record does not exist).
 *
 * Transpose of a device CSR, on its row ids directly (no shift by one): row v of A^T lists u for every stored u -> v,
 * ascending u, duplicates kept, a source row's repeated edges in stored order; n_rows is the same, max_deg the largest
 * new row length, at least 1.  The symmetrised adjacency is the union of the stored edges of A and A^T under
 * duplicates = "first", order = "id".  A stored id outside 0 .. n_rows - 1 sets *err_flag and is dropped.  Both refuse
 * weighted and temporal adjacencies (a device CSR keeps the CDF, not the weights; a transposed row is not in time
 * order).
 *
 * The pipeline.  b = ceil(log2(n_rows)) (at least 1; bit_length(n_rows) for the two CSR builds); a record's KEY is
 * row << b | neighbour in 0-based ids, the SENTINEL 2^(2b) - 1 stands for a record that does not exist: its row,
 * 2^b - 1, lies behind every row.  The sorts are gsage_sort_rows (stable, 8 bits per pass, 3 launches per pass).
 *     "id"         expand; sort 2b bits; [mark -> flag per sorted entry; inclusive scan, unless "all"]; finish; rowptr
 *     "insertion"  expand; ["first" / "sum": sort 2b bits; mark -> row key per RECORD, the sentinel row for a dropped
 *                  one | "all": row_keys]; sort b bits (stable: record order inside a row); finish; rowptr
 *     "time"       expand; time_keys; sort by time; row_keys through that order; sort b bits; finish; rowptr
 *     transpose    expand_csr (key = the column, rowof = the row); sort b bits; finish; rowptr
 *     symmetrise   expand_csr (keys (r, c) and (c, r)); then as "id" / "first"
 * Nothing is compacted between the stages, so the launch count depends on the key widths alone and the one readback
 * of a build is (nnz, max_deg) at its end (a temporal build reads the time range first: it sets a sort's width).
 *
 *   gsage_edges_expand      keys int64 [R], R = directed ? E : 2E, 16-byte aligned.  sel: one byte per node or NULL.
 *   gsage_edges_expand_csr  symmetric == 0: keys [nnz] = col[p] (sentinel 2^b - 1), rowof int32 [nnz] = the row of
 *                           position p;  != 0: keys [2 nnz] = (r << b | c, c << b | r), rowof unused.  n_rows < 2^b.
 *   gsage_edges_mark        over sorted (keys, positions): entry i is KEPT when its key is below the sentinel and
 *                           (keep_all or it is the first of its run).  Exactly one of flag int32 [n] (by sorted entry:
 *                           1 / 0) and row_keys int64 [n] (by record: key >> b, or 2^b - 1 when dropped).  weight /
 *                           wsum (both or neither): wsum[same index] = the run's sum, for kept entries; the weight of
 *                           record r is weight[r >> eshift].
 *   gsage_edges_row_keys    row_keys[j] = keys[perm ? perm[j] : j] >> b
 *   gsage_edges_time_keys   time_keys[r] = time[r >> eshift] - t_min
 *   gsage_edges_finish      over the last sort's (keys, positions): a kept entry i (incl != NULL: the inclusive scan of
 *                           the flags steps at i, its rank o = incl[i] - 1; NULL: key >> shift < n_lim, o = i) writes
 *                           col[o] = nbr32 ? nbr32[q] : ((nbr64 ? nbr64[q] : key) & (2^nbr_bits - 1)) + col_add with
 *                           q = perm ? perm[pos[i]] : pos[i], and w[o] / t[o] = wsrc / tsrc [by_entry ? i : q >> eshift].
 *                           Nothing is written at or beyond `cap`.
 *   gsage_edges_rowptr      rowptr[base + r] = the number of kept entries whose row key >> shift is below r, for
 *                           r = 0 .. n_lim; base == 1 also writes rowptr[0] = 0 (the dummy row).
 * All: GSAGE_EINVAL without a launch (and without a GPU) for a null pointer, a size outside the limits or a misaligned
 * key buffer, the message naming the argument; n == 0 returns GSAGE_OK without one (rowptr still launches: it writes
 * the zeros).  One launch each, recordable in a command list.
 * ---------------------------------------------------------------------------------------- */
int gsage_edges_expand(const int64_t *src, const int64_t *dst, int64_t E, int64_t n_nodes, const uint8_t *sel,
                       int32_t directed, int32_t b, int64_t *keys, int32_t *err_flag, void *stream);
int gsage_edges_expand_csr(const int64_t *rowptr, const int32_t *col, int64_t n_rows, int64_t nnz, int32_t symmetric,
                           int32_t b, int64_t *keys, int32_t *rowof, int32_t *err_flag, void *stream);
int gsage_edges_mark(const int64_t *keys_sorted, const int32_t *pos_sorted, int64_t n, int32_t b, int32_t keep_all,
                     int32_t *flag, int64_t *row_keys, const float *weight, int32_t eshift, float *wsum, void *stream);
int gsage_edges_row_keys(const int64_t *keys, const int32_t *perm, int64_t n, int32_t b, int64_t *row_keys,
                         void *stream);
int gsage_edges_time_keys(const int64_t *time, int64_t n, int32_t eshift, int64_t t_min, int64_t *time_keys,
                          void *stream);
int gsage_edges_finish(const int64_t *keys_sorted, const int32_t *pos_sorted, const int32_t *perm, const int32_t *incl,
                       int64_t n, int32_t shift, int64_t n_lim, const int32_t *nbr32, const int64_t *nbr64,
                       int32_t nbr_bits, int32_t col_add, const float *wsrc, const int64_t *tsrc, int32_t eshift,
                       int32_t by_entry, int32_t *col, float *w, int64_t *t, int64_t cap, void *stream);
int gsage_edges_rowptr(const int64_t *keys_sorted, const int32_t *incl, int64_t n, int32_t shift, int64_t n_lim,
                       int64_t *rowptr, int32_t base, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSAGE_H */
