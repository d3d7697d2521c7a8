"""The tail of a training step called directly (csrc/gsage_optim.hip, gsage_optim_dev.h) against the float64
restatements of update_tail_ref, at shapes chosen so that every code path runs:

gsage_finalize_grads   finalize_workgroup's five paths -- `vec16` (16-byte in-order), `SL2` .. `SL16` (SL threads per
                       4-column chunk meeting in LDS), `thr16` (16 threads per element), `wave4` (four waves per
                       element), `scalar` -- in two launches: FIN_SMALL (max_elems = 1 024: gx = 4, gstride = 1 024)
                       and FIN_BIG (max_elems > 65 536: gx = 256, gstride = 65 536, grid-stride loops taken twice).
                       The path of every descriptor is written next to it and checked against `finalize_path`, a
                       restatement of the kernel's conditions.
gsage_prep_weights     plain (`dst`), transposed (`dst_t`), fragment-ordered (`dst_p`) and fp32 (`dst_f32`) copies.
gsage_clip_adam_step   the 16-byte loop (n % 4 == 0, aligned, no descriptors) and the four-per-trip loop (bucket offset
                       by one float, n % 4 != 0, or operand-copy descriptors: first trip prefetched; second trip at
                       n = 2 048 * 1 024 + 1 028), supplied and in-call norm partials, both step_is_current meanings,
                       bit 2, norm_out, ticks, the copies refreshed by the update (prep_store).
gsage_clip_adam_meet   the in-launch norm (norm_slots) and the folded reduction (reduce_descs), refusals.

Tolerances.  A finalised element is within S 2^-24 sum_s |x_s| of the float64 sum (S = 1: exact).  p, m, v and the
clipped g are within (rtol 2e-6, atol 2e-7) PER ELEMENT of update_tail_ref.clip_adam (`excess` <= 1), or within 4 times
the excess torch's float32 update makes on the same inputs where that is larger.  Every comparison prints its figures
before it asserts and appends them to GSAGE_PARITY_LOG as `kernel_*`, `torch32_*` and `double_betas_*` (the distance to
an Adam whose betas are Python doubles, asserted against the rounding of beta to float32).
Recorded in profiles/update_tail_parity.jsonl: float32 torch on the CPU, on the 6-step schedule of
test_update_tail_host.py, has an excess of at most 0.03 (p), 0.08 (clipped g), 0.03 (m), 0.0004 (v); update_tail_ref.clip_adam_float32
(adam_update's arithmetic restated in numpy float32), on the inputs of test_clip_adam_step_against_float64, at most
0.06 (p), 0.03 (g), 0.05 (m), 0.04 (v) -- the start value holds with a factor of 12 to spare, and the one deviation
found so far (1 - float32(0.999) against 1 - 0.999: 1.23 on v at n = 1) is above it."""
import ctypes

import numpy as np
import pytest
import torch

import update_tail_ref as ut
from conftest import pkg
from util import note_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# The C ABI takes betas, eps, weight decay and max_norm as float and lr as a float32 device scalar: the update the
# kernels are ASKED for has the float32 roundings of 0.9, 0.999, ... as its hyperparameters, and the float64 reference
# is given those same numbers (f32).  It matters for beta2: 1 - float32(0.999) is 1.3e-5 (relative) below 0.001, which
# moves v by up to that much against an Adam whose betas are Python doubles -- recorded per case as `double_betas_*`
# in the parity log, next to the asserted figures.
def f32(x):
    return float(np.float32(x))


BETAS, EPS = (f32(0.9), f32(0.999)), f32(1e-8)
BETAS_DOUBLE = (0.9, 0.999)
SENT = np.float32(-1234.5)                         # fp32 sentinel (buckets, guards)
SENT16 = np.uint16(0xA5A5)                         # bf16 sentinel bit pattern
SENT32 = np.uint32(0xA5A5A5A5)                     # fp32-copy sentinel bit pattern (a finite negative float)



def _nat():
    return pkg()._native


def _eng():
    return pkg().engine.common


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _upload(descs, cls):
    return torch.frombuffer(bytearray(bytes((cls * len(descs))(*descs))), dtype=torch.uint8).to(DEV)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _i64(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


# =====================================================================================================================
# a. gsage_finalize_grads
# =====================================================================================================================
def finalize_path(S, rows, cols, ld, stride, aligned, gstride):
    """finalize_workgroup's choice, restated from its conditions"""
    chunks = rows * ((cols + 3) // 4)
    wide = ld % 4 == 0 and stride % 4 == 0 and aligned
    if wide and chunks >= gstride // 2:
        return "vec16"
    if S >= 64 and wide and chunks * 2 <= gstride:
        SL = 2
        while SL < 16 and chunks * (SL * 2) <= gstride:
            SL *= 2
        return "SL%d" % SL
    if S >= 128 and rows * cols * 16 <= gstride:
        return "thr16"
    if S >= 32 and rows * cols * 4 <= gstride:
        return "wave4"
    return "scalar"


# (id, path, S, rows, cols, ld, src offset in floats[, floats between two partial buffers beyond rows * ld])
# gx = 4, gstride = 1 024, max_elems = 1 024 (set by vec16-cols1-S24 and scalar-32x32-S31; the rest are small against it)
FIN_SMALL = [
    ("vec16-600x1-S8", "vec16", 8, 600, 1, 4, 0),                 # cols % 4 == 1: every chunk ragged; 600 >= 512 chunks
    ("vec16-1024x1-S24", "vec16", 24, 1024, 1, 4, 0),             # three rounds of 8 buffers
    ("vec16-512x2-S1", "vec16", 1, 512, 2, 4, 4),                 # a copy; src 16 bytes into its allocation
    ("vec16-700x1-S9", "vec16", 9, 700, 1, 8, 0),                 # one round of 8 and a tail buffer
    ("SL2-301x3-S65", "SL2", 65, 301, 3, 4, 0),                   # 301 chunks of 128 per trip; s0/s1 = 0/32/65
    ("SL4-37x19-S65", "SL4", 65, 37, 19, 20, 0),                  # 185 chunks of 64 per trip, last chunk of a row ragged
    ("SL4-129x4-S64", "SL4", 64, 129, 4, 8, 0),                   # even split, cols % 4 == 0
    ("SL8-9x41-S65", "SL8", 65, 9, 41, 44, 4),                    # 99 chunks of 32 per trip; 65 / 8 uneven
    ("SL8-65x1-S120", "SL8", 120, 65, 1, 4, 0),
    ("SL16-5x10-S120", "SL16", 120, 5, 10, 12, 0),                # 15 chunks of 16 per trip; 120 / 16 uneven
    ("SL16-1x1-S65", "SL16", 65, 1, 1, 4, 0),                     # 65 / 16: shares of 4 and 5 buffers
    ("thr16-1x1-S128", "thr16", 128, 1, 1, 3, 0),                 # ld % 4 != 0
    ("thr16-3x5-S130", "thr16", 130, 3, 5, 8, 1),                 # src offset by one float; 15 elements
    ("thr16-17x1-S512", "thr16", 512, 17, 1, 2, 0),               # 17 elements: a second group of 16
    ("thr16-5x10-S130", "thr16", 130, 5, 10, 11, 0),              # 50 elements, not a multiple of 16
    ("wave4-1x1-S32", "wave4", 32, 1, 1, 5, 0),
    ("wave4-3x5-S33", "wave4", 33, 3, 5, 6, 0),                   # 15 elements; 33 / 4 uneven
    ("wave4-17x1-S127", "wave4", 127, 17, 1, 4, 1),               # src offset by one float
    ("wave4-10x25-S33", "wave4", 33, 10, 25, 27, 0),              # 250 elements, not a multiple of 64
    ("wave4-10x10-S130", "wave4", 130, 10, 10, 13, 0),            # S >= 128 but 100 * 16 > gstride: not thr16
    ("scalar-1x1-S1", "scalar", 1, 1, 1, 2, 0),
    ("scalar-37x19-S9", "scalar", 9, 37, 19, 23, 0),
    ("scalar-32x32-S31", "scalar", 31, 32, 32, 33, 0),            # 1 024 elements: one per thread of the grid row
    ("scalar-16x16-S9-aligned", "scalar", 9, 16, 16, 20, 0),      # 16-byte loads possible, too few chunks, S < 32
    ("scalar-40x25-S200", "scalar", 200, 40, 25, 27, 0),          # many partials, too many elements for a split
    ("scalar-40x8-S65-oddstride", "scalar", 65, 40, 8, 12, 0, 2), # ld % 4 == 0 and aligned, but stride % 4 == 2
]
# gx = 256, gstride = 65 536 (max_elems = 229 390, set by vec16-32770x7-S7)
FIN_BIG = [
    ("vec16-33000x4-S1", "vec16", 1, 33000, 4, 8, 0),             # cols % 4 == 0; 33 000 >= 32 768 chunks
    ("vec16-32770x7-S7", "vec16", 7, 32770, 7, 8, 0),             # cols % 4 == 3; 65 540 chunks: the loop twice
    ("vec16-70001x1-S9", "vec16", 9, 70001, 1, 4, 4),             # cols % 4 == 1; the loop twice
    ("vec16-8200x17-S24", "vec16", 24, 8200, 17, 20, 0),          # cols % 4 == 1, five chunks per row
    ("vec16-16400x8-S8", "vec16", 8, 16400, 8, 12, 0),
    ("SL2-300x257-S65", "SL2", 65, 300, 257, 260, 0),             # 19 500 chunks of 128 per trip in 256 workgroups
    ("SL16-50x33-S64", "SL16", 64, 50, 33, 36, 0),
    ("thr16-61x67-S128", "thr16", 128, 61, 67, 69, 0),            # 4 087 elements, 16 per workgroup and trip
    ("wave4-127x129-S127", "wave4", 127, 127, 129, 131, 0),       # 16 383 elements, 64 per workgroup and trip
    ("scalar-300x257-S9", "scalar", 9, 300, 257, 259, 0),         # 77 100 elements: the loop twice
    ("scalar-100x100-S31", "scalar", 31, 100, 100, 101, 0),
]
FIN = {"small": (FIN_SMALL, 4), "big": (FIN_BIG, 256)}


def _fin_build(which):
    """host side of one launch: sources (pad columns and gaps NaN), descriptors, float64 reference"""
    cases, gx = FIN[which]
    rng = np.random.RandomState(len(cases))
    bufs, reds, off_out = [], [], 2
    for k, case in enumerate(cases):
        name, path, S, rows, cols, ld, off = case[:7]
        assert ld > cols
        stride = rows * ld + (case[7] if len(case) > 7 else (8 if ld % 4 == 0 else 3))
        buf = np.full(off + S * stride + 4, np.nan, dtype=np.float32)
        for s in range(S):
            lo = off + s * stride
            buf[lo:lo + rows * ld].reshape(rows, ld)[:, :cols] = rng.normal(size=(rows, cols)).astype(np.float32)
        bufs.append(buf)
        reds.append(ut.Red(k, off, stride, off_out, S, rows, cols, ld))
        off_out += rows * cols + 3                                  # gaps between the destination ranges
    n = off_out + 5
    flat, sq = ut.finalize(reds, bufs, n)
    return dict(cases=cases, gx=gx, bufs=bufs, reds=reds, n=n, flat=flat, sq=sq,
                bound=ut.finalize_bound(reds, bufs, n), max_elems=max(d.rows * d.cols for d in reds))


def _fin_launch(b, dbufs, ticks):
    """one gsage_finalize_grads launch over the build's descriptors -> (flat, partials) on the host"""
    nat, RD = _nat(), _eng()._ReduceDesc
    descs = []
    for d, t in zip(b["reds"], dbufs):
        assert t.data_ptr() % 16 == 0
        descs.append(RD(t.data_ptr() + 4 * d.off, d.stride, d.out_off, d.S, d.rows, d.cols, d.ld))
    dd = _upload(descs, RD)
    n_part = nat.lib().gsage_finalize_partials(len(descs), b["max_elems"])
    assert n_part == len(descs) * b["gx"]
    flat = torch.full((b["n"],), float(SENT), dtype=torch.float32, device=DEV)
    part = torch.full((n_part,), float("nan"), dtype=torch.float32, device=DEV)
    tk = [t.data_ptr() if t is not None else None for t in ticks]
    nat.check(nat.lib().gsage_finalize_grads(dd.data_ptr(), len(descs), b["max_elems"], flat.data_ptr(), part.data_ptr(),
                                             tk[0], tk[1], 3, tk[2], 11, _stream()), "finalize_grads")
    torch.cuda.synchronize()
    return _host(flat), _host(part)


@pytest.fixture(scope="module")
def fin():
    """which -> that launch's build with its results: each of the two launches is made once for the module"""
    made = {}

    def get(which):
        if which not in made:
            made[which] = _fin_run(which)
        return made[which]
    return get


def _fin_run(which):
    b = _fin_build(which)
    dbufs = [_dev(x) for x in b["bufs"]]
    ticks = [_i64(5), _i64(100), _i64(1000)]
    b["got"], b["part"] = _fin_launch(b, dbufs, ticks)
    b["ticks"] = [int(t.item()) for t in ticks]
    b["got2"], b["part2"] = _fin_launch(b, dbufs, [None, None, None])      # no counters: NULL is allowed
    b["ticks2"] = [int(t.item()) for t in ticks]
    return b


def _fin_compare(b, k, got, flat_ref):
    """descriptor k of a launch: every destination element within S 2^-24 sum |x_s| of the reference"""
    d = b["reds"][k]
    sl = slice(d.out_off, d.out_off + d.rows * d.cols)
    err = np.abs(got[sl].astype(np.float64) - flat_ref[sl])
    bad = err > b["bound"][sl]
    assert not bad.any(), (b["cases"][k][0], "%d of %d elements beyond S 2^-24 sum|x|; worst %g over bound %g"
                           % (int(bad.sum()), err.shape[0], float(err[bad].max()), float(b["bound"][sl][bad].max())))


_FIN_IDS = [(w, k) for w in ("small", "big") for k in range(len(FIN[w][0]))]


@pytest.mark.parametrize("which,k", _FIN_IDS, ids=["%s-%s" % (w, FIN[w][0][k][0]) for w, k in _FIN_IDS])
def test_finalize_path(fin, which, k):
    """one descriptor of a many-descriptor launch: the path is the one written in the table, the sums are within the
    float32 summation bound of the float64 sums, and its gx squared-norm partials add up to the sum of squares of what
    was stored"""
    b = fin(which)
    name, path, S, rows, cols, ld, off = b["cases"][k][:7]
    d = b["reds"][k]
    assert finalize_path(S, rows, cols, ld, d.stride, off % 4 == 0, 256 * b["gx"]) == path, name
    _fin_compare(b, k, b["got"], b["flat"])
    gx = b["gx"]
    mine = b["part"][k * gx:(k + 1) * gx].astype(np.float64)
    assert np.isfinite(mine).all()
    stored = b["got"][d.out_off:d.out_off + rows * cols].astype(np.float64)
    want = float((stored * stored).sum())
    # rows * cols products and additions in float32, 256 more in the block sum, each half an ulp of a running sum that
    # never exceeds the total: relative (rows * cols + 256) 2^-24
    assert abs(float(mine.sum()) - want) <= (rows * cols + 256) * ut.EPS24 * want, (name, float(mine.sum()), want)


@pytest.mark.parametrize("which", ["small", "big"])
def test_finalize_leaves_the_rest_alone(fin, which):
    """sentinel outside the destination ranges, all n_desc * gx partials finite, the three counters advance by exactly
    1, inc1, inc2 -- and a second launch without counters (NULL) stores the same bits and moves none"""
    b = fin(which)
    covered = ~np.isnan(b["flat"])
    assert covered.sum() == sum(d.rows * d.cols for d in b["reds"]) and not covered[:2].any() and not covered[-5:].any()
    for got, part in ((b["got"], b["part"]), (b["got2"], b["part2"])):
        assert np.array_equal(_bits(got[~covered]), np.full(int((~covered).sum()), _bits(SENT)))
        assert part.shape[0] == len(b["reds"]) * b["gx"] and np.isfinite(part).all()
    assert b["ticks"] == [5 + 1, 100 + 3, 1000 + 11]
    assert b["ticks2"] == b["ticks"]
    assert np.array_equal(_bits(b["got"]), _bits(b["got2"])) and np.array_equal(_bits(b["part"]), _bits(b["part2"]))


def test_finalize_comparison_bites(fin):
    """the same comparison against a reference that lost ONE partial buffer of a descriptor fails, for every descriptor
    of the small launch (every path)"""
    b = fin("small")
    for k, d in enumerate(b["reds"]):
        wrong, _ = ut.finalize(b["reds"], b["bufs"], b["n"], drop=(k, d.S - 1))
        with pytest.raises(AssertionError):
            _fin_compare(b, k, b["got"], wrong)
        _fin_compare(b, k, b["got"], b["flat"])


# =====================================================================================================================
# operand copies: destinations with sentinels and their check (gsage_prep_weights, prep_store in the update)
# =====================================================================================================================
class _Copies(object):
    """destination buffers of one descriptor.  mode: `dst` | `dst_t` | `all` (dst, dst_t with leading dimensions larger
    than needed, dst_p) | `f32` (dst_f32 = 1: dst and dst_t are fp32)"""

    def __init__(self, rows, cols, mode):
        self.rows, self.cols, self.mode = rows, cols, mode
        self.f32 = mode == "f32"
        wide = mode in ("all", "f32")
        self.ld, self.ld_t = cols + (5 if wide else 0), rows + (3 if wide else 0)
        dt = torch.int32 if self.f32 else torch.int16
        fill = int(SENT32.view(np.int32)) if self.f32 else int(SENT16.view(np.int16))
        new = lambda *shape: torch.full(shape, fill, dtype=dt, device=DEV)
        self.dst = new(rows, self.ld) if mode != "dst_t" else None
        self.dst_t = new(cols, self.ld_t) if mode != "dst" else None
        self.kc = ut.packed_kc(cols)
        self.dst_p = new(ut.packed_elems(rows, cols)) if mode == "all" else None

    def desc(self, src_ptr):
        ptr = lambda t: t.data_ptr() if t is not None else None
        return _eng()._PrepDesc(src_ptr, ptr(self.dst), ptr(self.dst_t), self.rows, self.cols, self.ld, self.ld_t,
                                ptr(self.dst_p), self.kc, 1 if self.f32 else 0, 0)

    def check(self, w, what):
        """w: the fp32 matrix [rows, cols] the copies were made from.  Written positions hold its bf16_rne bits (fp32:
        its bits), every other position the sentinel."""
        w = np.ascontiguousarray(w, dtype=np.float32).reshape(self.rows, self.cols)
        if self.f32:
            val, sent, view = w.view(np.uint32), SENT32, np.uint32
        else:
            val, sent, view = ut.bf16_rne(w), SENT16, np.uint16
        if self.dst is not None:
            want = np.full((self.rows, self.ld), sent, dtype=view)
            want[:, :self.cols] = val
            assert np.array_equal(_host(self.dst).view(view), want), (what, "dst")
        if self.dst_t is not None:
            want = np.full((self.cols, self.ld_t), sent, dtype=view)
            want[:, :self.rows] = val.T
            assert np.array_equal(_host(self.dst_t).view(view), want), (what, "dst_t")
        if self.dst_p is not None:
            got = _host(self.dst_p).view(np.uint16)
            rr, cc = np.meshgrid(np.arange(self.rows), np.arange(self.cols), indexing="ij")
            idx = ut.packed_index(rr, cc, self.kc)
            assert np.array_equal(got[idx], val), (what, "dst_p read through packed_index")
            want = np.full(got.shape[0], sent, dtype=np.uint16)
            want[idx.reshape(-1)] = val.reshape(-1)
            assert np.array_equal(got, want), (what, "dst_p padding written")


# =====================================================================================================================
# b. gsage_prep_weights
# =====================================================================================================================
PREP_SHAPES = [(1, 1), (37, 19), (33, 65), (128, 640), (300, 257)]


def _prep_sources():
    rng = np.random.RandomState(7)
    special = ut.special_values()
    out = []
    for rows, cols in PREP_SHAPES:
        w = rng.normal(size=(rows, cols)).astype(np.float32)
        if w.size >= special.shape[0]:
            w.reshape(-1)[:special.shape[0]] = special               # +-0, denormals, ties, overflow to inf, +-inf
            w.reshape(-1)[-special.shape[0]:] = special[::-1]
        else:
            w[0, 0] = np.float32(1 + 3 * 2.0 ** -8)                   # (1, 1): a tie that rounds up to even
        out.append(w)
    return out


@pytest.mark.parametrize("max_elems", [128 * 640, 256], ids=["gx256", "gx1"])
@pytest.mark.parametrize("mode", ["dst", "dst_t", "all", "f32"])
def test_prep_weights(mode, max_elems):
    """five matrices in one launch, with the true max_elems (256 workgroups per descriptor) and a small one (one
    workgroup walks each matrix): the four copy forms bit for bit, sentinel everywhere else, dst_p equal to
    gsage_pack_weight's operand at every non-pad position, the two counters"""
    nat = _nat()
    srcs = _prep_sources()
    dsrc = [_dev(w) for w in srcs]
    copies = [_Copies(r, c, mode) for r, c in PREP_SHAPES]
    dd = _upload([cp.desc(t.data_ptr()) for cp, t in zip(copies, dsrc)], _eng()._PrepDesc)
    t0, t1 = _i64(7), _i64(-2)
    nat.check(nat.lib().gsage_prep_weights(dd.data_ptr(), len(copies), max_elems, t0.data_ptr(), 4, t1.data_ptr(), 9,
                                           _stream()), "prep_weights")
    nat.check(nat.lib().gsage_prep_weights(dd.data_ptr(), len(copies), max_elems, None, 4, None, 9, _stream()),
              "prep_weights")                                        # NULL counters; the same stores again
    torch.cuda.synchronize()
    assert (int(t0.item()), int(t1.item())) == (11, 7)
    for cp, w in zip(copies, srcs):
        cp.check(w, (mode, cp.rows, cp.cols))
        if cp.dst_p is not None:
            wp = torch.full_like(cp.dst_p, int(SENT16.view(np.int16)))
            nat.check(nat.lib().gsage_pack_weight(_dev(w).data_ptr(), nat.F32, cp.cols, 0, cp.rows, cp.cols, 1,
                                                  wp.data_ptr(), _stream()), "pack_weight")
            torch.cuda.synchronize()
            rr, cc = np.meshgrid(np.arange(cp.rows), np.arange(cp.cols), indexing="ij")
            idx = ut.packed_index(rr, cc, cp.kc).reshape(-1)
            a, b = _host(cp.dst_p).view(np.uint16), _host(wp).view(np.uint16)
            assert np.array_equal(a[idx], b[idx]), ("dst_p != gsage_pack_weight", cp.rows, cp.cols)
            pad = np.ones(b.shape[0], dtype=bool)
            pad[idx] = False
            assert not b[pad].any()                                  # (gsage_pack_weight zeroes what dst_p leaves alone)


# =====================================================================================================================
# c. gsage_clip_adam_step
# =====================================================================================================================
_state = ut.adam_state


class _Bucket(object):
    """p, g, m, v on the device inside guarded allocations, `offset` floats in (offset 1: no 16-byte alignment)"""

    def __init__(self, st, offset=0):
        self.n, self.offset = st["p"].shape[0], offset
        self.raw, self.view = {}, {}
        for k in "pgmv":
            self.raw[k] = torch.full((self.n + offset + 8,), float(SENT), dtype=torch.float32, device=DEV)
            self.view[k] = self.raw[k][offset:offset + self.n]
            self.view[k].copy_(torch.from_numpy(st[k]))
            assert self.raw[k].data_ptr() % 16 == 0

    def ptr(self, k, start=0):
        return self.view[k].data_ptr() + 4 * start

    def read(self):
        """-> p, g, m, v as numpy; the guard elements around them must still hold the sentinel"""
        out = {}
        for k in "pgmv":
            raw = _host(self.raw[k])
            guard = np.concatenate([raw[:self.offset], raw[self.offset + self.n:]])
            assert np.array_equal(_bits(guard), np.full(guard.shape[0], _bits(SENT))), ("guard of %s overwritten" % k)
            out[k] = raw[self.offset:self.offset + self.n].copy()
        return out


def _step(st, t, lr, wd, max_norm, offset=0, copies=(), sic=0, step0=None, n_ready=0, partial=None, ticks=False):
    """one gsage_clip_adam_step.  copies: [(start, _Copies)].  -> dict(p, g, m, v, norm, step[, tick1, tick2])"""
    nat = _nat()
    bk = _Bucket(st, offset)
    n_part = max(nat.lib().gsage_adam_partials(bk.n), n_ready)
    part = torch.full((n_part + 4,), float("nan"), dtype=torch.float32, device=DEV)
    if partial is not None:
        part[:n_ready].copy_(partial[:n_ready])
    lr_t = torch.tensor([lr], dtype=torch.float32, device=DEV)
    step = _i64((t if (sic & 1) else t - 1) if step0 is None else step0)
    norm = torch.full((1,), float("nan"), dtype=torch.float32, device=DEV)
    dd = _upload([cp.desc(bk.ptr("p", s)) for s, cp in copies], _eng()._PrepDesc) if copies else None
    t1, t2 = (_i64(40), _i64(50)) if ticks else (None, None)
    nat.check(nat.lib().gsage_clip_adam_step(
        bk.ptr("p"), bk.ptr("g"), bk.ptr("m"), bk.ptr("v"), bk.n, part.data_ptr(), lr_t.data_ptr(), step.data_ptr(),
        BETAS[0], BETAS[1], EPS, wd, max_norm, norm.data_ptr(), sic, n_ready, dd.data_ptr() if copies else None,
        len(copies), t1.data_ptr() if ticks else None, 6, t2.data_ptr() if ticks else None, -2, _stream()),
        "clip_adam_step")
    torch.cuda.synchronize()
    out = bk.read()
    out.update(norm=float(norm.item()), step=int(step.item()))
    if ticks:
        out.update(tick1=int(t1.item()), tick2=int(t2.item()))
    for s, cp in copies:
        cp.check(out["p"][s:s + cp.rows * cp.cols], ("copies of the new p at", s))
    return out


def _check_update(got, st, t, lr, wd, max_norm, key):
    """p, m, v, clipped g within the tolerance of clip_adam in float64; the errors go to the parity log"""
    lr, wd, max_norm = f32(lr), f32(wd), f32(max_norm)               # what the kernel is given
    ref = ut.clip_adam(st["p"], st["g"], st["m"], st["v"], lr, t, BETAS, EPS, wd, max_norm)
    e32 = ut.float32_torch_excess(st["p"], st["g"], st["m"], st["v"], lr, t, BETAS, EPS, wd, max_norm)
    mine = {k: ut.excess(got[k], ref[k]) for k in "pgmv"}
    dbl = ut.clip_adam(st["p"], st["g"], st["m"], st["v"], lr, t, BETAS_DOUBLE, EPS, wd, max_norm)
    note_parity(key, **dict([("kernel_" + k, mine[k]) for k in "pgmv"] + [("torch32_" + k, e32[k]) for k in "pgmv"] +
                            [("double_betas_" + k, ut.excess(got[k], dbl[k])) for k in "pgmv"]))
    print(key, "kernel", mine, "torch float32", e32)
    for k in "pgmv":
        assert mine[k] <= max(1.0, 4.0 * e32[k]), (key, k, "excess %g over (2e-6, 2e-7); torch float32: %g"
                                                   % (mine[k], e32[k]))
    # against Adam with the betas as Python doubles (what torch.optim.Adam(betas=(0.9, 0.999)) computes): further away
    # by no more than the rounding of beta to float32 moves the moments -- d(beta m + (1 - beta) g) = dbeta (m - g),
    # d(beta2 v + (1 - beta2) g^2) = dbeta2 (v - g^2), g the clipped gradient with the weight decay added
    ge = dbl["g"] + wd * np.asarray(st["p"], dtype=np.float64)
    for k, d_beta, old, new_ in (("m", abs(BETAS[0] - BETAS_DOUBLE[0]), st["m"], ge),
                                 ("v", abs(BETAS[1] - BETAS_DOUBLE[1]), st["v"], ge * ge)):
        allow = max(1.0, 4.0 * e32[k]) * (ut.ATOL + ut.RTOL * np.abs(dbl[k])) + \
            d_beta * (np.abs(np.asarray(old, dtype=np.float64)) + np.abs(new_))
        err = np.abs(np.asarray(got[k], dtype=np.float64) - dbl[k])
        assert (err <= allow).all(), (key, k, "beyond the float32 rounding of beta", float((err / allow).max()))
    return ref


def _slice_copies(n, mode="dst"):
    """one descriptor over a slice of [0, n) that starts at element 1 (n > 1)"""
    start = 1 if n > 1 else 0
    cols = min(n - start, 19)
    rows = min((n - start) // cols, 300)
    return [(start, _Copies(rows, cols, mode))]


STEP_N = [1, 3, 4, 1023, 1024, 1025, 4096 + 4]
STEP_CASES = [(n, r) for n in STEP_N for r in ("plain", "offset", "desc")] + [(2048 * 1024 + 1028, "desc")]


@pytest.mark.parametrize("n,route", STEP_CASES)
def test_clip_adam_step_against_float64(n, route):
    """one update (t = 3) with the clip active and inactive, wd 0 and 1e-3, against clip_adam.
    plain: aligned bucket, no descriptors -- the 16-byte loop when n % 4 == 0, the four-per-trip loop otherwise;
    offset: the bucket one float off 16-byte alignment -- the four-per-trip loop (and the scalar norm pass);
    desc: an operand-copy descriptor -- the four-per-trip loop with its prefetched first trip on a quarter of the
    workgroups; at n = 2 048 * 1 024 + 1 028 the 2 048 workgroups take a second trip (a second descriptor lies in it)"""
    t, lr = 3, 0.01
    for norm, wd in ((12.0, 0.0), (12.0, 1e-3), (2.0, 0.0), (2.0, 1e-3)):
        st = _state(n, n % 1000 + int(norm), norm)
        copies = ()
        if route == "desc":
            copies = _slice_copies(n, "dst")
            if n > 2048 * 1024:
                copies = copies + [(4 * 2048 * 256 + 3, _Copies(37, 19, "all"))]
        got = _step(st, t, lr, wd, 5.0, offset=1 if route == "offset" else 0, copies=copies)
        ref = _check_update(got, st, t, lr, wd, 5.0, "step/n%d/%s/norm%g/wd%g" % (n, route, norm, wd))
        assert (ref["coef"] < 1.0) == (norm > 5.0)
        assert got["step"] == t
        # the norm: n products and additions, 256 more in the block sums, each half an ulp of the running sum
        assert abs(got["norm"] - ref["norm"]) <= (n + 256) * ut.EPS24 * ref["norm"]
        if norm < 5.0:
            assert np.array_equal(_bits(got["g"]), _bits(st["g"]))     # an unclipped gradient is left as it was


@pytest.mark.parametrize("n,route", [(1024, "plain"), (1025, "plain"), (1025, "desc")])
def test_clip_adam_step_first_update_from_zero_state(n, route):
    """the first update of a training run: m = v = 0, t = 1 (bias corrections 0.1 and 0.001: the update is
    lr * g / (|g| + eps sqrt(0.001)), about lr per element), clip active and inactive, wd 0 and 1e-3 -- on the 16-byte
    loop, the four-per-trip loop, and the latter with an operand-copy descriptor"""
    for norm, wd in ((12.0, 0.0), (12.0, 1e-3), (2.0, 0.0), (2.0, 1e-3)):
        st = _state(n, 7 + int(norm), norm)
        st["m"] = np.zeros(n, dtype=np.float32)
        st["v"] = np.zeros(n, dtype=np.float32)
        got = _step(st, 1, 0.01, wd, 5.0, copies=_slice_copies(n) if route == "desc" else ())
        _check_update(got, st, 1, 0.01, wd, 5.0, "step/zero_state/n%d/%s/norm%g/wd%g" % (n, route, norm, wd))
        assert got["step"] == 1


@pytest.mark.parametrize("n", [1024, 4096 + 4])
def test_clip_adam_step_paths_agree_bit_for_bit(n):
    """the same p, g, m, v and the same supplied norm partials (n_partial_ready > 0, made by gsage_grad_sqnorm) through
    the 16-byte loop, the four-per-trip loop (a descriptor over a slice) and the unaligned bucket: identical p, m, v
    and clipped g.  And n_partial_ready == 0 gives the bits of passing what gsage_grad_sqnorm writes with
    adam_grid(n, 1024) blocks."""
    nat = _nat()
    st = _state(n, 11, 12.0)
    st["g"][:3] = [0.0, -0.0, np.float32(1e-41)]
    n_part = nat.lib().gsage_adam_partials(n)
    assert n_part == min(-(-n // 256), 1024)
    for offset in (0, 1):                                            # (the norm pass has a 16-byte and a scalar loop)
        raw = torch.zeros(n + 8, dtype=torch.float32, device=DEV)
        g = raw[offset:offset + n]
        g.copy_(torch.from_numpy(st["g"]))
        part = torch.zeros(n_part, dtype=torch.float32, device=DEV)
        nat.check(nat.lib().gsage_grad_sqnorm(g.data_ptr(), n, part.data_ptr(), n_part, _stream()), "grad_sqnorm")
        torch.cuda.synchronize()
        given = _step(st, 5, 0.003, 1e-3, 5.0, offset=offset, n_ready=n_part, partial=part)
        own = _step(st, 5, 0.003, 1e-3, 5.0, offset=offset)
        for k in "pgmv":
            assert np.array_equal(_bits(given[k]), _bits(own[k])), (k, offset)
        assert given["norm"] == own["norm"]
        if offset == 0:
            vec, shared = given, part
    quad = _step(st, 5, 0.003, 1e-3, 5.0, copies=_slice_copies(n), n_ready=n_part, partial=shared)
    off1 = _step(st, 5, 0.003, 1e-3, 5.0, offset=1, n_ready=n_part, partial=shared)
    for k in "pgmv":
        assert np.array_equal(_bits(vec[k]), _bits(quad[k])), (k, "16-byte vs four-per-trip")
        assert np.array_equal(_bits(vec[k]), _bits(off1[k])), (k, "16-byte vs unaligned")
    assert not np.array_equal(_bits(vec["g"]), _bits(st["g"]))          # (the clip was active)


@pytest.mark.parametrize("n,route", [(1024, "plain"), (1025, "plain"), (1025, "desc")])
def test_clip_adam_step_counter_meanings_and_discard_bit(n, route):
    """step_is_current 0 with *step = t - 1 and 1 with *step = t: the same bits, the counter ends at t in both; bit 2
    with an active clip leaves g untouched and p, m, v as without it; an inactive clip never rewrites g; tick1 and
    tick2 advance by their increments"""
    t = 4
    st = _state(n, 21, 9.0)
    st["g"][:3] = [0.0, -0.0, np.float32(1e-41)]
    cps = (lambda: _slice_copies(n)) if route == "desc" else (lambda: ())
    a = _step(st, t, 0.01, 1e-3, 5.0, copies=cps(), sic=0, step0=t - 1, ticks=True)
    b = _step(st, t, 0.01, 1e-3, 5.0, copies=cps(), sic=1, step0=t)
    assert a["step"] == t and b["step"] == t
    assert (a["tick1"], a["tick2"]) == (46, 48)
    for k in "pgmv":
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    c = _step(st, t, 0.01, 1e-3, 5.0, copies=cps(), sic=1 | 2, step0=t)
    d = _step(st, t, 0.01, 1e-3, 5.0, copies=cps(), sic=2, step0=t - 1)
    for r in (c, d):
        assert r["step"] == t
        assert np.array_equal(_bits(r["g"]), _bits(st["g"]))
        assert not np.array_equal(_bits(a["g"]), _bits(st["g"]))
        for k in "pmv":
            assert np.array_equal(_bits(r[k]), _bits(a[k])), k
    calm = _state(n, 22, 3.0)
    calm["g"][:3] = [0.0, -0.0, np.float32(1e-41)]
    for sic in (0, 2):
        e = _step(calm, t, 0.01, 0.0, 5.0, copies=cps(), sic=sic)
        assert np.array_equal(_bits(e["g"]), _bits(calm["g"]))


@pytest.mark.parametrize("mode", ["dst", "dst_t", "all", "f32"])
def test_clip_adam_step_refreshes_operand_copies(mode):
    """prep_store from inside the update: two disjoint descriptors (37 x 19 at element 5, 33 x 65 at element 1 000) in a
    bucket of 4 001 elements, the stretches [0, 5), [708, 1 000) and [3 145, 4 001) covered by none.  Every copy form
    holds bf16_rne (fp32: the bits) of the p the kernel stored; sentinel elsewhere (checked in _step)."""
    st = _state(4001, 31, 12.0)
    got = _step(st, 2, 0.01, 1e-3, 5.0, copies=[(5, _Copies(37, 19, mode)), (1000, _Copies(33, 65, mode))])
    _check_update(got, st, 2, 0.01, 1e-3, 5.0, "step/copies/%s" % mode)


# =====================================================================================================================
# d. gsage_clip_adam_meet
# =====================================================================================================================
_MEET = {"slots": None, "step": 0}


def _meet_desc(bk, part, lr_t, step, norm, dd, n_prep, wd, max_norm):
    nat = _nat()
    if _MEET["slots"] is None:
        _MEET["slots"] = torch.zeros(1024, dtype=torch.int64, device=DEV)     # one tensor, zeroed once, never reset
    d = nat.AdamDesc()
    d.p, d.g, d.m, d.v, d.n = bk.ptr("p"), bk.ptr("g"), bk.ptr("m"), bk.ptr("v"), bk.n
    d.partial, d.lr, d.step = part.data_ptr(), lr_t.data_ptr(), step.data_ptr()
    d.beta1, d.beta2, d.eps, d.weight_decay, d.max_norm = BETAS[0], BETAS[1], EPS, wd, max_norm
    d.norm_out, d.step_is_current, d.n_partial_ready = norm.data_ptr(), 1, 0
    d.prep_descs, d.n_prep = (dd.data_ptr() if dd is not None else None), n_prep
    d.tick1, d.inc1, d.tick2, d.inc2 = None, 0, None, 0
    d.norm_slots, d.reduce_descs, d.n_reduce = _MEET["slots"].data_ptr(), None, 0
    return d


def _meet(st, lr, wd, max_norm, copies, reduce=None):
    """one gsage_clip_adam_meet as the NEXT update of this process's slots.  reduce: (descs, device buffers) -- the
    update sums the partial buffers itself.  -> dict(p, g, m, v, norm, t)"""
    nat = _nat()
    _MEET["step"] += 1                                # never reused, never 0: the slots' tag is the update number
    t = _MEET["step"]
    bk = _Bucket(st)
    part = torch.full((nat.lib().gsage_adam_partials(bk.n) + 4,), float("nan"), dtype=torch.float32, device=DEV)
    lr_t = torch.tensor([lr], dtype=torch.float32, device=DEV)
    step, norm = _i64(t), torch.full((1,), float("nan"), dtype=torch.float32, device=DEV)
    dd = _upload([cp.desc(bk.ptr("p", s)) for s, cp in copies], _eng()._PrepDesc)
    d = _meet_desc(bk, part, lr_t, step, norm, dd, len(copies), wd, max_norm)
    if reduce is not None:
        RD = _eng()._ReduceDesc
        rd = _upload([RD(tb.data_ptr() + 4 * r.off, r.stride, r.out_off, r.S, r.rows, r.cols, r.ld)
                      for r, tb in zip(*reduce)], RD)
        d.reduce_descs, d.n_reduce = rd.data_ptr(), len(reduce[0])
    nat.check(nat.lib().gsage_clip_adam_meet(ctypes.addressof(d), _stream()), "clip_adam_meet")
    torch.cuda.synchronize()
    out = bk.read()
    out.update(norm=float(norm.item()), t=t)
    assert int(step.item()) == t
    for s, cp in copies:
        cp.check(out["p"][s:s + cp.rows * cp.cols], ("copies of the new p at", s))
    return out


@pytest.mark.parametrize("n", [5, 1024, 5 * 1024 + 37])
def test_clip_adam_meet_in_launch_norm(n):
    """three consecutive updates on the same slots (clip active, inactive, active; the state carried from one to the
    next): each within the tolerance of clip_adam; with the clip inactive, the bits of gsage_clip_adam_step on the same
    inputs.  n = 5: one workgroup; 5 * 1 024 + 37: six, the last with 37 live elements."""
    st = _state(n, 41, 12.0)
    for k, norm in enumerate((12.0, 2.0, 30.0)):
        st["g"] = _state(n, 42 + k, norm)["g"]
        got = _meet(st, 0.01, 1e-3, 5.0, _slice_copies(n, "all"))
        ref = _check_update(got, st, got["t"], 0.01, 1e-3, 5.0, "meet/n%d/update%d/norm%g" % (n, k, norm))
        assert abs(got["norm"] - ref["norm"]) <= (n + 256) * ut.EPS24 * ref["norm"]
        if norm < 5.0:
            same = _step(st, got["t"], 0.01, 1e-3, 5.0, copies=_slice_copies(n, "all"), sic=1)
            for key in "pgmv":
                assert np.array_equal(_bits(got[key]), _bits(same[key])), key
            assert np.array_equal(_bits(got["g"]), _bits(st["g"]))
        st = dict(p=got["p"], g=None, m=got["m"], v=got["v"])


# descriptors that together cover [0, n): (S, rows, cols, ld) -- ragged cols, ld > cols; S < 32, so gsage_finalize_grads
# takes an in-order path for every one of them (scalar here: too few chunks for vec16 at these sizes)
REDUCE_SETS = {5: [(5, 1, 3, 4), (24, 2, 1, 3)],
               1024: [(24, 37, 19, 20), (1, 107, 3, 4)],
               5 * 1024 + 37: [(5, 100, 33, 36), (24, 37, 19, 23), (1, 1154, 1, 2)]}
# one in-order descriptor and two that gsage_finalize_grads sums in groups (max_elems = 703: gx = 3, gstride = 768)
REDUCE_SPLIT = [(5, 11, 3, 4), (33, 10, 15, 17), (65, 37, 19, 20)]       # scalar | wave4 | SL4


def _reduce_build(shapes, seed):
    rng = np.random.RandomState(seed)
    bufs, reds, out = [], [], 0
    for k, (S, rows, cols, ld) in enumerate(shapes):
        stride = rows * ld + (8 if ld % 4 == 0 else 3)
        buf = np.full(S * stride + 4, np.nan, dtype=np.float32)
        for s in range(S):
            buf[s * stride:s * stride + rows * ld].reshape(rows, ld)[:, :cols] = \
                rng.normal(size=(rows, cols)).astype(np.float32)
        bufs.append(buf)
        reds.append(ut.Red(k, 0, stride, out, S, rows, cols, ld))
        out += rows * cols
    return reds, bufs, out


def _finalized(reds, dbufs, n):
    """gsage_finalize_grads over the same descriptors -> the flat gradient (host)"""
    nat, RD = _nat(), _eng()._ReduceDesc
    dd = _upload([RD(tb.data_ptr() + 4 * r.off, r.stride, r.out_off, r.S, r.rows, r.cols, r.ld)
                  for r, tb in zip(reds, dbufs)], RD)
    mx = max(r.rows * r.cols for r in reds)
    flat = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    part = torch.zeros(nat.lib().gsage_finalize_partials(len(reds), mx), dtype=torch.float32, device=DEV)
    nat.check(nat.lib().gsage_finalize_grads(dd.data_ptr(), len(reds), mx, flat.data_ptr(), part.data_ptr(), None,
                                             None, 0, None, 0, _stream()), "finalize_grads")
    torch.cuda.synchronize()
    return _host(flat), mx


def _clipped_bound(reds, bufs, n, ref):
    """|g - coef * sum| allowed: the summation bound times the coefficient, one rounding of the product, and the float32
    coefficient itself -- a norm of n products and additions plus 256 in the block sums, a square root, an addition
    and a division (4 more roundings)"""
    flat, _ = ut.finalize(reds, bufs, n)
    return ref["coef"] * ut.finalize_bound(reds, bufs, n) + np.abs(ref["coef"] * flat) * (n + 256 + 4 + 1) * ut.EPS24


@pytest.mark.parametrize("n", sorted(REDUCE_SETS))
def test_clip_adam_meet_sums_the_partial_buffers(n):
    """reduce_descs: g is NaN beforehand and holds the float64 sum within the summation bound afterwards (times the clip
    coefficient when the clip is active); the update is as if g had been given; and where gsage_finalize_grads takes
    an in-order path -- every descriptor here -- g is what it stores, bit for bit"""
    reds, bufs, total = _reduce_build(REDUCE_SETS[n], n)
    assert total == n
    dbufs = [_dev(b) for b in bufs]
    flat64, _ = ut.finalize(reds, bufs, n)
    fin, mx = _finalized(reds, dbufs, n)
    gs = 256 * min(-(-mx // 256), 256)
    for r in reds:
        assert finalize_path(r.S, r.rows, r.cols, r.ld, r.stride, True, gs) in ("vec16", "scalar")
    scale = float(np.sqrt((flat64 * flat64).sum()))
    for max_norm in (2.0 * scale, 0.25 * scale):                       # clip inactive, active
        st = _state(n, 51, 1.0)
        given = dict(st, g=fin.copy())
        st["g"] = np.full(n, np.nan, dtype=np.float32)
        got = _meet(st, 0.01, 1e-3, max_norm, _slice_copies(n, "all"), reduce=(reds, dbufs))
        ref = ut.clip_adam(st["p"], flat64, st["m"], st["v"], f32(0.01), got["t"], BETAS, EPS, f32(1e-3), f32(max_norm))
        err = np.abs(got["g"].astype(np.float64) - ref["g"])
        assert (err <= _clipped_bound(reds, bufs, n, ref)).all(), ("g", n, float(err.max()))
        _check_update(got, given, got["t"], 0.01, 1e-3, max_norm, "meet/reduce/n%d/clip%d" % (n, ref["coef"] < 1.0))
        if ref["coef"] == 1.0:
            assert np.array_equal(_bits(got["g"]), _bits(fin)), "in-order paths: the bits of gsage_finalize_grads"
            same = _step(given, got["t"], 0.01, 1e-3, max_norm, copies=_slice_copies(n, "all"), sic=1)
            for key in "pmv":
                assert np.array_equal(_bits(got[key]), _bits(same[key])), key
        else:
            assert abs(float(ref["coef"]) - 0.25) < 1e-3


def test_clip_adam_meet_reduction_against_split_finalize_paths():
    """the folded reduction adds the buffers in order 0 .. S-1; gsage_finalize_grads does so on its in-order paths
    (vec16, scalar) and adds them in groups on the others (wave4: S = 33, SL4: S = 65 here).  Both are within the
    summation bound of the float64 sum; bit equality is required of the in-order descriptor only, and the number of
    elements that differ on the split paths is printed and logged (include/gsage.h, gsage_adam_desc.reduce_descs, makes
    the bit-for-bit claim for the in-order paths only)."""
    reds, bufs, n = _reduce_build(REDUCE_SPLIT, 3)
    dbufs = [_dev(b) for b in bufs]
    flat64, _ = ut.finalize(reds, bufs, n)
    bound = ut.finalize_bound(reds, bufs, n)
    fin, mx = _finalized(reds, dbufs, n)
    assert mx == 703
    paths = [finalize_path(r.S, r.rows, r.cols, r.ld, r.stride, True, 768) for r in reds]
    assert paths == ["scalar", "wave4", "SL4"]
    st = _state(n, 61, 1.0)
    st["g"] = np.full(n, np.nan, dtype=np.float32)
    got = _meet(st, 0.01, 0.0, 1e30, _slice_copies(n, "dst"), reduce=(reds, dbufs))
    assert (np.abs(got["g"].astype(np.float64) - flat64) <= bound).all()
    assert (np.abs(fin.astype(np.float64) - flat64) <= bound).all()
    differ = {}
    for r, path in zip(reds, paths):
        sl = slice(r.out_off, r.out_off + r.rows * r.cols)
        differ[path] = int((_bits(got["g"][sl]) != _bits(fin[sl])).sum())
    print("elements whose bits differ between the folded reduction and gsage_finalize_grads:", differ)
    note_parity("meet/reduce/split_paths_bits_differ", **differ)
    assert differ["scalar"] == 0


def test_clip_adam_meet_refusals():
    """what the entry point refuses returns an error code and launches nothing: supplied partials, no norm_slots,
    step_is_current == 0, no operand-copy descriptor, 17 reduce descriptors"""
    nat = _nat()
    n = 1024
    st = _state(n, 71, 12.0)
    bk = _Bucket(st)
    part = torch.zeros(8, dtype=torch.float32, device=DEV)
    lr_t = torch.tensor([0.01], dtype=torch.float32, device=DEV)
    step, norm = _i64(10 ** 6), torch.zeros(1, dtype=torch.float32, device=DEV)
    copies = _slice_copies(n)
    dd = _upload([cp.desc(bk.ptr("p", s)) for s, cp in copies], _eng()._PrepDesc)
    reds, bufs, _ = _reduce_build(REDUCE_SETS[n], 1)
    dbufs = [_dev(b) for b in bufs]
    RD = _eng()._ReduceDesc
    rd = _upload([RD(tb.data_ptr(), r.stride, r.out_off, r.S, r.rows, r.cols, r.ld) for r, tb in zip(reds, dbufs)] * 9, RD)

    def edit(**kw):
        d = _meet_desc(bk, part, lr_t, step, norm, dd, 1, 0.0, 5.0)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    bad = {"n_partial_ready != 0": edit(n_partial_ready=4),
           "no norm_slots": edit(norm_slots=None),
           "step_is_current == 0": edit(step_is_current=0),
           "no descriptor": edit(prep_descs=None, n_prep=0),
           "no descriptor (count 0)": edit(n_prep=0),
           "n_reduce of 17": edit(reduce_descs=rd.data_ptr(), n_reduce=17)}
    before = nat.launch_count()
    for what, d in bad.items():
        rc = nat.lib().gsage_clip_adam_meet(ctypes.addressof(d), _stream())
        assert rc != 0 and nat.lib().gsage_last_error(), what
    assert nat.lib().gsage_clip_adam_meet(None, _stream()) != 0
    torch.cuda.synchronize()
    assert nat.launch_count() == before
    got = bk.read()
    for k in "pgmv":
        assert np.array_equal(_bits(got[k]), _bits(st[k])), k
    assert int(step.item()) == 10 ** 6 and not _host(part).any()
