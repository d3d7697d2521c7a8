"""The gather kernels of csrc/gsage_gather.hip -- K2 gather+mean (single, multi-segment, FP8, and under a sampler side
role), its backward and the K6 scatter-add -- called directly through the C ABI against gather_ref.

Buffers.  Every output is filled with a sentinel bit pattern (0xA5A5 / 0xA5A5A5A5), has out_ld wider than what the launch
writes and two guard rows (the outputs of a multi launch are adjacent row slices of ONE such buffer, with a guard row in
front); everything outside the written set -- rows < M, columns < round_up(D, VEC); for FP8 the 16-byte pieces whose
first column is below D, or the elements below D -- must still hold the sentinel, and [D, round_up(D, VEC)) must be +0
bit for bit.  Tables hold NaN (FP8: the NaN code 0x7f) in every column >= D, the padding chunk included, in every row no
id names (the tables are larger than the id set) and behind the last row; FP8 scales are NaN past D.  A NaN that
reaches an output shows.  For the scatter-add the "sentinel" is the gradient's non-zero initial contents: bitwise
unchanged in the rows no id names and in the columns >= D.

CASES is the table; `vec`, `cols`, `store`, `path`, `rpi`, `first` and `kernel` are what each case CLAIMS, written as
literals or by the builders below, and test_gather_host.py holds them to gather_ref's restatement of dispatch_vec,
fill_multi, fp8_out_vec_ok and the wide predicate (and the union of the claims to its list of instantiations, paths,
fan-outs and item counts), so an edited case cannot silently stop covering its path.

  family  entry point                 cases                                                     claims
  sweep   gsage_gather_mean           M = 33, D = 40, ld = 64, all four type pairs; with ids    VEC 8 (bf16 -> bf16) or 4;
                                      n = 1 2 3 4 5 7 8 9 12 15 16 17 23 24 25 31 32 33 (the    the pipelined batches of 8:
                                      first mean all-equal ids, the second a duplicate);        full batch alone, next
                                      ids == NULL n = 1 3 4 5 7 8 9 11 12 13 16 21              batch of 1, two full; the
                                                                                                8 / 4 / 1 ladder
  vec     gsage_gather_mean           per type pair: D = 602 and D = 1 at the widest chunk; VEC VEC 8 / 4 / 2 / 1 and the
                                      4 by ld = 132 and by out_ld = 20; VEC 2 by ld = 602; VEC  zero tail [D, round_up)
                                      1 by ld = 131, by D = ld = 7, by a table and by an output
                                      one element off; D in 1 7 9 130 602, M in 1 33 257
  cap     gsage_gather_mean           bf16, n = 2, D = 40, M = 838 861: 16384 * 256 + 1 work    the stride loop; M = 0
                                      items; and M = 0 (nothing launched)
  single  gsage_gather_mean_multi     bf16, every n = 1: 1, 1023, 1024, 1025, 5000 and 5016     copy4 (four items per lane,
                                      items; 1, 3, 8 segments; row lists for all, none, some;   clamp + last-chunk masks)
                                      an empty segment in the middle; D = 8, 9, 602
  mixed   gsage_gather_mean_multi     n = 1 segments of M = 1 2 3 4 5 301 with and without row  rows4 next to mean; VEC 4
                                      lists next to n = 3 8 9 25; D = 42; also fp32 -> fp32 and without row copies
                                      fp32 -> bf16
  fp8     gsage_gather_mean_fp8,      n = 1 8 9 25 x D = 16 17 40 602 x bf16 / fp32 output x    VS, ES by out_ld, ES by the
          gsage_gather_rows_fp8,      {16-byte pieces, odd out_ld, out one element off};        base; multi: mean
          gsage_gather_mean_multi_fp8 multi launches with an empty and an ids == NULL segment
  role    gsage_gather_mean_multi_    adam = NULL, hops as in test_gpu_kernels (sampler_kat g2, k_gather_multi_adam_wide;
          adam                        B = 37, fans (6, 4)): n = 1 9 16 17 25 33 40 with row     k_gather_multi_adam with
                                      lists and n = 12 without (275 items); then M = 52 500,    the grid remapped round
                                      n = 9 (262 550 items > 256 Ki)                            the sampler's workgroups
  bwd     gsage_segment_mean_bwd      D = 4, 48 (16-byte kernel); D = 50, odd out_ld, either    k_segment_mean_bwd<4> / <1>
                                      base one float off (scalar); n = 1 3 10; M = 1 37
  scatter gsage_scatter_add_rows      n = 1 3; D = 1 16 50; scale 1, 0.25, 1/3; 37 * n ids over r / n row indexing, scale
                                      5 of 12 rows, once all equal; table_ld = D + 3
  refuse  all of the above            n = 0, ld < D, bad type pairs, FP8 to the plain entry points, 0 and 9 segments,
                                      ld % 8, a misaligned segment output, bf16 -> fp32 in multi, multi_adam with no
                                      role / out_dtype != dtype / a dense adjacency

Comparison.  Two tiers of data, both compared BIT FOR BIT with gather_ref.mean_in_order -- a float32 add chain from +0
in neighbour order, one float32 division by float32(n), round-to-nearest-even to bf16:
a. int: table values are integers in [-64, 64] (FP8: random e4m3 bytes without the two NaN codes: multiples of 2^-9 below
   448, so a sum of 25 needs 23 bits).  Every partial sum is exact in any order (test_gather_host.py checks < 2^24), so
   this tier checks addressing, masking and selection.
b. real: seeded normals, each table row scaled by 2^k, k in [-6, 6]; no denormals.  Summation order changes the low bits
   here, so this tier holds the order contract, and with it wide == narrow == multi == single launch: test_role_sampler runs
   the same segments through all four and compares each with the one reference.
That bit equality is attainable rests on two facts of the build, not on a measurement: the Makefile passes no fast-math
flag, and the device code of gsage_gather.hip divides with the v_div_scale / v_div_fmas / v_div_fixup sequence, the
correctly rounded float32 division.  The first run on the MI355X matched bit for bit at every n, powers of two or not,
so no weaker bound stands in for non-power-of-two n.
The backward is bit for bit float32(g) / float32(n).  The scatter-add with integer data and power-of-two scales is bit
for bit (atomic adds of exactly representable sums in any order); with real data and scale = float32(1/3) every cell is
within gather_ref.scatter_bound = (c + 1) 2^-24 (|init| + sum |scale row|), c the number of rows landing in the cell
(c adds and one multiply, worst case in any order).  The worst error / bound ratios are appended to GSAGE_PARITY_LOG and
recorded in profiles/gather_parity.jsonl (MI355X, 7 lines): at most 0.438 (n = 1, D = 50), 0.040 with all ids equal.

Value-only breaks, each tried once on the MI355X in a scratch copy of the kernel (none alters an index, a bound or a
pointer):
  accumulate all BATCH rows of a short last batch   21 of 30 tests fail: in each of the eight sweeps exactly the 14 fan-outs
                                                    with ids that are no multiple of 8 (n = 8, 16, 24, 32 and every
                                                    ids == NULL case pass); every vec case with ids (16 of 18 per type
                                                    pair); cap-bf16; the 30 FP8 cases with ids and n != 8 per output type;
                                                    all mixed, multi-FP8 and role cases (wide and narrow)
  drop the (c0 + e < D) zeroing (both forms)        9 tests fail: the ten vec cases per type pair with round_up(D, VEC) > D
                                                    (NaN in the zero tail); the eight FP8 16-byte-piece cases at D = 17 and
                                                    602 per output type and the D = 17 multi-FP8 launches; all mixed cases
                                                    (D = 42).  The all-single copies (their own masks) and everything at
                                                    D = 40 pass
  swap the half-word masks of the all-single path   single-items5000 fails (D = 9, the odd width: 1000 cells of its first
                                                    segment); at an even D both halves of every masked word are cleared
                                                    under either mask, so D = 8 and 602 cannot tell
  drop `scale` in the scatter kernel                14 of 20 scatter cases fail: all seven with scale 0.25 (bits differ) and
                                                    all seven with scale 1/3 (error / bound 1.6e5 .. 6.7e6); scale 1 passes

Left out: the Adam role of gsage_gather_mean_multi_adam (its in-launch norm is a meeting of resident workgroups: a test
that sizes it wrong hangs the card; test_gpu_update_tail.py covers it); the 64-bit branch of the row division (total >
2^32 work items: a 64 GB output); any search of compiled code and any sanitizer run."""
import collections
import ctypes
import os
import zlib

import numpy as np
import pytest
import torch

import gather_ref as gr
from conftest import load_golden, pkg
from util import csr_of, note_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = {"bf16": np.uint16(0xA5A5), "f32": np.uint32(0xA5A5A5A5)}
BITS = {"bf16": np.uint16, "f32": np.uint32}
GUARD = 2                                          # guard rows behind the last written row
POOL, NAMED = 64, 40                               # rows of a table read through ids, and how many of them ids may name
PAIRS = [("bf16", "bf16"), ("bf16", "f32"), ("f32", "f32"), ("f32", "bf16")]
SWEEP_IDS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 23, 24, 25, 31, 32, 33)
SWEEP_NULL = (1, 3, 4, 5, 7, 8, 9, 11, 12, 13, 16, 21)

# one launch of gsage_gather_mean / gsage_gather_mean_fp8 / gsage_gather_rows_fp8.  vec: the claimed chunk; cols: the
# claimed number of written columns; store (FP8): "VS" 16-byte pieces | "ES" element stores
Single = collections.namedtuple("Single", "name family fn dtype out_dtype M n D ld out_ld ids tab_off out_off data vec "
                                          "cols store")
# one multi-segment launch.  segs: ((M, n, has row list), ...); entry: multi | multi_fp8 | multi_adam; path: per segment
# copy4 | rows4 | mean; kernel: multi | multi_fp8 | narrow | wide
Multi = collections.namedtuple("Multi", "name family entry dtype out_dtype D ld out_ld segs data path rpi first kernel")


def _single(name, family, dtype, out_dtype, M, n, D, ld, out_ld, ids, data, vec, tab_off=0, out_off=0, fn="mean",
            store=None, cols=None):
    if cols is None:
        cols = gr.round_up(D, vec)
    return Single(name, family, fn, dtype, out_dtype, M, n, D, ld, out_ld, ids, tab_off, out_off, data, vec, cols, store)


def _multi(name, family, entry, dtype, out_dtype, D, ld, out_ld, segs, data, path, kernel):
    """rpi and first written out from the claimed path: a rows4 segment takes ceil(M / 4) * chunks work items"""
    v = {"fp8": 16, "bf16": 8, "f32": 4}[dtype]
    ch = -(-D // v)
    rpi = tuple(4 if p == "rows4" else 1 for p in path)
    first = [0]
    for (M, _n, _i), r in zip(segs, rpi):
        first.append(first[-1] + -(-M // r) * ch)
    return Multi(name, family, entry, dtype, out_dtype, D, ld, out_ld, tuple(segs), data, tuple(path), rpi, tuple(first),
                 kernel)


# vec family: tag -> (D, ld, out_ld, M, n, row list, table offset, output offset, VEC for bf16 -> bf16, VEC otherwise)
LAYOUTS = [("max-D602", 602, 608, 616, 257, 10, True, 0, 0, 8, 4),
           ("max-D1", 1, 8, 16, 1, 1, True, 0, 0, 8, 4),
           ("v4-ld132", 130, 132, 136, 257, 3, False, 0, 0, 4, 4),
           ("v4-outld20", 9, 16, 20, 1, 9, True, 0, 0, 4, 4),
           ("v2-ld602", 9, 602, 12, 33, 2, True, 0, 0, 2, 2),
           ("v1-ld131", 130, 131, 136, 33, 5, True, 0, 0, 1, 1),
           ("v1-D7-ld7", 7, 7, 16, 257, 1, True, 0, 0, 1, 1),
           ("v1-table-off", 9, 16, 24, 33, 17, True, 1, 0, 1, 1),
           ("v1-out-off", 9, 16, 24, 1, 4, True, 0, 1, 1, 1)]
CAP_M = 838861                                     # 838 861 rows x 5 chunks = 16384 * 256 + 1 work items
T, F = True, False
ROLE_WIDE = ((37, 1, T), (11, 9, T), (9, 16, T), (7, 17, T), (5, 25, T), (4, 33, T), (3, 40, T), (6, 12, F))
ROLE_NARROW = ((52500, 9, T), (37, 1, T))


def _cases():
    out = []
    for dt, od in PAIRS:
        v = 8 if (dt, od) == ("bf16", "bf16") else 4
        for data in ("int", "real"):
            for n in SWEEP_IDS:
                out.append(_single("sweep-%s-%s-ids-n%d-%s" % (dt, od, n, data), "sweep", dt, od, 33, n, 40, 64, 56, True,
                                   data, v))
            for n in SWEEP_NULL:
                out.append(_single("sweep-%s-%s-null-n%d-%s" % (dt, od, n, data), "sweep", dt, od, 33, n, 40, 64, 56,
                                   False, data, v))
            for tag, D, ld, old, M, n, ids, toff, ooff, v8, v4 in LAYOUTS:
                out.append(_single("vec-%s-%s-%s-%s" % (dt, od, tag, data), "vec", dt, od, M, n, D, ld, old, ids, data,
                                   v8 if (dt, od) == ("bf16", "bf16") else v4, tab_off=toff, out_off=ooff))
    out.append(_single("cap-bf16", "cap", "bf16", "bf16", CAP_M, 2, 40, 64, 48, True, "int", 8))
    out.append(_single("cap-M0", "cap", "bf16", "bf16", 0, 2, 40, 64, 48, True, "int", 8))
    # every n = 1, bf16: (name, D, segments)
    for name, D, segs in [("items1", 8, [(1, 1, T)]),
                          ("items1023", 8, [(500, 1, T), (0, 1, T), (523, 1, F)]),
                          ("items1024", 8, [(1024, 1, F)]),
                          ("items1025", 8, [(128, 1, T), (129, 1, T), (127, 1, T), (1, 1, T), (300, 1, T), (200, 1, T),
                                            (100, 1, T), (40, 1, T)]),
                          ("items5000", 9, [(1000, 1, T), (700, 1, F), (800, 1, T)]),
                          ("items5016", 602, [(30, 1, F), (0, 1, F), (36, 1, F)])]:
        ld = gr.round_up(D, 8) + 8
        out.append(_multi("single-" + name, "single", "multi", "bf16", "bf16", D, ld, ld, segs, "int",
                          ["copy4"] * len(segs), "multi"))
    mx1 = [(1, 1, T), (2, 1, F), (3, 1, T), (4, 1, F), (7, 3, T), (5, 8, T), (301, 1, T), (6, 25, T)]
    mx2 = [(1, 1, F), (2, 1, T), (3, 1, F), (4, 1, T), (9, 9, T), (5, 1, F), (301, 1, F), (5, 3, F)]
    mx3 = [(5, 1, T), (0, 8, T), (301, 1, F), (7, 3, T), (4, 9, T), (3, 25, F)]
    for data in ("int", "real"):
        for name, segs in (("a", mx1), ("b", mx2), ("c", mx3)):
            out.append(_multi("mixed-bf16-%s-%s" % (name, data), "mixed", "multi", "bf16", "bf16", 42, 64, 56, segs, data,
                              ["rows4" if n == 1 else "mean" for _m, n, _i in segs], "multi"))
        for od in ("f32", "bf16"):
            out.append(_multi("mixed-f32-%s-%s" % (od, data), "mixed", "multi", "f32", od, 42, 64, 56, mx3, data,
                              ["mean"] * len(mx3), "multi"))
    # FP8
    for od in ("bf16", "f32"):
        for i, D in enumerate((16, 17, 40, 602)):
            for n in (1, 8, 9, 25):
                ids = n == 1 or D != 40
                fn = "rows_fp8" if n == 1 and i % 2 == 0 else "fp8"
                ld, old = gr.round_up(D, 16) + 16, gr.round_up(D, 8) + 8
                e = 8 if od == "bf16" else 4
                for tag, o_ld, off, st in (("vs", old, 0, "VS"), ("es-ld", old + 1, 0, "ES"), ("es-ptr", old, 1, "ES")):
                    out.append(_single("fp8-%s-D%d-n%d-%s" % (od, D, n, tag), "fp8", "fp8", od, 33, n, D, ld, o_ld, ids,
                                       "int", 16, out_off=off, fn=fn, store=st,
                                       cols=gr.round_up(D, e) if st == "VS" else D))
        out.append(_multi("fp8-%s-multi-D40" % od, "fp8", "multi_fp8", "fp8", od, 40, 64, 48,
                          [(5, 1, T), (33, 8, T), (7, 9, F), (0, 3, T), (6, 25, T)], "int", ["mean"] * 5, "multi_fp8"))
        out.append(_multi("fp8-%s-multi-D17" % od, "fp8", "multi_fp8", "fp8", od, 17, 48, 32,
                          [(9, 1, T), (4, 1, F), (3, 1, T)], "int", ["mean"] * 3, "multi_fp8"))
    # the sampler side role
    for data in ("int", "real"):
        out.append(_multi("role-wide-%s" % data, "role", "multi_adam", "bf16", "bf16", 40, 64, 48, ROLE_WIDE, data,
                          ["rows4" if n == 1 else "mean" for _m, n, _i in ROLE_WIDE], "wide"))
    out.append(_multi("role-narrow-real", "role", "multi_adam", "bf16", "bf16", 40, 64, 48, ROLE_NARROW, "real",
                      ["mean", "rows4"], "narrow"))
    assert len({c.name for c in out}) == len(out)
    return out


CASES = _cases()
SINGLES = [c for c in CASES if isinstance(c, Single)]
MULTIS = [c for c in CASES if isinstance(c, Multi)]

# gsage_segment_mean_bwd: (name, D, ld, out_ld, dagg offset, output offset, claimed kernel VEC)
BWD = [("v4-D4", 4, 8, 12, 0, 0, 4), ("v4-D48", 48, 52, 56, 0, 0, 4), ("s-D50", 50, 52, 56, 0, 0, 1),
       ("s-outld57", 48, 52, 57, 0, 0, 1), ("s-out-off", 48, 52, 56, 0, 1, 1), ("s-in-off", 48, 52, 56, 1, 0, 1)]
BWD_N, BWD_M = (1, 3, 10), (1, 37)
# gsage_scatter_add_rows: (n, D, scale, data, ids all equal)
SCATTER = [(n, D, s, "int", False) for n in (1, 3) for D in (1, 16, 50) for s in (1.0, 0.25)] + \
          [(n, D, 1.0 / 3.0, "real", False) for n in (1, 3) for D in (1, 16, 50)] + \
          [(3, 16, 0.25, "int", True), (3, 16, 1.0 / 3.0, "real", True)]
SC_M, SC_ROWS, SC_NAMED = 37, 12, 5


# ---- logical inputs and their references: computed once per key, never modified --------------------------------------
_INPUTS = {}


def _rng(key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7fffffff)


def seg_inputs(key, dtype, data, M, n, D, has_ids, cache=True):
    """-> dict(R table rows, named [R] bool, ids [M * n] or None, values [R, D] float32 (what the kernel accumulates),
    codes [R, D] uint8 (FP8), scale [D] (FP8)).  The first mean's ids are all equal, the second holds a duplicate."""
    key = (key, dtype, data, M, n, D, has_ids)
    if cache and key in _INPUTS:
        return _INPUTS[key]
    rng = _rng(key)
    if has_ids:
        R = POOL
        pool = rng.permutation(R)[:NAMED]
        ids = pool[rng.randint(0, NAMED, size=M * n)].astype(np.int64)
        if n > 1 and M >= 1:
            ids[:n] = ids[0]
        if n > 1 and M >= 2:
            ids[n + 1] = ids[n]
        named = np.zeros(R, dtype=bool)
        named[ids] = True
    else:
        R = M * n + 3
        ids = None
        named = np.arange(R) < M * n
    codes = scale = None
    if dtype == "fp8":
        codes = rng.randint(0, 254, size=(R, D)).astype(np.uint8)
        codes[codes >= 0x7f] += 1                                     # 0x00 .. 0x7e, 0x80 .. 0xfe: no NaN code
        assert not ((codes & 0x7f) == 0x7f).any()
        values = gr.decode_e4m3(codes)
        scale = (2.0 ** rng.randint(-8, 9, size=D)).astype(np.float32)
    elif data == "int":
        values = rng.randint(-64, 65, size=(R, D)).astype(np.float32)
    else:
        values = (rng.standard_normal(size=(R, D)) * 2.0 ** rng.randint(-6, 7, size=(R, 1))).astype(np.float32)
        if dtype == "bf16":
            values = gr.bf16_value(gr.bf16_rne(values))
    inp = dict(R=R, named=named, ids=ids, values=values, codes=codes, scale=scale, M=M, n=n, D=D)
    if cache:
        _INPUTS[key] = inp
    return inp


def gathered(inp, lo, hi):
    """[hi - lo, n, D]: the rows means lo .. hi-1 accumulate, in neighbour order"""
    n = inp["n"]
    idx = inp["ids"][lo * n:hi * n] if inp["ids"] is not None else np.arange(lo * n, hi * n)
    return inp["values"][idx].reshape(hi - lo, n, inp["D"])


def ref_bits(inp, out_dtype):
    """[M, D] the bits the launch must store (in blocks of rows: the grid-cap case has 838 861)"""
    key = "ref-" + out_dtype
    if key not in inp:
        M = inp["M"]
        parts = [gr.out_bits(gr.mean_in_order(gathered(inp, lo, min(lo + 65536, M)), inp["scale"]), out_dtype)
                 for lo in range(0, M, 65536)]
        inp[key] = np.concatenate(parts) if parts else np.zeros((0, inp["D"]), dtype=BITS[out_dtype])
    return inp[key]


def case_inputs(case):
    if isinstance(case, Single):
        return seg_inputs(case.family if case.family in ("sweep", "fp8") else case.name, case.dtype, case.data, case.M,
                          case.n, case.D, case.ids, cache=case.M < 100000)
    inps = [seg_inputs((case.family, case.D, s), case.dtype, case.data, M, n, case.D, ids)
            for s, (M, n, ids) in enumerate(case.segs)]
    if case.dtype == "fp8":                                           # one scale vector per launch: the first segment's
        for inp in inps[1:]:
            if inp["scale"] is not inps[0]["scale"]:
                assert not any(k.startswith("ref-") for k in inp)
                inp["scale"] = inps[0]["scale"]
    return inps


def host_table(inp, dtype, ld, tab_off=0):
    """the table as the device sees it (bits): NaN in every column >= D, in every row no id names, in front of an
    offset table and behind the last row"""
    R, D = inp["R"], inp["D"]
    if dtype == "fp8":
        flat = np.full(tab_off + R * ld + 16, 0x7f, dtype=np.uint8)
        rows = flat[tab_off:tab_off + R * ld].reshape(R, ld)
        rows[inp["named"], :D] = inp["codes"][inp["named"]]
        return flat
    flat = np.full(tab_off + R * ld + 8, np.nan, dtype=np.float32)
    rows = flat[tab_off:tab_off + R * ld].reshape(R, ld)
    rows[inp["named"], :D] = inp["values"][inp["named"]]
    return gr.bf16_rne(flat) if dtype == "bf16" else flat


def host_scale(inp):
    """FP8 column scales: round_up(D, 16) floats are read; NaN past D"""
    s = np.full(gr.round_up(inp["D"], 16) + 4, np.nan, dtype=np.float32)
    s[:inp["D"]] = inp["scale"]
    return s


# ---- the device side -------------------------------------------------------------------------------------------------
def _nat():
    return pkg()._native


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype in (np.uint16, np.uint32):                            # (bit patterns travel as signed integers)
        a = a.view(np.int16 if a.dtype == np.uint16 else np.int32)
    t = torch.from_numpy(a).to(DEV)
    assert t.data_ptr() % 16 == 0
    return t


def _sentinel(n, dtype):
    wide = dtype == "f32"
    fill = int(SENT[dtype].view(np.int32 if wide else np.int16))
    t = torch.full((n,), fill, dtype=torch.int32 if wide else torch.int16, device=DEV)
    assert t.data_ptr() % 16 == 0
    return t


def _bits(t, dtype):
    return t.cpu().numpy().view(BITS[dtype])


def _code(nat, dtype):
    return {"f32": nat.F32, "bf16": nat.BF16, "fp8": nat.FP8}[dtype]


def check_out(name, flat, dtype, out_off, out_ld, regions):
    """flat: the bits of the whole allocation; regions: (first row, M, written columns, D, expected bits [M, D]).  The
    written cells bit for bit, [D, written columns) +0, everything else the sentinel."""
    assert not (flat[:out_off] != SENT[dtype]).any(), (name, "the elements in front of the output changed")
    body = flat[out_off:]
    assert body.size % out_ld == 0
    body = body.reshape(-1, out_ld)
    keep = np.ones(body.shape, dtype=bool)
    for row0, M, cols, D, want in regions:
        assert D <= cols <= out_ld and row0 + M + GUARD <= body.shape[0]
        keep[row0:row0 + M, :cols] = False
        got = body[row0:row0 + M, :D]
        bad = got != want
        assert not bad.any(), (name, "%d cells of the segment at row %d differ; first at (row, column) %s: got %#x, want %#x"
                               % (int(bad.sum()), row0, tuple(np.argwhere(bad)[0]), int(got[bad][0]), int(want[bad][0])))
        tail = body[row0:row0 + M, D:cols]
        assert not tail.any(), (name, "columns [D, round_up(D, VEC)) of the segment at row %d are not +0; first %#x"
                                % (row0, int(tail[tail != 0][0])))
    bad = keep & (body != SENT[dtype])
    assert not bad.any(), (name, "%d elements outside the written cells changed; first at (row, column) %s"
                           % (int(bad.sum()), tuple(np.argwhere(bad)[0])))


def launch_single(case, inp=None):
    """one single-segment launch -> the output allocation's bits"""
    nat, lib = _nat(), _nat().lib()
    inp = inp or case_inputs(case)
    tab = _dev(host_table(inp, case.dtype, case.ld, case.tab_off))
    ids = _dev(inp["ids"]) if inp["ids"] is not None else None
    out = _sentinel(case.out_off + (case.M + GUARD) * case.out_ld, case.out_dtype)
    tptr = tab.data_ptr() + case.tab_off * gr.ESZ[case.dtype]
    optr = out.data_ptr() + case.out_off * gr.ESZ[case.out_dtype]
    iptr = ids.data_ptr() if ids is not None else None
    before = nat.launch_count()
    if case.fn == "mean":
        assert gr.vec(case.dtype, case.out_dtype, case.ld, case.out_ld, tptr, optr, case.D) == case.vec
        rc = lib.gsage_gather_mean(tptr, _code(nat, case.dtype), case.ld, iptr, case.M, case.n, case.D, optr,
                                   _code(nat, case.out_dtype), case.out_ld, _stream())
    else:
        assert gr.fp8_out_vec_ok(optr, case.out_dtype, case.D, case.out_ld) == (case.store == "VS")
        scale = _dev(host_scale(inp))
        if case.fn == "rows_fp8":
            assert case.n == 1
            rc = lib.gsage_gather_rows_fp8(tptr, case.ld, scale.data_ptr(), iptr, case.M, case.D, optr,
                                           _code(nat, case.out_dtype), case.out_ld, _stream())
        else:
            rc = lib.gsage_gather_mean_fp8(tptr, case.ld, scale.data_ptr(), iptr, case.M, case.n, case.D, optr,
                                           _code(nat, case.out_dtype), case.out_ld, _stream())
    nat.check(rc, case.name)
    torch.cuda.synchronize()
    assert nat.launch_count() == before + (1 if case.M else 0), case.name
    return _bits(out, case.out_dtype)


def check_single(case):
    inp = case_inputs(case)
    flat = launch_single(case, inp)
    check_out(case.name, flat, case.out_dtype, case.out_off, case.out_ld,
              [(0, case.M, case.cols, case.D, ref_bits(inp, case.out_dtype))])


def seg_rows(case):
    """first output row of each segment: adjacent slices behind one guard row"""
    rows = [1]
    for M, _n, _i in case.segs:
        rows.append(rows[-1] + M)
    return rows


def launch_multi(case, hops=None):
    """one multi-segment launch -> the bits of the one output buffer all segments share"""
    nat, lib = _nat(), _nat().lib()
    inps = case_inputs(case)
    k = len(case.segs)
    tabs = [_dev(host_table(inp, case.dtype, case.ld)) for inp in inps]
    ids = [_dev(inp["ids"]) if inp["ids"] is not None else None for inp in inps]
    rows = seg_rows(case)
    out = _sentinel((rows[-1] + GUARD) * case.out_ld, case.out_dtype)
    esz = gr.ESZ[case.out_dtype]
    optrs = [out.data_ptr() + r * case.out_ld * esz for r in rows[:-1]]
    plan = gr.fill_multi([s[0] for s in case.segs], [s[1] for s in case.segs], case.dtype, case.out_dtype, case.ld, case.D,
                         case.out_ld, [t.data_ptr() for t in tabs], optrs)
    assert tuple(plan["first"]) == case.first and tuple(plan["rpi"]) == case.rpi
    Tp = (ctypes.c_void_p * k)(*[t.data_ptr() for t in tabs])
    Ip = (ctypes.c_void_p * k)(*[(i.data_ptr() if i is not None else None) for i in ids])
    Op = (ctypes.c_void_p * k)(*optrs)
    Ms = (ctypes.c_int64 * k)(*[s[0] for s in case.segs])
    ns = (ctypes.c_int32 * k)(*[s[1] for s in case.segs])
    before = nat.launch_count()
    if case.entry == "multi_fp8":
        scale = _dev(host_scale(inps[0]))
        rc = lib.gsage_gather_mean_multi_fp8(k, Tp, Ip, Op, Ms, ns, scale.data_ptr(), case.ld, case.D,
                                             _code(nat, case.out_dtype), case.out_ld, _stream())
    elif case.entry == "multi_adam":
        assert hops is not None
        rc = lib.gsage_gather_mean_multi_adam(k, Tp, Ip, Op, Ms, ns, _code(nat, case.dtype), case.ld, case.D,
                                              _code(nat, case.out_dtype), case.out_ld, None, ctypes.addressof(hops),
                                              _stream())
    else:
        rc = lib.gsage_gather_mean_multi(k, Tp, Ip, Op, Ms, ns, _code(nat, case.dtype), case.ld, case.D,
                                         _code(nat, case.out_dtype), case.out_ld, _stream())
    nat.check(rc, case.name)
    torch.cuda.synchronize()
    assert nat.launch_count() == before + 1, case.name
    return _bits(out, case.out_dtype)


def multi_cols(case):
    if case.dtype == "fp8":
        return gr.round_up(case.D, 8 if case.out_dtype == "bf16" else 4)
    return gr.round_up(case.D, 8 if case.dtype == "bf16" else 4)


def check_multi(case, flat):
    inps = case_inputs(case)
    rows = seg_rows(case)
    check_out(case.name, flat, case.out_dtype, 0, case.out_ld,
              [(rows[s], case.segs[s][0], multi_cols(case), case.D, ref_bits(inps[s], case.out_dtype))
               for s in range(len(case.segs))])


def _report(fails, total):
    """every failing case by name, then the first few messages"""
    return "%d of %d cases failed: %s\n%s" % (len(fails), total, " ".join(f[0] for f in fails),
                                              "\n".join("%s: %s" % f for f in fails[:6]))


def _each(cases, fn):
    """run fn over the cases; report every failing case by name"""
    fails = []
    for c in cases:
        try:
            fn(c)
        except AssertionError as e:
            fails.append((c.name, str(e).split("\n")[0][:300]))
    assert not fails, _report(fails, len(cases))


# =====================================================================================================================
# gsage_gather_mean and the FP8 single launches
# =====================================================================================================================
@pytest.mark.parametrize("data", ["int", "real"])
@pytest.mark.parametrize("dtype,out_dtype", PAIRS)
def test_fanout_sweep(dtype, out_dtype, data):
    """the pipelined batches of 8 (ids) and the 8 / 4 / 1 ladder (ids == NULL) at every fan-out of SWEEP_IDS / SWEEP_NULL"""
    mine = [c for c in SINGLES if c.family == "sweep" and (c.dtype, c.out_dtype, c.data) == (dtype, out_dtype, data)]
    assert len(mine) == len(SWEEP_IDS) + len(SWEEP_NULL)
    _each(mine, check_single)


@pytest.mark.parametrize("dtype,out_dtype", PAIRS)
def test_dispatch_vec(dtype, out_dtype):
    """every chunk width a type pair can reach, selected by ld, out_ld, D and either base address; the zero tail"""
    mine = [c for c in SINGLES if c.family == "vec" and (c.dtype, c.out_dtype) == (dtype, out_dtype)]
    assert len(mine) == 2 * len(LAYOUTS)
    _each(mine, check_single)


def test_grid_cap_and_empty():
    """16384 * 256 + 1 work items: the last one is the stride loop's second trip; M = 0 launches nothing"""
    _each([c for c in SINGLES if c.family == "cap"], check_single)


@pytest.mark.parametrize("out_dtype", ["bf16", "f32"])
def test_fp8_single(out_dtype):
    mine = [c for c in SINGLES if c.family == "fp8" and c.out_dtype == out_dtype]
    assert len(mine) == 48
    _each(mine, check_single)


def test_comparison_bites():
    """the same comparison against a reference with two columns swapped, against an output whose zero tail holds a
    value and against one whose neighbouring row was written fails"""
    case = next(c for c in SINGLES if c.name == "vec-bf16-bf16-max-D602-real")
    inp = case_inputs(case)
    flat = launch_single(case, inp)
    want = ref_bits(inp, case.out_dtype)
    check_out(case.name, flat, case.out_dtype, 0, case.out_ld, [(0, case.M, case.cols, case.D, want)])
    swapped = want.copy()
    swapped[:, [3, 4]] = swapped[:, [4, 3]]
    for edit in ("swap", "tail", "guard", "pad"):
        f2 = flat.copy()
        if edit == "tail":
            f2[5 * case.out_ld + case.D] = 0x3f80
        elif edit == "guard":
            f2[case.M * case.out_ld] = 0
        elif edit == "pad":
            f2[case.cols] = 0
        with pytest.raises(AssertionError):
            check_out(case.name, f2, case.out_dtype, 0, case.out_ld,
                      [(0, case.M, case.cols, case.D, swapped if edit == "swap" else want)])


# =====================================================================================================================
# the multi-segment launches
# =====================================================================================================================
def _check_multi_launch(case):
    check_multi(case, launch_multi(case))


def test_multi_all_single():
    """every n = 1 (bf16): four work items per lane, the clamp at total - 1, the last chunk's half-word masks"""
    mine = [c for c in MULTIS if c.family == "single"]
    assert len(mine) == 6
    _each(mine, _check_multi_launch)


def test_multi_mixed():
    """four-row copies next to means in one launch, outputs adjacent; fp32 tables without row copies"""
    mine = [c for c in MULTIS if c.family == "mixed"]
    assert len(mine) == 10
    _each(mine, _check_multi_launch)


def test_multi_fp8():
    mine = [c for c in MULTIS if c.family == "fp8"]
    assert len(mine) == 4
    _each(mine, _check_multi_launch)


# =====================================================================================================================
# the sampler side role: wide and narrow kernels
# =====================================================================================================================
def _role_setup():
    """graph, queue and counters exactly as test_gather_launch_carrying_a_sampler_equals_separate_launches"""
    gs = pkg()
    g = load_golden("sampler_kat.npz")
    adj = csr_of(g, "g2_")
    csr = gs.DeviceCSR.from_scipy(adj, torch.device(DEV))
    rng = np.random.RandomState(11)
    B, fans = 37, (6, 4)
    queue = torch.from_numpy(rng.randint(0, adj.shape[0], size=(4, B))).to(DEV)
    bidx = torch.full((1,), 2, dtype=torch.int64, device=DEV)
    ctr = torch.full((1,), 8, dtype=torch.int64, device=DEV)
    nat = _nat()

    def desc(ids, call_base, batch_base):
        d = nat.HopsDesc()
        d.rowptr, d.col, d.n_rows = csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.n_rows
        d.ids, d.B, d.n_hops = ids.data_ptr(), B, 2
        for k in range(5):
            d.fan[k] = fans[k] if k < 2 else 1
        d.max_deg, d.seed, d.call_ctr, d.call_base, d.rank = csr.max_deg, 5, ctr.data_ptr(), call_base, 1
        d.seed_queue, d.batch_idx, d.batch_base, d.n_batches = queue.data_ptr(), bidx.data_ptr(), batch_base, 4
        d.err_flag = csr.err_flag.data_ptr()
        return d

    size = B + B * 6 + B * 24
    return csr, queue, bidx, ctr, desc, size


@pytest.mark.parametrize("name", [c.name for c in MULTIS if c.family == "role"])
def test_role_sampler(name):
    """gsage_gather_mean_multi_adam with adam = NULL and a sampler: the gather outputs bit for bit with sentinels intact,
    the sampled frontier equal to the stand-alone gsage_sample_hops launch's, no counter ticked -- and the same segments
    through gsage_gather_mean_multi and through one gsage_gather_mean launch each give the same bits"""
    for var in ("GSAGE_GATHER_WIDE", "GSAGE_SIDE_ROLE_POS"):
        if os.environ.get(var) is not None:
            pytest.skip("%s is set: the kernel choice it overrides is read once per process" % var)
    case = next(c for c in MULTIS if c.name == name)
    nat = _nat()
    total = case.first[-1]
    assert gr.wide(case.dtype, [s[2] for s in case.segs], [s[1] for s in case.segs], total) == (case.kernel == "wide")
    csr, queue, bidx, ctr, desc, size = _role_setup()
    ref_next = torch.zeros(size, dtype=torch.int64, device=DEV)
    d = desc(ref_next, 2, 1)
    nat.check(nat.lib().gsage_sample_hops(ctypes.addressof(d), None), "sample_hops")
    torch.cuda.synchronize()
    assert torch.equal(ref_next[:37], queue[3]) and int(ref_next[37:].abs().sum()) > 0
    got_next = torch.zeros_like(ref_next)
    flat = launch_multi(case, hops=desc(got_next, 2, 1))
    check_multi(case, flat)
    assert torch.equal(got_next, ref_next)
    assert int(bidx.item()) == 2 and int(ctr.item()) == 8              # nothing ticked
    csr.check()
    # the same segments without a side role, and one launch each
    plain = case._replace(name=case.name + "-multi", entry="multi", kernel="multi")
    check_multi(plain, launch_multi(plain))
    inps = case_inputs(case)
    for s, (M, n, ids) in enumerate(case.segs):
        one = _single("%s-seg%d" % (case.name, s), "role", case.dtype, case.out_dtype, M, n, case.D, case.ld, case.out_ld,
                      ids, case.data, 8)
        got = launch_single(one, inps[s])
        check_out(one.name, got, one.out_dtype, 0, one.out_ld, [(0, M, one.cols, one.D, ref_bits(inps[s], one.out_dtype))])


# =====================================================================================================================
# backward and scatter-add
# =====================================================================================================================
@pytest.mark.parametrize("name,D,ld,out_ld,in_off,out_off,vec", BWD, ids=[b[0] for b in BWD])
def test_segment_mean_bwd(name, D, ld, out_ld, in_off, out_off, vec):
    """dneibs[i * n + j] = float32(g[i]) / float32(n) bit for bit; rows >= M * n, columns >= D and the element in front
    of an offset output keep the sentinel; dagg holds NaN in columns >= D and rows >= M"""
    nat, lib = _nat(), _nat().lib()
    for M in BWD_M:
        for n in BWD_N:
            what = "bwd-%s-M%d-n%d" % (name, M, n)
            rng = _rng(what)
            g = (rng.standard_normal(size=(M, D)) * 2.0 ** rng.randint(-6, 7, size=(M, 1))).astype(np.float32)
            host = np.full(in_off + (M + GUARD) * ld, np.nan, dtype=np.float32)
            host[in_off:in_off + M * ld].reshape(M, ld)[:, :D] = g
            dagg = _dev(host)
            out = _sentinel(out_off + (M * n + GUARD) * out_ld, "f32")
            iptr, optr = dagg.data_ptr() + 4 * in_off, out.data_ptr() + 4 * out_off
            assert gr.bwd_vec(D, ld, out_ld, iptr, optr) == vec
            before = nat.launch_count()
            nat.check(lib.gsage_segment_mean_bwd(iptr, ld, M, n, D, optr, out_ld, _stream()), what)
            torch.cuda.synchronize()
            assert nat.launch_count() == before + 1
            check_out(what, _bits(out, "f32"), "f32", out_off, out_ld,
                      [(0, M * n, D, D, gr.mean_bwd(g, n).view(np.uint32))])


def test_scatter_add_rows():
    """grad[ids[r]] += scale * rows[r / n]: integer data with power-of-two scales bit for bit, real data with scale 1/3
    within gather_ref.scatter_bound; rows no id names and columns >= D bitwise unchanged"""
    nat, lib = _nat(), _nat().lib()
    fails = []
    for n, D, scale, data, same in SCATTER:
        what = "scatter-n%d-D%d-s%.3g-%s%s" % (n, D, scale, data, "-same" if same else "")
        rng = _rng(what)
        ld, tld = D + 5, D + 3
        named = rng.permutation(SC_ROWS)[:SC_NAMED]
        ids = named[rng.randint(0, SC_NAMED, size=SC_M * n)].astype(np.int64)
        if same:
            ids[:] = ids[0]
        if data == "int":
            rows = rng.randint(-64, 65, size=(SC_M, D)).astype(np.float32)
            init = rng.randint(-64, 65, size=(SC_ROWS, tld)).astype(np.float32)
            init[init == 0] = 1.0
        else:
            rows = (rng.standard_normal(size=(SC_M, D)) * 2.0 ** rng.randint(-6, 7, size=(SC_M, 1))).astype(np.float32)
            init = rng.standard_normal(size=(SC_ROWS, tld)).astype(np.float32)
        host = np.full((SC_M + GUARD, ld), np.nan, dtype=np.float32)
        host[:SC_M, :D] = rows
        drows, dids, grad = _dev(host.reshape(-1)), _dev(ids), _dev(init.reshape(-1))
        before = nat.launch_count()
        nat.check(lib.gsage_scatter_add_rows(drows.data_ptr(), ld, dids.data_ptr(), SC_M, n, D, scale, grad.data_ptr(),
                                             tld, _stream()), what)
        torch.cuda.synchronize()
        assert nat.launch_count() == before + 1
        got = grad.cpu().numpy().reshape(SC_ROWS, tld)
        ref, mag, cnt = gr.scatter_add64(init[:, :D], rows, ids, n, scale)
        hit = cnt[:, 0] > 0
        try:
            assert hit.sum() == np.unique(ids).size < SC_ROWS
            assert np.array_equal(got[~hit].view(np.uint32), init[~hit].view(np.uint32)), "an unnamed row changed"
            assert np.array_equal(got[:, D:].view(np.uint32), init[:, D:].view(np.uint32)), "a column >= D changed"
            assert np.isfinite(got).all()
            if data == "int":
                assert np.array_equal(got[:, :D].view(np.uint32), ref.astype(np.float32).view(np.uint32)), "bits differ"
            else:
                bound = gr.scatter_bound(mag, cnt)
                ratio = float((np.abs(got[:, :D].astype(np.float64) - ref)[hit] / bound[hit]).max())
                print("gather/%s worst error / bound = %.4f" % (what, ratio))
                note_parity("gather/" + what, ratio=ratio)
                assert ratio <= 1.0, ratio
        except AssertionError as e:
            fails.append((what, str(e).split("\n")[0][:300]))
    assert not fails, _report(fails, len(SCATTER))


# =====================================================================================================================
# refusals
# =====================================================================================================================
def test_refusals():
    """every malformed call returns an error code with a message, launches nothing and leaves the output alone; the
    buffers are small valid device buffers, so a wrongly accepted call does nothing worse than fail this test"""
    nat, lib, s = _nat(), _nat().lib(), _stream()
    M, D, ld, R = 4, 16, 32, 16
    tab = torch.zeros(R * ld + 16, dtype=torch.bfloat16, device=DEV)
    ids = torch.zeros(M * 4, dtype=torch.int64, device=DEV)
    out = _sentinel((9 * M + GUARD) * ld, "f32")                      # (wide enough for either output type)
    B16, F32, FP8 = nat.BF16, nat.F32, nat.FP8

    def single(**k):
        return lib.gsage_gather_mean(tab.data_ptr(), k.get("dt", B16), k.get("ld", ld), ids.data_ptr(), M, k.get("n", 2),
                                     k.get("D", D), out.data_ptr(), k.get("odt", B16), k.get("old", ld), s)

    def multi(entry="multi", hops=None, **k):
        n_seg = k.get("n_seg", 2)
        Tp = (ctypes.c_void_p * 9)(*[tab.data_ptr()] * 9)
        Ip = (ctypes.c_void_p * 9)(*[ids.data_ptr()] * 9)
        Op = (ctypes.c_void_p * 9)(*[out.data_ptr() + j * M * ld * 4 + k.get("out_shift", 0) for j in range(9)])
        Ms = (ctypes.c_int64 * 9)(*[M] * 9)
        ns = (ctypes.c_int32 * 9)(*[2] * 9)
        if entry == "multi":
            return lib.gsage_gather_mean_multi(n_seg, Tp, Ip, Op, Ms, ns, k.get("dt", B16), k.get("ld", ld), D,
                                               k.get("odt", B16), ld, s)
        return lib.gsage_gather_mean_multi_adam(n_seg, Tp, Ip, Op, Ms, ns, k.get("dt", B16), k.get("ld", ld), D,
                                                k.get("odt", B16), ld, None,
                                                ctypes.addressof(hops) if hops is not None else None, s)

    _csr, _queue, _bidx, _ctr, desc, size = _role_setup()
    nxt = torch.zeros(size, dtype=torch.int64, device=DEV)
    dense = desc(nxt, 2, 1)
    dense.dense_adj, dense.dense_ld, dense.sel = tab.data_ptr(), 4, ids.data_ptr()
    calls = {"n = 0": lambda: single(n=0), "ld < D": lambda: single(ld=8), "out_ld < D": lambda: single(old=8),
             "table dtype 7": lambda: single(dt=7), "output dtype 5": lambda: single(odt=5),
             "FP8 to gather_mean": lambda: single(dt=FP8), "FP8 output": lambda: single(odt=FP8),
             "0 segments": lambda: multi(n_seg=0), "9 segments": lambda: multi(n_seg=9),
             "multi ld % 8": lambda: multi(ld=36), "misaligned segment output": lambda: multi(out_shift=2),
             "multi bf16 -> fp32": lambda: multi(odt=F32), "FP8 to multi": lambda: multi(dt=FP8),
             "FP8 to multi_adam": lambda: multi("adam", hops=desc(nxt, 2, 1), dt=FP8),
             "multi_adam without a role": lambda: multi("adam"),
             "multi_adam fp32 -> bf16": lambda: multi("adam", hops=desc(nxt, 2, 1), dt=F32, odt=B16),
             "multi_adam dense adjacency": lambda: multi("adam", hops=dense)}
    torch.cuda.synchronize()
    before = nat.launch_count()
    for what, call in calls.items():
        assert call() != 0 and lib.gsage_last_error(), what
    torch.cuda.synchronize()
    assert nat.launch_count() == before
    assert (_bits(out, "f32") == SENT["f32"]).all() and int(nxt.abs().sum()) == 0
    nat.check(single(), "the well-formed single call")
    nat.check(multi(), "the well-formed multi call")
    nat.check(multi("adam", hops=desc(nxt, 2, 1)), "the well-formed multi_adam call")
    torch.cuda.synchronize()
    assert nat.launch_count() == before + 3
