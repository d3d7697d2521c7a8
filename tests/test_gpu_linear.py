"""The K5 projection GEMM gsage_linear_nt (csrc/gsage_linear.hip) called directly through the C ABI against
linear_ref, at the shapes where its dispatch changes.  The output buffer is filled with a sentinel bit pattern (0xA5A5 /
0xA5A5A5A5), has ldc > groups * N and two guard rows; whatever lies outside the written cells (the columns before and
after each group's N, rows >= M, the guard rows, the elements before an offset C) must still hold it afterwards.  In A
and W everything the contract neither requires to be zero nor allows to be read holds NaN: the columns past
round_up(K, line) (DMA kernel) or past ceil(K / epc) * epc (staged kernel), W rows >= N, A rows >= M, table rows no
a_rows entry names, the slack between groups.  A NaN that reaches an accumulator shows in the output.

CASES below is the table; `kernel`, `halfw` and `stores` are what each case CLAIMS to run, written out as literals, and
test_linear_host.py holds them to linear_ref.k5_path / half_w / store_path (and the union of the claims to the list of
instantiations, ring phases and store paths), so an edited case cannot silently stop covering its path.

  family   cases                                          kernel                         ring phase       store path
  ring     K = 8, 64, 65, 128, 129, 192, 256, 320, 384,   k_linear_nt_dma<T, *, 1|2|3>   nk = 1, 1, 2, 2, wide, wide
           448, 1433 (bf16; fp32: 4, 32, 33, 64, 65, 96,                                 3, 3, 4, 5, 6,   (tile 1: 8 columns,
           128, 160, 192, 224, 1433) and ragged K = 1,                                   7, 23 (fp32 45)  half_w)
           70, 602; M = 65 (a second row tile with one                                   ragged: 1, 2|3,
           real row), N = 136                                                            10|19
           -staged: lda = ldw = round_up(K, epc) + epc    k_linear_nt<T, false, *>       the same nk      wide, wide
           (+ epc again where that is a whole line)
           -stagedw: only ldw off a line multiple         k_linear_nt<T, false, *>
  cols     N = 1, 32, 41, 64, 65, 72, 128, 129, 136, 200  k_linear_nt_dma<T, *, 3>       nk = 4; half_w   E, W, E, W, E, W, W,
           at nk = 4; lda, ldw one and two lines wider                                   T T T T F F F    WE, WW, WW
           than round_up(K, line): NaN past it                                           FT FT FF
  store    N = 136 (wide), N = 130 (tile 0 wide, tile 1   k_linear_nt_dma<T, *, 3>       nk = 3           WW, WE, EE, WW|EE,
           element), ldc = 153, groups = 2 with c_gstride                                                 EE, E
           = 137, C four bytes off, and the engines' prep
           shape (N = K = 64 written at element 602 of
           704-wide rows); every input x output type
  groups   groups = 2, 3 with distinct a_gstride,         both kernels                   nk = 3           wide
           w_gstride, c_gstride and a per-group bias;
           a_rows absent / for all groups / group 0 only,
           a permutation with repeats into a larger table
  edges    M = 1, 63, 64, 65, 129 and bias = NULL         both kernels                   nk = 3 (fp32 5)  wide
  real     seeded normals, W / sqrt(K); N = 130, M = 65;  dma<T, act, 1>, <.., 2>,       nk = 1, 2, 5,    WE
           every act x input type x output type           <.., 3> twice, staged          23 (fp32 45), 5
  busy     512 groups of one half_w tile (M = N = 64)     k_linear_nt_dma<T, relu, 3|2>  nk = 7, 2        wide
           that share ONE A (a_gstride = 0: it stays in
           the cache) and stream a W each from memory

The busy cases are what holds the counted waits: with idle memory the lines of a tile land together, and a wait that is
short by W's two instructions still finds them there.  Tried once on the MI355X with the kernel broken in a scratch copy:
  in-loop half_w wait vmcnt(4) -> vmcnt(6)      every other case passed; busy-bf16-K448 failed (81 001 of 2 097 152 cells)
  two-tile prologue half_w wait, the same       every other case passed; busy-bf16-K128 (840 511 cells) and busy-f32-K64
                                                (121 360 cells) failed
Being races, such breaks are caught with high probability, not with certainty; a correct kernel never fails them.
Dropping `cbase % epc == 0` from store_tile's `wide` sends group 1 of the store-*-gstride cases through 16-byte stores
at a 2- or 4-byte aligned address: the same bytes where the hardware tolerates that, a fault where it does not -- no
comparison of outputs can tell, and it was not run.  The host test pins that those tiles are claimed as element stores.

a. exact (`data` = int): operands are integers in [-8, 8] and the bias an integer in [-100, 100], so every partial sum
   is below 2^24 (64 * 1433 + 100) and any float32 / MFMA summation order gives the exact integer: the float32 output
   is compared BIT FOR BIT, the bf16 output with the reference's round-to-nearest-even.  The DMA and the staged kernel
   are compared with one reference, so they agree bit for bit; test_kernels_agree_on_real_data requires the same of
   them on the real-valued operands of (b) (both feed the same chunks to the same accumulators in the same order).
b. real (`data` = real): |got - ref| <= linear_ref.out_bound per cell: (K + 2) 2^-24 (sum |a w| + |bias|) for the
   pre-activation -- the worst case of the float32 fused multiply-add chain the fp32 MFMA is documented to be; for bf16
   operands the same bound is an ASSUMPTION (exact products, but the accumulation order inside the instruction is not
   documented) -- unchanged under relu and tanh (1-Lipschitz), plus linear_ref.tanh_term for the float32 evaluation of
   1 - 2 / (expf(2|v|) + 1) (expf taken at 3 ulp, an assumed figure: see linear_ref.EXPF_ULP), plus 2^-8 |ref| for a
   bf16 output.  None is tuned.  Every comparison prints its worst error / bound ratio and appends it to
   GSAGE_PARITY_LOG; recorded in profiles/linear_parity.jsonl (MI355X,
   60 lines, every ratio <= 0.992, the same figure from the DMA and the staged kernel on the same operands):
     fp32 operands, fp32 output   dma1 <= 0.110, dma2 <= 0.065, dma3 and staged <= 0.026, long (K = 1433) <= 0.0024: the
                                  measured error grows like sqrt(K) 2^-24, the bound like K 2^-24
     bf16 operands, fp32 output   dma1 <= 0.016, dma2 <= 0.010, dma3 and staged <= 0.004, long <= 0.0008
     bf16 output, either operand  0.961 - 0.992 at K <= 128, 0.865 - 0.976 at five k-tiles, 0.475 - 0.853 at K = 1433: the
                                  output's own rounding, 2^-8 |ref|, fills the bound
     tanh                         fp32 output <= 0.044 (below the same shape without it), bf16 output <= 0.982
c. refusals: every malformed call returns an error with a message, launches nothing and leaves the output alone."""
import collections
import zlib

import numpy as np
import pytest
import torch

import linear_ref as lr
from conftest import pkg
from util import note_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = {"bf16": np.uint16(0xA5A5), "f32": np.uint32(0xA5A5A5A5)}
BITS = {"bf16": np.uint16, "f32": np.uint32}
GUARD = 2                                          # guard rows of the output, and spare rows of W and of a direct A

# kernel: ("dma", NBUF, nk) | ("staged", nk); halfw: one T / F per column tile (None for the staged kernel); stores:
# one W / E per column tile, groups separated by |
Case = collections.namedtuple("Case", "name family data dtype c_dtype M N K lda ldw ldc act bias groups a_rows "
                                      "c_gstride c_off kernel halfw stores a_shared")


def _lds(dtype, K, layout):
    """(lda, ldw) of a layout: dma = exactly round_up(K, line); dma+ = one and two lines more; staged = round_up(K,
    epc) + epc, and epc more where that is a whole line; stagedw = only ldw off a line multiple"""
    line, epc = lr.LINE[dtype], lr.EPC[dtype]
    kp = lr.round_up(K, line)
    off = lr.round_up(K, epc) + epc
    if off % line == 0:
        off += epc
    return {"dma": (kp, kp), "dma+": (kp + line, kp + 2 * line), "staged": (off, off), "stagedw": (kp, off)}[layout]


def _mk(name, family, dtype, M, N, K, layout, kernel, halfw, stores, data="int", c_dtype=None, act="none", bias=True,
        groups=1, a_rows="none", ldc=None, c_gstride=None, c_off=0, a_shared=False):
    lda, ldw = _lds(dtype, K, layout)
    if c_gstride is None:
        c_gstride = lr.round_up(N, 8) + 8
    if ldc is None:
        ldc = groups * c_gstride + 8
    return Case(name, family, data, dtype, c_dtype or dtype, M, N, K, lda, ldw, ldc, act, bias, groups, a_rows,
                c_gstride, c_off, kernel, halfw if kernel[0] == "dma" else None, stores, a_shared)


# (K, nk): the ring phases -- NBUF = 1 (nk = 1), 2 (nk = 2), 3: exactly full (3), first refill (4), buffer wrap (5), even
# and odd drains (6, 7), a long chain; then the ragged K (a partial last chunk and a partial last line)
RING = {"bf16": [(8, 1), (64, 1), (65, 2), (128, 2), (129, 3), (192, 3), (256, 4), (320, 5), (384, 6), (448, 7), (1433, 23),
                 (1, 1), (70, 2), (602, 10)],
        "f32": [(4, 1), (32, 1), (33, 2), (64, 2), (65, 3), (96, 3), (128, 4), (160, 5), (192, 6), (224, 7), (1433, 45),
                (1, 1), (70, 3), (602, 19)]}
# N -> (half_w per column tile, store path per column tile) with ldc % 8 == 0 and an aligned C
COLS = [(1, "T", "E"), (32, "T", "W"), (41, "T", "E"), (64, "T", "W"), (65, "F", "E"), (72, "F", "W"), (128, "F", "W"),
        (129, "FT", "WE"), (136, "FT", "WW"), (200, "FF", "WW")]
NK3 = {"bf16": 192, "f32": 96}                     # K of three k-tiles: the first kernel whose ring never refills
NK4 = {"bf16": 256, "f32": 128}
NK7 = {"bf16": 448, "f32": 224}
NK2 = {"bf16": 128, "f32": 64}
BUSY_GROUPS = 512
# the real-valued shapes: name -> (K per dtype, layout, kernel per dtype)
REAL = [("dma1", {"bf16": 64, "f32": 32}, "dma", {"bf16": ("dma", 1, 1), "f32": ("dma", 1, 1)}),
        ("dma2", {"bf16": 100, "f32": 50}, "dma", {"bf16": ("dma", 2, 2), "f32": ("dma", 2, 2)}),
        ("dma3", {"bf16": 300, "f32": 150}, "dma", {"bf16": ("dma", 3, 5), "f32": ("dma", 3, 5)}),
        ("long", {"bf16": 1433, "f32": 1433}, "dma", {"bf16": ("dma", 3, 23), "f32": ("dma", 3, 45)}),
        ("staged", {"bf16": 300, "f32": 150}, "staged", {"bf16": ("staged", 5), "f32": ("staged", 5)})]


def _cases():
    out = []
    for dt in ("bf16", "f32"):
        for i, (K, nk) in enumerate(RING[dt]):
            act = ("none", "relu")[i % 2]
            out.append(_mk("ring-%s-K%d-dma" % (dt, K), "ring", dt, 65, 136, K, "dma", ("dma", min(nk, 3), nk), "FT", "WW",
                           act=act))
            for lay in ("staged", "stagedw"):
                out.append(_mk("ring-%s-K%d-%s" % (dt, K, lay), "ring", dt, 65, 136, K, lay, ("staged", nk), None, "WW",
                               act=act))
        for i, (N, hw, st) in enumerate(COLS):
            out.append(_mk("cols-%s-N%d" % (dt, N), "cols", dt, 65, N, NK4[dt], "dma+", ("dma", 3, 4), hw, st,
                           act=("relu", "none")[i % 2]))
        for cd in ("bf16", "f32"):
            tag, esz = "store-%s-%s-" % (dt, cd), lr.ESZ[cd]
            kw = dict(c_dtype=cd)
            out += [_mk(tag + "wide", "store", dt, 65, 136, NK3[dt], "dma", ("dma", 3, 3), "FT", "WW", **kw),
                    _mk(tag + "N130", "store", dt, 65, 130, NK3[dt], "dma", ("dma", 3, 3), "FT", "WE", act="relu", **kw),
                    _mk(tag + "ldc-odd", "store", dt, 65, 136, NK3[dt], "dma", ("dma", 3, 3), "FT", "EE", ldc=153, **kw),
                    _mk(tag + "gstride", "store", dt, 65, 136, NK3[dt], "dma", ("dma", 3, 3), "FT", "WW|EE", groups=2,
                        c_gstride=137, ldc=288, **kw),
                    _mk(tag + "ptr4", "store", dt, 65, 136, NK3[dt], "dma", ("dma", 3, 3), "FT", "EE", c_off=4 // esz,
                        act="relu", **kw),
                    # the engines' embedding prep: E = 64 columns written behind D0 = 602 feature columns of a 704-wide
                    # row, D0 * esz % 16 != 0
                    _mk(tag + "engine-D0", "store", dt, 65, 64, 64, "dma", ("dma", 1, 1) if dt == "bf16" else ("dma", 2, 2),
                        "T", "E", c_off=602, ldc=704, **kw)]
        for G in (2, 3):
            for ar in ("none", "all", "g0"):
                for lay in ("dma", "staged"):
                    kern = ("dma", 3, 3) if lay == "dma" else ("staged", 3)
                    out.append(_mk("groups-%s-G%d-%s-%s" % (dt, G, ar, lay), "groups", dt, 70, 72, NK3[dt], lay, kern, "F",
                                   "|".join("W" * G), groups=G, a_rows=ar, c_gstride=80, act=("none", "relu")[G % 2]))
        nk = 3 if dt == "bf16" else 5
        for M in (1, 63, 64, 65, 129):
            out.append(_mk("edges-%s-M%d" % (dt, M), "edges", dt, M, 40, 130, "dma", ("dma", 3, nk), "T", "W"))
        out += [_mk("edges-%s-nobias-dma" % dt, "edges", dt, 65, 40, 130, "dma", ("dma", 3, nk), "T", "W", bias=False),
                _mk("edges-%s-nobias-staged" % dt, "edges", dt, 65, 40, 130, "staged", ("staged", nk), None, "W", bias=False,
                    act="relu")]
        # BUSY_GROUPS workgroups of half_w tiles over seven k-tiles that share ONE A (a_gstride = 0: it stays in the
        # cache) while each streams a W of its own from memory: W's lines land well after A's
        for K, kern in ((NK7[dt], ("dma", 3, 7)), (NK2[dt], ("dma", 2, 2))):
            out.append(_mk("busy-%s-K%d" % (dt, K), "busy", dt, 64, 64, K, "dma", kern, "T", "|".join("W" * BUSY_GROUPS),
                           groups=BUSY_GROUPS, c_gstride=72, a_shared=True, act="relu"))
        for shape, Ks, lay, kerns in REAL:
            for cd in ("bf16", "f32"):
                for act in lr.ACTS:
                    out.append(_mk("real-%s-%s-%s-%s" % (dt, shape, cd, act), "real", dt, 65, 130, Ks[dt], lay, kerns[dt], "FT",
                                   "WE", data="real", c_dtype=cd, act=act))
    assert len({c.name for c in out}) == len(out)
    return out


CASES = _cases()
EXACT = [c for c in CASES if c.data == "int"]
BOUNDED = [c for c in CASES if c.data == "real"]


def table_rows(case):
    """rows of each group's A table: a larger table under a_rows, GUARD spare rows otherwise"""
    return case.M + (29 if case.a_rows != "none" else GUARD)


def strides(case):
    """(a_gstride, w_gstride): whole chunks, distinct, each with slack behind the group's rows; a_gstride = 0 where the
    groups share one A"""
    epc = lr.EPC[case.dtype]
    return 0 if case.a_shared else table_rows(case) * case.lda + 3 * epc, (case.N + GUARD) * case.ldw + 5 * epc


def indirect(case, g):
    return case.a_rows == "all" or (case.a_rows == "g0" and g == 0)


# ---- logical operands and their references: computed once per key, never modified ----------------------------------
_LOGICAL = {}


def logical(case):
    """-> dict(tabs [G][T, K], ids [M] or None, used [G] row lists, A [G][M, K], W [G][N, K], bias [G, N] or None, pre
    [G][M, N] float64, bound [G][M, N] (real data)).  Cases that differ only in layout share their operands."""
    key = (case.data, case.dtype, case.M, case.N, case.K, case.groups, case.a_rows, case.bias, case.a_shared)
    if key in _LOGICAL:
        return _LOGICAL[key]
    rng = np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7fffffff)
    M, N, K, G, T = case.M, case.N, case.K, case.groups, table_rows(case)

    def draw(rows, scale):
        if case.data == "int":
            return rng.randint(-8, 9, size=(rows, K)).astype(np.float32)
        x = (rng.standard_normal(size=(rows, K)) * scale).astype(np.float32)
        return lr.bf16_value(lr.bf16_rne(x)) if case.dtype == "bf16" else x

    ids = None
    if case.a_rows != "none":
        ids = rng.randint(0, T, size=M).astype(np.int64)
        ids[M // 2] = ids[0]                                          # a repeat
    tabs, Ws, used, As = [], [], [], []
    for g in range(G):
        tabs.append(tabs[0] if g and case.a_shared else draw(T, 1.0))
        Ws.append(draw(N, 1.0 / np.sqrt(K)))
        used.append(np.unique(ids) if indirect(case, g) else np.arange(M))
        As.append(tabs[g][ids] if indirect(case, g) else tabs[g][:M])
    bias = None
    if case.bias:
        bias = (rng.randint(-100, 101, size=(G, N)) if case.data == "int" else rng.standard_normal(size=(G, N))).astype(np.float32)
    pre = [lr.linear_pre(As[g], Ws[g], None if bias is None else bias[g], case.dtype) for g in range(G)]
    if case.data == "int":
        assert all(np.array_equal(p, np.rint(p)) and float(np.abs(p).max()) < 2 ** 24 for p in pre if p.size)
        bound = None
    else:
        bound = [lr.abs_bound(As[g], Ws[g], None if bias is None else bias[g], K, case.dtype) for g in range(G)]
    _LOGICAL[key] = dict(tabs=tabs, ids=ids, used=used, A=As, W=Ws, bias=bias, pre=pre, bound=bound)
    return _LOGICAL[key]


def host_buffers(case):
    """-> (A, W) as flat float32 arrays in the case's layout: the named rows hold their K values and zeros up to what
    the kernel of this layout may read (a whole line: DMA; a whole chunk: staged); NaN everywhere else"""
    L = logical(case)
    K, G, T = case.K, case.groups, table_rows(case)
    kern = lr.k5_path(case.dtype, case.lda, case.ldw, K)
    kz = lr.round_up(K, lr.LINE[case.dtype] if kern[0] == "dma" else lr.EPC[case.dtype])
    a_gs, w_gs = strides(case)
    A = np.full((G - 1) * a_gs + T * case.lda + 3 * lr.EPC[case.dtype], np.nan, dtype=np.float32)
    W = np.full(G * w_gs, np.nan, dtype=np.float32)
    for g in range(G):
        ra = A[g * a_gs:g * a_gs + T * case.lda].reshape(T, case.lda)
        ra[L["used"][g], :K] = L["tabs"][g][L["used"][g]]
        ra[L["used"][g], K:kz] = 0.0
        rw = W[g * w_gs:g * w_gs + case.N * case.ldw].reshape(case.N, case.ldw)
        rw[:, :K] = L["W"][g]
        rw[:, K:kz] = 0.0
    return A, W


def cell_index(case):
    """[G, M, N] flat element positions of the written cells in the output allocation"""
    g = np.arange(case.groups)[:, None, None] * case.c_gstride
    m = np.arange(case.M)[None, :, None] * case.ldc
    return case.c_off + g + m + np.arange(case.N)[None, None, :]


def out_elems(case):
    return case.c_off + (case.M + GUARD) * case.ldc


# ---- the device side -----------------------------------------------------------------------------------------------
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


def _operand(a, dtype):
    return _dev(a if dtype == "f32" else lr.bf16_rne(a))


def _sentinel(n, c_dtype):
    wide = c_dtype == "f32"
    fill = int(SENT[c_dtype].view(np.int32 if wide else np.int16))
    t = torch.full((n,), fill, dtype=torch.int32 if wide else torch.int16, device=DEV)
    assert t.data_ptr() % 16 == 0
    return t


def _code(nat, dtype):
    return nat.F32 if dtype == "f32" else nat.BF16


def _act(nat, act):
    return {"none": nat.ACT_NONE, "relu": nat.ACT_RELU, "tanh": nat.ACT_TANH}[act]


def launch(case):
    """one gsage_linear_nt call -> the output allocation's bits (flat)"""
    nat, L = _nat(), logical(case)
    assert lr.k5_path(case.dtype, case.lda, case.ldw, case.K) == case.kernel
    hA, hW = host_buffers(case)
    A, W = _operand(hA, case.dtype), _operand(hW, case.dtype)
    bias = _dev(L["bias"].reshape(-1)) if L["bias"] is not None else None
    ids = _dev(L["ids"]) if L["ids"] is not None else None
    C = _sentinel(out_elems(case), case.c_dtype)
    c_ptr = C.data_ptr() + case.c_off * lr.ESZ[case.c_dtype]
    want = [[lr.store_path(case.c_dtype, c_ptr, case.ldc, g, case.c_gstride, case.N, n0)[0].upper()
             for n0 in lr.column_tiles(case.N)] for g in range(case.groups)]
    assert "|".join("".join(w) for w in want) == case.stores
    a_gs, w_gs = strides(case)
    before = nat.launch_count()
    nat.check(nat.lib().gsage_linear_nt(A.data_ptr(), _code(nat, case.dtype), case.lda, ids.data_ptr() if ids is not None else None,
                                        1 if case.a_rows == "g0" else 0, W.data_ptr(), case.ldw,
                                        bias.data_ptr() if bias is not None else None, c_ptr, _code(nat, case.c_dtype),
                                        case.ldc, case.M, case.N, case.K, _act(nat, case.act), case.groups, a_gs, w_gs,
                                        case.c_gstride, _stream()), "linear_nt")
    torch.cuda.synchronize()
    assert nat.launch_count() == before + (1 if case.M else 0)
    return C.cpu().numpy().view(BITS[case.c_dtype])


def split(case, flat):
    """-> the written cells [G, M, N] (bits); asserts that everything else still holds the sentinel"""
    idx = cell_index(case)
    rest = np.ones(flat.shape[0], dtype=bool)
    rest[idx.reshape(-1)] = False
    bad = rest & (flat != SENT[case.c_dtype])
    assert not bad.any(), (case.name, "%d elements outside the written cells changed; first at element %d (row %d, "
                           "column %d of the output)" % (int(bad.sum()), int(np.argmax(bad)),
                                                         (int(np.argmax(bad)) - case.c_off) // case.ldc,
                                                         (int(np.argmax(bad)) - case.c_off) % case.ldc))
    return flat[idx]


def exact_bits(case):
    """[G, M, N] the bits an exact case must store"""
    L = logical(case)
    v = np.stack([lr.activate(p, case.act) for p in L["pre"]]).astype(np.float32)
    return v.view(np.uint32) if case.c_dtype == "f32" else lr.bf16_rne(v)


def values(case, bits):
    return bits.view(np.float32) if case.c_dtype == "f32" else lr.bf16_value(bits)


# =====================================================================================================================
# a. exact cases
# =====================================================================================================================
@pytest.mark.parametrize("case", EXACT, ids=[c.name for c in EXACT])
def test_exact_bits(case):
    """integer operands: every written cell bit for bit, everything else the sentinel"""
    got = split(case, launch(case))
    want = exact_bits(case)
    bad = got != want
    assert not bad.any(), (case.name, "%d cells differ; first at (group, row, column) %s: got %#x, want %#x"
                           % (int(bad.sum()), tuple(np.argwhere(bad)[0]), int(got[bad][0]), int(want[bad][0])))


def test_comparison_bites():
    """the same comparison against a reference with two W rows swapped, and against an output one column to the right,
    fails"""
    case = next(c for c in EXACT if c.name == "ring-bf16-K256-dma")
    flat = launch(case)
    got, want = split(case, flat), exact_bits(case)
    assert np.array_equal(got, want)
    swapped = want.copy()
    swapped[:, :, [3, 4]] = swapped[:, :, [4, 3]]
    assert not np.array_equal(got, swapped)
    with pytest.raises(AssertionError):
        split(case._replace(c_off=1), np.concatenate([flat, flat[:1]]))


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_empty(dtype):
    """M = 0: OK, no launch, nothing written"""
    case = next(c for c in EXACT if c.name == "edges-%s-M1" % dtype)
    flat = launch(case._replace(M=0, name="edges-%s-M0" % dtype))
    assert (flat == SENT[dtype]).all()


# =====================================================================================================================
# b. real-valued cases
# =====================================================================================================================
def _bounded(case, got_bits):
    L = logical(case)
    pre, pb = np.stack(L["pre"]), np.stack(L["bound"])
    ref = lr.activate(pre, case.act)
    bound = lr.out_bound(pre, pb, case.act, case.c_dtype)
    got = values(case, got_bits).astype(np.float64)
    assert np.isfinite(got).all(), (case.name, "non-finite output")
    assert (bound > 0).all()
    ratio = float((np.abs(got - ref) / bound).max())
    what = "linear/%s" % case.name
    print(what, "worst error / bound = %.4f" % ratio)
    note_parity(what, ratio=ratio)
    assert ratio <= 1.0, (what, ratio)


@pytest.mark.parametrize("case", BOUNDED, ids=[c.name for c in BOUNDED])
def test_real_bounded(case):
    """seeded normals against float64 within linear_ref.out_bound; everything outside the cells the sentinel"""
    _bounded(case, split(case, launch(case)))


@pytest.mark.parametrize("act", lr.ACTS)
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_kernels_agree_on_real_data(dtype, act):
    """the DMA kernel, the staged kernel and the staged kernel with only ldw off a line multiple give equal bits on the
    same real-valued operands, at one, two, five and many k-tiles"""
    for shape, Ks, lay, kerns in REAL[:4]:
        dma = next(c for c in BOUNDED if c.name == "real-%s-%s-f32-%s" % (dtype, shape, act))
        ref = split(dma, launch(dma))
        for lay2 in ("staged", "stagedw"):
            lda, ldw = _lds(dtype, dma.K, lay2)
            other = dma._replace(name=dma.name + "-" + lay2, lda=lda, ldw=ldw, kernel=("staged", dma.kernel[2]), halfw=None)
            got = split(other, launch(other))
            bad = got != ref
            assert not bad.any(), (other.name, "%d cells differ from the DMA kernel's; first at %s: %#x vs %#x"
                                   % (int(bad.sum()), tuple(np.argwhere(bad)[0]), int(got[bad][0]), int(ref[bad][0])))


# =====================================================================================================================
# c. refusals
# =====================================================================================================================
def test_refusals():
    """every malformed call returns an error code with a message, launches nothing and leaves the output alone; the
    buffers are small valid device buffers, so a wrongly accepted call does nothing worse than fail this test"""
    nat, lib, s = _nat(), _nat().lib(), _stream()
    M, N, K, ld = 8, 16, 64, 128
    A = torch.zeros(M + 1, ld, dtype=torch.bfloat16, device=DEV)
    W = torch.zeros(N + 1, ld, dtype=torch.bfloat16, device=DEV)
    bias = torch.zeros(N, dtype=torch.float32, device=DEV)
    C = _sentinel((M + GUARD) * 32, "f32")
    assert A.data_ptr() % 16 == 0 and W.data_ptr() % 16 == 0

    def call(**k):
        return lib.gsage_linear_nt(k.get("A", A.data_ptr()), k.get("dt", nat.BF16), k.get("lda", ld), None, 0,
                                   k.get("W", W.data_ptr()), k.get("ldw", ld), bias.data_ptr(), k.get("C", C.data_ptr()),
                                   k.get("cdt", nat.F32), 32, k.get("M", M), k.get("N", N), k.get("K", K),
                                   k.get("act", nat.ACT_NONE), k.get("groups", 1), 0, 0, 0, s)

    calls = {"bad dtype": dict(dt=7), "bad c_dtype": dict(cdt=5), "lda not a chunk multiple": dict(lda=68),
             "ldw not a chunk multiple": dict(ldw=100), "round_up(K, epc) > lda": dict(K=70, lda=64),
             "round_up(K, epc) > ldw": dict(K=70, ldw=64), "A 8 bytes off": dict(A=A.data_ptr() + 8),
             "W 8 bytes off": dict(W=W.data_ptr() + 8), "C = NULL": dict(C=None), "groups = 0": dict(groups=0),
             "groups = 65536": dict(groups=65536), "act = 3": dict(act=3), "N = 0": dict(N=0), "K = 0": dict(K=0)}
    torch.cuda.synchronize()
    before = nat.launch_count()
    for what, kw in calls.items():
        assert call(**kw) != 0 and lib.gsage_last_error(), what
    torch.cuda.synchronize()
    assert nat.launch_count() == before
    assert (C.cpu().numpy().view(np.uint32) == SENT["f32"]).all()
    nat.check(call(), "the well-formed call")
    torch.cuda.synchronize()
    assert nat.launch_count() == before + 1
