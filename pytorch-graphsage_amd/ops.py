"""
ops.py -- tensor-level operators of the hot path, bound to libgsage_hip.so through ctypes.

PyTorch is plumbing here: it owns device memory, streams and autograd bookkeeping; the work is
done by the HIP kernels behind include/gsage.h.  Dispatch rule (no silent fallback):
  * CUDA tensors  -> the native library, always; a missing / stale library raises
                     NativeLibraryError (see _native.py).
  * CPU tensors   -> "host mode": the same operator written with stock torch ops, used only for
                     the reference's CPU configuration (`train.py --no-cuda`, BASELINE config 1)
                     and for the multi-process gloo tests.  Never reached from a CUDA tensor.

Reference call sites each operator replaces are cited per function.
"""
import ctypes
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import _native as nat
from .store import FP8, FeatureStore, RowRef, _round_up, quantize_fp8_host

_vp = ctypes.c_void_p


class _Config(object):
    compute_dtype = "bf16"      # "bf16": MFMA bf16 in / fp32 accumulate;  "fp32": exact-fp32 MFMA


config = _Config()


def set_compute_dtype(name):
    assert name in ("bf16", "fp32")
    config.compute_dtype = name


def torch_dtype(name=None):
    return {"bf16": torch.bfloat16, "fp32": torch.float32}[name or config.compute_dtype]


def _code(dtype):
    if dtype == torch.float32:
        return nat.F32
    if dtype == torch.bfloat16:
        return nat.BF16
    if dtype == FP8:
        return nat.FP8
    raise TypeError("gsage: unsupported dtype %s" % dtype)


def _ptr(t):
    return _vp(t.data_ptr()) if t is not None else None


def _stream():
    return _vp(torch.cuda.current_stream().cuda_stream)


def warmup(device):
    """Load the library (raises loudly when it is missing) before any graph capture."""
    nat.lib()


def _dgrad(gc, wa, K):
    """d input = gc @ W[:, :K] -- gc [M, N] in the compute type, wa [N, >= K] the weight's operand copy -- on K5
    (gsage_linear_nt: the NT kernel against the TRANSPOSED operand copy), fp32 result [M, K].  The backward of the
    module path (the literal aggregator_lookup[...] plug-in under autograd, reference nn_modules.py:196-204,
    :223-232) runs no library GEMM: round 4 still called torch.mm here."""
    cdt = gc.dtype
    epc = 8 if cdt == torch.bfloat16 else 4
    M, N = gc.shape
    out = torch.empty(M, K, dtype=torch.float32, device=gc.device)
    if M == 0:
        return out
    ga = _pad_cast(gc, cdt, 8 * epc)
    wt = _pad_cast(wa[:, :K].t(), cdt, 8 * epc)              # [K, round_up(N)]: rows = this product's outputs
    _linear_launch(_ptr(ga), ga.stride(0), None, 0, _ptr(wt), wt.stride(0), None, _ptr(out), K, M, K, N,
                   nat.ACT_NONE, 1, 0, 0, 0, _code(cdt), nat.F32)
    return out


def _wgrad_any(gc, xa, K):
    """d W = gc^T @ xa[:, :K] on K5b (gsage_wgrad: bf16 MFMA, or its fp32 twin in the parity mode) for ANY shape:
    the columns of gc are padded to whole 16-byte chunks (zero columns: zero rows of the result, dropped), the rows of
    xa taken as they are when they already are.  fp32 result [N, K]."""
    cdt = gc.dtype
    mult = 8 if cdt == torch.bfloat16 else 4
    M, N = gc.shape
    if M == 0:
        return torch.zeros(N, K, dtype=torch.float32, device=gc.device)
    g = _pad_cast(gc, cdt, mult)
    ok = (xa.dtype == cdt and xa.stride(1) == 1 and xa.stride(0) % mult == 0 and xa.data_ptr() % 16 == 0 and
          xa.stride(0) >= _round_up(K, 4))
    x = xa if ok else _pad_cast(xa[:, :K], cdt, mult)
    Np = g.shape[1]
    return wgrad(g, x, x.stride(0), 0, M, Np, K, Np)[0][:N]


def mark_zero_padded(view):
    """Tag a [:, :D] view of a buffer THIS library filled (rows gathered with their zero padding) so
    that _pad_cast may hand it to the GEMM kernels as is."""
    view._gsage_zero_padded = True
    return view


def _trusted(t):
    return bool(getattr(t, "_gsage_zero_padded", False))


def _pad_cast(t, dtype, mult, trusted=False):
    """[M, D] -> contiguous [M, round_up(D, mult)] of `dtype`, zero padded (no copy if already so).
    The GEMM kernels read whole padded rows, so a strided [:, :D] view is passed through only when the
    caller vouches for its pad columns (`trusted`: buffers this library produced, see
    mark_zero_padded); a user tensor sliced out of a wider buffer is copied into a zeroed one."""
    M, D = t.shape
    ld = _round_up(D, mult)
    if t.dtype == dtype and ld == D and t.is_contiguous():
        return t
    if trusted and t.dtype == dtype and t.stride(1) == 1 and t.stride(0) == ld and t.data_ptr() % 16 == 0:
        return t              # [:, :D] view of rows that are already padded (pad columns zero: gathered rows)
    out = torch.zeros(M, ld, dtype=dtype, device=t.device) if ld != D else \
        torch.empty(M, ld, dtype=dtype, device=t.device)
    out[:, :D] = t
    return out


# =============================================================================================
# K1  sampler
# =============================================================================================
def _philox_host(seed, call, g0, count, max_deg):
    """numpy Philox4x32-10 for host mode; same definition as the kernel (include/gsage.h)."""
    g = np.arange(g0, g0 + count, dtype=np.uint64)
    blk = g >> np.uint64(2)
    c = [(blk & np.uint64(0xFFFFFFFF)), (blk >> np.uint64(32)),
         np.full(count, call & 0xFFFFFFFF, dtype=np.uint64),
         np.full(count, (call >> 32) & 0xFFFFFFFF, dtype=np.uint64)]
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)) & mask, p1 & mask,
             ((p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)) & mask, p0 & mask]
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    words = np.stack(c, axis=1)[np.arange(count), (g & np.uint64(3)).astype(np.int64)]
    return ((words * np.uint64(max_deg)) >> np.uint64(32)).astype(np.int64)


_JUMP_TABLE = {}
MT_PAR_MIN = 400000          # requests below this many values stay on the one-workgroup kernel (~1 ms)
MT_PAR_MAX = 80000000        # values per parallel call: 4096 jump units of 64 refills reach 1.6e8 raw words


JUMP_TABLE_SHA256 = "2d7b0a6ba6b6c1566432f44eda5f747868391536bc0ceb09fd7efa9bc4420669"    # 39 936 words


def jump_table_ok(tab):
    """The jump polynomials are a constant of MT19937 (no seed enters them): a file is trusted by content, not by size."""
    import hashlib
    return hashlib.sha256(tab.tobytes()).hexdigest() == JUMP_TABLE_SHA256


def mt_jump_table(device):
    """The seed-independent jump polynomials of numpy's MT19937 (gsage_mt_jump_table: 128 x 312 words) on `device`.
    Computed by the library (~1 s: Berlekamp-Massey + square-and-multiply) the first time ever, then read from
    mt19937_jump_table.bin next to the library (written by __graft_entry__.build(), or here when missing)."""
    key = str(device)
    if key not in _JUMP_TABLE:
        import numpy as np
        L = nat.lib()
        words = int(L.gsage_mt_jump_table_words())
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mt19937_jump_table.bin")
        tab = None
        if os.path.exists(path) and os.path.getsize(path) == 8 * words:
            tab = np.fromfile(path, dtype=np.uint64)
            if not jump_table_ok(tab):           # a torn or stale file: recompute (the table is seed-independent)
                tab = None
        if tab is None:
            tab = np.zeros(words, dtype=np.uint64)
            nat.check(L.gsage_mt_jump_table(tab.ctypes.data, words), "mt_jump_table")
            assert jump_table_ok(tab), "gsage_mt_jump_table produced a table that is not MT19937's"
            tmp = "%s.%d.tmp" % (path, os.getpid())        # (every rank of a data-parallel run may get here at once)
            try:
                tab.tofile(tmp)
                os.replace(tmp, path)
            except OSError:
                try:
                    os.remove(tmp)
                except OSError:
                    pass
        _JUMP_TABLE[key] = torch.from_numpy(tab.view(np.int64)).to(device)
    return _JUMP_TABLE[key]


def _mt_choice_par(state, high, segs, flat):
    """the requests served by up to 256 workgroups at once (gsage_mt_choice_par); segs as in mt_choice_segments"""
    L = nat.lib()
    top = high - 1
    mask = (1 << top.bit_length()) - 1
    rate = (top + 1) / (mask + 1)
    table = mt_jump_table(flat.device)
    i = 0
    while i < len(segs):                          # (pieces of <= MT_PAR_MAX values: the jump table's reach)
        j, total = i, 0
        while j < len(segs) and (j == i or total + segs[j][1] <= MT_PAR_MAX):
            total += segs[j][1]
            j += 1
        part = segs[i:j]
        if total > MT_PAR_MAX:                    # one request larger than the reach: cut it
            o, c = part[0]
            part, segs = [(o, MT_PAR_MAX)], segs[:i] + [(o, MT_PAR_MAX), (o + MT_PAR_MAX, c - MT_PAR_MAX)] + segs[i + 1:]
            total, j = MT_PAR_MAX, i + 1
        units = int(total / (624.0 * rate) * 1.015 / 64) + 2
        per = -(-units // 256)
        n_wg = -(-units // per)
        cum = [0]
        for _, c in part:
            cum.append(cum[-1] + c)
        host = torch.tensor([cum, [o for o, _ in part] + [0]], dtype=torch.int64)
        dev = host.to(flat.device)
        scratch = torch.empty(int(L.gsage_mt_choice_par_scratch(n_wg)), dtype=torch.uint8, device=flat.device)
        nat.check(L.gsage_mt_choice_par(_ptr(state), int(high), len(part), _ptr(dev[0]), _ptr(dev[1]), total, _ptr(flat),
                                        _ptr(table), _ptr(scratch), scratch.numel(), n_wg, per, _stream()),
                  "mt_choice_par")
        i = j
    return flat


def mt_choice_segments(state, high, segs, out):
    """numpy's legacy stream on the device (`state`: helpers.legacy_stream.acquire), many np.random.choice(high, .)
    requests in ONE call: segs = [(offset into out, count)], served in order; out: int32 CUDA tensor (any shape,
    offsets address its flat view).  Large requests (an epoch's sampler draws) are served by many workgroups at
    once (gsage_mt_choice_par: jump-ahead), small ones by the one-workgroup kernel; values, state and position are
    numpy's either way."""
    segs = [(int(o), int(c)) for o, c in segs if c > 0]
    if not segs:
        return out
    flat = out.view(-1)
    assert flat.dtype == torch.int32 and flat.is_cuda and max(o + c for o, c in segs) <= flat.numel()
    if high < 2:                                   # a range of one value: numpy draws nothing
        for o, c in segs:
            flat[o:o + c].zero_()
        return out
    if sum(c for _, c in segs) >= MT_PAR_MIN and os.environ.get("GSAGE_MT_PARALLEL", "1") == "1":
        _mt_choice_par(state, int(high), segs, flat)
        return out
    host = torch.tensor([[o for o, _ in segs], [c for _, c in segs]], dtype=torch.int64)
    dev = host.to(flat.device)
    nat.check(nat.lib().gsage_mt_choice_segments(_ptr(state), int(high), len(segs), _ptr(dev[0]), _ptr(dev[1]),
                                                 _ptr(flat), _stream()), "mt_choice_segments")
    return out              # (`dev` may be freed: the caching allocator reuses it in stream order only)


def sample_csr(csr, ids, n, sel=None, philox=None, out=None):
    """SparseUniformNeighborSampler.__call__ (nn_modules.py:80-101).

    ids: LongTensor [M] on csr.device.  Exactly one of
      sel    : IntTensor [M*n] in [0, max_deg)   (parity level 1 / compat mode)
      philox : dict(seed, call_base, g0, call_ctr=None|cuda uint64-as-int64 tensor[1])
    Returns LongTensor [M*n] on the same device."""
    assert n > 0, "SparseUniformNeighborSampler: n_samples must be set explicitly"
    ids = ids.contiguous().view(-1)
    M = int(ids.shape[0])
    if ids.is_cuda:
        L = nat.lib()
        if out is None:
            out = torch.empty(M * n, dtype=torch.int64, device=ids.device)
        assert out.dtype == torch.int64 and out.numel() == M * n and out.is_contiguous()
        if sel is not None:
            sel = sel.contiguous().view(-1)
            assert sel.dtype == torch.int32 and sel.shape[0] == M * n and sel.is_cuda
            nat.check(L.gsage_sample_csr_sel(_ptr(csr.rowptr), _ptr(csr.col), csr.n_rows, _ptr(ids),
                                             M, n, _ptr(sel), _ptr(out), _ptr(csr.err_flag),
                                             _stream()), "sample_csr_sel")
        else:
            ctr = philox.get("call_ctr")
            sel_out = philox.get("sel_out")
            nat.check(L.gsage_sample_csr_philox(_ptr(csr.rowptr), _ptr(csr.col), csr.n_rows,
                                                _ptr(ids), M, n, csr.max_deg, int(philox["seed"]),
                                                _ptr(ctr), int(philox.get("call_base", 0)),
                                                int(philox.get("g0", 0)), _ptr(out), _ptr(sel_out),
                                                _ptr(csr.err_flag), _stream()), "sample_csr_philox")
        return out
    # ---- host mode
    idn = ids.numpy()
    if idn.size and (idn.min() < 0 or idn.max() >= csr.n_rows):
        raise IndexError("sampler: node id out of range of the adjacency")
    if sel is None:
        ctr = philox.get("call_ctr")
        call = int(philox.get("call_base", 0)) + (int(ctr.item()) if ctr is not None else 0)
        seln = _philox_host(int(philox["seed"]), call, int(philox.get("g0", 0)), M * n, csr.max_deg)
    else:
        seln = sel.numpy().reshape(-1).astype(np.int64)
    rp = csr.rowptr.numpy()
    beg = np.repeat(rp[idn], n)
    deg = np.repeat(rp[idn + 1] - rp[idn], n)
    off = np.where(deg > 0, seln % np.maximum(deg, 1), 0)
    col = csr.col.numpy()
    vals = col[np.minimum(beg + off, max(col.shape[0] - 1, 0))] if col.shape[0] else np.zeros_like(off)
    return torch.from_numpy(np.where(deg > 0, vals, 0).astype(np.int64))


# =============================================================================================
# Weighted adjacencies: the per-edge integer CDF and the edge-weight sampler (csrc/gsage_weighted.hip)
# =============================================================================================
WEIGHTED_TAG = 0x57000000                                                             # include/gsage.h


def edge_cdf(rowptr, weight, n_rows):
    """The table of a weighted adjacency (include/gsage.h, gsage_edge_cdf_build): weight fp32 [nnz] (already
    validated: finite, >= 0) -> int64 [nnz] holding the uint64 bits of each row's inclusive running sum of quanta
    q_e = floor(w_e * 2^(24 - E)), (f, E) = frexp(the row's largest weight); an all-zero row stays 0.  Set-up, once per
    adjacency.  CPU tensors: the same integers in numpy (float64 holds every scaled weight exactly)."""
    n_rows, nnz = int(n_rows), int(weight.shape[0])
    assert weight.dtype == torch.float32 and weight.is_contiguous() and rowptr.dtype == torch.int64
    if weight.is_cuda:
        cdf = torch.zeros(nnz, dtype=torch.int64, device=weight.device)
        if nnz:
            nat.check(nat.lib().gsage_edge_cdf_build(_ptr(rowptr), _ptr(weight), n_rows, _ptr(cdf), _stream()),
                      "edge_cdf_build")
        return cdf
    rp, w = rowptr.numpy(), weight.numpy().astype(np.float64)
    if nnz == 0:
        return torch.zeros(0, dtype=torch.int64)
    deg = np.diff(rp)
    rows = np.flatnonzero(deg > 0)
    m = np.zeros(n_rows, dtype=np.float64)
    m[rows] = np.maximum.reduceat(w, rp[rows])
    _, E = np.frexp(m)
    shift = np.repeat(24 - E.astype(np.int64), deg)
    q = np.where(np.repeat(m, deg) > 0, np.floor(np.ldexp(w, shift)), 0.0).astype(np.uint64)
    run = np.cumsum(q, dtype=np.uint64)
    before = np.concatenate([[0], run]).astype(np.uint64)[rp[:-1]]         # the running sum in front of each row
    return torch.from_numpy((run - np.repeat(before, deg)).view(np.int64))


def _mulhi64(a, b):
    """high 64 bits of the 128-bit product of two uint64 arrays (numpy has no such product: four 32-bit pieces)"""
    m, s = np.uint64(0xFFFFFFFF), np.uint64(32)
    a0, a1, b0, b1 = a & m, a >> s, b & m, b >> s
    mid = (a1 * b0 & m) + (a0 * b1 & m) + (a0 * b0 >> s)
    return a1 * b1 + (a1 * b0 >> s) + (a0 * b1 >> s) + (mid >> s)


def sample_csr_weighted(csr, ids, n, philox, out=None):
    """SparseWeightedNeighborSampler.__call__ (include/gsage.h, gsage_sample_csr_weighted): n neighbours of every id,
    each drawn in proportion to its edge's quantum; a row without a drawable edge yields the dummy 0.
    csr: a store.DeviceCSR with an edge_cdf; philox: dict(seed, call_base, g0, call_ctr) as for sample_csr.
    Returns LongTensor [M*n] on the ids' device.  CPU tensors: the same definition in numpy (host mode)."""
    assert n > 0, "SparseWeightedNeighborSampler: n_samples must be set explicitly"
    if csr.edge_cdf is None:
        raise ValueError("sample_csr_weighted: the adjacency carries no edge weights (DeviceCSR.with_weights)")
    ids = ids.contiguous().view(-1)
    M = int(ids.shape[0])
    seed, base, g0 = int(philox["seed"]), int(philox.get("call_base", 0)), int(philox.get("g0", 0))
    ctr = philox.get("call_ctr")
    if ids.is_cuda:
        if out is None:
            out = torch.empty(M * n, dtype=torch.int64, device=ids.device)
        assert out.dtype == torch.int64 and out.numel() == M * n and out.is_contiguous()
        nat.check(nat.lib().gsage_sample_csr_weighted(_ptr(csr.rowptr), _ptr(csr.col), _ptr(csr.edge_cdf), csr.n_rows,
                                                      _ptr(ids), M, n, seed, _ptr(ctr), base, g0, _ptr(out),
                                                      _ptr(csr.err_flag), _stream()), "sample_csr_weighted")
        return out
    # ---- host mode
    idn = ids.numpy()
    if idn.size and (idn.min() < 0 or idn.max() >= csr.n_rows):
        raise IndexError("sampler: node id out of range of the adjacency")
    count = M * n
    if count == 0 or csr.nnz == 0:
        return torch.zeros(count, dtype=torch.int64)
    call = (base + (int(ctr.item()) if ctr is not None else 0)) & 0xFFFFFFFFFFFFFFFF
    g = (np.arange(count, dtype=np.uint64) + np.uint64(g0 & 0xFFFFFFFFFFFFFFFF))
    blk = g >> np.uint64(1)
    mask, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    c = [blk & mask, blk >> s32, np.full(count, call & 0xFFFFFFFF, dtype=np.uint64),
         np.full(count, call >> 32, dtype=np.uint64)]
    k0, k1 = seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ WEIGHTED_TAG
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> s32) ^ c[1] ^ np.uint64(k0)) & mask, p1 & mask, ((p0 >> s32) ^ c[3] ^ np.uint64(k1)) & mask, p0 & mask]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    odd = (g & np.uint64(1)).astype(bool)
    r64 = (np.where(odd, c[2], c[0]) << s32) | np.where(odd, c[3], c[1])
    rp, col, cdf = csr.rowptr.numpy(), csr.col.numpy(), csr.edge_cdf.numpy().view(np.uint64)
    beg, end = np.repeat(rp[idn], n), np.repeat(rp[idn + 1], n)
    T = np.where(end > beg, cdf[np.maximum(end, 1) - 1], np.uint64(0)).astype(np.uint64)
    live = T > 0
    x = _mulhi64(r64, T)
    lo, hi = np.where(live, beg, 0), np.where(live, end - 1, 0)          # cdf[end - 1] = T > x: the answer is in [lo, hi]
    while True:
        act = lo < hi
        if not act.any():
            break
        mid = (lo + hi) >> 1
        gt = cdf[mid] > x
        hi = np.where(act & gt, mid, hi)
        lo = np.where(act & ~gt, mid + 1, lo)
    vals = col[lo].astype(np.int64) if col.shape[0] else np.zeros(count, dtype=np.int64)
    return torch.from_numpy(np.where(live, vals, 0).astype(np.int64))


def sample_hops_weighted(csr, ids, B, fans, philox):
    """Every hop of a weighted frontier (include/gsage.h, gsage_sample_hops_weighted: one launch): ids is the
    concatenated buffer [hop 0 | hop 1 | ... | hop L] (int64, B (1 + n1 + n1 n2 + ...) entries) with hop 0 filled; hop k
    is written as sample_csr_weighted(hop k - 1, fans[k - 1]) under call index call_base + k - 1 and
    g0 = rank * |hop k|.  philox: dict(seed, call_base, call_ctr, optional rank).  Returns ids.
    CPU tensors: the host definition of the per-hop draw, hop after hop (host mode)."""
    fans = [int(n) for n in fans]
    assert 1 <= len(fans) <= 5 and all(n > 0 for n in fans), "sample_hops_weighted: 1..5 hops of n_samples > 0"
    if csr.edge_cdf is None:
        raise ValueError("sample_hops_weighted: the adjacency carries no edge weights (DeviceCSR.with_weights)")
    B = int(B)
    sizes = [B]
    for n in fans:
        sizes.append(sizes[-1] * n)
    assert ids.dtype == torch.int64 and ids.dim() == 1 and ids.is_contiguous() and ids.numel() == sum(sizes)
    seed, base, rank = int(philox["seed"]), int(philox.get("call_base", 0)), int(philox.get("rank", 0))
    ctr = philox.get("call_ctr")
    if ids.is_cuda:
        d = nat.HopsDesc()
        d.rowptr, d.col, d.n_rows = csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.n_rows
        d.ids, d.B, d.n_hops = ids.data_ptr(), B, len(fans)
        for k in range(5):
            d.fan[k] = fans[k] if k < len(fans) else 1
        d.max_deg, d.seed, d.call_base, d.rank = 1, seed, base, rank
        d.call_ctr = ctr.data_ptr() if ctr is not None else None
        d.err_flag = csr.err_flag.data_ptr()
        nat.check(nat.lib().gsage_sample_hops_weighted(ctypes.addressof(d), _ptr(csr.edge_cdf), _stream()),
                  "sample_hops_weighted")
        return ids
    off = 0
    for k, n in enumerate(fans):
        ph = {"seed": seed, "call_base": base + k, "g0": rank * sizes[k + 1]}
        if ctr is not None:
            ph["call_ctr"] = ctr
        ids[off + sizes[k]:off + sizes[k] + sizes[k + 1]] = sample_csr_weighted(csr, ids[off:off + sizes[k]], n, ph)
        off += sizes[k]
    return ids


# =============================================================================================
# Distinct neighbours: sampling without replacement (csrc/gsage_distinct.hip)
# =============================================================================================
DISTINCT_TAG = 0x44000000                                                             # include/gsage.h
DISTINCT_N_MAX = 256


def _philox_words_host(seed, tag, call, g0, count):
    """uint64 [count]: word g & 3 of Philox block g >> 2 for g = g0 .. g0 + count - 1 under the key
    {lo(seed), hi(seed) ^ tag} (the uniform sampler's addressing, include/gsage.h)"""
    g = np.arange(count, dtype=np.uint64) + np.uint64(g0 & 0xFFFFFFFFFFFFFFFF)
    blk = g >> np.uint64(2)
    mask, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    call &= 0xFFFFFFFFFFFFFFFF
    c = [blk & mask, blk >> s32, np.full(count, call & 0xFFFFFFFF, dtype=np.uint64),
         np.full(count, call >> 32, dtype=np.uint64)]
    k0, k1 = seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ tag
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> s32) ^ c[1] ^ np.uint64(k0)) & mask, p1 & mask, ((p0 >> s32) ^ c[3] ^ np.uint64(k1)) & mask, p0 & mask]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, axis=1)[np.arange(count), (g & np.uint64(3)).astype(np.int64)]


def sample_csr_distinct(csr, ids, n, philox, out=None):
    """SparseDistinctNeighborSampler.__call__ (include/gsage.h, "Distinct neighbours", gsage_sample_csr_distinct): n
    neighbours of every id WITHOUT replacement -- a row of degree <= n returns every stored edge floor(n / deg) or
    ceil(n / deg) times (the row rotated by a uniform r), a longer row n distinct stored edges (n steps of a
    Fisher-Yates shuffle); a row of degree 0 yields the dummy 0.  csr: a store.DeviceCSR (edge weights, if any, are
    not read); philox: dict(seed, call_base, g0, call_ctr) as for sample_csr.  Returns LongTensor [M*n] on the ids'
    device.  CPU tensors: the same definition in numpy (host mode)."""
    n = int(n)
    assert 1 <= n <= DISTINCT_N_MAX, "SparseDistinctNeighborSampler: n_samples must be in 1..%d" % DISTINCT_N_MAX
    ids = ids.contiguous().view(-1)
    M = int(ids.shape[0])
    seed, base, g0 = int(philox["seed"]), int(philox.get("call_base", 0)), int(philox.get("g0", 0))
    ctr = philox.get("call_ctr")
    if ids.is_cuda:
        if out is None:
            out = torch.empty(M * n, dtype=torch.int64, device=ids.device)
        assert out.dtype == torch.int64 and out.numel() == M * n and out.is_contiguous()
        nat.check(nat.lib().gsage_sample_csr_distinct(_ptr(csr.rowptr), _ptr(csr.col), csr.n_rows, _ptr(ids), M, n, seed,
                                                      _ptr(ctr), base, g0, _ptr(out), _ptr(csr.err_flag), _stream()),
                  "sample_csr_distinct")
        return out
    # ---- host mode
    idn = ids.numpy()
    if idn.size and (idn.min() < 0 or idn.max() >= csr.n_rows):
        raise IndexError("sampler: node id out of range of the adjacency")
    if M == 0 or csr.nnz == 0:
        return torch.zeros(M * n, dtype=torch.int64)
    call = base + (int(ctr.item()) if ctr is not None else 0)
    w = _philox_words_host(seed, DISTINCT_TAG, call, g0, M * n).reshape(M, n)
    rp, col = csr.rowptr.numpy(), csr.col.numpy()
    beg, deg = rp[idn], (rp[idn + 1] - rp[idn]).astype(np.uint64)
    s32, slot = np.uint64(32), np.arange(n, dtype=np.uint64)
    off = np.zeros((M, n), dtype=np.uint64)
    short = (deg > 0) & (deg <= n)
    if short.any():                                    # every neighbour: the row rotated by r = (w_0 deg) >> 32
        d = deg[short]
        off[short] = (slot[None, :] + ((w[short, 0] * d) >> s32)[:, None]) % d[:, None]
    rows = np.flatnonzero(deg > n)
    if rows.size:                                      # n distinct edges: the shuffle's per-slot form, all rows at once
        t = slot[None, :] + ((w[rows] * (deg[rows, None] - slot[None, :])) >> s32)
        for j in range(n):
            x = t[:, j].copy()
            for i in range(j - 1, -1, -1):
                x[t[:, i] == x] = i
            off[rows, j] = x
    vals = col[np.minimum(beg[:, None] + off.astype(np.int64), col.shape[0] - 1)].astype(np.int64)
    return torch.from_numpy(np.where(deg[:, None] > 0, vals, 0).reshape(-1))


def sample_hops_distinct(csr, ids, B, fans, philox):
    """Every hop of a distinct-draw frontier (include/gsage.h, gsage_sample_hops_distinct: one launch): ids is the
    concatenated buffer [hop 0 | hop 1 | ... | hop L] (int64, B (1 + n1 + n1 n2 + ...) entries) with hop 0 filled; hop k
    is written as sample_csr_distinct(hop k - 1, fans[k - 1]) under call index call_base + k - 1 and
    g0 = rank * |hop k|.  philox: dict(seed, call_base, call_ctr, optional rank).  Returns ids.
    CPU tensors: the host definition of the per-hop draw, hop after hop (host mode)."""
    fans = [int(n) for n in fans]
    assert 1 <= len(fans) <= 5 and all(1 <= n <= DISTINCT_N_MAX for n in fans), \
        "sample_hops_distinct: 1..5 hops of n_samples in 1..%d" % DISTINCT_N_MAX
    B = int(B)
    sizes = [B]
    for n in fans:
        sizes.append(sizes[-1] * n)
    assert ids.dtype == torch.int64 and ids.dim() == 1 and ids.is_contiguous() and ids.numel() == sum(sizes)
    seed, base, rank = int(philox["seed"]), int(philox.get("call_base", 0)), int(philox.get("rank", 0))
    ctr = philox.get("call_ctr")
    if ids.is_cuda:
        d = nat.HopsDesc()
        d.rowptr, d.col, d.n_rows = csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.n_rows
        d.ids, d.B, d.n_hops = ids.data_ptr(), B, len(fans)
        for k in range(5):
            d.fan[k] = fans[k] if k < len(fans) else 1
        d.max_deg, d.seed, d.call_base, d.rank = 1, seed, base, rank
        d.call_ctr = ctr.data_ptr() if ctr is not None else None
        d.err_flag = csr.err_flag.data_ptr()
        nat.check(nat.lib().gsage_sample_hops_distinct(ctypes.addressof(d), _stream()), "sample_hops_distinct")
        return ids
    off = 0
    for k, n in enumerate(fans):
        ph = {"seed": seed, "call_base": base + k, "g0": rank * sizes[k + 1]}
        if ctr is not None:
            ph["call_ctr"] = ctr
        ids[off + sizes[k]:off + sizes[k] + sizes[k + 1]] = sample_csr_distinct(csr, ids[off:off + sizes[k]], n, ph)
        off += sizes[k]
    return ids


# =============================================================================================
# Temporal neighbours: sampling over the edges before a query time, snapshots (csrc/gsage_temporal.hip)
# =============================================================================================
TEMPORAL_TAG = 0x54000000                                                             # include/gsage.h
TEMPORAL_STRATEGIES = {"uniform": 0, "recent": 1}                                     # GSAGE_TEMPORAL_UNIFORM / _RECENT
TEMPORAL_INHERIT = {"seed": 0, "edge": 1}                                             # GSAGE_TEMPORAL_INHERIT_SEED / _EDGE
INT64_MAX = (1 << 63) - 1


def _temporal_csr(csr, who):
    if getattr(csr, "etime", None) is None:
        raise ValueError("%s: the adjacency carries no edge times (DeviceCSR.with_times)" % who)
    return csr


def _temporal_count_host(rp, et, rows, t):
    """cnt int64 [len(rows)]: per row the number of edges with etime < t (t: an array per row); the rows are in time
    order, so one binary search over all rows at once"""
    lo, hi = rp[rows].copy(), rp[rows + 1].copy()
    beg = lo.copy()
    while True:
        act = lo < hi
        if not act.any():
            break
        mid = (lo + hi) >> 1
        before = np.zeros(lo.shape, dtype=bool)
        before[act] = et[mid[act]] < t[act]
        lo = np.where(act & before, mid + 1, lo)
        hi = np.where(act & ~before, mid, hi)
    return lo - beg


def sample_csr_temporal(csr, ids, times, n, philox, strategy="uniform", inherit="seed", out=None, out_time=None):
    """SparseTemporalNeighborSampler.__call__ (include/gsage.h, "Temporal neighbours", gsage_sample_csr_temporal): n
    neighbours of every id among the edges that happened strictly BEFORE the id's query time -- strategy "uniform":
    uniformly with replacement, off = (w * cnt) >> 32; "recent": the min(n, cnt) latest, most recent first, cycled -- and
    the query times of the next hop: the parent's own (inherit "seed") or the walked edge's (inherit "edge").  A
    parent without an eligible edge yields the dummy 0 and its own time.  csr: a store.DeviceCSR with `.etime`; times:
    int64 [M] on the ids' device; philox: dict(seed, call_base, g0, call_ctr) as for sample_csr.  Returns
    (LongTensor [M*n], LongTensor [M*n]) on the ids' device.  CPU tensors: the same definition in numpy (host mode)."""
    n = int(n)
    assert n >= 1, "SparseTemporalNeighborSampler: n_samples must be set explicitly"
    _temporal_csr(csr, "sample_csr_temporal")
    if strategy not in TEMPORAL_STRATEGIES:
        raise ValueError("sample_csr_temporal: unknown strategy %r (known: uniform, recent)" % (strategy,))
    if inherit not in TEMPORAL_INHERIT:
        raise ValueError("sample_csr_temporal: unknown inherit rule %r (known: seed, edge)" % (inherit,))
    ids = ids.contiguous().view(-1)
    times = times.contiguous().view(-1)
    M = int(ids.shape[0])
    assert times.dtype == torch.int64 and int(times.shape[0]) == M and times.device == ids.device, \
        "sample_csr_temporal: times must be int64 [M] on the ids' device"
    seed, base, g0 = int(philox["seed"]), int(philox.get("call_base", 0)), int(philox.get("g0", 0))
    ctr = philox.get("call_ctr")
    if ids.is_cuda:
        if out is None:
            out = torch.empty(M * n, dtype=torch.int64, device=ids.device)
        if out_time is None:
            out_time = torch.empty(M * n, dtype=torch.int64, device=ids.device)
        for o in (out, out_time):
            assert o.dtype == torch.int64 and o.numel() == M * n and o.is_contiguous()
        nat.check(nat.lib().gsage_sample_csr_temporal(_ptr(csr.rowptr), _ptr(csr.col), _ptr(csr.etime), csr.n_rows,
                                                      _ptr(ids), _ptr(times), M, n, TEMPORAL_STRATEGIES[strategy],
                                                      TEMPORAL_INHERIT[inherit], seed, _ptr(ctr), base, g0, _ptr(out),
                                                      _ptr(out_time), _ptr(csr.err_flag), _stream()),
                  "sample_csr_temporal")
        return out, out_time
    # ---- host mode
    idn, tn = ids.numpy(), times.numpy()
    if idn.size and (idn.min() < 0 or idn.max() >= csr.n_rows):
        raise IndexError("sampler: node id out of range of the adjacency")
    keep = np.repeat(tn, n)
    if M == 0 or csr.nnz == 0:
        return torch.zeros(M * n, dtype=torch.int64), torch.from_numpy(keep)
    rp, col, et = csr.rowptr.numpy(), csr.col.numpy(), csr.etime.numpy()
    beg = rp[idn]
    cnt = _temporal_count_host(rp, et, idn, tn).astype(np.uint64)
    live = cnt > 0
    safe = np.maximum(cnt, np.uint64(1))[:, None]
    slot = np.arange(n, dtype=np.uint64)[None, :]
    if strategy == "recent":
        off = safe - np.uint64(1) - slot % safe
    else:
        call = base + (int(ctr.item()) if ctr is not None else 0)
        w = _philox_words_host(seed, TEMPORAL_TAG, call, g0, M * n).reshape(M, n)
        off = (w * safe) >> np.uint64(32)
    pos = np.minimum(beg[:, None] + off.astype(np.int64), col.shape[0] - 1)
    vals = np.where(live[:, None], col[pos].astype(np.int64), 0).reshape(-1)
    if inherit == "edge":
        keep = np.where(live[:, None], et[pos], tn[:, None]).reshape(-1)
    return torch.from_numpy(vals), torch.from_numpy(np.ascontiguousarray(keep, dtype=np.int64))


def sample_hops_temporal(csr, ids, times, B, fans, philox, strategy="uniform", inherit="seed", out_times=None):
    """Every hop of a temporal frontier (include/gsage.h, gsage_sample_hops_temporal: one launch): ids is the
    concatenated buffer [hop 0 | hop 1 | ... | hop L] (int64, B (1 + n1 + n1 n2 + ...) entries) with hop 0 filled, times
    int64 [B] the seeds' query times on the ids' device; hop k is written as sample_csr_temporal(hop k - 1 and its times,
    fans[k - 1]) under call index call_base + k - 1 and g0 = rank * |hop k|.  out_times (optional): int64 of ids' layout,
    receives every entry's query time, hop 0 included; allocated when None.  philox: dict(seed, call_base, call_ctr,
    optional rank).  Returns (ids, out_times).  CPU tensors: the host definition of the per-hop draw, hop after hop
    (host mode)."""
    _temporal_csr(csr, "sample_hops_temporal")
    if strategy not in TEMPORAL_STRATEGIES:
        raise ValueError("sample_hops_temporal: unknown strategy %r (known: uniform, recent)" % (strategy,))
    if inherit not in TEMPORAL_INHERIT:
        raise ValueError("sample_hops_temporal: unknown inherit rule %r (known: seed, edge)" % (inherit,))
    fans = [int(n) for n in fans]
    assert 1 <= len(fans) <= 5 and all(n >= 1 for n in fans), "sample_hops_temporal: 1..5 hops of n_samples >= 1"
    B = int(B)
    sizes = [B]
    for n in fans:
        sizes.append(sizes[-1] * n)
    assert ids.dtype == torch.int64 and ids.dim() == 1 and ids.is_contiguous() and ids.numel() == sum(sizes)
    times = times.contiguous().view(-1)
    assert times.dtype == torch.int64 and int(times.shape[0]) == B and times.device == ids.device, \
        "sample_hops_temporal: times must be int64 [B] on the ids' device"
    if out_times is None:
        out_times = torch.empty_like(ids)
    assert out_times.dtype == torch.int64 and out_times.numel() == ids.numel() and out_times.is_contiguous() and \
        out_times.device == ids.device, "sample_hops_temporal: out_times must be int64 of ids' layout on its device"
    seed, base, rank = int(philox["seed"]), int(philox.get("call_base", 0)), int(philox.get("rank", 0))
    ctr = philox.get("call_ctr")
    if ids.is_cuda:
        d = nat.HopsDesc()
        d.rowptr, d.col, d.n_rows = csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.n_rows
        d.ids, d.B, d.n_hops = ids.data_ptr(), B, len(fans)
        for k in range(5):
            d.fan[k] = fans[k] if k < len(fans) else 1
        d.max_deg, d.seed, d.call_base, d.rank = 1, seed, base, rank
        d.call_ctr = ctr.data_ptr() if ctr is not None else None
        d.err_flag = csr.err_flag.data_ptr()
        nat.check(nat.lib().gsage_sample_hops_temporal(ctypes.addressof(d), _ptr(csr.etime), _ptr(times), None,
                                                       TEMPORAL_STRATEGIES[strategy], TEMPORAL_INHERIT[inherit],
                                                       _ptr(out_times), _stream()), "sample_hops_temporal")
        return ids, out_times
    off = 0
    out_times[:B] = times
    for k, n in enumerate(fans):
        ph = {"seed": seed, "call_base": base + k, "g0": rank * sizes[k + 1]}
        if ctr is not None:
            ph["call_ctr"] = ctr
        lo, hi = off + sizes[k], off + sizes[k] + sizes[k + 1]
        ids[lo:hi], out_times[lo:hi] = sample_csr_temporal(csr, ids[off:lo], out_times[off:lo], n, ph,
                                                           strategy=strategy, inherit=inherit)
        off += sizes[k]
    return ids, out_times


def temporal_count(csr, ids=None, times=None, t=None):
    """cnt int64 [M] (include/gsage.h, gsage_temporal_count): per row ids[i] -- every row of the graph when ids is
    None -- the number of edges with etime < times[i], or < the one scalar t when times is None.  One launch, the hop
    kernel's cooperative search.  CPU adjacencies: the same counts in numpy (host mode)."""
    _temporal_csr(csr, "temporal_count")
    if (times is None) == (t is None):
        raise ValueError("temporal_count: exactly one of times (a tensor per row) and t (one scalar) must be given")
    dev = csr.device
    if ids is not None:
        ids = ids.contiguous().view(-1)
        assert ids.dtype == torch.int64 and ids.device == dev, "temporal_count: ids must be int64 on the adjacency's device"
    M = int(ids.shape[0]) if ids is not None else csr.n_rows
    if times is not None:
        times = times.contiguous().view(-1)
        assert times.dtype == torch.int64 and int(times.shape[0]) == M and times.device == dev, \
            "temporal_count: times must be int64 [M] on the adjacency's device"
    else:
        t = int(t)
        if not -INT64_MAX - 1 <= t <= INT64_MAX:
            raise ValueError("temporal_count: t = %d is not an int64" % t)
    if dev.type != "cpu":
        cnt = torch.zeros(M, dtype=torch.int64, device=dev)
        nat.check(nat.lib().gsage_temporal_count(_ptr(csr.rowptr), _ptr(csr.etime), csr.n_rows, _ptr(ids), M, _ptr(times),
                                                 t if times is None else 0, _ptr(cnt), _ptr(csr.err_flag), _stream()),
                  "temporal_count")
        return cnt
    # ---- host mode
    rows = ids.numpy() if ids is not None else np.arange(M, dtype=np.int64)
    if rows.size and (rows.min() < 0 or rows.max() >= csr.n_rows):
        raise IndexError("sampler: node id out of range of the adjacency")
    tn = times.numpy() if times is not None else np.full(M, t, dtype=np.int64)
    if M == 0 or csr.nnz == 0:
        return torch.zeros(M, dtype=torch.int64)
    return torch.from_numpy(_temporal_count_host(csr.rowptr.numpy(), csr.etime.numpy(), rows, tn).astype(np.int64))


def temporal_compact(csr, cnt, rowptr):
    """(col int32 [nnz'], etime int64 [nnz']) of the CSR that keeps the first cnt[v] entries of every row of `csr`
    (include/gsage.h, gsage_temporal_compact); rowptr int64 [n_rows + 1]: 0 followed by the running sum of cnt.  One
    launch, a row copy.  CPU adjacencies: the same copy in numpy (host mode)."""
    _temporal_csr(csr, "temporal_compact")
    assert cnt.dtype == torch.int64 and cnt.numel() == csr.n_rows and cnt.is_contiguous() and cnt.device == csr.device
    assert rowptr.dtype == torch.int64 and rowptr.numel() == csr.n_rows + 1 and rowptr.is_contiguous() and \
        rowptr.device == csr.device
    total = int(rowptr[-1]) if csr.n_rows else 0
    col = torch.empty(total, dtype=torch.int32, device=csr.device)
    etime = torch.empty(total, dtype=torch.int64, device=csr.device)
    if csr.device.type != "cpu":
        nat.check(nat.lib().gsage_temporal_compact(_ptr(csr.rowptr), _ptr(csr.col), _ptr(csr.etime), csr.n_rows, _ptr(cnt),
                                                   _ptr(rowptr), _ptr(col), _ptr(etime), total, _stream()),
                  "temporal_compact")
        return col, etime
    if total:
        c = cnt.numpy()
        src = np.repeat(csr.rowptr.numpy()[:-1] - rowptr.numpy()[:-1], c) + np.arange(total, dtype=np.int64)
        col.copy_(csr.col[torch.from_numpy(src)])
        etime.copy_(csr.etime[torch.from_numpy(src)])
    return col, etime


def temporal_snapshot(csr, t):
    """(rowptr, col, etime) of the graph "as of t" (store.DeviceCSR.snapshot): the edges with etime < t, by
    temporal_count, one torch.cumsum and temporal_compact on the adjacency's device."""
    cnt = temporal_count(csr, t=t)
    rowptr = torch.zeros(csr.n_rows + 1, dtype=torch.int64, device=csr.device)
    if csr.n_rows:
        torch.cumsum(cnt, 0, out=rowptr[1:])
    col, etime = temporal_compact(csr, cnt, rowptr)
    return rowptr, col, etime


# =============================================================================================
# Importance neighbourhoods: visit counts of short random walks and their top-T (csrc/gsage_importance.hip)
# =============================================================================================
IMPORTANCE_TAG = 0x49000000                                                           # include/gsage.h
IMPORTANCE_MAX_LANDINGS, IMPORTANCE_MAX_LEN, IMPORTANCE_MAX_TOP = 4096, 16, 64


def importance_check(n_walks, walk_len, top):
    """ValueError for sizes outside the limits of gsage_importance_walks (the library's own sentences)."""
    if n_walks < 1:
        raise ValueError("importance_walks: n_walks must be >= 1")
    if not 1 <= walk_len <= IMPORTANCE_MAX_LEN:
        raise ValueError("importance_walks: walk_len must be in 1..%d" % IMPORTANCE_MAX_LEN)
    if not 1 <= top <= IMPORTANCE_MAX_TOP:
        raise ValueError("importance_walks: top must be in 1..%d" % IMPORTANCE_MAX_TOP)
    if n_walks * walk_len > IMPORTANCE_MAX_LANDINGS:
        raise ValueError("importance_walks: n_walks * walk_len = %d, more than %d landings per source"
                         % (n_walks * walk_len, IMPORTANCE_MAX_LANDINGS))


def _philox4_np(c, k0, k1):
    """Philox4x32-10 over four uint64 arrays of 32-bit counter words -> four such arrays (host mode)"""
    mask, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    c = list(c)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> s32) ^ c[1] ^ np.uint64(k0)) & mask, p1 & mask, ((p0 >> s32) ^ c[3] ^ np.uint64(k1)) & mask, p0 & mask]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


# ---- biased walks (include/gsage.h, "Biased walks"): node2vec's return / in-out parameters, restarts
WALK_BIAS_TAG = 0x42000000                            # | (step << 8) | round: the builder's rounds, a Philox block each
WALK_ROUNDS = 32
WALK_PQ_MIN, WALK_PQ_MAX = 0.125, 8.0


def walk_bias_check(p, q, restart=0.0, who="unsup_batch_biased"):
    """ValueError for p, q or restart outside the limits of the biased entries (the library's own sentences)."""
    p, q, restart = float(p), float(q), float(restart)
    if not WALK_PQ_MIN <= p <= WALK_PQ_MAX:                                          # (False for NaN)
        raise ValueError("%s: p must be in [1/8, 8] (got %g)" % (who, p))
    if not WALK_PQ_MIN <= q <= WALK_PQ_MAX:
        raise ValueError("%s: q must be in [1/8, 8] (got %g)" % (who, q))
    if not 0.0 <= restart < 1.0:
        raise ValueError("%s: restart must be in [0, 1) (got %g)" % (who, restart))
    return p, q, restart


def walk_thresholds(p, q, restart=0.0):
    """-> (theta_return, theta_near, theta_far, theta_restart): the integers the biased kernels compare 32-bit words
    with, from the same double arithmetic as the library's host code."""
    p, q, restart = walk_bias_check(p, q, restart, "walk_thresholds")
    a = (1.0 / p, 1.0, 1.0 / q)
    a_max = max(a)
    th = tuple(1 << 32 if x == a_max else int(math.floor((x / a_max) * 4294967296.0)) for x in a)
    return th + (int(math.floor(restart * 4294967296.0)),)


def _importance_host(csr, idn, R, L, T, seed, bias=None):
    """gsage_importance_walks in numpy: every (source, walk) pair is one element, the steps are the loop.
    bias: None, or walk_thresholds(p, q, restart) -- gsage_importance_walks_biased: up to 32 rounds per step over the
    elements still without an accepted proposal; "x is stored in row t" is a search in the sorted (row, column) keys.
    -> (col int32 [M, T], w fp32 [M, T], deg int32 [M], err)"""
    rp, col, n_rows = csr.rowptr.numpy(), csr.col.numpy(), csr.n_rows
    cdf = csr.edge_cdf.numpy().view(np.uint64) if csr.edge_cdf is not None else None
    M = int(idn.shape[0])
    out_col, out_w = np.zeros((M, T), dtype=np.int32), np.zeros((M, T), dtype=np.float32)
    out_deg = np.zeros(M, dtype=np.int32)
    in_range = (idn >= 0) & (idn < n_rows)
    err = not bool(in_range.all())
    if col.shape[0] == 0:
        return out_col, out_w, out_deg, err
    k0, k1 = seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ IMPORTANCE_TAG
    s32 = np.uint64(32)
    th_ret = th_near = th_far = 1 << 32
    th_restart = 0
    if bias is not None:
        th_ret, th_near, th_far, th_restart = bias
    second = min(th_ret, th_near, th_far) < (1 << 32)         # thresholds that can reject
    if second:
        row_of = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(rp[:n_rows + 1]))
        edge_keys = np.unique((row_of << 32) | (col.astype(np.int64) & 0xFFFFFFFF))
    per = max(1, (1 << 21) // R)                          # sources per piece: the working arrays stay at ~2 M elements
    for o in range(0, M, per):
        v = idn[o:o + per]
        m = int(v.shape[0])
        src, vv = np.repeat(np.arange(m, dtype=np.int64), R), np.repeat(v, R)
        r = np.tile(np.arange(R, dtype=np.uint64), m)
        alive = np.repeat(in_range[o:o + per], R)
        u = np.where(alive, vv, 0)
        prev = np.full(m * R, -1, dtype=np.int64)
        c0, zero = vv.astype(np.uint64) & np.uint64(0xFFFFFFFF), np.zeros(m * R, dtype=np.uint64)
        land_src, land_id = [], []
        for s in range(L):
            if not s & 1:
                w = _philox4_np([c0, r, np.full(m * R, s >> 1, dtype=np.uint64), zero], k0, k1)
            r64 = (w[2] << s32) | w[3] if s & 1 else (w[0] << s32) | w[1]
            moving = alive
            nb0 = None
            if second or (th_restart and s >= 1):
                nb0 = _philox4_np([c0, r, np.full(m * R, s, dtype=np.uint64), zero + np.uint64(1)], k0, k1)
            if th_restart and s >= 1:                     # back on the source: nothing counted, the step is consumed
                again = moving & (nb0[3] < np.uint64(th_restart))
                u, prev, moving = np.where(again, vv, u), np.where(again, -1, prev), moving & ~again
            beg, end = rp[u], rp[u + 1]
            if cdf is None:
                go = moving & (end > beg)
                Tu = None
            else:
                Tu = np.where(end > beg, cdf[np.maximum(end, 1) - 1], np.uint64(0)).astype(np.uint64)
                go = moving & (Tu > 0)

            def propose(idx, rr):
                """the first-order step of elements idx (all of them in go) under the draws rr -> edge index"""
                if cdf is None:
                    return beg[idx] + _mulhi64(rr, (end[idx] - beg[idx]).astype(np.uint64)).astype(np.int64)
                x = _mulhi64(rr, Tu[idx])
                lo, hi = beg[idx].copy(), end[idx] - 1                             # cdf[end - 1] = T_u > x
                while True:
                    act = lo < hi
                    if not act.any():
                        break
                    mid = (lo + hi) >> 1
                    gt = cdf[mid] > x
                    hi = np.where(act & gt, mid, hi)
                    lo = np.where(act & ~gt, mid + 1, lo)
                return lo

            x = np.zeros(m * R, dtype=np.int64)
            pending = go.copy()
            for k in range(WALK_ROUNDS if second else 1):
                idx = np.flatnonzero(pending)
                if idx.size == 0:
                    break
                if k == 0:
                    rr, acc = r64[idx], (nb0[2][idx] if second else None)
                else:
                    nb = _philox4_np([c0[idx], r[idx], np.full(idx.size, s, dtype=np.uint64),
                                      np.full(idx.size, 1 + k, dtype=np.uint64)], k0, k1)
                    rr, acc = (nb[0] << s32) | nb[1], nb[2]
                nx = col[propose(idx, rr)].astype(np.int64)
                inside = (nx >= 0) & (nx < n_rows)
                err = err or not bool(inside.all())
                x[idx] = nx
                go[idx[~inside]] = False                  # a stored id outside the graph: the walk ends, not counted
                done = ~inside
                if second:
                    t = prev[idx]
                    key = (np.maximum(t, 0) << 32) | np.where(inside, nx, 0)
                    at = np.minimum(np.searchsorted(edge_keys, key), edge_keys.shape[0] - 1)
                    th = np.where(nx == t, th_ret, np.where(edge_keys[at] == key, th_near, th_far)).astype(np.uint64)
                    done = done | (t < 0) | (acc < th)
                else:
                    done = np.ones(idx.size, dtype=bool)
                pending[idx[done]] = False                # (still pending after the last round: that round's proposal)
            alive = np.where(moving, go, alive)
            prev, u = np.where(go, u, prev), np.where(go, x, u)
            counted = go & (u != vv)
            land_src.append(src[counted])
            land_id.append(u[counted])
        uniq, count = np.unique((np.concatenate(land_src) << 32) | np.concatenate(land_id), return_counts=True)
        us, ui = uniq >> 32, uniq & 0xFFFFFFFF
        order = np.lexsort((ui, -count, us))              # by source, then count descending, then id ascending
        us, ui, count = us[order], ui[order], count[order]
        pos = np.arange(us.shape[0]) - np.searchsorted(us, np.arange(m))[us]
        keep = pos < T
        out_col[o + us[keep], pos[keep]] = ui[keep]
        out_w[o + us[keep], pos[keep]] = count[keep]
        out_deg[o:o + m] = np.minimum(np.bincount(us, minlength=m), T)
    return out_col, out_w, out_deg, err


def importance_walks(csr, ids, n_walks, walk_len, top, seed, p=1.0, q=1.0, restart=0.0, _biased=None):
    """Importance neighbourhoods (include/gsage.h, gsage_importance_walks): from every source in ids (LongTensor [M]
    on csr.device), n_walks random walks of walk_len steps -- weighted steps exactly when csr.edge_cdf is not None --
    and the `top` most-visited nodes, visit count descending then id ascending.
    p, q (in [1/8, 8]) and restart (in [0, 1)): node2vec's return and in-out parameters and a restart probability
    (include/gsage.h, "Biased walks", gsage_importance_walks_biased); the neutral values 1, 1, 0 call the entry this
    function always called (_biased=True: the biased entry all the same -- the same bits).
    -> (col int32 [M, top], w fp32 [M, top] = the counts, deg int32 [M]); entries at and beyond deg are 0.
    An id outside the graph (a source, or a stored neighbour a walk reaches) raises csr.err_flag: csr.check().
    CPU tensors: the same definition in numpy (host mode), the same bits."""
    n_walks, walk_len, top, seed = int(n_walks), int(walk_len), int(top), int(seed) & 0xFFFFFFFFFFFFFFFF
    p, q, restart = walk_bias_check(p, q, restart, "importance_walks_biased")
    biased = (p, q, restart) != (1.0, 1.0, 0.0) if _biased is None else bool(_biased)
    importance_check(n_walks, walk_len, top)
    ids = ids.contiguous().view(-1)
    assert ids.dtype == torch.int64 and ids.device == csr.rowptr.device
    M = int(ids.shape[0])
    if ids.is_cuda:
        col = torch.empty(M, top, dtype=torch.int32, device=ids.device)
        w = torch.empty(M, top, dtype=torch.float32, device=ids.device)
        deg = torch.empty(M, dtype=torch.int32, device=ids.device)
        if biased:
            nat.check(nat.lib().gsage_importance_walks_biased(
                _ptr(csr.rowptr), _ptr(csr.col), _ptr(csr.edge_cdf), csr.n_rows, _ptr(ids), M, n_walks, walk_len, top,
                seed, p, q, restart, _ptr(col), _ptr(w), _ptr(deg), _ptr(csr.err_flag), _stream()),
                "importance_walks_biased")
            return col, w, deg
        nat.check(nat.lib().gsage_importance_walks(_ptr(csr.rowptr), _ptr(csr.col), _ptr(csr.edge_cdf), csr.n_rows,
                                                   _ptr(ids), M, n_walks, walk_len, top, seed, _ptr(col), _ptr(w),
                                                   _ptr(deg), _ptr(csr.err_flag), _stream()), "importance_walks")
        return col, w, deg
    col, w, deg, err = _importance_host(csr, ids.numpy(), n_walks, walk_len, top, seed,
                                        walk_thresholds(p, q, restart) if biased else None)
    if err:
        csr.err_flag.fill_(1)
    return torch.from_numpy(col), torch.from_numpy(w), torch.from_numpy(deg)


def importance_compact(col, w, deg):
    """The padded rows of importance_walks packed into a CSR's arrays (gsage_importance_compact; the row offsets are a
    torch.cumsum: set-up, once per graph).  -> (col int32 [nnz], w fp32 [nnz]), nnz = deg.sum()."""
    M, top = int(col.shape[0]), int(col.shape[1])
    if not col.is_cuda:
        keep = torch.arange(top)[None, :] < deg[:, None]
        return col[keep], w[keep]
    ends = torch.cumsum(deg, 0, dtype=torch.int64)
    nnz = int(ends[-1]) if M else 0
    col_new = torch.empty(nnz, dtype=torch.int32, device=col.device)
    w_new = torch.empty(nnz, dtype=torch.float32, device=col.device)
    if nnz:
        begs = ends - deg
        nat.check(nat.lib().gsage_importance_compact(_ptr(col), _ptr(w), _ptr(deg), _ptr(begs), M, top, _ptr(col_new),
                                                     _ptr(w_new), _stream()), "importance_compact")
    return col_new, w_new


# =============================================================================================
# Unsupervised batches: random-walk positives + degree^0.75 negatives (csrc/gsage_unsup.hip)
# =============================================================================================
UNSUP_TAG_LEN, UNSUP_TAG_STEP, UNSUP_TAG_NEG = 0x4C000000, 0x53000000, 0x4E000000     # include/gsage.h
UNSUP_TAG_WSTEP = 0x5A000000                                                          # weighted steps, two to a block


def _philox4(ctr, key):
    """Philox4x32-10 on Python integers: four counter words, two key words -> four words (host mode)."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    m = 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & m, p1 & m, ((p0 >> 32) ^ c3 ^ k1) & m, p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & m, (k1 + 0xBB67AE85) & m
    return c0, c1, c2, c3


def neg_cdf(csr, weighted=False):
    """The negatives' table of gsage_unsup_batch for `csr`: float64 inclusive running sum of degree^0.75, on the
    adjacency's device (set-up, once per adjacency).  Its last element is read to the host here, once.
    weighted=True (the table of gsage_unsup_batch_weighted; csr carries an edge_cdf): a row without a drawable edge
    (T_v == 0) behaves everywhere as a row of degree 0, so it gets weight 0; every other row keeps degree^0.75 of its
    stored degree."""
    deg = (csr.rowptr[1:] - csr.rowptr[:-1]).to(torch.float64)
    if weighted:
        if csr.edge_cdf is None:
            raise ValueError("neg_cdf: weighted=True needs an adjacency with edge weights (DeviceCSR.with_weights)")
        if csr.nnz:
            last = (csr.rowptr[1:] - 1).clamp(min=0)           # (an empty row reads some entry: its degree is 0 anyway)
            deg = torch.where(csr.edge_cdf[last] != 0, deg, torch.zeros_like(deg))
    cdf = torch.cumsum(deg.clamp(min=0).pow(0.75), 0).contiguous()
    cdf._gsage_total = float(cdf[-1].item())
    return cdf


def unsup_batch(csr, seeds, walk_len, Q, cdf, philox, weighted=False, p=1.0, q=1.0, _biased=None):
    """The id batch of one unsupervised step (include/gsage.h, gsage_unsup_batch): -> (ids int64 [2B + Q] =
    [seeds | random-walk positives | negatives], pair_w fp32 [B]: 0 where a walk ended on its own seed).
    cdf: neg_cdf(csr) (any float64 inclusive running sum of row weights will do); philox: dict(seed, call_base,
    g0, call_ctr) as for sample_csr.  weighted=True: every step is drawn in proportion to the edge quanta of
    csr.edge_cdf (gsage_unsup_batch_weighted; cdf: neg_cdf(csr, weighted=True)).
    p, q (in [1/8, 8]): node2vec's return and in-out parameters -- every step after a walk's first is a second-order
    step (include/gsage.h, "Biased walks", gsage_unsup_batch_biased); p = q = 1 calls the entries this function
    always called (_biased=True: the biased entry all the same -- the same bits).
    CPU tensors: the same definition in numpy / Python integers (host mode)."""
    if weighted and csr.edge_cdf is None:
        raise ValueError("unsup_batch: weighted=True needs an adjacency with edge weights (DeviceCSR.with_weights)")
    p, q, _ = walk_bias_check(p, q, 0.0, "unsup_batch_biased")
    biased = (p, q) != (1.0, 1.0) if _biased is None else bool(_biased)
    seeds = seeds.contiguous().view(-1)
    B, Q, walk_len = int(seeds.shape[0]), int(Q), int(walk_len)
    total = getattr(cdf, "_gsage_total", None)
    if total is None:
        total = float(cdf[-1].item())
    seed, base, g0 = int(philox["seed"]), int(philox.get("call_base", 0)), int(philox.get("g0", 0))
    ctr = philox.get("call_ctr")
    if seeds.is_cuda:
        assert cdf.dtype == torch.float64 and cdf.is_cuda and cdf.is_contiguous() and cdf.numel() == csr.n_rows
        ids = torch.empty(2 * B + Q, dtype=torch.int64, device=seeds.device)
        pair_w = torch.empty(B, dtype=torch.float32, device=seeds.device)
        if biased:
            nat.check(nat.lib().gsage_unsup_batch_biased(
                _ptr(csr.rowptr), _ptr(csr.col), _ptr(csr.edge_cdf) if weighted else None, csr.n_rows, _ptr(seeds), B,
                walk_len, Q, _ptr(cdf), total, seed, _ptr(ctr), base, g0, p, q, _ptr(ids), _ptr(pair_w),
                _ptr(csr.err_flag), _stream()), "unsup_batch_biased")
            return ids, pair_w
        if weighted:
            nat.check(nat.lib().gsage_unsup_batch_weighted(
                _ptr(csr.rowptr), _ptr(csr.col), _ptr(csr.edge_cdf), csr.n_rows, _ptr(seeds), B, walk_len, Q, _ptr(cdf),
                total, seed, _ptr(ctr), base, g0, _ptr(ids), _ptr(pair_w), _ptr(csr.err_flag), _stream()),
                "unsup_batch_weighted")
            return ids, pair_w
        nat.check(nat.lib().gsage_unsup_batch(_ptr(csr.rowptr), _ptr(csr.col), csr.n_rows, _ptr(seeds), B, walk_len, Q,
                                              _ptr(cdf), total, seed, _ptr(ctr), base, g0, _ptr(ids), _ptr(pair_w),
                                              _ptr(csr.err_flag), _stream()), "unsup_batch")
        return ids, pair_w
    # ---- host mode
    if not (B > 0 and Q > 0 and 1 <= walk_len <= 16):
        raise ValueError("unsup_batch: needs B > 0, Q > 0 and 1 <= walk_len <= 16")
    if not (total > 0.0 and total < float("inf")):
        raise ValueError("unsup_batch: the negatives' weights sum to %g" % total)
    call = (base + (int(ctr.item()) if ctr is not None else 0)) & 0xFFFFFFFFFFFFFFFF
    clo, chi = call & 0xFFFFFFFF, call >> 32
    klo, khi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    rp, col, sd, n_rows = csr.rowptr.numpy(), csr.col.numpy(), seeds.numpy(), csr.n_rows
    ecdf = csr.edge_cdf.numpy().view(np.uint64) if weighted else None
    if sd.min() < 0 or sd.max() >= n_rows:
        raise IndexError("unsup_batch: node id out of range of the adjacency")
    th_ret, th_near, th_far, _ = walk_thresholds(p, q) if biased else (1 << 32, 1 << 32, 1 << 32, 0)
    rejecting = min(th_ret, th_near, th_far) < (1 << 32)
    ids = np.zeros(2 * B + Q, dtype=np.int64)
    pair_w = np.zeros(B, dtype=np.float32)
    for i in range(B):
        g = (g0 + i) & 0xFFFFFFFFFFFFFFFF
        c = (g & 0xFFFFFFFF, g >> 32, clo, chi)
        t = 1 + ((_philox4(c, (klo, khi ^ UNSUP_TAG_LEN))[0] * walk_len) >> 32)
        v, prev, r = int(sd[i]), -1, None
        for j in range(t):
            beg = int(rp[v])
            deg = int(rp[v + 1]) - beg
            if deg <= 0:
                break
            if weighted:
                T = int(ecdf[beg + deg - 1])
                if T == 0:
                    break
                if j & 1 == 0:
                    r = _philox4(c, (klo, khi ^ (UNSUP_TAG_WSTEP | (j >> 1))))
            elif j & 3 == 0:
                r = _philox4(c, (klo, khi ^ (UNSUP_TAG_STEP | (j >> 2))))
            second = rejecting and j > 0                       # a second-order step: up to 32 rounds of rejection
            for k in range(WALK_ROUNDS if second else 1):
                nb = _philox4(c, (klo, khi ^ (WALK_BIAS_TAG | (j << 8) | k))) if second else None
                if weighted:
                    r64 = (r[2 * (j & 1)] << 32) | r[2 * (j & 1) + 1] if k == 0 else (nb[0] << 32) | nb[1]
                    x = (r64 * T) >> 64
                    x = int(col[beg + int(np.searchsorted(ecdf[beg:beg + deg], np.uint64(x), side="right"))])
                else:
                    word = r[j & 3] if k == 0 else nb[0]
                    x = int(col[beg + ((word * deg) >> 32 if deg <= 0xFFFFFFFF else word)])
                if x < 0 or x >= n_rows:
                    raise IndexError("unsup_batch: node id out of range of the adjacency")
                if not second:
                    break
                if x == prev:
                    th = th_ret
                else:
                    th = th_near if bool((col[int(rp[prev]):int(rp[prev + 1])] == x).any()) else th_far
                if nb[2] < th:
                    break
            prev, v = v, x
        ids[i], ids[B + i], pair_w[i] = sd[i], v, 0.0 if v == sd[i] else 1.0
    cn = cdf.numpy()
    for q_ in range(Q):
        r = _philox4((q_ & 0xFFFFFFFF, q_ >> 32, clo, chi), (klo, khi ^ UNSUP_TAG_NEG))
        x = np.float64((r[0] << 21) | (r[1] >> 11)) * np.float64(2.0 ** -53) * np.float64(total)
        ids[2 * B + q_] = min(int(np.searchsorted(cn, x, side="right")), n_rows - 1)
    return torch.from_numpy(ids), torch.from_numpy(pair_w)


UNSUP_TAG_TSTEP = 0x56000000                                                          # temporal steps, four to a block


def unsup_batch_temporal(csr, seeds, times, walk_len, Q, cdf, philox, inherit="seed", n_valid=None):
    """The id batch of one unsupervised step over a temporal adjacency (include/gsage.h, "Temporal walks",
    gsage_unsup_batch_temporal): -> (ids int64 [2B + Q] = [seeds | positives | negatives], pair_w fp32 [B], times int64
    [2B + Q]).  Every step of a seed's walk is drawn uniformly among the edges of the current row that happened strictly
    before the walk's time: the seed's query time times[i] (inherit "seed"), or the time of the edge just walked
    (inherit "edge": edge times strictly decrease along the walk).  A seed without such an edge is its own positive and
    gets pair_w 0.  Seeds and positives are to be embedded as of times[i]; negative q as of times[q % b], b =
    clamp(n_valid, 1, B) -- n_valid: an int32 device word (a tensor of one element) or an int, None: b = B.
    csr: a store.DeviceCSR with `.etime`; cdf: neg_cdf(csr); philox: dict(seed, call_base, g0, call_ctr) as for
    unsup_batch.  CPU tensors: the same definition in numpy / Python integers (host mode)."""
    _temporal_csr(csr, "unsup_batch_temporal")
    if inherit not in TEMPORAL_INHERIT:
        raise ValueError("unsup_batch_temporal: unknown inherit rule %r (known: seed, edge)" % (inherit,))
    seeds = seeds.contiguous().view(-1)
    times = times.contiguous().view(-1)
    B, Q, walk_len = int(seeds.shape[0]), int(Q), int(walk_len)
    assert times.dtype == torch.int64 and int(times.shape[0]) == B and times.device == seeds.device, \
        "unsup_batch_temporal: times must be int64 [B] on the seeds' device"
    total = getattr(cdf, "_gsage_total", None)
    if total is None:
        total = float(cdf[-1].item())
    seed, base, g0 = int(philox["seed"]), int(philox.get("call_base", 0)), int(philox.get("g0", 0))
    ctr = philox.get("call_ctr")
    if seeds.is_cuda:
        assert cdf.dtype == torch.float64 and cdf.is_cuda and cdf.is_contiguous() and cdf.numel() == csr.n_rows
        if n_valid is not None and not torch.is_tensor(n_valid):
            n_valid = torch.full((1,), max(min(int(n_valid), 2 ** 31 - 1), -2 ** 31), dtype=torch.int32,
                                 device=seeds.device)
        assert n_valid is None or (n_valid.dtype == torch.int32 and n_valid.is_cuda and n_valid.numel() == 1)
        ids = torch.empty(2 * B + Q, dtype=torch.int64, device=seeds.device)
        out_times = torch.empty(2 * B + Q, dtype=torch.int64, device=seeds.device)
        pair_w = torch.empty(B, dtype=torch.float32, device=seeds.device)
        nat.check(nat.lib().gsage_unsup_batch_temporal(
            _ptr(csr.rowptr), _ptr(csr.col), _ptr(csr.etime), csr.n_rows, _ptr(seeds), _ptr(times), B, walk_len, Q,
            _ptr(cdf), total, seed, _ptr(ctr), base, g0, TEMPORAL_INHERIT[inherit], _ptr(n_valid), _ptr(ids),
            _ptr(out_times), _ptr(pair_w), _ptr(csr.err_flag), _stream()), "unsup_batch_temporal")
        return ids, pair_w, out_times
    # ---- host mode
    if not (B > 0 and Q > 0 and 1 <= walk_len <= 16):
        raise ValueError("unsup_batch_temporal: needs B > 0, Q > 0 and 1 <= walk_len <= 16")
    if not (total > 0.0 and total < float("inf")):
        raise ValueError("unsup_batch_temporal: the negatives' weights sum to %g" % total)
    call = (base + (int(ctr.item()) if ctr is not None else 0)) & 0xFFFFFFFFFFFFFFFF
    clo, chi = call & 0xFFFFFFFF, call >> 32
    klo, khi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    rp, col, et, n_rows = csr.rowptr.numpy(), csr.col.numpy(), csr.etime.numpy(), csr.n_rows
    sd, tn = seeds.numpy(), times.numpy()
    if sd.min() < 0 or sd.max() >= n_rows:
        raise IndexError("unsup_batch_temporal: node id out of range of the adjacency")
    ids = np.zeros(2 * B + Q, dtype=np.int64)
    out_times = np.zeros(2 * B + Q, dtype=np.int64)
    pair_w = np.zeros(B, dtype=np.float32)
    for i in range(B):
        g = (g0 + i) & 0xFFFFFFFFFFFFFFFF
        c = (g & 0xFFFFFFFF, g >> 32, clo, chi)
        t = 1 + ((_philox4(c, (klo, khi ^ UNSUP_TAG_LEN))[0] * walk_len) >> 32)
        v, tau, r = int(sd[i]), int(tn[i]), None
        for j in range(t):
            beg, end = int(rp[v]), int(rp[v + 1])
            cnt = int(np.searchsorted(et[beg:end], tau, side="left")) if end - beg <= 0xFFFFFFFF else 0
            if cnt == 0:
                break
            if j & 3 == 0:
                r = _philox4(c, (klo, khi ^ (UNSUP_TAG_TSTEP | (j >> 2))))
            e = beg + ((r[j & 3] * cnt) >> 32)
            v = int(col[e])
            if v < 0 or v >= n_rows:
                raise IndexError("unsup_batch_temporal: node id out of range of the adjacency")
            if inherit == "edge":
                tau = int(et[e])
        ids[i], ids[B + i], pair_w[i] = sd[i], v, 0.0 if v == sd[i] else 1.0
        out_times[i] = out_times[B + i] = tn[i]
    cn = cdf.numpy()
    for q_ in range(Q):
        r = _philox4((q_ & 0xFFFFFFFF, q_ >> 32, clo, chi), (klo, khi ^ UNSUP_TAG_NEG))
        x = np.float64((r[0] << 21) | (r[1] >> 11)) * np.float64(2.0 ** -53) * np.float64(total)
        ids[2 * B + q_] = min(int(np.searchsorted(cn, x, side="right")), n_rows - 1)
    b = B if n_valid is None else min(max(int(n_valid), 1), B)
    out_times[2 * B:] = tn[np.arange(Q) % b]
    return torch.from_numpy(ids), torch.from_numpy(pair_w), torch.from_numpy(out_times)


# =============================================================================================
# K2 / K6  gather + mean, segment mean, scatter-add
# =============================================================================================
def _gather_mean_raw(table, D, ids, M, n, out_dtype, out_ld=None, out=None):
    """out[i] = mean_j table[ids[i*n+j]] (ids None: rows i*n+j).  table: [R, ld] tensor.
    `out`: optional preallocated [M, out_ld] destination (a row slice of a larger buffer)."""
    if out_ld is None:
        out_ld = D
    if table.is_cuda:
        if out is None:
            out = (torch.zeros if out_ld != D else torch.empty)(M, out_ld, dtype=out_dtype,
                                                                device=table.device)
        else:
            assert out.dtype == out_dtype and out.stride(0) == out_ld and out.shape[0] == M
        nat.check(nat.lib().gsage_gather_mean(_ptr(table), _code(table.dtype), table.stride(0),
                                              _ptr(ids), M, n, D, _ptr(out), _code(out_dtype),
                                              out_ld, _stream()), "gather_mean")
        return out
    rows = table[ids.view(-1), :D] if ids is not None else table[:M * n, :D]
    res = rows.float().view(M, n, D).mean(dim=1) if n > 1 else rows.float().view(M, D)
    out = torch.zeros(M, out_ld, dtype=out_dtype)
    out[:, :D] = res.to(out_dtype)
    return out


def quantize_fp8(table, D, ld_q):
    """[R, ld] fp32 / bf16 table (columns [0, D) live) -> (table_q [R, ld_q] float8_e4m3fn, scale [ld_q] fp32): the
    FP8 feature-table format of include/gsage.h (gsage_quantize_fp8; CPU tensors: store.quantize_fp8_host)."""
    R = int(table.shape[0])
    assert table.dtype in (torch.float32, torch.bfloat16) and table.stride(1) == 1 and ld_q % 16 == 0 and ld_q >= D
    if table.is_cuda:
        q = torch.empty(R, ld_q, dtype=FP8, device=table.device)
        scale = torch.empty(ld_q, dtype=torch.float32, device=table.device)
        nat.check(nat.lib().gsage_quantize_fp8(_ptr(table), _code(table.dtype), table.stride(0), R, D, _ptr(q), ld_q,
                                               _ptr(scale), _stream()), "quantize_fp8")
        return q, scale
    q = torch.zeros(R, ld_q, dtype=torch.uint8).view(FP8)
    scale = torch.ones(ld_q, dtype=torch.float32)
    q[:, :D], scale[:D] = quantize_fp8_host(table[:, :D])
    return q, scale


def _gather_mean_fp8_raw(table_q, scale, D, ids, M, n, out_dtype, out_ld=None, out=None):
    """_gather_mean_raw on an FP8 table: out[i] = (sum_j e4m3(table_q[ids[i*n+j]])) * scale / n, the sum in fp32
    in neighbour order -- bit for bit what _gather_mean_raw gives on a bf16 table of the decoded values."""
    assert table_q.dtype == FP8 and scale is not None and scale.dtype == torch.float32
    if out_ld is None:
        out_ld = D
    if table_q.is_cuda:
        if out is None:
            out = (torch.zeros if out_ld != D else torch.empty)(M, out_ld, dtype=out_dtype, device=table_q.device)
        else:
            assert out.dtype == out_dtype and out.stride(0) == out_ld and out.shape[0] == M
        nat.check(nat.lib().gsage_gather_mean_fp8(_ptr(table_q), table_q.stride(0), _ptr(scale), _ptr(ids), M, n, D,
                                                  _ptr(out), _code(out_dtype), out_ld, _stream()), "gather_mean_fp8")
        return out
    rows = table_q[ids.view(-1), :D] if ids is not None else table_q[:M * n, :D]
    # the lines of _gather_mean_raw's host mode on the unscaled e4m3 values, then the scales: a power of two commutes
    # with every rounding of the mean, so this IS that host mode on the decoded table, bit for bit
    res = (rows.float().view(M, n, D).mean(dim=1) if n > 1 else rows.float().view(M, D)) * scale[:D]
    out = torch.zeros(M, out_ld, dtype=out_dtype)
    out[:, :D] = res.to(out_dtype)
    return out


def _store_gather(store, D, ids, M, n, out_dtype, out_ld=None):
    if store.is_fp8:
        return _gather_mean_fp8_raw(store.data, store.scale, D, ids, M, n, out_dtype, out_ld)
    return _gather_mean_raw(store.data, D, ids, M, n, out_dtype, out_ld)


def decoded_rows(ref, compute_dtype=None):
    """A RowRef into an FP8 store -> its rows decoded into the compute type by the FP8 row gather (a [:, :D] view
    of zero-padded rows); anything else is returned as it is.  K5 and the aggregator kernels gather bf16 / fp32
    table rows through a row list (`a_rows`); they never see FP8 bytes."""
    if not (isinstance(ref, RowRef) and ref.store.is_fp8):
        return ref
    st = ref.store
    cdt = torch_dtype(compute_dtype)
    ld = _round_up(st.dim, 64 if cdt == torch.bfloat16 else 32)
    buf = _gather_mean_fp8_raw(st.data, st.scale, st.dim, ref.ids, int(ref.ids.shape[0]), 1, cdt, ld)
    return mark_zero_padded(buf[:, :st.dim])


class _GatherTrainable(torch.autograd.Function):
    """Row gather from a TRAINABLE fp32 table with the reference's dense gradient
    (nn.Embedding, nn_modules.py:134,146-149): backward = K6 scatter-add into a zeroed table."""

    @staticmethod
    def forward(ctx, table, ids):
        ctx.save_for_backward(ids)
        ctx.tshape = table.shape
        ctx.table = table if (table.is_leaf and table.requires_grad) else None
        return _gather_mean_raw(table.detach(), table.shape[1], ids, int(ids.shape[0]), 1,
                                torch.float32)

    @staticmethod
    def backward(ctx, g):
        (ids,) = ctx.saved_tensors
        g = g.contiguous().float()
        t = ctx.table
        if (g.is_cuda and t is not None and t.grad is not None and t.grad.dtype == torch.float32 and
                t.grad.shape == t.shape and t.grad.is_contiguous() and not torch.is_grad_enabled()):
            # The parameter already has a (zeroed, persistent) gradient buffer -- optim.FlatAdam's view:
            # scatter-add straight into it.  The stock route materialises a dense zero table per use of
            # the embedding and lets autograd add it to .grad: 4 extra passes over the table per use
            # (Pokec: 3 uses x 418 MB).  Same result: the adds commute.
            nat.check(nat.lib().gsage_scatter_add_rows(_ptr(g), g.stride(0), _ptr(ids), int(ids.shape[0]), 1,
                                                       g.shape[1], 1.0, _ptr(t.grad), t.grad.stride(0),
                                                       _stream()), "scatter_add_rows")
            return None, None
        grad = torch.zeros(ctx.tshape, dtype=torch.float32, device=g.device)
        if g.is_cuda:
            nat.check(nat.lib().gsage_scatter_add_rows(_ptr(g), g.stride(0), _ptr(ids),
                                                       int(ids.shape[0]), 1, g.shape[1], 1.0,
                                                       _ptr(grad), grad.stride(0), _stream()),
                      "scatter_add_rows")
        else:
            grad.index_add_(0, ids, g)
        return grad, None


def embedding_rows(table, ids):
    """table[ids] for a trainable parameter (dense-grad semantics of the reference)."""
    return _GatherTrainable.apply(table, ids.contiguous().view(-1))


def gather_rows(store, ids, out_dtype=torch.float32):
    """feats[ids] (models.py:76,80) materialised: [M, D] tensor of `out_dtype`."""
    ids = ids.contiguous().view(-1)
    return _store_gather(store, store.dim, ids, int(ids.shape[0]), 1, out_dtype)


def gather_mean(store, ids, M, n, out_dtype=torch.float32, out_ld=None):
    """feats[ids].view(M, n, D).mean(1) without materialising feats[ids]
    (models.py:80 + nn_modules.py:197-198)."""
    ids = ids.contiguous().view(-1)
    assert ids.shape[0] == M * n
    if out_ld is not None and out_ld == store.ld:
        # the table's pad columns are zero, so averaging them writes the output's pad columns
        return _store_gather(store, store.ld, ids, M, n, out_dtype, out_ld)
    return _store_gather(store, store.dim, ids, M, n, out_dtype, out_ld)


class _SegmentMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, neibs, M, out_dtype):
        n = neibs.shape[0] // M
        ctx.dims = (M, n, neibs.shape[1], neibs.dtype)
        src = neibs.detach()
        if not src.is_contiguous():
            src = src.contiguous()
        return _gather_mean_raw(src, src.shape[1], None, M, n, out_dtype)

    @staticmethod
    def backward(ctx, g):
        M, n, D, dt = ctx.dims
        g = g.contiguous().float()
        if g.is_cuda:
            out = torch.empty(M * n, D, dtype=torch.float32, device=g.device)
            nat.check(nat.lib().gsage_segment_mean_bwd(_ptr(g), g.stride(0), M, n, D, _ptr(out), D,
                                                       _stream()), "segment_mean_bwd")
        else:
            out = (g / n).repeat_interleave(n, dim=0)
        return out.to(dt), None, None


def segment_mean(neibs, M, out_dtype=torch.float32):
    """neibs.view(M, -1, D).mean(dim=1) (nn_modules.py:197-198) for an in-order tensor."""
    assert neibs.shape[0] % M == 0
    return _SegmentMean.apply(neibs, M, out_dtype)


# =============================================================================================
# K5  projection GEMM
# =============================================================================================
def _linear_launch(A, lda, a_rows, a_rows_g0, W, ldw, bias, C, ldc, M, N, K, act, groups,
                   a_gs, w_gs, c_gs, dtype_code, c_code):
    nat.check(nat.lib().gsage_linear_nt(A, dtype_code, lda, a_rows, a_rows_g0, W, ldw, bias, C,
                                        c_code, ldc, M, N, K, act, groups, a_gs, w_gs, c_gs,
                                        _stream()), "linear_nt")


def pack_weight(W, K=None, out=None):
    """[groups, N, ld] (or [N, ld]) fp32 / bf16 weights -> the MFMA-fragment-ordered bf16 operand of
    gsage_linear_nt_packed (include/gsage.h).  K: logical inner size (default: the last dimension)."""
    W3 = W if W.dim() == 3 else W.unsqueeze(0)
    assert W3.stride(2) == 1 and W3.is_cuda
    groups, N, _ = W3.shape
    K = int(W3.shape[2] if K is None else K)
    n = nat.lib().gsage_packed_weight_elems(N, K, groups)
    if out is None:
        out = torch.empty(n, dtype=torch.bfloat16, device=W.device)
    assert out.numel() >= n and out.dtype == torch.bfloat16
    code = nat.BF16 if W3.dtype == torch.bfloat16 else nat.F32
    assert W3.dtype in (torch.bfloat16, torch.float32)
    nat.check(nat.lib().gsage_pack_weight(W3.data_ptr(), code, W3.stride(1), W3.stride(0) if groups > 1 else 0,
                                          N, K, groups, out.data_ptr(), _stream()), "pack_weight")
    return out


def _linear_packed_launch(A, lda, a_rows, a_rows_g0, Wp, bias, C, ldc, M, N, K, act, groups, a_gs, c_gs, c_code):
    nat.check(nat.lib().gsage_linear_nt_packed(A, lda, a_rows, a_rows_g0, Wp, bias, C, c_code, ldc, M, N, K,
                                               act, groups, a_gs, c_gs, _stream()), "linear_nt_packed")


def _prep_weight(W, cdt, epc):
    """[N, K] fp32 parameter -> [N, round_up(K, epc)] compute dtype, zero padded."""
    return _pad_cast(W.detach(), cdt, epc)


def gather_mean_multi(segments, ld, D, out_ld, adam=None, hops=None, scale=None):
    """All hops of a level in one K2 launch.  segments: list of (table, ids|None, out, M, n) with
    bf16 (or, parity mode, fp32) row-major tensors sharing ld / out_ld.  adam: optional _native.AdamDesc -- the clip + Adam
    update of the previous batch rides in the same launch; hops: optional _native.HopsDesc -- so does
    the frontier sampling of a later batch (gsage_gather_mean_multi_adam).  scale: the column scales of an FP8 store
    whose `data` every segment reads (gsage_gather_mean_multi_fp8: bf16 or fp32 outputs, no side roles)."""
    k = len(segments)
    T = (ctypes.c_void_p * k)(*[s[0].data_ptr() for s in segments])
    I = (ctypes.c_void_p * k)(*[(s[1].data_ptr() if s[1] is not None else None) for s in segments])
    O = (ctypes.c_void_p * k)(*[s[2].data_ptr() for s in segments])
    Ms = (ctypes.c_int64 * k)(*[int(s[3]) for s in segments])
    ns = (ctypes.c_int32 * k)(*[int(s[4]) for s in segments])
    code, ocode = _code(segments[0][0].dtype), _code(segments[0][2].dtype)
    assert all(s[0].dtype == segments[0][0].dtype and s[2].dtype == segments[0][2].dtype for s in segments)
    assert (code == nat.FP8) == (scale is not None), "an FP8 table, and only an FP8 table, comes with its scales"
    if code == nat.FP8:
        assert adam is None and hops is None, "gather_mean_multi: the FP8 launch carries no side roles"
        nat.check(nat.lib().gsage_gather_mean_multi_fp8(k, T, I, O, Ms, ns, _ptr(scale), ld, D, ocode, out_ld,
                                                        _stream()), "gather_mean_multi_fp8")
        return
    if adam is not None or hops is not None:
        nat.check(nat.lib().gsage_gather_mean_multi_adam(
            k, T, I, O, Ms, ns, code, ld, D, code, out_ld,
            ctypes.addressof(adam) if adam is not None else None,
            ctypes.addressof(hops) if hops is not None else None, _stream()), "gather_mean_multi_adam")
        return
    nat.check(nat.lib().gsage_gather_mean_multi(k, T, I, O, Ms, ns, code, ld, D, ocode, out_ld,
                                                _stream()), "gather_mean_multi")


def wgrad_plan(M, Ntot, K, target=240):
    """(rows_per_split, n_slabs, ldk) used by wgrad.  A workgroup owns one 128 x 128 output tile and
    one M-slice (its four waves quarter the slice and meet in LDS), one workgroup fits per CU, and
    every slice costs a partial tile in HBM: so aim at ~240 workgroups (MI355X: 256 CUs, the rest is
    left to the small problems sharing a gsage_wgrad_multi launch) and never below 64 rows per wave.
    target: workgroups to aim at (small problems that share a launch with a big one take fewer, longer
    slices: fewer partial tiles to write and to sum)."""
    ldk = _round_up(K, 4)
    tiles = ((Ntot + 127) // 128) * ((ldk + 127) // 128)
    s_target = max(1, target // tiles)
    rps = max(256, _round_up((M + s_target - 1) // s_target, 16))
    return rps, (M + rps - 1) // rps, ldk


def wgrad_balance(shapes, budget=248, group=8):
    """Workgroup targets for K5b problems that share gsage_wgrad_multi launches (issued `group` at a time, in this
    order).  One workgroup fits per CU, so a launch with more workgroups than CUs runs in rounds and its small problems
    then cost a round of their own (the max-pool step's six problems used 572 workgroups: 150 us where the big one
    alone takes 98).  Per launch: the smallest slice length R (rows, multiple of 16, >= 256) for which
    sum_i tiles_i * ceil(M_i / R) <= budget -- every problem gets slices of about the same length, so they finish
    together, in one round.  shapes: [(M, Ntot, K)]; returns the per-problem `target` for wgrad_plan."""
    targets = []
    for i in range(0, len(shapes), group):
        chunk = shapes[i:i + group]
        tiles = [((nt + 127) // 128) * ((_round_up(k, 4) + 127) // 128) for (_m, nt, k) in chunk]
        R = 256
        while sum(t * ((m + R - 1) // R) for t, (m, _nt, _k) in zip(tiles, chunk)) > budget and R < max(m for m, _, _ in chunk):
            R += 16
        targets += [t * ((m + R - 1) // R) for t, (m, _nt, _k) in zip(tiles, chunk)]
    return targets


def wgrad(dC, A, lda, a_gstride, M, Ntot, K, n_per_group, out=None, slabs=None, reduce=True):
    """dW_g = dC_g^T @ A_g on the matrix cores (K5b), bf16 operands, fp32 result
    [groups, n_per_group, K].  dC: contiguous bf16 [M, >=Ntot]; A: bf16 [M, lda] row-major.
    reduce=False leaves the per-slice partial tiles in `slabs` ([S, Ntot, ldk]) for
    gsage_finalize_grads and returns the slabs."""
    groups = (Ntot + n_per_group - 1) // n_per_group
    rps, S, ldk = wgrad_plan(M, Ntot, K)
    if slabs is None:
        slabs = torch.empty(S, Ntot, ldk, dtype=torch.float32, device=dC.device)
    if reduce and out is None:
        out = torch.empty(groups, n_per_group, K, dtype=torch.float32, device=dC.device)
    nat.check(nat.lib().gsage_wgrad(_ptr(dC), _code(dC.dtype), dC.stride(0), _ptr(A), lda, a_gstride, M, Ntot, K,
                                    n_per_group, rps, _ptr(slabs), ldk, _ptr(out) if reduce else None,
                                    n_per_group * K, _stream()), "wgrad")
    return out if reduce else slabs


def wgrad_multi(problems):
    """Several K5b problems in one launch; partial tiles stay in each problem's slabs
    (gsage_finalize_grads sums them).  problems: list of (dC, A, lda, a_gstride, M, Ntot, K,
    n_per_group, slabs[, workgroup target[, a_rows]]) with the meaning of wgrad(); a_rows (int64 [M], 16-byte
    aligned): reduction index m reads row a_rows[m] of A -- a frontier's table rows in place."""
    descs = (nat.WgradDesc * len(problems))()
    for d, prob in zip(descs, problems):
        dC, A, lda, a_gs, M, Ntot, K, npg, slabs = prob[:9]
        rps, S, ldk = wgrad_plan(M, Ntot, K, *[v for v in prob[9:10] if v is not None])
        assert tuple(slabs.shape) == (S, Ntot, ldk) and slabs.is_contiguous()
        rows = prob[10] if len(prob) > 10 else None
        assert rows is None or (rows.dtype == torch.int64 and rows.is_contiguous() and rows.numel() >= M)
        d.a_rows = _ptr(rows) if rows is not None else None
        d.dC, d.A, d.slabs = _ptr(dC), _ptr(A), _ptr(slabs)
        d.ldc, d.lda, d.a_gstride = dC.stride(0), lda, a_gs
        d.M, d.Ntot, d.K, d.n_per_group, d.ldk, d.rows_per_split = M, Ntot, K, npg, ldk, rps
    code = _code(problems[0][0].dtype)
    assert all(prob[0].dtype == prob[1].dtype == problems[0][0].dtype for prob in problems)
    nat.check(nat.lib().gsage_wgrad_multi(len(problems), ctypes.cast(descs, ctypes.c_void_p), code, _stream()),
              "wgrad_multi")


class _Linear(torch.autograd.Function):
    """act(x @ W^T + b) on the matrix cores; the backward contractions too (K5 against the transposed operand copy for the
    input gradient, K5b for the weight gradient)."""

    @staticmethod
    def forward(ctx, x, W, b, act, cdt_name, out_dtype):
        cdt = torch_dtype(cdt_name)
        epc = 8 if cdt == torch.bfloat16 else 4
        M, K = x.shape
        N = W.shape[0]
        xa = _pad_cast(x.detach(), cdt, 8 * epc, _trusted(x))   # whole 128-byte rows: LDS-DMA GEMM path
        wa = _prep_weight(W, cdt, 8 * epc)
        out = torch.empty(M, N, dtype=out_dtype, device=x.device)
        bf = b.detach().float().contiguous() if b is not None else None
        _linear_launch(_ptr(xa), xa.stride(0), None, 0, _ptr(wa), wa.stride(0), _ptr(bf),
                       _ptr(out), N, M, N, K, act, 1, 0, 0, 0, _code(cdt), _code(out_dtype))
        ctx.save_for_backward(xa, wa, out if act != nat.ACT_NONE else None)
        ctx.meta = (act, K, x.dtype, b is not None, W.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        xa, wa, out = ctx.saved_tensors
        act, K, xdt, has_b, wdt = ctx.meta
        g = g.float()
        if act == nat.ACT_RELU:
            g = g * (out > 0)
        elif act == nat.ACT_TANH:
            o = out.float()
            g = g * (1 - o * o)
        gc = g.to(xa.dtype)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _dgrad(gc, wa, K).to(xdt)
        if ctx.needs_input_grad[1]:
            # K5b (the library GEMM behind gc.t() @ xa ran at ~20 TF/s on these skinny shapes)
            dw = _wgrad_any(gc, xa, K).to(wdt)
        if has_b and ctx.needs_input_grad[2]:
            db = g.sum(dim=0)
        return dx, dw, db, None, None, None


def linear(x, W, b=None, act=nat.ACT_NONE, compute_dtype=None, out_dtype=torch.float32):
    """nn.Linear (+ fused activation) on CUDA through K5; host mode uses F.linear."""
    if not x.is_cuda:
        y = F.linear(x.float(), W, b)
        if act == nat.ACT_RELU:
            y = torch.relu(y)
        elif act == nat.ACT_TANH:
            y = torch.tanh(y)
        return y
    return _Linear.apply(x, W, b, act, compute_dtype or config.compute_dtype, out_dtype)


class _SageProject(torch.autograd.Function):
    """act(cat[x @ Wx^T, agg @ Wn^T], dim=1) (nn_modules.py:200-202 and its twins at :228-230,
    :317-319) as ONE grouped MFMA launch writing both halves of the concat.  x may be a row
    reference (table, ids): then the A tile of group 0 is gathered inside the kernel."""

    @staticmethod
    def forward(ctx, x, agg, Wx, Wn, x_table, x_ids, x_dim, act, cdt_name, out_dtype):
        cdt = torch_dtype(cdt_name)
        epc = 8 if cdt == torch.bfloat16 else 4
        h = Wx.shape[0]
        M = agg.shape[0]
        Dn = Wn.shape[1]
        an = _pad_cast(agg.detach(), cdt, 8 * epc, _trusted(agg))
        if x_ids is not None:
            Dx = x_dim
            if x_table.dtype != cdt or x_table.stride(0) % epc != 0:
                xa = _gather_mean_raw(x_table, Dx, x_ids, M, 1, cdt, _round_up(Dx, epc))
                a_rows = None
            else:
                xa, a_rows = x_table, x_ids
        else:
            Dx = x.shape[1]
            xa, a_rows = _pad_cast(x.detach(), cdt, 8 * epc, _trusted(x)), None
        out = torch.empty(M, 2 * h, dtype=out_dtype, device=agg.device)
        esz = xa.element_size()
        delta = an.data_ptr() - xa.data_ptr()
        # one grouped launch when both halves share K and a leading dimension: group 1's A
        # operand is addressed as A + a_gstride, i.e. the agg buffer relative to the x operand
        grouped = (Dx == Dn and delta % esz == 0 and xa.stride(0) == an.stride(0))
        if grouped:
            ldw = _round_up(Dx, 8 * epc)
            w2 = torch.zeros(2, h, ldw, dtype=cdt, device=agg.device)
            w2[0, :, :Dx] = Wx.detach()
            w2[1, :, :Dn] = Wn.detach()
        if grouped:
            _linear_launch(_ptr(xa), xa.stride(0), _ptr(a_rows), 1, _ptr(w2), ldw, None, _ptr(out),
                           2 * h, M, h, Dx, act, 2, delta // esz, h * ldw, h, _code(cdt),
                           _code(out_dtype))
            wxa, wna = w2[0], w2[1]
        else:
            wxa = _prep_weight(Wx, cdt, 8 * epc)
            wna = _prep_weight(Wn, cdt, 8 * epc)
            _linear_launch(_ptr(xa), xa.stride(0), _ptr(a_rows), 1, _ptr(wxa), wxa.stride(0), None,
                           _ptr(out), 2 * h, M, h, Dx, act, 1, 0, 0, 0, _code(cdt), _code(out_dtype))
            _linear_launch(_ptr(an), an.stride(0), None, 0, _ptr(wna), wna.stride(0), None,
                           _vp(out.data_ptr() + h * out.element_size()), 2 * h, M, h, Dn, act, 1,
                           0, 0, 0, _code(cdt), _code(out_dtype))
        ctx.save_for_backward(xa, a_rows, an, wxa, wna, out if act == nat.ACT_RELU else None)
        ctx.grouped = (delta // esz) if grouped else None
        ctx.meta = (act, h, Dx, Dn, x.dtype if x is not None else None, agg.dtype, Wx.dtype, cdt, epc)
        return out

    @staticmethod
    def backward(ctx, g):
        xa, a_rows, an, wxa, wna, out = ctx.saved_tensors
        act, h, Dx, Dn, xdt, adt, wdt, cdt, epc = ctx.meta
        g = g.float()
        if act == nat.ACT_RELU:
            g = g * (out > 0)
        gc = g.to(cdt)
        gx, gn = gc[:, :h], gc[:, h:]
        dx = dagg = dwx = dwn = None
        fused_w = (cdt == torch.bfloat16 and ctx.grouped is not None and h % 128 == 0 and
                   xa.stride(0) % 8 == 0 and ctx.needs_input_grad[2] and ctx.needs_input_grad[3])
        # halves with different K (pool / attention aggregators): one K5b launch each -- the library
        # GEMM behind gx.t() @ xm ran at ~20 TF/s on these skinny, transposed operands
        k5b_ok = cdt == torch.bfloat16 and h % 8 == 0 and gc.shape[0] >= 64 and gc.is_contiguous()
        if fused_w:
            # both weight gradients in one MFMA launch (x rows re-gathered when they were lazy)
            xm = xa if a_rows is None else _gather_mean_raw(xa, an.stride(0), a_rows, an.shape[0], 1,
                                                            cdt, an.stride(0))
            dw = wgrad(gc.contiguous(), xm, xm.stride(0), (an.data_ptr() - xm.data_ptr()) // 2,
                       an.shape[0], 2 * h, Dx, h)
            dwx, dwn = dw[0].to(wdt), dw[1].to(wdt)
        if ctx.needs_input_grad[2] and not fused_w:
            if a_rows is not None:
                M = an.shape[0]
                xm = _gather_mean_raw(xa, Dx, a_rows, M, 1, cdt, _round_up(Dx, epc))
            else:
                xm = xa
            if k5b_ok and xm.stride(0) % 8 == 0:
                dwx = wgrad(gx, xm, xm.stride(0), 0, gc.shape[0], h, Dx, h)[0].to(wdt)
            else:
                dwx = _wgrad_any(gx, xm, Dx).to(wdt)
        if ctx.needs_input_grad[3] and not fused_w:
            if k5b_ok and an.stride(0) % 8 == 0:
                dwn = wgrad(gn, an, an.stride(0), 0, gc.shape[0], h, Dn, h)[0].to(wdt)
            else:
                dwn = _wgrad_any(gn, an, Dn).to(wdt)
        if ctx.needs_input_grad[0]:
            dx = _dgrad(gx, wxa, Dx).to(xdt)
        if ctx.needs_input_grad[1]:
            dagg = _dgrad(gn, wna, Dn).to(adt)
        return dx, dagg, dwx, dwn, None, None, None, None, None, None


def sage_project(x, agg, Wx, Wn, act=nat.ACT_NONE, compute_dtype=None, out_dtype=torch.float32):
    """x: Tensor [M, Dx] or RowRef; agg: Tensor [M, Dn].  Returns [M, 2h]."""
    if not agg.is_cuda:
        xt = x.materialize() if isinstance(x, RowRef) else x
        y = torch.cat([F.linear(xt.float(), Wx), F.linear(agg.float(), Wn)], dim=1)
        return torch.relu(y) if act == nat.ACT_RELU else y
    cd = compute_dtype or config.compute_dtype
    x = decoded_rows(x, cd)
    if isinstance(x, RowRef):
        return _SageProject.apply(None, agg, Wx, Wn, x.store.data, x.ids, x.store.dim, act, cd,
                                  out_dtype)
    return _SageProject.apply(x, agg, Wx, Wn, None, None, 0, act, cd, out_dtype)


# =============================================================================================
# K3  pooling MLP
# =============================================================================================
class _PoolMLP(torch.autograd.Function):
    """pool_r relu(neibs @ Wm^T + bm) over each group of n rows (nn_modules.py:224-226,:240,:252);
    the [M*n, H] hidden activations stay on chip.  Backward recomputes nothing it can route
    through argmax: d hidden is non-zero only at the winning row of each (segment, channel)."""

    @staticmethod
    def forward(ctx, neibs, Wm, bm, table, ids, dim, M, n, mode, cdt_name):
        cdt = torch_dtype(cdt_name)
        epc = 8 if cdt == torch.bfloat16 else 4
        H = Wm.shape[0]
        if ids is not None:
            K = dim
            if table.dtype != cdt or table.stride(0) % epc != 0:
                A = _gather_mean_raw(table, K, ids, M * n, 1, cdt, _round_up(K, epc))
                a_rows = None
            else:
                A, a_rows = table, ids
        else:
            K = neibs.shape[1]
            A, a_rows = _pad_cast(neibs.detach(), cdt, epc, _trusted(neibs)), None
        wa = _prep_weight(Wm, cdt, epc)
        bf = bm.detach().float().contiguous()
        pooled = torch.empty(M, H, dtype=torch.float32, device=A.device)
        argmax = torch.empty(M, H, dtype=torch.int32, device=A.device) if mode == nat.POOL_MAX else None
        nat.check(nat.lib().gsage_pool_mlp(_ptr(A), _code(cdt), A.stride(0), _ptr(a_rows), _ptr(wa),
                                           wa.stride(0), _ptr(bf), M, n, H, K, mode, _ptr(pooled),
                                           H, _ptr(argmax), None, 0, None, _stream()), "pool_mlp")
        ctx.save_for_backward(A, a_rows, wa, bf, pooled, argmax)
        ctx.meta = (M, n, H, K, mode, cdt, neibs.dtype if neibs is not None else None, Wm.dtype, epc)
        return pooled

    @staticmethod
    def backward(ctx, g):
        A, a_rows, wa, bf, pooled, argmax = ctx.saved_tensors
        M, n, H, K, mode, cdt, ndt, wdt, epc = ctx.meta
        g = g.float()
        rows = A if a_rows is None else _gather_mean_raw(A, K, a_rows, M * n, 1, cdt,
                                                         _round_up(K, epc))
        dn = dw = db = None
        fast = mode == nat.POOL_MAX and cdt == torch.bfloat16 and H % 128 == 0 and g.is_cuda
        if fast:
            # routed gradient written once as the bf16 operand K5b wants (no fp32 [M, n, H] scatter)
            g = g.contiguous()
            ghc = torch.empty(M * n, H, dtype=torch.bfloat16, device=g.device)
            nat.check(nat.lib().gsage_pool_route_bwd(_ptr(g), H, _ptr(pooled), H, _ptr(argmax), H, M, n, H,
                                                     _ptr(ghc), nat.BF16, H, _stream()), "pool_route_bwd")
            if ctx.needs_input_grad[2]:
                db = (g * (pooled > 0)).sum(dim=0)
            if ctx.needs_input_grad[1]:
                dw = wgrad(ghc, rows, rows.stride(0), 0, M * n, H, K, H)[0].to(wdt)
        else:
            if mode == nat.POOL_MAX:
                gh = torch.zeros(M, n, H, dtype=torch.float32, device=g.device)
                gh.scatter_(1, argmax.long().unsqueeze(1), (g * (pooled > 0)).unsqueeze(1))
                gh = gh.view(M * n, H)
            else:
                hid = torch.empty(M * n, H, dtype=torch.float32, device=g.device)     # recompute (mean pool only): K5
                ra = _pad_cast(rows, cdt, 8 * epc, True) if rows.stride(0) % (8 * epc) == 0 else _pad_cast(rows[:, :K], cdt, 8 * epc)
                wl = _pad_cast(wa[:, :K], cdt, 8 * epc)
                _linear_launch(_ptr(ra), ra.stride(0), None, 0, _ptr(wl), wl.stride(0), _ptr(bf), _ptr(hid), H, M * n, H, K,
                               nat.ACT_RELU, 1, 0, 0, 0, _code(cdt), nat.F32)
                gh = (g / n).repeat_interleave(n, dim=0) * (hid > 0)
            ghc = gh.to(cdt)
            if ctx.needs_input_grad[1]:
                dw = _wgrad_any(ghc, rows, K).to(wdt)
            if ctx.needs_input_grad[2]:
                db = gh.sum(dim=0)
        if ctx.needs_input_grad[0]:
            dn = _dgrad(ghc, wa, K).to(ndt)
        return dn, dw, db, None, None, None, None, None, None, None


def pool_mlp(neibs, Wm, bm, M, mode, compute_dtype=None):
    """neibs: Tensor [M*n, D] or RowRef.  Returns pooled [M, H] fp32."""
    total = neibs.shape[0]
    assert total % M == 0
    n = total // M
    if not neibs.is_cuda:
        nb = neibs.materialize() if isinstance(neibs, RowRef) else neibs
        hid = torch.relu(F.linear(nb.float(), Wm, bm)).view(M, n, -1)
        return hid.max(dim=1)[0] if mode == nat.POOL_MAX else hid.mean(dim=1)
    cd = compute_dtype or config.compute_dtype
    neibs = decoded_rows(neibs, cd)
    if n > 64:      # tile holds whole segments only up to 64 rows: unfused route, still K5
        nb = neibs.materialize() if isinstance(neibs, RowRef) else neibs
        hid = linear(nb, Wm, bm, nat.ACT_RELU, cd).view(M, n, -1)
        return hid.max(dim=1)[0] if mode == nat.POOL_MAX else hid.mean(dim=1)
    if isinstance(neibs, RowRef):
        return _PoolMLP.apply(None, Wm, bm, neibs.store.data, neibs.ids, neibs.store.dim, M, n,
                              mode, cd)
    return _PoolMLP.apply(neibs, Wm, bm, None, None, 0, M, n, mode, cd)


# =============================================================================================
# K4  attention weighting
# =============================================================================================
class _AttnAggregate(torch.autograd.Function):
    """softmax_r(<na[i,r], xa[i]>) weighted sum of the raw neighbour rows (nn_modules.py:309-315)."""

    @staticmethod
    def forward(ctx, na, xa, neibs, table, ids, dim, M, n):
        na = na.contiguous().float()
        xa = xa.contiguous().float()
        if ids is not None:
            T, D, rows_ids = table, dim, ids
        else:
            T = neibs.detach()
            T = T if T.is_contiguous() else T.contiguous()
            D, rows_ids = T.shape[1], None
        agg = torch.empty(M, D, dtype=torch.float32, device=na.device)
        ws = torch.empty(M, n, dtype=torch.float32, device=na.device)
        nat.check(nat.lib().gsage_attn_aggregate(_ptr(na), na.stride(0), _ptr(xa), xa.stride(0),
                                                 _ptr(T), _code(T.dtype), T.stride(0),
                                                 _ptr(rows_ids), M, n, na.shape[1], D, _ptr(agg), D,
                                                 _ptr(ws), _stream()), "attn_aggregate")
        ctx.save_for_backward(na, xa, T, rows_ids, ws)
        ctx.meta = (M, n, D, neibs.dtype if neibs is not None else None)
        return agg

    @staticmethod
    def backward(ctx, g):
        na, xa, T, rows_ids, ws = ctx.saved_tensors
        M, n, D, ndt = ctx.meta
        g = g.float().contiguous()
        vec = 8 if T.dtype == torch.bfloat16 else 4
        wide = (T.dtype in (torch.bfloat16, torch.float32) and n <= 32 and T.stride(0) % vec == 0 and
                T.data_ptr() % 16 == 0 and _round_up(D, vec) <= T.stride(0))
        if wide:
            # dws, the softmax backward and both products in one launch; the rows are read once, in
            # storage precision, straight from the table
            Ha = na.shape[1]
            dna = torch.empty(M * n, Ha, dtype=torch.float32, device=g.device)
            dxa = torch.empty(M, Ha, dtype=torch.float32, device=g.device)
            nat.check(nat.lib().gsage_attn_bwd(_ptr(g), g.stride(0), _ptr(ws), _ptr(na), na.stride(0), _ptr(xa),
                                               xa.stride(0), _ptr(T), _code(T.dtype), T.stride(0), _ptr(rows_ids),
                                               M, n, Ha, D, _ptr(dna), Ha, _ptr(dxa), Ha, _stream()), "attn_bwd")
            dneibs = None
            if ctx.needs_input_grad[2]:
                dneibs = (ws.unsqueeze(2) * g.unsqueeze(1)).reshape(M * n, D).to(ndt)
            return dna, dxa, dneibs, None, None, None, None, None
        rows = T if rows_ids is None else _gather_mean_raw(T, D, rows_ids, M * n, 1, torch.float32)
        rows = rows[:, :D].float().view(M, n, D)
        dws = torch.bmm(rows, g.unsqueeze(2)).squeeze(2)                    # [M, n]
        ds = ws * (dws - (dws * ws).sum(dim=1, keepdim=True))               # softmax backward
        nav = na.view(M, n, -1)
        dna = (ds.unsqueeze(2) * xa.unsqueeze(1)).reshape(M * n, -1)
        dxa = torch.bmm(ds.unsqueeze(1), nav).squeeze(1)
        dneibs = None
        if ctx.needs_input_grad[2]:
            dneibs = (ws.unsqueeze(2) * g.unsqueeze(1)).reshape(M * n, D).to(ndt)
        return dna, dxa, dneibs, None, None, None, None, None


def attn_aggregate(na, xa, neibs, M):
    """na: att(neibs) [M*n, Ha]; xa: att(x) [M, Ha]; neibs: Tensor [M*n, D] or RowRef."""
    n = na.shape[0] // M
    if not na.is_cuda:
        nb = neibs.materialize() if isinstance(neibs, RowRef) else neibs
        s = torch.bmm(na.view(M, n, -1), xa.view(M, -1, 1)).squeeze(2)
        w = torch.softmax(s, dim=1)
        return (nb.float().view(M, n, -1) * w.unsqueeze(-1)).sum(dim=1)
    neibs = decoded_rows(neibs)
    if n > 64:
        nb = neibs.materialize() if isinstance(neibs, RowRef) else neibs
        s = torch.bmm(na.view(M, n, -1), xa.view(M, -1, 1)).squeeze(2)
        w = torch.softmax(s, dim=1)
        return (nb.float().view(M, n, -1) * w.unsqueeze(-1)).sum(dim=1)
    if isinstance(neibs, RowRef):
        return _AttnAggregate.apply(na, xa, None, neibs.store.data, neibs.ids, neibs.store.dim, M, n)
    return _AttnAggregate.apply(na, xa, neibs, None, None, 0, M, n)


# =============================================================================================
# LSTM aggregator: last position of a batch_first LSTM over each node's neighbour rows
# =============================================================================================
def lstm_ok(H, n, compute_dtype=None):
    """Whether the recurrence kernels take a direction of H hidden units over n steps (gsage_lstm_ok)."""
    return bool(nat.lib().gsage_lstm_ok(_code(torch_dtype(compute_dtype)), int(H), int(n)))


def _lstm_pack_whh(w_hh, cdt):
    """weight_hh [4H, H] -> both fragment-ordered operand copies (forward half, backward half) in the compute type."""
    H = int(w_hh.shape[1])
    w = w_hh.detach().float().contiguous()
    wp = torch.empty(int(nat.lib().gsage_lstm_packed_elems(H)), dtype=cdt, device=w.device)
    nat.check(nat.lib().gsage_lstm_pack_whh(_ptr(w), w.stride(0), H, _code(cdt), _ptr(wp), _stream()), "lstm_pack_whh")
    return wp


def _off(t, elems):
    return _vp(t.data_ptr() + elems * t.element_size())


class _LSTMLast(torch.autograd.Function):
    """seq, _ = lstm(neibs.view(M, n, D)); seq[:, -1, :] (nn_modules.py:278-279) without the sequence: the forward
    direction's final h, and for a bidirectional LSTM the reverse direction's FIRST step -- one cell evaluation on the
    last neighbour from a zero state.  Input projection on K5 (gather fused for a RowRef), recurrence on
    gsage_lstm_fwd / _bwd, weight and input gradients on K5b / K5 over the dG the backward recurrence writes.
    Reserve per direction: activated gates (over GX, compute type), c (fp32) and the steps' input states."""

    @staticmethod
    def forward(ctx, neibs, table, ids, dim, M, n, cdt_name, w_ih, w_hh, b_ih, b_hh, rw_ih, rw_hh, rb_ih, rb_hh):
        cdt = torch_dtype(cdt_name)
        epc = 8 if cdt == torch.bfloat16 else 4
        code = _code(cdt)
        L = nat.lib()
        H = int(w_hh.shape[1])
        Hr = int(rw_hh.shape[1]) if rw_ih is not None else 0
        if ids is not None:
            K = dim
            if table.dtype != cdt or table.stride(0) % epc != 0:
                A = _gather_mean_raw(table, K, ids, M * n, 1, cdt, _round_up(K, epc))
                a_rows = None
            else:
                A, a_rows = table, ids
        else:
            K = neibs.shape[1]
            A, a_rows = _pad_cast(neibs.detach(), cdt, epc, _trusted(neibs)), None
        dev = A.device
        out = torch.empty(M, H + Hr, dtype=cdt, device=dev)

        def project(w, b1, b2, rows, a_ptr, lda, r_ids):
            wa = _prep_weight(w, cdt, epc)
            bias = (b1.detach().float() + b2.detach().float()).contiguous()
            N = int(w.shape[0])
            ldg = _round_up(N, epc)
            gates = (torch.zeros if ldg != N else torch.empty)(rows, ldg, dtype=cdt, device=dev)
            _linear_launch(a_ptr, lda, _ptr(r_ids), 0, _ptr(wa), wa.stride(0), _ptr(bias), _ptr(gates), ldg, rows, N, K,
                           nat.ACT_NONE, 1, 0, 0, 0, code, code)
            return wa, gates, bias

        wa, gates, bias = project(w_ih, b_ih, b_hh, M * n, _ptr(A), A.stride(0), a_rows)
        wp = _lstm_pack_whh(w_hh, cdt) if n > 1 else None
        cseq = torch.empty(M * n, H, dtype=torch.float32, device=dev)
        ldh = _round_up(H, epc)
        hprev = torch.zeros(M * n, ldh, dtype=cdt, device=dev) if n > 1 else None
        nat.check(L.gsage_lstm_fwd(_ptr(gates), code, gates.stride(0), _ptr(wp), M, n, H, _ptr(cseq), _ptr(hprev), ldh,
                                   _ptr(out), H + Hr, _stream()), "lstm_fwd")
        rwa = rgates = rcseq = r_ids = rbias = None
        if Hr:
            # the reverse direction's output at the last position is its first step: project the last neighbour only
            if a_rows is not None:
                r_ids = a_rows.view(M, n)[:, n - 1].contiguous()
                rwa, rgates, rbias = project(rw_ih, rb_ih, rb_hh, M, _ptr(A), A.stride(0), r_ids)
            else:
                rwa, rgates, rbias = project(rw_ih, rb_ih, rb_hh, M, _off(A, (n - 1) * A.stride(0)), n * A.stride(0),
                                             None)
            rcseq = torch.empty(M, Hr, dtype=torch.float32, device=dev)
            nat.check(L.gsage_lstm_fwd(_ptr(rgates), code, rgates.stride(0), None, M, 1, Hr, _ptr(rcseq), None, 0,
                                       _off(out, H), H + Hr, _stream()), "lstm_fwd (reverse)")
        # (the summed biases are kept too: a recorded forward reads every operand again at each replay)
        ctx.save_for_backward(A, a_rows, r_ids, wa, wp, gates, cseq, hprev, rwa, rgates, rcseq, bias, rbias)
        ctx.meta = (M, n, H, Hr, K, cdt, epc, neibs.dtype if neibs is not None else None, w_ih.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        A, a_rows, r_ids, wa, wp, gates, cseq, hprev, rwa, rgates, rcseq = ctx.saved_tensors[:11]
        M, n, H, Hr, K, cdt, epc, ndt, wdt = ctx.meta
        L = nat.lib()
        code = _code(cdt)
        dev = g.device
        g = g.float().contiguous()
        need = ctx.needs_input_grad
        ldg = gates.stride(0)
        dG = (torch.zeros if ldg != 4 * H else torch.empty)(M * n, ldg, dtype=cdt, device=dev)
        carry = torch.empty(M, 2 * H, dtype=torch.float32, device=dev) if n > 1 else None
        Hp = _round_up(H, 32)
        nat.check(L.gsage_lstm_bwd(_ptr(gates), code, ldg, _off(wp, 4 * Hp * Hp) if wp is not None else None, M, n, H,
                                   _ptr(cseq), _ptr(g), H + Hr, _ptr(dG), ldg, _ptr(carry), _stream()), "lstm_bwd")
        ones = torch.ones(M * n, epc, dtype=cdt, device=dev)          # bias gradient = dG^T 1 on K5b

        def params(dg, rows, n_out, hp):
            dw_ih = _wgrad_any(dg, rows, K)[:n_out].to(wdt) if rows is not None else None
            dw_hh = _wgrad_any(dg, hp, n_out // 4)[:n_out].to(wdt) if hp is not None else None
            db = _wgrad_any(dg, ones[:dg.shape[0]], 1)[:n_out, 0].to(wdt).contiguous()
            return dw_ih, dw_hh, db

        rows = None
        if need[7]:           # the rows in storage precision, as the forward's projection read them
            rows = A if a_rows is None else _gather_mean_raw(A, K, a_rows, M * n, 1, cdt, _round_up(K, epc))
        dw_ih, dw_hh, db = params(dG, rows, 4 * H, hprev)
        if dw_hh is None:
            dw_hh = torch.zeros(4 * H, H, dtype=wdt, device=dev)     # n == 1: no recurrent term
        dn = None
        if need[0]:
            dn = _dgrad(dG[:, :4 * H], wa, K)
        rdw_ih = rdw_hh = rdb = None
        if Hr:
            ldr = rgates.stride(0)
            rdG = (torch.zeros if ldr != 4 * Hr else torch.empty)(M, ldr, dtype=cdt, device=dev)
            nat.check(L.gsage_lstm_bwd(_ptr(rgates), code, ldr, None, M, 1, Hr, _ptr(rcseq), _off(g, H), H + Hr,
                                       _ptr(rdG), ldr, None, _stream()), "lstm_bwd (reverse)")
            rrows = None
            if need[11]:
                rrows = A[n - 1::n] if a_rows is None else _gather_mean_raw(A, K, r_ids, M, 1, cdt, _round_up(K, epc))
            rdw_ih, _, rdb = params(rdG, rrows, 4 * Hr, None)
            rdw_hh = torch.zeros(4 * Hr, Hr, dtype=wdt, device=dev)  # its one step starts from a zero state
            if dn is not None:
                dn.view(M, n, K)[:, n - 1, :] += _dgrad(rdG[:, :4 * Hr], rwa, K)
        if dn is not None:
            dn = dn.to(ndt)
        return (dn, None, None, None, None, None, None, dw_ih, dw_hh, db, db, rdw_ih, rdw_hh, rdb, rdb)


def lstm_last(neibs, M, w_ih, w_hh, b_ih, b_hh, reverse=None, compute_dtype=None):
    """neibs: Tensor [M*n, D] or RowRef; (w_ih, w_hh, b_ih, b_hh): one nn.LSTM direction; reverse: the four parameters
    of the reverse direction or None.  Returns [M, hidden_dim] in the compute type: the LSTM's output at the LAST
    position, the two directions side by side.  CUDA only (host mode keeps nn.LSTM, nn_modules.LSTMAggregator)."""
    total = neibs.shape[0]
    assert total % M == 0 and neibs.is_cuda
    n = total // M
    cd = compute_dtype or config.compute_dtype
    rev = tuple(reverse) if reverse is not None else (None, None, None, None)
    neibs = decoded_rows(neibs, cd)
    if isinstance(neibs, RowRef):
        return _LSTMLast.apply(None, neibs.store.data, neibs.ids, neibs.store.dim, M, n, cd, w_ih, w_hh, b_ih, b_hh, *rev)
    return _LSTMLast.apply(neibs, None, None, 0, M, n, cd, w_ih, w_hh, b_ih, b_hh, *rev)


# =============================================================================================
# Skip-gram head of the unsupervised model (csrc/gsage_unsup.hip)
# =============================================================================================
def _skipgram_host(E, B, Q, pair_w, neg_weight):
    """The head's definition in torch ops (host mode): -> (loss, aff [B, 1 + Q])."""
    z = F.normalize(E.float(), dim=1)
    a = (z[:B] * z[B:2 * B]).sum(1)
    n = z[:B] @ z[2 * B:2 * B + Q].t()
    loss = ((pair_w * F.softplus(-a)).sum() + neg_weight * F.softplus(n).sum()) / B
    return loss, torch.cat([a.unsqueeze(1), n], dim=1)


def skipgram_head(E, B, Q, pair_w, neg_weight=1.0, grad_dtype=torch.float32, grad_ld=None, n_valid=None):
    """gsage_head_skipgram on the un-normalised rows E [2B + Q, D] = [seeds | positives | negatives] (CUDA, fp32, unit
    column stride): -> (loss [1], aff [B, 1 + Q] = [a_i | n_iq], dE [2B + Q, D] = d loss / d E in `grad_dtype`).
        loss = (1/B) sum_i [pair_w_i softplus(-a_i) + neg_weight sum_q softplus(n_iq)],  a, n = cosines of the rows
    n_valid (an int, or an int32 device word): gsage_head_skipgram_live -- only the first b = clamp(n_valid, 1, B) seeds
    are live: the loss is their mean, rows i and B + i of dE are zero for i >= b, and aff[b:] is returned as zeros."""
    assert E.is_cuda and E.dtype == torch.float32 and E.dim() == 2 and int(E.shape[0]) == 2 * B + Q
    if E.stride(1) != 1:
        E = E.contiguous()
    D = int(E.shape[1])
    pair_w = pair_w.to(torch.float32).contiguous()
    assert pair_w.is_cuda and pair_w.numel() == B
    L = nat.lib()
    ldd = D if grad_ld is None else int(grad_ld)
    dE = torch.empty(2 * B + Q, ldd, dtype=grad_dtype, device=E.device) if ldd == D else \
        torch.zeros(2 * B + Q, ldd, dtype=grad_dtype, device=E.device)
    loss = torch.empty(1, dtype=torch.float32, device=E.device)
    scratch = torch.empty(max(int(L.gsage_head_skipgram_scratch(B, Q, D)), 1), dtype=torch.float32, device=E.device)
    if n_valid is None:
        aff = torch.empty(B, 1 + Q, dtype=torch.float32, device=E.device)
        nat.check(L.gsage_head_skipgram(_ptr(E), E.stride(0), B, Q, D, _ptr(pair_w), float(neg_weight), _ptr(dE),
                                        _code(grad_dtype), ldd, _ptr(loss), _ptr(aff), _ptr(scratch), _stream()),
                  "head_skipgram")
        return loss, aff, dE[:, :D]
    if not torch.is_tensor(n_valid):
        n_valid = torch.tensor([int(n_valid)], dtype=torch.int32, device=E.device)
    assert n_valid.is_cuda and n_valid.dtype == torch.int32 and n_valid.numel() == 1
    aff = torch.zeros(B, 1 + Q, dtype=torch.float32, device=E.device)
    nat.check(L.gsage_head_skipgram_live(_ptr(E), E.stride(0), B, Q, D, _ptr(pair_w), float(neg_weight), _ptr(n_valid),
                                         _ptr(dE), _code(grad_dtype), ldd, _ptr(loss), _ptr(aff), _ptr(scratch),
                                         _stream()), "head_skipgram_live")
    return loss, aff, dE[:, :D]


class _SkipgramLoss(torch.autograd.Function):
    """forward and backward are the head's two launches, run in forward; backward scales the saved dE."""

    @staticmethod
    def forward(ctx, E, B, Q, pair_w, neg_weight):
        loss, _, dE = skipgram_head(E, B, Q, pair_w, neg_weight)
        ctx.save_for_backward(dE)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        dE, = ctx.saved_tensors
        return dE * g, None, None, None, None


def skipgram_loss(E, B, Q, pair_w, neg_weight=1.0):
    """Skip-gram loss of an unsupervised batch (GSUnsupervised.train_step): E [2B + Q, D] un-normalised encoder rows in
    the order of unsup_batch; differentiable in E.  CUDA: gsage_head_skipgram; CPU: the torch expression (host mode)."""
    if E.is_cuda:
        return _SkipgramLoss.apply(E.float(), int(B), int(Q), pair_w, float(neg_weight))
    return _skipgram_host(E, int(B), int(Q), pair_w, float(neg_weight))[0]


# =============================================================================================
# Retrieval over embeddings: top-k rows by inner product (csrc/gsage_retrieve.hip)
# =============================================================================================
TOPK_EXCLUDE = {"none": 0, "self": 1, "neighbours": 2}
TOPK_K_MAX, TOPK_D_MAX = 128, 1024


def topk_ip_workspace(Q, N, k, splits=0):
    """(bytes of gsage_topk_ip's workspace, the split count used) for Q queries over N rows -- host arithmetic."""
    used = ctypes.c_int64(0)
    nbytes = int(nat.lib().gsage_topk_ip_workspace(int(Q), int(N), int(k), int(splits), ctypes.byref(used)))
    if nbytes < 0:
        raise ValueError("topk_ip: Q = %d, N = %d, k = %d, splits = %d are outside the kernel's limits "
                         "(1 <= k <= %d, N < 2^31, 0 <= splits <= 1024)" % (Q, N, k, splits, TOPK_K_MAX))
    return nbytes, int(used.value)


def _topk_ip_host(table, queries, k, query_ids, csr, exclude):
    """The definition in numpy (host mode): operands rounded as the compute mode sees them, float64 products, a stable
    sort on (-score, id) over the allowed rows."""
    dt = torch_dtype()
    E = table.detach().to(dt).double().numpy()
    Qm = queries.detach().to(dt).double().numpy()
    S = (Qm @ E.T).astype(np.float32)
    Q, N = S.shape
    ids = np.full((Q, k), -1, dtype=np.int64)
    scores = np.full((Q, k), -np.inf, dtype=np.float32)
    qid = None if query_ids is None else query_ids.detach().cpu().numpy().astype(np.int64)
    if exclude == "neighbours":
        rowptr, col = csr.rowptr.cpu().numpy(), csr.col.cpu().numpy()
    for q in range(Q):
        allowed = ~np.isnan(S[q])
        if exclude != "none" and 0 <= qid[q] < N:
            allowed[qid[q]] = False
            if exclude == "neighbours":
                nb = col[rowptr[qid[q]]:rowptr[qid[q] + 1]].astype(np.int64)
                allowed[nb[(nb >= 0) & (nb < N)]] = False
        cand = np.flatnonzero(allowed)
        best = cand[np.argsort(-S[q, cand], kind="stable")][:k]
        ids[q, :best.size] = best
        scores[q, :best.size] = S[q, best]
    return torch.from_numpy(ids), torch.from_numpy(scores)


def topk_ip(table, queries, k, query_ids=None, csr=None, exclude="none", splits=0, workspace=None, out=None):
    """The k rows of `table` [N, D] nearest to each row of `queries` [Q, D] by inner product, under the total order
    (score descending, row id ascending), best first: -> (ids int64 [Q, k], scores fp32 [Q, k]); include/gsage.h,
    "Retrieval over embeddings".  exclude: "none"; "self" (not row query_ids[q]); "neighbours" (neither that row nor
    the columns of row query_ids[q] of `csr`, a store.DeviceCSR).  Fewer than k allowed rows: id -1, score -inf.
    Operands are taken in ops.config.compute_dtype (fp32 data is rounded to bf16 once in the bf16 mode).

    CUDA: gsage_topk_ip (two launches, recordable in a command list when the caller hands in `workspace` -- a uint8
    tensor of topk_ip_workspace(...) bytes -- and `out` = (ids, scores)); the result does not depend on `splits`
    (0 = chosen by the library).  CPU: the same definition in numpy."""
    if exclude not in TOPK_EXCLUDE:
        raise ValueError("topk_ip: exclude must be one of %s, not %r" % (sorted(TOPK_EXCLUDE), exclude))
    if table.dim() != 2 or queries.dim() != 2 or int(table.shape[1]) != int(queries.shape[1]):
        raise ValueError("topk_ip: table [N, D] and queries [Q, D] must share D")
    if not (table.is_floating_point() and queries.is_floating_point()):
        raise ValueError("topk_ip: table and queries must be floating point")
    N, D = int(table.shape[0]), int(table.shape[1])
    Q, k = int(queries.shape[0]), int(k)
    if not 1 <= k <= TOPK_K_MAX:
        raise ValueError("topk_ip: k must be in [1, %d], not %d" % (TOPK_K_MAX, k))
    if not 1 <= D <= TOPK_D_MAX:
        raise ValueError("topk_ip: D must be in [1, %d], not %d" % (TOPK_D_MAX, D))
    if N < 1:
        raise ValueError("topk_ip: the table has no rows")
    if exclude != "none":
        if query_ids is None:
            raise ValueError("topk_ip: exclude=%r needs query_ids" % exclude)
        query_ids = torch.as_tensor(query_ids).to(device=table.device, dtype=torch.int64).contiguous().view(-1)
        if int(query_ids.shape[0]) != Q:
            raise ValueError("topk_ip: %d query_ids for %d queries" % (int(query_ids.shape[0]), Q))
    else:
        query_ids = None
    if exclude == "neighbours":
        if csr is None:
            raise ValueError("topk_ip: exclude='neighbours' needs csr")
        if int(csr.n_rows) < N or csr.rowptr.device != table.device:
            raise ValueError("topk_ip: csr must live on the table's device and have a row for each of its %d rows" % N)
    else:
        csr = None
    if not table.is_cuda:
        if Q == 0:
            return torch.empty(0, k, dtype=torch.int64), torch.empty(0, k, dtype=torch.float32)
        return _topk_ip_host(table, queries, k, query_ids, csr, exclude)
    dev = table.device
    if out is None:
        out = (torch.empty(Q, k, dtype=torch.int64, device=dev), torch.empty(Q, k, dtype=torch.float32, device=dev))
    ids, scores = out
    assert ids.is_contiguous() and scores.is_contiguous() and tuple(ids.shape) == (Q, k) == tuple(scores.shape)
    if Q == 0:
        return ids, scores
    cdt = torch_dtype()

    def operand(t):
        t = t.detach()
        return t if t.dtype == cdt and t.stride(1) == 1 and t.stride(0) >= D else t.to(cdt).contiguous()
    E, Qm = operand(table), operand(queries)
    nbytes, _ = topk_ip_workspace(Q, N, k, splits)
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    nat.check(nat.lib().gsage_topk_ip(_ptr(E), _code(cdt), E.stride(0), N, _ptr(Qm), _code(cdt), Qm.stride(0), Q, D,
                                      _ptr(query_ids), _ptr(csr.rowptr) if csr is not None else None,
                                      _ptr(csr.col) if csr is not None else None, TOPK_EXCLUDE[exclude], k, int(splits),
                                      _ptr(workspace), int(workspace.numel()) * workspace.element_size(), _ptr(ids),
                                      _ptr(scores), _stream()), "topk_ip")
    return ids, scores


# =============================================================================================
# Exact link ranking over embeddings: the rank of a target row among all rows (csrc/gsage_rank.hip)
# =============================================================================================
def rank_ip_workspace(Q, N, splits=0):
    """(bytes of gsage_rank_ip's workspace, the split count used) for Q pairs over N rows -- host arithmetic."""
    used = ctypes.c_int64(0)
    nbytes = int(nat.lib().gsage_rank_ip_workspace(int(Q), int(N), int(splits), ctypes.byref(used)))
    if nbytes < 0:
        raise ValueError("rank_ip: Q = %d, N = %d, splits = %d are outside the kernel's limits "
                         "(Q >= 1, 1 <= N < 2^31, 0 <= splits <= 1024)" % (Q, N, splits))
    return nbytes, int(used.value)


RANK_UNSORTED = ("rank_ip: a row of the filter csr is not strictly ascending (sorted columns, no duplicates) -- "
                 "infer.link_rank builds such a filter from any adjacency")


def _rank_ip_host(table, queries, target_ids, query_ids, csr, exclude):
    """The definition in numpy (host mode): operands rounded as the compute mode sees them, float64 products rounded
    to fp32, the count of allowed rows that beat the target under (score descending, id ascending)."""
    dt = torch_dtype()
    E = table.detach().to(dt).double().numpy()
    Qm = queries.detach().to(dt).double().numpy()
    Q, N = Qm.shape[0], E.shape[0]
    tg = target_ids.numpy()
    qid = None if query_ids is None else query_ids.numpy()
    if exclude == "neighbours":
        rowptr, col = csr.rowptr.cpu().numpy(), csr.col.cpu().numpy()
    rank = np.zeros(Q, dtype=np.int64)
    score = np.full(Q, -np.inf, dtype=np.float32)
    ids = np.arange(N)
    for q in range(Q):
        t = int(tg[q])
        if not 0 <= t < N:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            s = (E @ Qm[q]).astype(np.float32)
        score[q] = s[t]
        allowed = np.ones(N, dtype=bool)
        if exclude != "none" and 0 <= qid[q] < N:
            allowed[qid[q]] = False
            if exclude == "neighbours":
                nb = col[rowptr[qid[q]]:rowptr[qid[q] + 1]].astype(np.int64)
                if nb.size > 1 and (np.diff(nb) <= 0).any():
                    raise ValueError(RANK_UNSORTED)
                allowed[nb[(nb >= 0) & (nb < N)]] = False
        allowed[t] = False
        if np.isnan(s[t]):
            continue
        with np.errstate(invalid="ignore"):
            beats = (s > s[t]) | ((s == s[t]) & (ids < t))
        rank[q] = 1 + int((beats & allowed).sum())
    return torch.from_numpy(rank), torch.from_numpy(score)


def rank_ip(table, queries, target_ids, query_ids=None, csr=None, exclude="none", splits=0, workspace=None, out=None):
    """The rank of row target_ids[q] of `table` [N, D] among all allowed rows for each row of `queries` [Q, D] by inner
    product: rank = 1 + the number of allowed rows j != target that beat it under the total order (score descending,
    row id ascending) -> (rank int64 [Q], score fp32 [Q] = the target's score); include/gsage.h, "Exact link ranking
    over embeddings".  exclude: "none"; "self" (row query_ids[q] does not count); "neighbours" (neither that row nor
    the columns of row query_ids[q] of `csr`, a store.DeviceCSR whose rows are STRICTLY ASCENDING -- ValueError
    otherwise; infer.link_rank builds one from any adjacency).  The target itself is never excluded.  A target whose
    score is NaN is unranked: rank 0.  A target or query id outside the table is an IndexError -- except in the
    recorded form below, which cannot read ids back: there a target outside the table gets rank 0, score -inf.
    Operands are taken in ops.config.compute_dtype (fp32 data is rounded to bf16 once in the bf16 mode).

    CUDA: gsage_rank_ip (two launches, three for "neighbours"; recordable in a command list when the caller hands in
    `workspace` -- a uint8 tensor of rank_ip_workspace(...) bytes -- and `out` = (rank, score); the filter's row
    contract is then reported through csr.err_flag alone); the result does not depend on `splits` (0 = chosen by
    the library).  CPU: the same definition in numpy."""
    if exclude not in TOPK_EXCLUDE:
        raise ValueError("rank_ip: exclude must be one of %s, not %r" % (sorted(TOPK_EXCLUDE), exclude))
    if table.dim() != 2 or queries.dim() != 2 or int(table.shape[1]) != int(queries.shape[1]):
        raise ValueError("rank_ip: table [N, D] and queries [Q, D] must share D")
    if not (table.is_floating_point() and queries.is_floating_point()):
        raise ValueError("rank_ip: table and queries must be floating point")
    N, D = int(table.shape[0]), int(table.shape[1])
    Q = int(queries.shape[0])
    if not 1 <= D <= TOPK_D_MAX:
        raise ValueError("rank_ip: D must be in [1, %d], not %d" % (TOPK_D_MAX, D))
    if N < 1:
        raise ValueError("rank_ip: the table has no rows")
    if not 0 <= int(splits) <= 1024:
        raise ValueError("rank_ip: splits must be in [0, 1024] (0 = chosen by the library), not %d" % int(splits))
    recorded = workspace is not None and out is not None

    def id_vector(ids, name):
        ids = torch.as_tensor(ids)
        if ids.is_floating_point() or ids.dtype == torch.bool:
            raise ValueError("rank_ip: %s must be integers, not %s" % (name, ids.dtype))
        ids = ids.to(device=table.device, dtype=torch.int64).contiguous().view(-1)
        if int(ids.shape[0]) != Q:
            raise ValueError("rank_ip: %d %s for %d queries" % (int(ids.shape[0]), name, Q))
        if not recorded and Q and (int(ids.min()) < 0 or int(ids.max()) >= N):
            raise IndexError("rank_ip: one of the %s is out of range of the %d table rows" % (name, N))
        return ids
    target_ids = id_vector(target_ids, "target_ids")
    if exclude != "none":
        if query_ids is None:
            raise ValueError("rank_ip: exclude=%r needs query_ids" % exclude)
        query_ids = id_vector(query_ids, "query_ids")
    else:
        query_ids = None
    if exclude == "neighbours":
        if csr is None:
            raise ValueError("rank_ip: exclude='neighbours' needs csr")
        if int(csr.n_rows) < N or csr.rowptr.device != table.device:
            raise ValueError("rank_ip: csr must live on the table's device and have a row for each of its %d rows" % N)
    else:
        csr = None
    if not table.is_cuda:
        if Q == 0:
            return torch.empty(0, dtype=torch.int64), torch.empty(0, dtype=torch.float32)
        return _rank_ip_host(table, queries, target_ids, query_ids, csr, exclude)
    dev = table.device
    if out is None:
        out = (torch.empty(Q, dtype=torch.int64, device=dev), torch.empty(Q, dtype=torch.float32, device=dev))
    rank, score = out
    assert rank.is_contiguous() and score.is_contiguous() and tuple(rank.shape) == (Q,) == tuple(score.shape)
    assert rank.dtype == torch.int64 and score.dtype == torch.float32
    if Q == 0:
        return rank, score
    cdt = torch_dtype()

    def operand(t):
        t = t.detach()
        return t if t.dtype == cdt and t.stride(1) == 1 and t.stride(0) >= D else t.to(cdt).contiguous()
    E, Qm = operand(table), operand(queries)
    nbytes, _ = rank_ip_workspace(Q, N, splits)
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    nat.check(nat.lib().gsage_rank_ip(_ptr(E), _code(cdt), E.stride(0), N, _ptr(Qm), _code(cdt), Qm.stride(0), Q, D,
                                      _ptr(target_ids), _ptr(query_ids), _ptr(csr.rowptr) if csr is not None else None,
                                      _ptr(csr.col) if csr is not None else None, TOPK_EXCLUDE[exclude], int(splits),
                                      _ptr(workspace), int(workspace.numel()) * workspace.element_size(), _ptr(rank),
                                      _ptr(score), _ptr(csr.err_flag) if csr is not None else None, _stream()), "rank_ip")
    if csr is not None and not recorded and int(csr.err_flag.item()) != 0:
        csr.err_flag.zero_()
        raise ValueError(RANK_UNSORTED)
    return rank, score


# =============================================================================================
# Linear probe over embeddings: one loss-and-gradient pass of a linear classifier (csrc/gsage_probe.hip)
# =============================================================================================
PROBE_TASKS = {"classification": 0, "multilabel_classification": 1}
PROBE_C_MAX, PROBE_D_MAX = 128, 1024


def probe_task(task):
    """The kernel's code of a probe task; regression has no probe."""
    if task not in PROBE_TASKS:
        raise ValueError("probe: a linear probe is a classifier -- the task must be classification or "
                         "multilabel_classification, not %r" % (task,))
    return PROBE_TASKS[task]


def probe_check(table, ids, targets, C, D, task, who="probe_pass"):
    """Shape and dtype checks shared by probe_pass and infer.linear_probe -> (ids int64 [n], targets) on the table's
    device: int64 [n] for classification, fp32 [n, >= C] (unit column stride) for multilabel_classification."""
    code = probe_task(task)
    if not torch.is_tensor(table) or table.dim() != 2 or not table.is_floating_point():
        raise ValueError("%s: the table must be a [N, D] float tensor" % who)
    if int(table.shape[1]) != D:
        raise ValueError("%s: the table has %d columns, the classifier D = %d" % (who, int(table.shape[1]), D))
    if not 1 <= C <= PROBE_C_MAX:
        raise ValueError("%s: the number of classes must be in [1, %d], not %d (one workgroup holds every class of a row)"
                         % (who, PROBE_C_MAX, C))
    if not 1 <= D <= PROBE_D_MAX:
        raise ValueError("%s: D must be in [1, %d], not %d" % (who, PROBE_D_MAX, D))
    ids = torch.as_tensor(ids)
    if ids.is_floating_point() or ids.dtype == torch.bool:
        raise ValueError("%s: node ids must be integers, not %s" % (who, ids.dtype))
    ids = ids.to(table.device).long().contiguous().view(-1)
    n = int(ids.shape[0])
    if n < 1:
        raise ValueError("%s: no rows to fit on" % who)
    targets = torch.as_tensor(targets).to(table.device)
    if code == 0:
        if targets.is_floating_point() or targets.dtype == torch.bool:
            raise ValueError("%s: classification targets must be integer class ids, not %s" % (who, targets.dtype))
        if targets.numel() != n or targets.dim() > 2 or (targets.dim() == 2 and int(targets.shape[1]) != 1):
            raise ValueError("%s: classification targets must have shape [%d] (one class id per row), not %s"
                             % (who, n, tuple(targets.shape)))
        targets = targets.long().contiguous().view(-1)
    else:
        if not targets.is_floating_point():
            raise ValueError("%s: multilabel targets must be floating point (values in [0, 1]), not %s" % (who, targets.dtype))
        if targets.dim() != 2 or int(targets.shape[0]) != n or int(targets.shape[1]) < C:
            raise ValueError("%s: multilabel targets must have shape [%d, %d], not %s" % (who, n, C, tuple(targets.shape)))
        if targets.dtype != torch.float32 or targets.stride(1) != 1 or targets.stride(0) < C:
            targets = targets.float().contiguous()
    return ids, targets


def probe_scratch(n, C, D, splits=0):
    """(floats of gsage_probe_pass's partial buffer, its rows S) -- host arithmetic."""
    floats = int(nat.lib().gsage_probe_pass_scratch(int(n), int(C), int(D), int(splits)))
    if floats < 0:
        raise ValueError("probe_pass: n = %d, C = %d, D = %d, splits = %d are outside the kernel's limits "
                         "(C <= %d, D <= %d, n < 2^31, 0 <= splits <= 1024)" % (n, C, D, splits, PROBE_C_MAX, PROBE_D_MAX))
    return floats, floats // (C * D + C + 1)


def probe_operand(table, D):
    """The table as the compute mode sees it (fp32 data is rounded to bf16 once in the bf16 mode)."""
    cdt = torch_dtype()
    t = table.detach()
    return t if t.dtype == cdt and t.stride(1) == 1 and t.stride(0) >= D else t.to(cdt).contiguous()


def _probe_pass_host(table, ids, targets, W, b, code):
    """The definition in float64 torch (host mode): operands rounded as the compute mode sees them."""
    dt = torch_dtype()
    C, D = int(W.shape[0]), int(W.shape[1])
    X = table.detach()[ids].to(dt).double()
    z = X @ W.detach().to(dt).double().t() + b.detach().double()
    n = int(ids.shape[0])
    if code == 0:
        lse = torch.logsumexp(z, dim=1)
        loss = (lse - z.gather(1, targets.view(-1, 1)).view(-1)).mean()
        G = torch.softmax(z, dim=1)
        G[torch.arange(n), targets] -= 1.0
    else:
        y = targets[:, :C].double()
        loss = ((F.softplus(z) - y * z).sum(dim=1) / C).mean()
        G = (torch.sigmoid(z) - y) / C
    return loss.float(), (G.t() @ X / n).float(), (G.sum(dim=0) / n).float()


def probe_pass(table, ids, targets, W, b, task, splits=0):
    """One full-batch loss-and-gradient evaluation of the linear classifier z = table[ids] @ W~^T + b ->
    (loss fp32 scalar, dW fp32 [C, D], db fp32 [C]); include/gsage.h, "Linear probe over embeddings".
    task: "classification" (targets int64 [n], F.cross_entropy) or "multilabel_classification" (targets float
    [n, >= C], F.multilabel_soft_margin_loss).  W [C, D], b [C]: fp32 masters.  Operands are taken in
    ops.config.compute_dtype (fp32 data is rounded to bf16 once in the bf16 mode, W when it is staged).

    CUDA: gsage_probe_pass + gsage_finalize_grads (three launches); `splits` = partial rows (0 = chosen by the
    library), bit-identical from call to call.  CPU: the same definition in float64 torch."""
    if not (torch.is_tensor(W) and W.dim() == 2 and W.dtype == torch.float32 and torch.is_tensor(b)
            and b.dtype == torch.float32 and tuple(b.shape) == (int(W.shape[0]),)):
        raise ValueError("probe_pass: W must be fp32 [C, D] and b fp32 [C]")
    C, D = int(W.shape[0]), int(W.shape[1])
    code = probe_task(task)
    ids, targets = probe_check(table, ids, targets, C, D, task)
    if not table.is_cuda:
        return _probe_pass_host(table, ids, targets, W, b, code)
    from .engine.common import _ReduceDesc
    dev, f32 = table.device, torch.float32
    E = probe_operand(table, D)
    n, width = int(ids.shape[0]), C * D + C + 1
    floats, S = probe_scratch(n, C, D, splits)
    Wc, bc = W.detach().contiguous(), b.detach().contiguous()
    partial = torch.empty(floats, dtype=f32, device=dev)
    loss = torch.zeros(1, dtype=f32, device=dev)
    nat.check(nat.lib().gsage_probe_pass(_ptr(E), _code(E.dtype), E.stride(0), int(E.shape[0]), _ptr(ids), n,
                                         _ptr(targets), code, targets.stride(0) if code else 0, _ptr(Wc), _ptr(bc), C, D,
                                         int(splits), _ptr(partial), _ptr(loss), _stream()), "probe_pass")
    desc = _ReduceDesc(partial.data_ptr(), width, 0, S, 1, width - 1, width)
    descs = torch.frombuffer(bytearray(bytes(desc)), dtype=torch.uint8).to(dev)
    flat = torch.empty(width - 1, dtype=f32, device=dev)
    sq = torch.empty(nat.lib().gsage_finalize_partials(1, width - 1), dtype=f32, device=dev)
    nat.check(nat.lib().gsage_finalize_grads(_ptr(descs), 1, width - 1, _ptr(flat), _ptr(sq), None, None, 0, None, 0,
                                             _stream()), "finalize_grads")
    return loss[0], flat[:C * D].view(C, D), flat[C * D:]


# =============================================================================================
# K-means over embeddings: the assignment-and-accumulate pass and the centroid update (csrc/gsage_kmeans.hip)
# =============================================================================================
KMEANS_K_MAX, KMEANS_D_MAX = 128, 1024


class KMeansPass(tuple):
    """What kmeans_pass returns: (sums, counts, inertia, changed, labels[, dist]), and in `.partial` the [S, K D + K + 2]
    rows [sums | counts | inertia | changed] they were summed from -- what kmeans_update takes."""
    partial = None


def kmeans_check(table, ids, K, D, who="kmeans_pass"):
    """Shape and dtype checks shared by kmeans_pass and infer.kmeans -> ids int64 [n] on the table's device."""
    if not torch.is_tensor(table) or table.dim() != 2 or not table.is_floating_point():
        raise ValueError("%s: the table must be a [N, D] float tensor" % who)
    if int(table.shape[1]) != D:
        raise ValueError("%s: the table has %d columns, the centroids D = %d" % (who, int(table.shape[1]), D))
    if not 1 <= K <= KMEANS_K_MAX:
        raise ValueError("%s: the number of clusters must be in [1, %d], not %d (one workgroup holds every cluster of a row)"
                         % (who, KMEANS_K_MAX, K))
    if not 1 <= D <= KMEANS_D_MAX:
        raise ValueError("%s: D must be in [1, %d], not %d" % (who, KMEANS_D_MAX, D))
    ids = torch.as_tensor(ids)
    if ids.is_floating_point() or ids.dtype == torch.bool:
        raise ValueError("%s: node ids must be integers, not %s" % (who, ids.dtype))
    ids = ids.to(table.device).long().contiguous().view(-1)
    if int(ids.shape[0]) < 1:
        raise ValueError("%s: no rows to cluster" % who)
    return ids


def kmeans_scratch(n, K, D, splits=0):
    """(floats of gsage_kmeans_pass's partial buffer, its rows S) -- host arithmetic."""
    floats = int(nat.lib().gsage_kmeans_pass_scratch(int(n), int(K), int(D), int(splits)))
    if floats < 0:
        raise ValueError("kmeans_pass: n = %d, K = %d, D = %d, splits = %d are outside the kernel's limits (K <= %d, "
                         "D <= %d, n < 2^31, 0 <= splits <= 1024, fewer than 2^24 rows per split)"
                         % (n, K, D, splits, KMEANS_K_MAX, KMEANS_D_MAX))
    return floats, floats // (K * D + K + 2)


def _kmeans_centroid_args(centroids, bias, who):
    if not (torch.is_tensor(centroids) and centroids.dim() == 2 and centroids.dtype == torch.float32
            and torch.is_tensor(bias) and bias.dtype == torch.float32 and tuple(bias.shape) == (int(centroids.shape[0]),)):
        raise ValueError("%s: centroids must be fp32 [K, D] and bias fp32 [K]" % who)
    return int(centroids.shape[0]), int(centroids.shape[1])


def _kmeans_pass_host(table, ids, centroids, bias, k_live, labels_in, accumulate, want_dist):
    """The definition in numpy float64 (host mode): operands rounded as the compute mode sees them."""
    dt = torch_dtype()
    K, D = int(centroids.shape[0]), int(centroids.shape[1])
    N = int(table.shape[0])
    ok = ((ids >= 0) & (ids < N)).numpy()
    X = table.detach()[ids.clamp(0, N - 1)].to(dt).double().numpy() * ok[:, None]     # an id outside reads as a zero row
    Cr = centroids.detach().to(dt).double().numpy()
    s = X @ Cr[:k_live].T + bias.detach().double().numpy()[:k_live]
    a = np.argmax(s, axis=1)                                                          # the first of equal scores
    n = X.shape[0]
    d2 = np.maximum(0.0, (X * X).sum(axis=1) - 2.0 * s[np.arange(n), a])
    labels = torch.from_numpy(a.astype(np.int32))
    dist = torch.from_numpy(d2.astype(np.float32))
    if not accumulate:
        return (labels, dist) if want_dist else (labels,)
    sums = np.zeros((K, D))
    np.add.at(sums, a, X)
    counts = np.bincount(a, minlength=K)
    changed = int((labels_in.numpy() != a).sum()) if labels_in is not None else 0
    row = np.concatenate([sums.reshape(-1), counts.astype(np.float64), [d2.sum(), float(changed)]])
    out = (torch.from_numpy(sums.astype(np.float32)), torch.from_numpy(counts.astype(np.int64)),
           torch.tensor(d2.sum(), dtype=torch.float32), torch.tensor(changed, dtype=torch.int64), labels)
    res = KMeansPass(out + ((dist,) if want_dist else ()))
    res.partial = torch.from_numpy(row.astype(np.float32)).view(1, -1)
    return res


def kmeans_pass(table, ids, centroids, bias, k_live=None, labels_in=None, splits=0, want_dist=False, accumulate=True):
    """One assignment-and-accumulate pass of Lloyd's algorithm over the rows `ids` of `table` ->
    KMeansPass (sums fp32 [K, D], counts int64 [K], inertia fp32 scalar, changed int64 scalar, labels int32 [n]
    [, dist fp32 [n]]); include/gsage.h, "K-means over embeddings".  centroids fp32 [K, D], bias fp32 [K] (-1/2 |c|^2:
    kmeans_update writes it); only the clusters below k_live (default K) compete; labels_in int32 [n]: `changed` counts
    the rows whose label differs from it.  Operands are taken in ops.config.compute_dtype (fp32 data is rounded to
    bf16 once in the bf16 mode).  accumulate=False: labels only -> (labels[, dist]).

    CUDA: ONE launch of gsage_kmeans_pass; `splits` = partial rows (0 = chosen by the library); the S rows are in
    `.partial` and the returned sums are their float64 torch sum.  Labels do not depend on splits; everything is
    bit-identical from call to call.  CPU: the same definition in numpy float64 (one partial row)."""
    K, D = _kmeans_centroid_args(centroids, bias, "kmeans_pass")
    ids = kmeans_check(table, ids, K, D)
    n = int(ids.shape[0])
    k_live = K if k_live is None else int(k_live)
    if not 1 <= k_live <= K:
        raise ValueError("kmeans_pass: k_live must be in [1, K = %d], not %d" % (K, k_live))
    if labels_in is not None:
        if not torch.is_tensor(labels_in) or labels_in.dtype != torch.int32 or tuple(labels_in.shape) != (n,):
            raise ValueError("kmeans_pass: labels_in must be int32 [%d]" % n)
        labels_in = labels_in.to(table.device).contiguous()
    if not table.is_cuda:
        return _kmeans_pass_host(table, ids, centroids, bias, k_live, labels_in, accumulate, want_dist)
    dev, f32 = table.device, torch.float32
    E = probe_operand(table, D)
    Cc, bc = centroids.detach().contiguous(), bias.detach().contiguous()
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    dist = torch.empty(n, dtype=f32, device=dev) if want_dist else None
    partial = None
    if accumulate:
        floats, S = kmeans_scratch(n, K, D, splits)
        partial = torch.empty(floats, dtype=f32, device=dev)
    nat.check(nat.lib().gsage_kmeans_pass(_ptr(E), _code(E.dtype), E.stride(0), int(E.shape[0]), _ptr(ids), n, _ptr(Cc),
                                          _ptr(bc), K, D, k_live, _ptr(labels_in) if labels_in is not None else None,
                                          int(splits), _ptr(partial) if accumulate else None, _ptr(labels),
                                          _ptr(dist) if want_dist else None, _stream()), "kmeans_pass")
    if not accumulate:
        return (labels, dist) if want_dist else (labels,)
    partial = partial.view(S, K * D + K + 2)
    tot = partial.double().sum(dim=0)
    out = (tot[:K * D].view(K, D).float(), tot[K * D:K * D + K].round().long(), tot[K * D + K].float(),
           tot[K * D + K + 1].round().long(), labels)
    res = KMeansPass(out + ((dist,) if want_dist else ()))
    res.partial = partial
    return res


def kmeans_update(centroids, bias, partial=None, spherical=False, history=None):
    """The update step of Lloyd's algorithm, IN PLACE on centroids fp32 [K, D] and bias fp32 [K] (gsage_kmeans_update):
    with `partial` (kmeans_pass(...).partial, [S, K D + K + 2]) every cluster with count > 0 becomes sums / count (then
    unit length if spherical), an empty cluster keeps its centroid; bias = -1/2 |c~|^2 in the compute mode's rounding (0
    if spherical).  partial None: only the bias, from the centroids as they are.
    history: (inertia fp32 [cap], changed int64 [cap], empty int32 [cap], index int64 [1]) -- slot index[0] is written
    and index ticked; None: one fresh slot, returned as (inertia, changed, empty); otherwise -> None.

    CUDA: one launch.  CPU: the same definition in numpy float64."""
    K, D = _kmeans_centroid_args(centroids, bias, "kmeans_update")
    if not (centroids.is_contiguous() and bias.is_contiguous()):
        raise ValueError("kmeans_update: centroids and bias are updated in place and must be contiguous")
    if not 1 <= K <= KMEANS_K_MAX or not 1 <= D <= KMEANS_D_MAX:
        raise ValueError("kmeans_update: K must be in [1, %d] and D in [1, %d], not %d and %d"
                         % (KMEANS_K_MAX, KMEANS_D_MAX, K, D))
    dev = centroids.device
    dt = torch_dtype()
    spherical = bool(spherical)
    S = 0
    if partial is not None:
        if not torch.is_tensor(partial) or partial.dtype != torch.float32 or partial.dim() != 2 or \
                int(partial.shape[1]) != K * D + K + 2 or not partial.is_contiguous() or partial.device != dev:
            raise ValueError("kmeans_update: partial must be fp32 [S, %d] (kmeans_pass(...).partial)" % (K * D + K + 2))
        S = int(partial.shape[0])
        if history is None:
            history = (torch.zeros(1, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
                       torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
            slot = 0
        else:
            slot = None
        ih, chh, eh, index = history
        cap = int(ih.shape[0])
        if not (ih.dtype == torch.float32 and chh.dtype == torch.int64 and eh.dtype == torch.int32
                and index.dtype == torch.int64 and int(chh.shape[0]) == cap and int(eh.shape[0]) == cap and cap >= 1):
            raise ValueError("kmeans_update: history must be (fp32 [cap], int64 [cap], int32 [cap], int64 [1])")
    if not centroids.is_cuda:
        Cd = centroids.double().numpy()
        if partial is not None:
            P = partial.double().numpy()
            counts = np.rint(P[:, K * D:K * D + K]).astype(np.int64).sum(axis=0)
            sums = P[:, :K * D].sum(axis=0).reshape(K, D)
            live = counts > 0
            Cd[live] = sums[live] / counts[live][:, None]
            if spherical:
                norm = np.linalg.norm(Cd, axis=1)
                scale = live & (norm > 0)
                Cd[scale] /= norm[scale][:, None]
            centroids[torch.from_numpy(live)] = torch.from_numpy(Cd[live].astype(np.float32))
            at = int(index[0])
            if 0 <= at < cap:
                ih[at] = float(P[:, K * D + K].sum())
                chh[at] = int(np.rint(P[:, K * D + K + 1]).sum())
                eh[at] = int((~live).sum())
            index += 1
        Cr = centroids.to(dt).double().numpy()
        bias.copy_(torch.from_numpy((np.zeros(K) if spherical else -0.5 * (Cr * Cr).sum(axis=1)).astype(np.float32)))
    else:
        args = (None, None, None, None, 0) if partial is None else (_ptr(ih), _ptr(chh), _ptr(eh), _ptr(index), cap)
        nat.check(nat.lib().gsage_kmeans_update(_ptr(partial) if partial is not None else None, S, K, D, _code(dt),
                                                int(spherical), _ptr(centroids), _ptr(bias), *args, _stream()),
                  "kmeans_update")
    if partial is None or slot is None:
        return None
    return ih[0], chh[0], eh[0]


# =============================================================================================
# The head for a wide class dimension: normalize + fc + loss + gradients in one launch (csrc/gsage_head_wide.hip)
# =============================================================================================
WIDE_HEAD_C_MAX, WIDE_HEAD_D_MAX = 128, 1024


def wide_head_scratch(B, C, D):
    """(floats of gsage_head_wide's scratch, its partial rows) -- host arithmetic."""
    floats = int(nat.lib().gsage_head_wide_scratch(int(B), int(C), int(D)))
    if floats < 0:
        raise ValueError("wide_head: B = %d, C = %d, D = %d are outside the kernel's limits (B >= 1, C <= %d, D <= %d)"
                         % (B, C, D, WIDE_HEAD_C_MAX, WIDE_HEAD_D_MAX))
    return floats, floats // (C * D + C + 1)


def _wide_head_host(E, W, b, targets, code, bv, dE_dtype):
    """The definition in torch float32 (host mode)."""
    C = int(W.shape[0])
    Ed = E.detach().float().clone().requires_grad_(True)
    Wd, bd = W.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    preds = F.normalize(Ed, dim=1) @ Wd.t() + bd
    if targets is None:
        return preds.detach(), None, None, None, None
    live = preds[:bv]
    if code == 0:
        loss = (torch.logsumexp(live, dim=1) - live.gather(1, targets[:bv].view(-1, 1)).view(-1)).sum() / bv
    else:
        y = targets[:bv, :C].float()
        loss = ((F.softplus(live) - y * live).sum(dim=1) / C).sum() / bv
    dE, dW, db = torch.autograd.grad(loss, [Ed, Wd, bd])
    return preds.detach(), loss.detach(), dE.to(dE_dtype), dW, db


def wide_head(E, W, b, targets, task, n_valid=None, dE_dtype=None):
    """gsage_head_wide: z = normalize(E), preds = z W^T + b, the task's loss over the first n_valid rows and its
    gradients -> (preds fp32 [B, C], loss fp32 scalar, dE [B, D], dW fp32 [C, D], db fp32 [C]); include/gsage.h.
    E fp32 [B, D] (unit column stride), W fp32 [C, D], b fp32 [C]; task: "classification" (targets int64 [B],
    F.cross_entropy) or "multilabel_classification" (targets fp32 [B, >= C], F.multilabel_soft_margin_loss), the codes
    of PROBE_TASKS.  1 <= C <= 128, 1 <= D <= 1024.  n_valid (an int in [1, B], default B): rows past it are padding --
    predictions, no loss, zero rows of dE.  dE_dtype: torch.float32 (default) or torch.bfloat16.
    targets None: forward only -> (preds, None, None, None, None).

    CUDA: one launch plus the deterministic sum of its partial rows.  CPU: the same definition in torch float32."""
    code = probe_task(task)
    if not (torch.is_tensor(E) and E.dim() == 2 and E.dtype == torch.float32):
        raise ValueError("wide_head: E must be an fp32 [B, D] tensor")
    if not (torch.is_tensor(W) and W.dim() == 2 and W.dtype == torch.float32):
        raise ValueError("wide_head: W must be an fp32 [C, D] tensor")
    C, D = int(W.shape[0]), int(W.shape[1])
    B = int(E.shape[0])
    if not (torch.is_tensor(b) and b.dtype == torch.float32 and tuple(b.shape) == (C,)):
        raise ValueError("wide_head: b must be an fp32 [%d] tensor (one bias per row of W)" % C)
    if int(E.shape[1]) != D:
        raise ValueError("wide_head: E has %d columns, W %d" % (int(E.shape[1]), D))
    if not 1 <= C <= WIDE_HEAD_C_MAX:
        raise ValueError("wide_head: W must have between 1 and %d rows (classes), not %d" % (WIDE_HEAD_C_MAX, C))
    if not 1 <= D <= WIDE_HEAD_D_MAX:
        raise ValueError("wide_head: W must have between 1 and %d columns, not %d" % (WIDE_HEAD_D_MAX, D))
    if B < 1:
        raise ValueError("wide_head: E has no rows")
    if W.device != E.device or b.device != E.device:
        raise ValueError("wide_head: W and b must be on E's device")
    dE_dtype = torch.float32 if dE_dtype is None else dE_dtype
    if dE_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("wide_head: dE_dtype must be torch.float32 or torch.bfloat16, not %s" % (dE_dtype,))
    bv = B if n_valid is None else int(n_valid)
    if not 1 <= bv <= B:
        raise ValueError("wide_head: n_valid must be in [1, %d], not %d" % (B, bv))
    if targets is not None:
        if not torch.is_tensor(targets) or targets.device != E.device:
            raise ValueError("wide_head: targets must be a tensor on E's device")
        if code == 0:
            if targets.dtype != torch.int64 or targets.numel() != B or targets.dim() > 2:
                raise ValueError("wide_head: classification targets must be int64 [%d], not %s %s"
                                 % (B, targets.dtype, tuple(targets.shape)))
            targets = targets.contiguous().view(-1)
        else:
            if targets.dtype != torch.float32 or targets.dim() != 2 or int(targets.shape[0]) != B or \
                    int(targets.shape[1]) < C:
                raise ValueError("wide_head: multilabel targets must be fp32 [%d, >= %d], not %s %s"
                                 % (B, C, targets.dtype, tuple(targets.shape)))
            if targets.stride(1) != 1 or targets.stride(0) < C:
                targets = targets.contiguous()
    if not E.is_cuda:
        return _wide_head_host(E, W, b, targets, code, bv, dE_dtype)
    dev, f32 = E.device, torch.float32
    Ec = E.detach()
    if Ec.stride(1) != 1 or Ec.stride(0) < D:
        Ec = Ec.contiguous()
    Wc, bc = W.detach().contiguous(), b.detach().contiguous()
    preds = torch.empty(B, C, dtype=f32, device=dev)
    L = nat.lib()
    if targets is None:
        nat.check(L.gsage_head_wide(_ptr(Ec), Ec.stride(0), _ptr(Wc), _ptr(bc), None, code, 0, B, C, D, _ptr(preds),
                                    None, nat.F32, 0, None, None, None, None, None, 0, _stream()), "head_wide")
        return preds, None, None, None, None
    floats, _rows = wide_head_scratch(B, C, D)
    scratch = torch.empty(floats, dtype=f32, device=dev)
    dE = torch.empty(B, D, dtype=dE_dtype, device=dev)
    dW, db = torch.empty(C, D, dtype=f32, device=dev), torch.empty(C, dtype=f32, device=dev)
    loss = torch.empty(1, dtype=f32, device=dev)
    nv = None
    if bv != B:
        nv = torch.full((1,), bv, dtype=torch.int32, device=dev)
        nat.check(L.gsage_head_n_valid_next(_ptr(nv)), "head_n_valid_next")
    nat.check(L.gsage_head_wide(_ptr(Ec), Ec.stride(0), _ptr(Wc), _ptr(bc), _ptr(targets), code,
                                targets.stride(0) if code else 0, B, C, D, _ptr(preds), _ptr(dE), _code(dE_dtype),
                                dE.stride(0), _ptr(dW), _ptr(db), _ptr(loss), _ptr(scratch), None, 0, _stream()),
              "head_wide")
    return preds, loss[0], dE, dW, db


# =============================================================================================
# Graph propagation: one step of label / residual propagation over a CSR adjacency (csrc/gsage_propagate.hip)
# =============================================================================================
PROP_NORMS = {"sym": 0, "row": 1, "col": 2}
PROP_C_MAX = 1024


def propagate_norm(norm):
    if norm not in PROP_NORMS:
        raise ValueError("propagate: norm must be one of %s, not %r" % (sorted(PROP_NORMS), norm))
    return PROP_NORMS[norm]


def propagate_scales(rowptr, n_rows, norm):
    """(a, b) fp32 [n_rows] of propagate_step from the row degrees (include/gsage.h, "Graph propagation"): "sym"
    a = b = deg^-1/2, "row" a = 1 / deg, b = 1, "col" a = 1, b = 1 / deg; 0 where deg == 0.  CUDA: one launch
    (gsage_propagate_scales); CPU: the same arithmetic in torch."""
    code, n = propagate_norm(norm), int(n_rows)
    dev = rowptr.device
    if rowptr.is_cuda:
        a, b = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2))
        nat.check(nat.lib().gsage_propagate_scales(_ptr(rowptr), n, code, _ptr(a), _ptr(b), _stream()), "propagate_scales")
        return a, b
    deg = (rowptr[1:n + 1] - rowptr[:n]).float()
    one, zero = torch.ones(n), torch.zeros(n)
    inv = torch.where(deg > 0, 1.0 / deg.clamp(min=1), zero)
    if code == 0:
        s = torch.where(deg > 0, 1.0 / torch.sqrt(deg.clamp(min=1)), zero)
        return s, s.clone()
    return (inv, one) if code == 1 else (one, inv)


def _propagate_step_host(adj, y, base, a, b, alpha, beta, lo, hi, C, out, yout):
    n = int(adj.n_rows)
    rowptr, col = adj.rowptr[:n + 1], adj.col.long()
    deg = rowptr[1:] - rowptr[:-1]
    dst = torch.repeat_interleave(torch.arange(n, dtype=torch.int64), deg)
    ok = (col >= 0) & (col < n)
    if not bool(ok.all()):
        adj.err_flag.fill_(1)                              # the id contributes nothing
    acc = torch.zeros(n, C, dtype=torch.float32).index_add_(0, dst[ok], y[col[ok], :C].float())
    if a is not None:
        acc = a.view(-1, 1) * acc
    r = alpha * acc
    if base is not None:
        r = beta * base[:n, :C].float() + r
    r = torch.minimum(torch.maximum(r, torch.tensor(lo)), torch.tensor(hi))
    if out is not None:
        out[:n, :C] = r
    if yout is not None:
        yout[:n, :C] = r if b is None else b.view(-1, 1) * r
    return out, yout


def propagate_step(adj, plan, y, base, a, b, alpha, beta, lo, hi, C, out=None, yout=None, partials=None):
    """One propagation step over the rows of `adj` (a store.DeviceCSR) -- include/gsage.h, "Graph propagation":

        acc[v]  = sum of y[u, :C] over the stored neighbours u of v        (an empty row: 0; an id outside the graph: 0,
                                                                            and adj.err_flag is raised)
        out[v]  = min(max(beta * base[v] + alpha * a[v] * acc[v], lo), hi)
        yout[v] = b[v] * out[v]

    y: fp32 [n_rows, >= round_up(C, 4)] (the pre-scaled iterate), base likewise or None with beta == 0; a, b: fp32
    [n_rows] or None (= 1); out / yout: fp32 [n_rows, >= C] views with 16-byte rows, one of them may be None; `plan`:
    infer.plan(adj); partials: fp32 [n_slices, gsage_segment_reduce_ldp(C)] scratch (allocated when None).
    CUDA: gsage_propagate, two launches, no synchronisation, recordable in a command list.  CPU: the same definition in
    torch (host mode).  -> (out, yout)."""
    C = int(C)
    if out is None and yout is None:
        raise ValueError("propagate_step: out and yout are both None")
    if base is None and beta != 0:
        raise ValueError("propagate_step: base is None and beta is not 0")
    if not y.is_cuda:
        if not 1 <= C <= PROP_C_MAX:
            raise ValueError("propagate_step: the width must lie in [1, %d], not %d" % (PROP_C_MAX, C))
        return _propagate_step_host(adj, y, base, a, b, float(alpha), float(beta), float(lo), float(hi), C, out, yout)
    n = int(adj.n_rows)
    for t in (y, base, out, yout):
        assert t is None or (t.dtype == torch.float32 and t.stride(1) == 1 and int(t.shape[0]) >= n)
    lib = nat.lib()
    ldp = int(lib.gsage_segment_reduce_ldp(C))
    if partials is None and plan["n_slices"]:
        partials = torch.empty(plan["n_slices"], ldp, dtype=torch.float32, device=y.device)

    def ld(t):
        return 0 if t is None else t.stride(0)
    nat.check(lib.gsage_propagate(
        _ptr(y), ld(y), _ptr(base), ld(base), _ptr(a), _ptr(b), float(alpha), float(beta), float(lo), float(hi), C,
        _ptr(adj.rowptr), _ptr(adj.col), n, _ptr(plan["order"]), plan["n_short"], _ptr(plan["slices"]), plan["n_slices"],
        _ptr(plan["long_rows"]), plan["n_long"], plan["slice_len"], _ptr(partials), ldp if partials is None else
        partials.stride(0), _ptr(out), ld(out), _ptr(yout), ld(yout), _ptr(adj.err_flag), _stream()), "propagate")
    return out, yout


# =============================================================================================
# Graph construction: edge list -> CSR, transpose, symmetrise (csrc/gsage_build.hip; include/gsage.h, "Graph
# construction").  The GPU pipeline and the numpy host mode state one definition and agree bit for bit.
# =============================================================================================
EDGE_ORDERS = ("insertion", "id", "time")
EDGE_DUPLICATES = ("first", "sum", "all")
_OUT_OF_RANGE = "sampler: node id out of range of the adjacency"


def edges_check(E, n_nodes, weighted, timed, directed, order, duplicates, who="edges_to_csr"):
    """(order, duplicates) with the defaults filled in; ValueError, one sentence each, for a combination the definition
    does not have and for shapes outside the limits -- from the shapes alone, before anything is allocated."""
    if weighted and timed:
        raise ValueError("%s: weights and times together are not supported" % who)
    if order is None:
        order = "time" if timed else "insertion"
    if duplicates is None:
        duplicates = "all" if timed else "first"
    if order not in EDGE_ORDERS:
        raise ValueError("%s: order must be one of %s, not %r" % (who, ", ".join(EDGE_ORDERS), order))
    if duplicates not in EDGE_DUPLICATES:
        raise ValueError("%s: duplicates must be one of %s, not %r" % (who, ", ".join(EDGE_DUPLICATES), duplicates))
    if timed and (order != "time" or duplicates != "all"):
        raise ValueError("%s: with edge times the rows are in time order and keep every record (order='time', "
                         "duplicates='all')" % who)
    if order == "time" and not timed:
        raise ValueError("%s: order='time' needs edge times" % who)
    if duplicates == "sum" and not weighted:
        raise ValueError("%s: duplicates='sum' needs edge weights" % who)
    if n_nodes < 0 or E < 0:
        raise ValueError("%s: negative size" % who)
    if (E if directed else 2 * E) >= 2 ** 31:
        raise ValueError("%s: %d records; the record count must stay below 2^31 (the sort carries int32 positions)"
                         % (who, E if directed else 2 * E))
    if 2 * max(int(n_nodes).bit_length(), 1) > 62:
        raise ValueError("%s: %d rows; a packed (row, neighbour) key must fit 62 bits" % (who, n_nodes + 1))
    return order, duplicates


def _edges_rows_host(rrow, rnbr, ridx, n_lim, order, duplicates, w, t):
    """Host mode of the build over the EXISTING records (rrow, rnbr: 0-based int64; ridx: their record indices,
    ascending; w / t: their payloads or None) -> (counts int64 [n_lim], neighbour ids, payload) in final order."""
    if duplicates != "all" and rrow.size:
        o = np.lexsort((ridx, rnbr, rrow))
        r_, n_ = rrow[o], rnbr[o]
        first = np.ones(o.size, dtype=bool)
        first[1:] = (r_[1:] != r_[:-1]) | (n_[1:] != n_[:-1])
        starts = np.flatnonzero(first)
        if duplicates == "sum":
            wo = w[o]
            lens = np.diff(np.append(starts, o.size))
            s = wo[starts].astype(np.float32)
            for k in range(1, int(lens.max())):              # record order inside a run, sequentially, in fp32
                m = lens > k
                s[m] = s[m] + wo[starts[m] + k]
            w = np.zeros(rrow.size, dtype=np.float32)
            w[o[starts]] = s
        kept = np.sort(o[starts])
        rrow, rnbr, ridx = rrow[kept], rnbr[kept], ridx[kept]
        w = None if w is None else w[kept]
        t = None if t is None else t[kept]
    if order == "insertion":
        o = np.lexsort((ridx, rrow))
    elif order == "id":
        o = np.lexsort((ridx, rnbr, rrow))
    else:
        o = np.lexsort((ridx, t, rrow))
    counts = np.bincount(rrow, minlength=n_lim).astype(np.int64) if rrow.size else np.zeros(n_lim, dtype=np.int64)
    pay = w[o] if w is not None else (t[o] if t is not None else None)
    return counts, rnbr[o], pay


def _edges_sort(keys, n, bits):
    """gsage_sort_rows over keys int64 [n] (n > 0): (keys sorted, original positions int32), stable"""
    lib = nat.lib()
    nb = int(lib.gsage_sort_rows_temp_bytes(n, bits))
    assert nb > 0, "gsage_sort_rows_temp_bytes failed"
    temp = torch.empty(nb, dtype=torch.uint8, device=keys.device)
    ks = torch.empty(n, dtype=torch.int64, device=keys.device)
    ps = torch.empty(n, dtype=torch.int32, device=keys.device)
    nat.check(lib.gsage_sort_rows(_ptr(keys), n, 0, 0, bits, _ptr(ks), _ptr(ps), _ptr(temp), nb, _stream()), "sort_rows")
    return ks, ps


def _edges_rows_device(keys, R, b, n_lim, base, col_add, order, duplicates, weight, time, eshift, err_flag):
    """The stages behind the expand kernel (include/gsage.h, "The pipeline") -> (rowptr, col, max_deg, payload)."""
    lib, dev, s = nat.lib(), keys.device, _stream()
    rowptr = torch.empty(base + n_lim + 1, dtype=torch.int64, device=dev)
    col = torch.empty(R, dtype=torch.int32, device=dev)
    w = torch.empty(R, dtype=torch.float32, device=dev) if weight is not None else None
    t = torch.empty(R, dtype=torch.int64, device=dev) if time is not None else None
    wsum = torch.empty(R, dtype=torch.float32, device=dev) if duplicates == "sum" else None
    summed = wsum is not None
    perm = incl = None
    if order == "id":
        ks, ps = _edges_sort(keys, R, 2 * b)
        if duplicates != "all":
            flag = torch.empty(R, dtype=torch.int32, device=dev)
            nat.check(lib.gsage_edges_mark(_ptr(ks), _ptr(ps), R, b, 0, _ptr(flag), None, _ptr(weight) if summed else None,
                                           eshift, _ptr(wsum), s), "edges_mark")
            incl = torch.cumsum(flag, 0, dtype=torch.int32)
        shift, nbr64 = b, None
        wsrc, pay_shift, by_entry = (wsum, 0, 1) if summed else (weight, eshift, 0)
    else:
        if order == "time":
            lo, hi = (int(v) for v in torch.stack(torch.aminmax(time)).cpu())
            if hi - lo >= 2 ** 63:
                raise ValueError("edges_to_csr: the edge times span 2^63 or more")
            tk = torch.empty(R, dtype=torch.int64, device=dev)
            nat.check(lib.gsage_edges_time_keys(_ptr(time), R, eshift, lo, _ptr(tk), s), "edges_time_keys")
            _, perm = _edges_sort(tk, R, max((hi - lo).bit_length(), 1))
            del tk
        rk = torch.empty(R, dtype=torch.int64, device=dev)
        if duplicates == "all":
            nat.check(lib.gsage_edges_row_keys(_ptr(keys), _ptr(perm), R, b, _ptr(rk), s), "edges_row_keys")
        else:
            ks, ps = _edges_sort(keys, R, 2 * b)
            nat.check(lib.gsage_edges_mark(_ptr(ks), _ptr(ps), R, b, 0, None, _ptr(rk), _ptr(weight) if summed else None,
                                           eshift, _ptr(wsum), s), "edges_mark")
        ks, ps = _edges_sort(rk, R, b)
        shift, nbr64 = 0, keys
        wsrc, pay_shift, by_entry = (wsum, 0, 0) if summed else (weight, eshift, 0)
    nat.check(lib.gsage_edges_finish(_ptr(ks), _ptr(ps), _ptr(perm), _ptr(incl), R, shift, n_lim, None, _ptr(nbr64), b,
                                     col_add, _ptr(wsrc), _ptr(time), pay_shift if time is None else eshift, by_entry,
                                     _ptr(col), _ptr(w), _ptr(t), R, s), "edges_finish")
    nat.check(lib.gsage_edges_rowptr(_ptr(ks), _ptr(incl), R, shift, n_lim, _ptr(rowptr), base, s), "edges_rowptr")
    return _edges_trim(rowptr, col, w if w is not None else t, err_flag)


def _edges_trim(rowptr, col, payload, err_flag):
    """The one readback of a build: (nnz, largest row, error flag).  IndexError -- the flag cleared -- for an id outside
    the graph; otherwise the outputs cut to nnz entries."""
    stats = torch.stack([rowptr[-1], (rowptr[1:] - rowptr[:-1]).max(), err_flag[0].to(torch.int64)]).cpu()
    nnz, max_deg, err = (int(v) for v in stats)
    if err:
        err_flag.zero_()
        raise IndexError(_OUT_OF_RANGE)
    if nnz < int(col.shape[0]):                                   # (a copy: the full-length buffers are let go)
        col = col[:nnz].clone()
        payload = None if payload is None else payload[:nnz].clone()
    return rowptr, col, max(max_deg, 1), payload


def edges_to_csr(src, dst, n_nodes, sel=None, weight=None, time=None, directed=False, order=None, duplicates=None,
                 err_flag=None):
    """(rowptr int64 [n_nodes + 2], col int32 [nnz], max_deg, payload) of the edge list (src, dst: int64 [E] tensors on
    one device) in the reference's sparse convention -- include/gsage.h, "Graph construction", has the definition:
    records, `sel`, duplicates in first / sum / all, order in insertion / id / time.  payload: the kept records' fp32
    weights (summed under "sum") or int64 times, aligned with col, or None.  On the GPU a fixed pipeline of launches
    around gsage_sort_rows and one readback; CPU tensors: the same definition in numpy (host mode).  ValueError for a
    combination or a size outside the definition, IndexError for an id outside 0..n_nodes-1 (err_flag, a device int32
    word, is left clear)."""
    n_nodes = int(n_nodes)
    src, dst = src.contiguous().view(-1), dst.contiguous().view(-1)
    if src.dtype != torch.int64 or dst.dtype != torch.int64 or src.shape != dst.shape or src.device != dst.device:
        raise ValueError("edges_to_csr: src and dst must be int64 tensors of one length on one device")
    E, dev = int(src.shape[0]), src.device
    order, duplicates = edges_check(E, n_nodes, weight is not None, time is not None, directed, order, duplicates)
    if sel is not None:
        sel = sel.contiguous().view(-1)
        if sel.dtype != torch.bool or int(sel.shape[0]) != n_nodes or sel.device != dev:
            raise ValueError("edges_to_csr: sel must be a bool tensor [n_nodes] on the edges' device")
    if weight is not None:
        weight = weight.contiguous().view(-1)
        if weight.dtype != torch.float32 or int(weight.shape[0]) != E or weight.device != dev:
            raise ValueError("edges_to_csr: weight must be an fp32 tensor [E] on the edges' device")
    if time is not None:
        time = time.contiguous().view(-1)
        if time.dtype != torch.int64 or int(time.shape[0]) != E or time.device != dev:
            raise ValueError("edges_to_csr: time must be an int64 tensor [E] on the edges' device")
    if E == 0:
        pay = None if weight is None and time is None else (weight if weight is not None else time)[:0].clone()
        return torch.zeros(n_nodes + 2, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev), 1, pay
    if dev.type != "cpu":
        if err_flag is None:
            err_flag = torch.zeros(1, dtype=torch.int32, device=dev)
        R, b = (E if directed else 2 * E), max(n_nodes.bit_length(), 1)
        keys = torch.empty(R, dtype=torch.int64, device=dev)
        nat.check(nat.lib().gsage_edges_expand(_ptr(src), _ptr(dst), E, n_nodes, _ptr(sel), int(bool(directed)), b,
                                               _ptr(keys), _ptr(err_flag), _stream()), "edges_expand")
        return _edges_rows_device(keys, R, b, n_nodes, 1, 1, order, duplicates, weight, time, 0 if directed else 1,
                                  err_flag)
    # ---- host mode
    s_, d_ = src.numpy(), dst.numpy()
    if min(s_.min(), d_.min()) < 0 or max(s_.max(), d_.max()) >= n_nodes:
        raise IndexError(_OUT_OF_RANGE)
    if directed:
        rrow, rnbr, live, edge = s_, d_, np.ones(E, dtype=bool), np.arange(E)
    else:
        rrow, rnbr = np.stack([s_, d_], 1).ravel(), np.stack([d_, s_], 1).ravel()
        live = np.ones(2 * E, dtype=bool)
        live[1::2] = s_ != d_
        edge = np.arange(2 * E) >> 1
    if sel is not None:
        sn = sel.numpy()
        live &= sn[rrow] & sn[rnbr]
    ridx = np.flatnonzero(live)
    w = None if weight is None else weight.numpy()[edge[ridx]]
    t = None if time is None else time.numpy()[edge[ridx]]
    counts, nbr, pay = _edges_rows_host(rrow[ridx], rnbr[ridx], ridx, n_nodes, order, duplicates, w, t)
    rowptr = np.zeros(n_nodes + 2, dtype=np.int64)
    np.cumsum(counts, out=rowptr[2:])
    return torch.from_numpy(rowptr), torch.from_numpy((nbr + 1).astype(np.int32)), max(int(counts.max(initial=0)), 1), \
        None if pay is None else torch.from_numpy(np.ascontiguousarray(pay))


def csr_transpose(csr, symmetric=False):
    """(rowptr int64 [n_rows + 1], col int32 [nnz'], max_deg) of the transpose of a store.DeviceCSR -- row v lists u for
    every stored u -> v, ascending u, duplicates kept -- or, symmetric=True, of the union of its stored edges and their
    reverses, each pair once, ascending neighbour id (include/gsage.h, "Graph construction").  On the row ids as they
    are stored.  One expand launch, one sort, finish and rowptr (the symmetrised graph: the "id" / "first" pipeline);
    CPU adjacencies: numpy.  ValueError for a weighted or temporal adjacency, IndexError for a stored id outside the
    graph (csr.err_flag is left clear)."""
    who = "csr_symmetrize" if symmetric else "csr_transpose"
    if csr.edge_cdf is not None:
        raise ValueError("%s: a weighted adjacency is refused (a DeviceCSR keeps the CDF, not the weights)" % who)
    if csr.etime is not None:
        raise ValueError("%s: a temporal adjacency is refused (a transposed row is not in time order)" % who)
    n_rows, nnz, dev = csr.n_rows, csr.nnz, csr.device
    R = 2 * nnz if symmetric else nnz
    if R >= 2 ** 31:
        raise ValueError("%s: %d records; the record count must stay below 2^31 (the sort carries int32 positions)"
                         % (who, R))
    if nnz == 0:
        return torch.zeros(n_rows + 1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev), 1
    if dev.type != "cpu":
        lib, b, s = nat.lib(), max(int(n_rows).bit_length(), 1), _stream()
        keys = torch.empty(R, dtype=torch.int64, device=dev)
        if symmetric:
            nat.check(lib.gsage_edges_expand_csr(_ptr(csr.rowptr), _ptr(csr.col), n_rows, nnz, 1, b, _ptr(keys), None,
                                                 _ptr(csr.err_flag), s), "edges_expand_csr")
            return _edges_rows_device(keys, R, b, n_rows, 0, 0, "id", "first", None, None, 0, csr.err_flag)[:3]
        rowof = torch.empty(nnz, dtype=torch.int32, device=dev)
        nat.check(lib.gsage_edges_expand_csr(_ptr(csr.rowptr), _ptr(csr.col), n_rows, nnz, 0, b, _ptr(keys), _ptr(rowof),
                                             _ptr(csr.err_flag), s), "edges_expand_csr")
        ks, ps = _edges_sort(keys, nnz, b)
        rowptr = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
        col = torch.empty(nnz, dtype=torch.int32, device=dev)
        nat.check(lib.gsage_edges_finish(_ptr(ks), _ptr(ps), None, None, nnz, 0, n_rows, _ptr(rowof), None, b, 0, None,
                                         None, 0, 0, _ptr(col), None, None, nnz, s), "edges_finish")
        nat.check(lib.gsage_edges_rowptr(_ptr(ks), None, nnz, 0, n_rows, _ptr(rowptr), 0, s), "edges_rowptr")
        return _edges_trim(rowptr, col, None, csr.err_flag)[:3]
    # ---- host mode
    rp, c = csr.rowptr.numpy(), csr.col.numpy().astype(np.int64)
    if c.min() < 0 or c.max() >= n_rows:
        raise IndexError(_OUT_OF_RANGE)
    r = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(rp))
    if symmetric:
        rrow, rnbr = np.stack([r, c], 1).ravel(), np.stack([c, r], 1).ravel()
        counts, nbr, _ = _edges_rows_host(rrow, rnbr, np.arange(2 * nnz), n_rows, "id", "first", None, None)
    else:
        counts, nbr, _ = _edges_rows_host(c, r, np.arange(nnz), n_rows, "insertion", "all", None, None)
    rowptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(counts, out=rowptr[1:])
    return torch.from_numpy(rowptr), torch.from_numpy(nbr.astype(np.int32)), max(int(counts.max(initial=0)), 1)
