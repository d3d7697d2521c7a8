"""What the direct tests of gsage_segment_reduce (csrc/gsage_fullgraph.hip) share: a float64 restatement of its three
reductions with an explicit loop over rows, a plain float32 restatement of the softmax mode (the yardstick of that
mode's bound), the graph whose degrees sit on every edge of the kernel's schedule, a launch helper that takes any plan,
and the comparison with its derived tolerances."""
import numpy as np
import torch

from conftest import pkg

MODES = ("mean", "max", "softmax")
U32 = 2.0 ** -24                    # unit roundoff of fp32
BF16_STORE = 2.0 ** -8              # the project's bound for one bf16 store (tests/test_gpu_kernels.py)
TORCH_DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
VEC = {"bf16": 8, "fp32": 4}        # elements per 16-byte chunk


# ---- the definition ------------------------------------------------------------------------------------------
def _neighbours(rowptr, col, v, n):
    """N(v) as the kernel reads it: degree 0 -> the dummy 0; an id outside [0, n) -> row 0."""
    nb = np.asarray(col[rowptr[v]:rowptr[v + 1]], dtype=np.int64)
    if nb.size == 0:
        return np.zeros(1, dtype=np.int64)
    return np.where((nb < 0) | (nb >= n), 0, nb)


def reference(rowptr, col, table, keys, mode, act="none", drop=None):
    """float64: (out [n, D], S [n, D]) with S[v, c] = sum_u |w_u x[u, c]|, w_u = 1 / deg (mean), the softmax weight
    (softmax) or 1 on the winner (max).  table: the STORED values [n, D]; keys: [n, >= 32] (softmax only).
    drop = (row, k): row loses its k-th edge but keeps its degree -- what a kernel that skipped one edge computes."""
    X = np.asarray(table, dtype=np.float64)
    n = len(rowptr) - 1
    K = None if keys is None else np.asarray(keys, dtype=np.float64)[:, :32]
    out, S = np.empty((n, X.shape[1])), np.empty((n, X.shape[1]))
    for v in range(n):
        nb = _neighbours(rowptr, col, v, n)
        deg = nb.size
        if drop is not None and drop[0] == v:
            nb = np.delete(nb, drop[1])
        x = X[nb]
        if mode == "max":
            out[v] = x.max(0)
            S[v] = np.abs(out[v])
            continue
        if mode == "mean":
            w = np.full(nb.size, 1.0 / max(deg, 1))
        else:
            s = K[nb] @ K[v]
            w = np.exp(s - s.max())
            w /= w.sum()
        out[v] = (w[:, None] * x).sum(0)
        S[v] = (w[:, None] * np.abs(x)).sum(0)
    if act == "relu":
        out = np.maximum(out, 0.0)
    return out, S


def softmax_float32(rowptr, col, table, keys):
    """The softmax mode restated in plain float32: two passes over the whole row, no batches, no slices."""
    X = np.asarray(table, dtype=np.float32)
    K = np.asarray(keys, dtype=np.float32)[:, :32]
    n = len(rowptr) - 1
    out = np.empty((n, X.shape[1]), dtype=np.float32)
    for v in range(n):
        nb = _neighbours(rowptr, col, v, n)
        s = (K[nb] * K[v]).sum(1, dtype=np.float32)
        w = np.exp(s - s.max())
        out[v] = (w[:, None] * X[nb]).sum(0, dtype=np.float32) / w.sum(dtype=np.float32)
    return out


def float32_error(f32, ref, S):
    """max over the elements of |f32 - ref| / S: the float32 restatement's error in units of the magnitude sum"""
    ok = S > 0
    return float((np.abs(np.asarray(f32, dtype=np.float64) - ref)[ok] / S[ok]).max()) if ok.any() else 0.0


# ---- graphs --------------------------------------------------------------------------------------------------
class Graph(object):
    """rowptr int64 [n + 1], col int32 [nnz] (numpy: the reference and the device see the same arrays), the slice
    length L its degrees are written in, and `at`: degree -> one row that has it."""

    def __init__(self, rowptr, col, L, at):
        self.rowptr, self.col, self.L, self.at = rowptr, col, L, at
        self.n = len(rowptr) - 1
        self.deg = np.diff(rowptr)

    def csr(self, device="cpu"):
        gs = pkg()
        return gs.DeviceCSR(torch.from_numpy(self.rowptr).to(device), torch.from_numpy(self.col).to(device), self.n,
                            max(int(self.deg.max()), 1))

    def with_ids(self, edits):
        """a copy with col[e] = id for (e, id) in edits"""
        col = self.col.copy()
        for e, i in edits:
            col[e] = i
        return Graph(self.rowptr, col, self.L, self.at)


def edge_degrees(L):
    return sorted({1, 7, 8, 9, 15, 16, 17, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 3 * L + 5})


def from_degrees(deg, rng, L, at=None):
    """Neighbour ids uniform in [0, n) -- the dummy 0 and repeats occur by themselves -- and, placed on purpose: the
    dummy first in every third row, the row itself second in every even row, its last edge twice in every fourth."""
    deg = np.asarray(deg, dtype=np.int64)
    n = deg.shape[0]
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.randint(0, n, size=int(rowptr[-1])).astype(np.int32)
    for v in range(n):
        b, e = int(rowptr[v]), int(rowptr[v + 1])
        if e - b < 3:
            continue
        if v % 3 == 0:
            col[b] = 0
        if v % 2 == 0:
            col[b + 1] = v
        if v % 4 == 1:
            col[e - 1] = col[e - 2]
    return Graph(rowptr, col, L, at or {})


def build_graph(L, n=700, seed=0, rand_hi=24):
    """About 700 rows.  Degree 0: row 0 and every 41st row from 5.  Long rows (for slice length L) at the first
    non-dummy index (L + 1), in the middle (3L + 5) and at the last index (2L + 1).  Every degree of edge_degrees(L)
    once, from row 20 in steps of 17.  Degrees uniform in [1, rand_hi] elsewhere: with L = 8 two thirds of them are
    long rows, with L = 256 none is."""
    rng = np.random.RandomState(seed)
    deg = rng.randint(1, rand_hi + 1, size=n)
    deg[0] = 0
    deg[5::41] = 0
    deg[1], deg[n // 2], deg[n - 1] = L + 1, 3 * L + 5, 2 * L + 1
    at = {}
    for i, d in enumerate(edge_degrees(L)):
        deg[20 + 17 * i] = d
        at[d] = 20 + 17 * i
    return from_degrees(deg, rng, L, at)


_GRAPHS = {}


def graph(L):
    if L not in _GRAPHS:
        _GRAPHS[L] = build_graph(L, seed=L)
    return _GRAPHS[L]


# ---- inputs and the cached reference ---------------------------------------------------------------------------
def stored(x, tdt):
    """float32 values after the table's rounding (bf16: nearest even), as float32"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(TORCH_DT[tdt]).float().numpy()


def cast(x, dt):
    """float64 -> the output type, round to nearest even, as a CPU tensor"""
    return torch.tensor(np.asarray(x)).to(torch.float32).to(TORCH_DT[dt])


def inputs(n, D, tdt, seed, key_scale=1.33):
    """(stored table values [n, D] float32 -- row 0, the dummy, is NOT zero: a row of degree 0 must be seen to read it
    -- and keys [n, 32] float32 whose scores are of order key_scale^2 * sqrt(32))"""
    rng = np.random.RandomState(seed)
    table = stored(rng.normal(size=(n, D)), tdt)
    keys = (rng.normal(size=(n, 32)) * key_scale).astype(np.float32)
    return table, keys


_REFS = {}


def cached(g, D, tdt, tag, key_scale=1.33):
    """Per (graph, width, table type): the inputs, the float64 (out, S) of every mode without activation, the float32
    softmax restatement and its error.  Computed once; the arrays are read-only."""
    key = (tag, D, tdt)
    if key not in _REFS:
        table, keys = inputs(g.n, D, tdt, seed=1000 + D, key_scale=key_scale)
        r = {"table": table, "keys": keys}
        for mode in MODES:
            r[mode] = reference(g.rowptr, g.col, table, keys, mode)
        r["f32"] = softmax_float32(g.rowptr, g.col, table, keys)
        r["e32"] = float32_error(r["f32"], *r["softmax"])
        for v in r.values():
            for a in (v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]


# ---- the device side ---------------------------------------------------------------------------------------------
TABLE_PAD = 1e30            # columns [D, ld) of the table: finite, and ruinous if a live column ever read them
OUT_PAD = -7.5              # columns [D, out_ld) of the output buffer (exact in bf16)


def device_table(values, tdt, wide, device):
    """[n, ld] table holding `values` in [:, :D] and TABLE_PAD in [D, ld); ld = D rounded up to the 16-byte chunk, plus
    two chunks when `wide`"""
    n, D = values.shape
    vec = VEC[tdt]
    ld = (D + vec - 1) // vec * vec + (2 * vec if wide else 0)
    t = torch.full((n, ld), TABLE_PAD, dtype=TORCH_DT[tdt])
    t[:, :D] = torch.tensor(values).to(TORCH_DT[tdt])
    return t.to(device)


def device_keys(keys, wide, device):
    """[n, 32] keys; `wide`: a view of a [n, 36] buffer (ldk > 32)"""
    k = torch.tensor(keys)
    if wide:
        buf = torch.full((k.shape[0], 36), TABLE_PAD, dtype=torch.float32)
        buf[:, :32] = k
        return buf.to(device)[:, :32]
    return k.to(device)


def out_buffer(n, D, odt, device):
    """(buffer [n, D + 3] pre-filled with OUT_PAD, its [:, :D] view)"""
    buf = torch.full((n, D + 3), OUT_PAD, dtype=TORCH_DT[odt], device=device)
    return buf, buf[:, :D]


def launch(adj, plan, table, D, mode, out, act="none", keys=None):
    """gsage_segment_reduce on `plan` (infer.segment_reduce always takes the default one).  table: [n, ld] with D
    logical columns; out: a [n, D] view; -> out"""
    gs = pkg()
    nat, ops = gs._native, gs.ops
    code = {"mean": nat.SEG_MEAN, "max": nat.SEG_MAX, "softmax": nat.SEG_SOFTMAX_WEIGHTED}[mode]
    rowptr, col, n = adj.rowptr, adj.col, adj.n_rows
    assert table.stride(1) == 1 and out.stride(1) == 1 and int(table.shape[0]) >= n and int(out.shape[0]) >= n
    assert int(out.shape[1]) == D <= int(table.shape[1])
    ldp = int(nat.lib().gsage_segment_reduce_ldp(D))
    partials = torch.empty(max(plan["n_slices"], 1), ldp, dtype=torch.float32, device=table.device)
    kp, ldk = (None, 0) if keys is None else (ops._ptr(keys), keys.stride(0))
    nat.check(nat.lib().gsage_segment_reduce(
        code, ops._ptr(table), ops._code(table.dtype), table.stride(0), D, kp, ldk, ops._ptr(rowptr), ops._ptr(col), n,
        ops._ptr(plan["order"]), plan["n_short"], ops._ptr(plan["slices"]), plan["n_slices"],
        ops._ptr(plan["long_rows"]), plan["n_long"], plan["slice_len"], ops._ptr(partials), ldp, ops._ptr(out),
        ops._code(out.dtype), out.stride(0), nat.ACT_RELU if act == "relu" else nat.ACT_NONE, ops._ptr(adj.err_flag),
        ops._stream()), "segment_reduce")
    return out


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---- the comparison ----------------------------------------------------------------------------------------------
def compare(got, ref, S, deg, mode, odt, what, act="none", e32=None):
    """got: the kernel's [n, D] output (a CPU tensor of type odt) against the float64 (ref, S) WITHOUT activation.
    Max, and every row of effective degree 1: equal to ref cast to odt.  Elsewhere, per element,
        mean     |got - ref| <= (deg + 2) 2^-24 S      any fp32 summation order, plus the division
        softmax  |got - ref| <= 8 e32 S                e32: the float32 restatement's error on the same inputs
        bf16 out + 2^-8 |ref|                          one bf16 store
    -> the largest |got - ref| / S.  Raises AssertionError naming mode, types, width, row and degree."""
    want = np.maximum(ref, 0.0) if act == "relu" else ref
    deg = np.maximum(np.asarray(deg), 1)
    exact = np.ones_like(deg, dtype=bool) if mode == "max" else deg == 1
    g64 = got.double().numpy()
    assert g64.shape == want.shape, (what, g64.shape, want.shape)
    assert np.isfinite(g64).all(), (what, "not finite in row %d (degree %d)"
                                    % (int(np.argwhere(~np.isfinite(g64))[0][0]),
                                       int(deg[np.argwhere(~np.isfinite(g64))[0][0]])))
    if exact.any():
        rows = torch.from_numpy(np.flatnonzero(exact))
        same = got[rows] == cast(want, odt)[rows]
        if not bool(same.all()):
            r, c = (int(x) for x in torch.nonzero(~same)[0])
            v = int(rows[r])
            raise AssertionError((what, "row %d (degree %d) column %d: got %r, exactly %r expected"
                                  % (v, int(deg[v]), c, float(g64[v, c]), float(want[v, c]))))
    err = np.abs(g64 - want)
    if mode == "max":
        return 0.0
    if mode == "mean":
        bound = (deg[:, None] + 2.0) * U32 * S
    else:
        assert e32 is not None
        bound = 8.0 * e32 * S
    if odt == "bf16":
        bound = bound + BF16_STORE * np.abs(want)
    bad = (err > bound) & ~exact[:, None]
    if bad.any():
        over = np.where(bad, err / np.maximum(bound, 1e-300), 0.0)
        v, c = np.unravel_index(int(np.argmax(over)), over.shape)
        raise AssertionError((what, "%d elements beyond the bound; worst: row %d (degree %d) column %d: got %r, "
                              "reference %r, |difference| %.3g, bound %.3g"
                              % (int(bad.sum()), v, int(deg[v]), c, float(g64[v, c]), float(want[v, c]),
                                 float(err[v, c]), float(bound[v, c]))))
    ok = (S > 0) & ~exact[:, None]
    return float((err[ok] / S[ok]).max()) if ok.any() else 0.0
