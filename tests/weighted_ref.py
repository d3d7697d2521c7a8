"""What the weighted-graph tests share, written from the formulas of include/gsage.h ("Weighted adjacency") in Python
integers and fractions on oracle.cpu.philox4x32_10 -- no code of the product: the per-edge integer CDF, the weighted
sampler, the weight-normalised mean in float64 with its derived comparison, the test graph whose rows sit on every edge
of the definition and of the kernels' schedules, and the small weighted problem of the model tests."""
import math
from fractions import Fraction

import numpy as np
import torch
from scipy import sparse

from conftest import pkg
from oracle import cpu as ocpu

U32 = 2.0 ** -24                    # unit roundoff of fp32
BF16_STORE = 2.0 ** -8              # the project's bound for one bf16 store (tests/segment_reduce_ref.py)
TAG = 0x57000000
M64 = (1 << 64) - 1


# ---- the table ---------------------------------------------------------------------------------------------------
def quanta(w):
    """[q_e] of one row of float32 weights: floor(w_e * 2^(24 - E)), (f, E) = frexp(max); all 0 when the maximum is."""
    w = [float(np.float32(x)) for x in w]
    m = max(w) if w else 0.0
    if m == 0.0:
        return [0] * len(w)
    _, E = math.frexp(m)
    scale = Fraction(2) ** (24 - E)
    q = [int(Fraction(x) * scale) for x in w]             # (non-negative: int() is the floor)
    assert all(0 <= v < (1 << 24) for v in q) and max(q) >= (1 << 23)
    return q


def build_cdf(rowptr, weight):
    """uint64 [nnz]: per row, the inclusive running sum of its quanta"""
    cdf = np.zeros(len(weight), dtype=np.uint64)
    for v in range(len(rowptr) - 1):
        run = 0
        for e, q in zip(range(int(rowptr[v]), int(rowptr[v + 1])), quanta(weight[rowptr[v]:rowptr[v + 1]])):
            run += q
            cdf[e] = run
    return cdf


# ---- the sampler -------------------------------------------------------------------------------------------------
def draw_x(seed, call, g, T):
    """x = (r64 * T) >> 64 of draw g"""
    blk = (g & M64) >> 1
    w = ocpu.philox4x32_10((blk & 0xFFFFFFFF, blk >> 32, call & 0xFFFFFFFF, (call >> 32) & 0xFFFFFFFF),
                           (seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ TAG))
    k = 2 * (g & 1)
    return (((w[k] << 32) | w[k + 1]) * int(T)) >> 64


def sample(rowptr, col, cdf, n_rows, ids, n, seed, call, g0):
    """-> (out int64 [M * n], err): gsage_sample_csr_weighted"""
    out, err = np.zeros(len(ids) * n, dtype=np.int64), 0
    for i, v in enumerate(ids):
        v = int(v)
        if v < 0 or v >= n_rows:
            err = 1
            continue
        b, e = int(rowptr[v]), int(rowptr[v + 1])
        T = int(cdf[e - 1]) if e > b else 0
        if T == 0:
            continue
        row = [int(c) for c in cdf[b:e]]
        for j in range(n):
            x = draw_x(seed, call, g0 + i * n + j, T)
            out[i * n + j] = col[b + next(k for k, c in enumerate(row) if c > x)]
    return out, err


# ---- the weight-normalised mean ------------------------------------------------------------------------------------
def weighted_mean(rowptr, col, cdf, table, drop=None, equal=False):
    """float64 (out [n, D], S [n, D], drawable [n]): out[v] = sum_e p_e x[col[e]], p_e = (cdf[e] - cdf[e-1]) / T_v, S the
    same sum over |x|, drawable = the number of edges with p_e > 0 (1 for a row that reads the dummy).
    drop = (row, k): the row loses its k-th edge but keeps T -- what a kernel that skipped one edge computes;
    equal: every drawable edge of a row counts the same -- what a kernel that ignored the weights computes."""
    X = np.asarray(table, dtype=np.float64)
    n = len(rowptr) - 1
    out, S, k = np.zeros((n, X.shape[1])), np.zeros((n, X.shape[1])), np.ones(n, dtype=np.int64)
    for v in range(n):
        b, e = int(rowptr[v]), int(rowptr[v + 1])
        T = int(cdf[e - 1]) if e > b else 0
        if T == 0:
            out[v], S[v] = X[0], np.abs(X[0])
            continue
        q = np.diff(np.concatenate([[0], cdf[b:e].astype(np.int64)]))
        k[v] = int((q > 0).sum())
        p = (q > 0) / float(k[v]) if equal else q / float(T)
        nb = np.asarray(col[b:e], dtype=np.int64)
        nb = np.where((nb < 0) | (nb >= n), 0, nb)
        if drop is not None and drop[0] == v:
            p, nb = np.delete(p, drop[1]), np.delete(nb, drop[1])
        out[v] = (p[:, None] * X[nb]).sum(0)
        S[v] = (p[:, None] * np.abs(X[nb])).sum(0)
    return out, S, k


def cast(x, dt):
    return torch.tensor(np.asarray(x)).to(torch.float32).to(dt)


def compare(got, ref, S, drawable, odt, what, act="none"):
    """got: the kernel's [n, D] output (CPU tensor of type odt) against float64 (ref, S) WITHOUT activation.
    A row with one drawable edge (or none: the dummy): equal to ref cast to odt -- p = q / T = 1.  Elsewhere, with k
    drawable edges,  |got - ref| <= (k + 2) 2^-24 S  (+ 2^-8 |ref| for a bf16 store): one rounding for float(T), one
    for the division q / float(T) -- float(q) is exact, q < 2^24 -- and one per fused multiply-add, k in all (an edge
    of quantum 0 adds an exact 0; so does a slice of such edges in the merge, and a term meets no more roundings split
    over slices than in one run).  A looser (deg + 6) would also be defensible; this is what the kernel can be held to.
    -> the largest |got - ref| / S over the inexact rows."""
    want = np.maximum(ref, 0.0) if act == "relu" else ref
    g64 = got.double().numpy()
    assert g64.shape == want.shape, (what, g64.shape, want.shape)
    assert np.isfinite(g64).all(), (what, "not finite")
    exact = np.asarray(drawable) == 1
    rows = torch.from_numpy(np.flatnonzero(exact))
    same = got[rows] == cast(want, got.dtype)[rows]
    if not bool(same.all()):
        r, c = (int(x) for x in torch.nonzero(~same)[0])
        raise AssertionError((what, "row %d (one drawable edge) column %d: got %r, exactly %r expected"
                              % (int(rows[r]), c, float(g64[int(rows[r]), c]), float(want[int(rows[r]), c]))))
    err = np.abs(g64 - want)
    bound = (np.asarray(drawable)[:, None] + 2.0) * U32 * S
    if odt == "bf16":
        bound = bound + BF16_STORE * np.abs(want)
    bad = (err > bound) & ~exact[:, None]
    if bad.any():
        over = np.where(bad, err / np.maximum(bound, 1e-300), 0.0)
        v, c = np.unravel_index(int(np.argmax(over)), over.shape)
        raise AssertionError((what, "%d elements beyond the bound; worst: row %d (%d drawable edges) column %d: got %r, "
                              "reference %r, |difference| %.3g, bound %.3g"
                              % (int(bad.sum()), v, int(drawable[v]), c, float(g64[v, c]), float(want[v, c]),
                                 float(err[v, c]), float(bound[v, c]))))
    ok = (S > 0) & ~exact[:, None]
    return float((err[ok] / S[ok]).max()) if ok.any() else 0.0


# ---- the test graph ----------------------------------------------------------------------------------------------
ROWS = {                            # name -> row
    "degree 0": 0, "degree 1": 1, "all zero": 2, "all zero, 12 edges": 3, "zero between": 4, "equal": 5,
    "span beyond 2^24": 6, "denormal beside normal": 7, "all denormal": 8, "maximum a power of two": 9,
    "maximum 3.4e38": 10, "degree 0 again": 11,
    63: 12, 64: 13, 65: 14, 256: 15, 257: 16, 300: 17, 1000: 18,
    "all zero, 300 edges": 19, "one drawable of 20": 20,
}


class Graph(object):
    def __init__(self, rowptr, col, weight):
        self.rowptr, self.col, self.weight = rowptr, col, weight
        self.n = len(rowptr) - 1
        self.deg = np.diff(rowptr)
        self.cdf = build_cdf(rowptr, weight)

    def csr(self, device="cpu", weighted=True):
        gs = pkg()
        adj = gs.DeviceCSR(torch.from_numpy(self.rowptr).to(device), torch.from_numpy(self.col).to(device), self.n,
                           max(int(self.deg.max()), 1))
        return adj.with_weights(torch.from_numpy(self.weight).to(device)) if weighted else adj


_GRAPH = []


def graph():
    """72 rows: the arranged ones of ROWS, then degrees uniform in [1, 24] with weights of every scale."""
    if _GRAPH:
        return _GRAPH[0]
    rng = np.random.RandomState(2024)
    n = 72
    f32 = lambda xs: np.asarray(xs, dtype=np.float32)
    fixed = {
        0: f32([]), 1: f32([2.5]), 2: f32([0] * 5), 3: f32([0] * 12), 4: f32([1.0, 0.0, 2.0]), 5: f32([0.7] * 6),
        6: f32([1.0, 2.0 ** -25, 2.0 ** -30, 0.5, 3e-8, 2.0 ** -24, 2.0 ** -23]),
        7: f32([1e-42, 1.0, 1e-38, 5e-45, 0.25]), 8: f32([1e-44, 3e-45, 1.4e-45, 7e-45]),
        9: f32([4.0, 1.0, 3.0, 0.25, 4.0]), 10: f32([3.4e38, 1e38, 1.0, 3e31, 3.3e38]), 11: f32([]),
        19: f32([0] * 300), 20: f32([0] * 13 + [0.3] + [0] * 6),
    }
    rows = []
    for v in range(n):
        if v in fixed:
            rows.append(fixed[v])
            continue
        d = {12: 63, 13: 64, 14: 65, 15: 256, 16: 257, 17: 300, 18: 1000}.get(v, int(rng.randint(1, 25)))
        w = np.exp(rng.normal(size=d) * 3.0).astype(np.float32) * np.float32(10.0 ** rng.randint(-6, 7))
        w[rng.rand(d) < 0.1] = 0.0
        if d > 1:
            w[rng.randint(d)] = np.float32(1.5) * w.max() + np.float32(1e-3)      # one clear maximum, never all zero
        rows.append(w.astype(np.float32))
    deg = np.array([len(r) for r in rows], dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    weight = np.concatenate(rows).astype(np.float32)
    col = rng.randint(0, n, size=int(rowptr[-1])).astype(np.int32)
    g = Graph(rowptr, col, weight)
    assert g.n == n and all(g.deg[ROWS[d]] == d for d in (63, 64, 65, 256, 257, 300, 1000))
    _GRAPH.append(g)
    return g


# ---- the weighted problem of the model tests ---------------------------------------------------------------------------
def weighted_problem(n=200, D=16, C=3, seed=7):
    """dict(adj, weight (scipy, the structure of adj), indptr, data, w, feats, folds, targets): a 200-node graph in the
    reference's convention with rows of degree 0, zero weights and an all-zero row"""
    rng = np.random.RandomState(seed)
    deg = rng.randint(1, 12, size=n + 1)
    deg[0] = 0
    deg[9::23] = 0
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    data = rng.randint(1, n + 1, size=int(indptr[-1]))
    cols = np.arange(indptr[-1]) - np.repeat(indptr[:-1], deg)
    w = np.exp(rng.normal(size=int(indptr[-1])) * 1.5).astype(np.float32)
    w[rng.rand(w.shape[0]) < 0.1] = 0.0
    w[indptr[5]:indptr[6]] = 0.0                               # an all-zero row
    shape = (n + 1, int(deg.max()))
    adj = sparse.csr_matrix((data, cols, indptr), shape=shape)
    weight = sparse.csr_matrix((w, cols, indptr), shape=shape)
    feats = rng.normal(size=(n + 1, D)).astype(np.float32)
    feats[0] = 0
    folds = np.array(["train"] * 130 + ["val"] * 40 + ["test"] * (n + 1 - 170))
    folds[0] = "dummy"
    targets = feats[:, :C].argmax(1).reshape(-1, 1)
    return dict(adj=adj, weight=weight, indptr=indptr, data=data, w=w, feats=feats, folds=folds, targets=targets, C=C)


def dense_reference(model, feats, indptr, data, w):
    """float64 (logits, embeddings) of layer-wise inference under the weight-normalised mean, with explicit loops:
    mean and mean-pool aggregators, identity / linear prep"""
    gs = pkg()
    npd = lambda t: t.detach().cpu().double().numpy()
    n = len(indptr) - 1
    cdf = build_cdf(indptr, w)
    shares = []
    for v in range(n):
        b, e = int(indptr[v]), int(indptr[v + 1])
        T = int(cdf[e - 1]) if e > b else 0
        if T == 0:
            shares.append([(0, 1.0)])
        else:
            q = np.diff(np.concatenate([[0], cdf[b:e].astype(np.int64)]))
            shares.append([(int(u), float(Fraction(int(k), T))) for u, k in zip(data[b:e], q)])
    H = np.asarray(feats, dtype=np.float64)[:n]
    if isinstance(model.prep, gs.nn_modules.LinearPrep):
        H = H @ npd(model.prep.fc.weight).T
    for layer in model.agg_layers.children():
        X = H
        if isinstance(layer, gs.nn_modules.PoolAggregator):
            assert layer.pool_fn == "mean"
            X = np.maximum(H @ npd(layer.mlp[0].weight).T + npd(layer.mlp[0].bias), 0)
        agg = np.zeros((n, X.shape[1]))
        for v in range(n):
            for u, p in shares[v]:
                agg[v] += p * X[u]
        out = np.concatenate([H @ npd(layer.fc_x.weight).T, agg @ npd(layer.fc_neib.weight).T], axis=1)
        H = np.maximum(out, 0) if layer.activation is torch.nn.functional.relu else out
    emb = H / np.maximum(np.linalg.norm(H, axis=1, keepdims=True), 1e-12)
    return emb @ npd(model.fc.weight).T + npd(model.fc.bias), emb
