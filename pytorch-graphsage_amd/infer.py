"""
infer.py -- layer-wise full-neighbourhood inference and node-embedding export for a trained GSSupervised or
GSUnsupervised.

The sampled forward (`model(ids, feats, train=False)`) draws new neighbour samples on every call and pays, per seed,
the product of the fan-outs.  Here every layer is computed ONCE for every row of the adjacency, over each row's
WHOLE neighbourhood:

    H^0    = prep(all rows)                    IdentityPrep: feats;  LinearPrep: feats @ W_p^T
    H^l[v] = act(concat(fc_x(H^{l-1}[v]), fc_neib(agg_{u in N(v)} H^{l-1}[u])))
    emb    = F.normalize(H^L),  logits = fc(emb)

agg is the aggregator's own reduction: mean; max / mean of relu(W_m h + b_m) (pool aggregators); the softmax over
N(v) of att(H[u]) . att(H[v]) weighting the raw rows (attention).  N(v) is row v of the sparse adjacency (a row of
degree 0 has the single neighbour 0, the dummy, as the sampler draws it) or all K columns of row v of the dense one
(duplicates count).  On a WEIGHTED adjacency (store.DeviceCSR.edge_cdf) the mean is the weight-normalised mean
sum_e (q_e / T_v) H[u_e] over the table's integer quanta -- what the sampled mean estimates under the weighted sampler;
a row without a drawable edge reads the dummy.  Max-pool and attention have no weighted form here.  With the dense sampler and n_val_samples == K the sampled forward takes every column of every
row, i.e. computes this same thing up to summation order.

On the GPU, fc_neib is applied BEFORE the reduction where that is exact (mean, mean-pool, attention: the reduction
is linear in the rows), so the segment-reduce kernel (csrc/gsage_fullgraph.hip) gathers output-width rows; max-pool
reduces the MLP output and projects afterwards.  The projections run on K5 (ops.linear).  CPU tensors take a plain
torch restatement of the same definition (host mode).

For a QUERY SET the exact answer depends only on its k-hop closure: with L layers, level L needs the queries, level
L - 1 the queries and their neighbours, and so on down.  closure() builds the node sets S_L c ... c S_0 and one block
per layer (csrc/gsage_block.hip: deduplicated frontier expansion and relabelling on the device), query() gathers the
feature rows of S_0 and runs every layer over its block -- H^l has |S_l| rows -- with the same projections and the same
segment-reduce kernels (gsage_segment_reduce_block).  The cost follows the closure, not the graph.
"""
import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import _native as nat
from . import ops
from .nn_modules import (AttentionAggregator, IdentityPrep, LinearPrep, LSTMAggregator, MeanAggregator,
                         NodeEmbeddingPrep, PoolAggregator, concat_combine, _split_activation)
from .store import DenseAdj, DeviceCSR, FeatureStore, TemporalAdj, WeightedAdj, _round_up

SLICE_LEN = 256          # rows of higher degree are cut into slices of this many edges (one team each)


# --------------------------------------------------------------------------------------------
# what is supported
# --------------------------------------------------------------------------------------------
def _weighted(adj):
    return getattr(adj, "edge_cdf", None) is not None


def check_supported(model, adj=None):
    """Raise ValueError naming why `model` has no layer-wise full-neighbourhood form (over `adj`, when given: a
    weighted adjacency takes mean and mean-pool aggregators only); else return None."""
    if isinstance(model.prep, NodeEmbeddingPrep):
        raise ValueError("full-neighbour inference does not support NodeEmbeddingPrep: its seed hop reads the spare "
                         "row n_nodes, so every layer would need two tables")
    if not isinstance(model.prep, (IdentityPrep, LinearPrep)):
        raise ValueError("full-neighbour inference supports the identity and linear preps, not %s"
                         % type(model.prep).__name__)
    for layer in model.agg_layers.children():
        if isinstance(layer, LSTMAggregator):
            raise ValueError("full-neighbour inference does not support LSTMAggregator: it is order-dependent and has "
                             "no full-neighbourhood meaning")
        if not isinstance(layer, (MeanAggregator, PoolAggregator, AttentionAggregator)):
            raise ValueError("full-neighbour inference does not support %s" % type(layer).__name__)
        if layer.combine_fn is not concat_combine:
            raise ValueError("full-neighbour inference needs combine_fn = concat_combine, not a custom combine_fn")
        if isinstance(layer, PoolAggregator) and layer.pool_fn not in ("max", "mean"):
            raise ValueError("full-neighbour inference needs a PoolAggregator pool_fn of \"max\" or \"mean\", "
                             "not a callable")
        if isinstance(layer, AttentionAggregator) and layer.att[2].weight.shape[0] > 32:
            raise ValueError("full-neighbour inference needs an attention hidden_dim of at most 32")
        if adj is not None and _weighted(adj) and (isinstance(layer, AttentionAggregator) or
                                                   (isinstance(layer, PoolAggregator) and layer.pool_fn == "max")):
            raise ValueError("full-neighbour inference on a weighted adjacency supports the mean and mean-pool "
                             "aggregators; max-pool and attention have no weighted form")


# --------------------------------------------------------------------------------------------
# adjacency -> CSR + schedule (once per adjacency object)
# --------------------------------------------------------------------------------------------
def _csr(adj):
    """(rowptr int64 [n+1], col int32 [nnz], n_rows) of a DeviceCSR, or of a DenseAdj read as K edges per row."""
    if isinstance(adj, DenseAdj):
        got = getattr(adj, "_fullgraph_csr", None)
        if got is None:
            dev = adj.device
            rowptr = torch.arange(adj.n_rows + 1, dtype=torch.int64, device=dev) * adj.K
            if adj.adj.numel() and (int(adj.adj.min()) < 0 or int(adj.adj.max()) >= adj.n_rows):
                raise IndexError("full-neighbour inference: dense adjacency holds ids outside [0, n_rows)")
            got = (rowptr, adj.adj.reshape(-1).to(torch.int32), adj.n_rows)
            adj._fullgraph_csr = got
        return got
    return adj.rowptr, adj.col, adj.n_rows


def plan(adj, slice_len=SLICE_LEN):
    """The schedule of gsage_segment_reduce for `adj`, cached on it: short rows in degree-descending order, the
    slices of the rows longer than `slice_len` and, per long row, the index of its first slice."""
    cache = getattr(adj, "_fullgraph_plan", None)
    if cache is not None and cache["slice_len"] == slice_len:
        return cache
    rowptr, col, n = _csr(adj)
    deg = rowptr[1:] - rowptr[:-1]
    short = deg <= slice_len
    sdeg = torch.where(short, deg, torch.full_like(deg, -1))
    _, order = torch.sort(sdeg, descending=True, stable=True)
    n_short = int(short.sum())
    order = order[:n_short].to(torch.int32).contiguous()
    long_rows = torch.nonzero(~short).view(-1)
    ns = (deg[long_rows] + slice_len - 1) // slice_len
    first = torch.cumsum(ns, 0) - ns
    slice_row = torch.repeat_interleave(long_rows, ns)
    k = torch.arange(slice_row.numel(), dtype=torch.int64, device=rowptr.device) - torch.repeat_interleave(first, ns)
    slices = torch.stack([slice_row, rowptr[slice_row] + k * slice_len], 1).contiguous()
    longs = torch.stack([long_rows, first], 1).contiguous()
    cache = {"slice_len": slice_len, "order": order, "n_short": n_short, "slices": slices,
             "n_slices": int(slices.shape[0]), "long_rows": longs, "n_long": int(longs.shape[0])}
    adj._fullgraph_plan = cache
    return cache


def segment_reduce(adj, table, mode, out, act=nat.ACT_NONE, keys=None):
    """out[v, :D] = reduce over N(v) of table[u, :D] for every row v of `adj` (gsage_segment_reduce: two launches).
    `adj` may be a Block of a closure: out has its n_dst rows, table and keys the n_src rows of its source set.
    table: [n_rows, D] bf16 / fp32 CUDA tensor whose row stride is a multiple of 16 bytes; out: a (possibly
    strided) fp32 / bf16 [n_rows, D] view; keys (SOFTMAX_WEIGHTED): fp32 [n_rows, 32].  mode SEG_WEIGHTED_MEAN
    (gsage_segment_reduce_weighted) reads the adjacency's edge_cdf."""
    rowptr, col, n = _csr(adj)
    p = plan(adj)
    D = int(table.shape[1])
    n_src = adj.n_src if isinstance(adj, Block) else n
    assert table.stride(1) == 1 and out.stride(1) == 1 and int(table.shape[0]) >= n_src and int(out.shape[0]) >= n
    ldp = int(nat.lib().gsage_segment_reduce_ldp(D))
    partials = torch.empty(max(p["n_slices"], 1), ldp, dtype=torch.float32, device=table.device)
    if isinstance(adj, Block):
        # a block of a closure: n output rows over a table (and keys) of n_src rows, the dummy at adj.dummy
        assert (mode == nat.SEG_WEIGHTED_MEAN) == _weighted(adj) and (keys is None or int(keys.shape[0]) >= n_src)
        kp, ldk = (None, 0) if keys is None else (ops._ptr(keys), keys.stride(0))
        nat.check(nat.lib().gsage_segment_reduce_block(
            mode, ops._ptr(table), ops._code(table.dtype), table.stride(0), D, kp, ldk, ops._ptr(rowptr), adj.col_ptr(),
            adj.cdf_ptr(), n, n_src, adj.dummy, ops._ptr(p["order"]), p["n_short"],
            ops._ptr(p["slices"]), p["n_slices"], ops._ptr(p["long_rows"]), p["n_long"], p["slice_len"],
            ops._ptr(partials), ldp, ops._ptr(out), ops._code(out.dtype), out.stride(0), act, ops._ptr(adj.err_flag),
            ops._stream()), "segment_reduce_block")
        return out
    if mode == nat.SEG_WEIGHTED_MEAN:
        assert _weighted(adj) and int(adj.edge_cdf.shape[0]) == int(col.shape[0])
        nat.check(nat.lib().gsage_segment_reduce_weighted(
            ops._ptr(table), ops._code(table.dtype), table.stride(0), D, ops._ptr(rowptr), ops._ptr(col),
            ops._ptr(adj.edge_cdf), n, ops._ptr(p["order"]), p["n_short"], ops._ptr(p["slices"]), p["n_slices"],
            ops._ptr(p["long_rows"]), p["n_long"], p["slice_len"], ops._ptr(partials), ldp, ops._ptr(out),
            ops._code(out.dtype), out.stride(0), act, ops._ptr(adj.err_flag), ops._stream()), "segment_reduce_weighted")
        return out
    kp, ldk = (None, 0) if keys is None else (ops._ptr(keys), keys.stride(0))
    nat.check(nat.lib().gsage_segment_reduce(
        mode, ops._ptr(table), ops._code(table.dtype), table.stride(0), D, kp, ldk, ops._ptr(rowptr), ops._ptr(col), n,
        ops._ptr(p["order"]), p["n_short"], ops._ptr(p["slices"]), p["n_slices"], ops._ptr(p["long_rows"]),
        p["n_long"], p["slice_len"], ops._ptr(partials), ldp, ops._ptr(out), ops._code(out.dtype), out.stride(0), act,
        ops._ptr(adj.err_flag), ops._stream()), "segment_reduce")
    return out


def _table(t):
    """t as a table the segment reduce can walk: rows of a whole number of 16-byte chunks."""
    vec = 16 // t.element_size()
    if t.stride(1) == 1 and t.stride(0) % vec == 0 and t.stride(0) >= _round_up(t.shape[1], vec) \
            and t.data_ptr() % 16 == 0:
        return t
    out = torch.zeros(t.shape[0], _round_up(t.shape[1], vec), dtype=t.dtype, device=t.device)
    out[:, :t.shape[1]] = t
    return out


# --------------------------------------------------------------------------------------------
# one layer
# --------------------------------------------------------------------------------------------
def _layer_device(layer, H, adj):
    """One layer over the whole graph, or over a Block: H holds the rows of the block's source set, the result its
    n_dst destination rows (a destination's local index is its index in H: fc_x reads H[:n_dst])."""
    code, post = _split_activation(layer.activation)
    cdt = ops.torch_dtype()
    h = layer.output_dim_
    n_src = int(H.shape[0])
    N = adj.n_dst if isinstance(adj, Block) else n_src
    out = torch.empty(N, 2 * h, dtype=torch.float32, device=H.device)
    Hd = H
    if N != n_src:                  # (a row prefix of rows this library padded keeps their tag: no padding copy)
        Hd = ops.mark_zero_padded(H[:N]) if ops._trusted(H) else H[:N]
    out[:, :h] = ops.linear(Hd, layer.fc_x.weight, None, code)
    right = out[:, h:]
    mean = nat.SEG_WEIGHTED_MEAN if _weighted(adj) else nat.SEG_MEAN
    if isinstance(layer, PoolAggregator) and layer.pool_fn == "max":
        lin = layer.mlp[0]
        Q = _table(ops.linear(H, lin.weight, lin.bias, nat.ACT_RELU, out_dtype=cdt))
        agg = torch.empty(N, lin.weight.shape[0], dtype=torch.float32, device=H.device)
        segment_reduce(adj, Q[:, :lin.weight.shape[0]], nat.SEG_MAX, agg)
        right.copy_(ops.linear(agg, layer.fc_neib.weight, None, code))
    elif isinstance(layer, PoolAggregator):
        lin = layer.mlp[0]
        Q = ops.linear(H, lin.weight, lin.bias, nat.ACT_RELU, out_dtype=cdt)
        P = _table(ops.linear(Q, layer.fc_neib.weight, None, nat.ACT_NONE, out_dtype=cdt))
        segment_reduce(adj, P[:, :h], mean, right, code)
    elif isinstance(layer, AttentionAggregator):
        P = _table(ops.linear(H, layer.fc_neib.weight, None, nat.ACT_NONE, out_dtype=cdt))
        A = layer._att(H)
        keys = torch.zeros(n_src, 32, dtype=torch.float32, device=H.device)
        keys[:, :A.shape[1]] = A
        segment_reduce(adj, P[:, :h], nat.SEG_SOFTMAX_WEIGHTED, right, code, keys=keys)
    else:
        P = _table(ops.linear(H, layer.fc_neib.weight, None, nat.ACT_NONE, out_dtype=cdt))
        segment_reduce(adj, P[:, :h], mean, right, code)
    return post(out) if post is not None else out


def _edges_weighted(adj):
    """_edges for a weighted adjacency, plus each edge's share p_e = q_e / T_v (float32: q_e < 2^24 is exact, one
    division).  Edges of quantum 0 are kept with p_e = 0; a row with T_v == 0 reads the dummy with p = 1."""
    rowptr, col, n = _csr(adj)
    deg = rowptr[1:] - rowptr[:-1]
    cdf = adj.edge_cdf                                   # (< 2^63: the int64 view orders and subtracts like the uint64)
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64), deg)
    first = torch.zeros(cdf.numel(), dtype=torch.bool)
    first[rowptr[:-1][deg > 0]] = True
    prev = torch.cat([torch.zeros(1, dtype=torch.int64), cdf[:-1]])
    q = cdf - torch.where(first, torch.zeros_like(prev), prev)
    T = torch.zeros(n, dtype=torch.int64)
    T[deg > 0] = cdf[rowptr[1:][deg > 0] - 1]
    keep = T[rows] > 0
    empty = torch.nonzero(T == 0).view(-1)
    dst = torch.cat([rows[keep], empty])
    src = torch.cat([col.long()[keep], torch.full_like(empty, int(getattr(adj, "dummy", 0)))])
    p = torch.cat([q[keep].float() / T[rows[keep]].float(), torch.ones(empty.numel())])
    order = torch.argsort(dst, stable=True)              # row-major, a row's edges in their stored order
    return src[order], dst[order], p[order], n


def _edges(adj):
    """(src, dst) of every edge of N(v), v = 0..n_rows-1, degree-0 rows reading the dummy (row 0; a Block: its local
    index there) (host mode)."""
    if _weighted(adj):
        return _edges_weighted(adj)
    rowptr, col, n = _csr(adj)
    deg = rowptr[1:] - rowptr[:-1]
    dst = torch.repeat_interleave(torch.arange(n, dtype=torch.int64), deg.clamp(min=1))
    src = torch.full((dst.numel(),), int(getattr(adj, "dummy", 0)), dtype=torch.int64)
    has = torch.repeat_interleave(deg > 0, deg.clamp(min=1))
    src[has] = col.long()
    return src, dst, deg.clamp(min=1), n


def _layer_host(layer, H, edges):
    src, dst, cnt, n = edges                             # (a Block: H has the n_src source rows, n = n_dst)
    code, post = _split_activation(layer.activation)
    if cnt.dtype.is_floating_point:                      # a weighted adjacency: cnt holds the edges' shares p_e
        X = torch.relu(F.linear(H, layer.mlp[0].weight, layer.mlp[0].bias)) if isinstance(layer, PoolAggregator) else H
        agg = torch.zeros(n, X.shape[1]).index_add_(0, dst, X[src] * cnt.unsqueeze(1))
    elif isinstance(layer, PoolAggregator):
        lin = layer.mlp[0]
        Q = torch.relu(F.linear(H, lin.weight, lin.bias))
        if layer.pool_fn == "max":
            agg = torch.full((n, Q.shape[1]), float("-inf")).scatter_reduce(
                0, dst.unsqueeze(1).expand(-1, Q.shape[1]), Q[src], "amax", include_self=True)
        else:
            agg = torch.zeros(n, Q.shape[1]).index_add_(0, dst, Q[src]) / cnt.unsqueeze(1).float()
    elif isinstance(layer, AttentionAggregator):
        A = F.linear(torch.tanh(F.linear(H, layer.att[0].weight)), layer.att[2].weight)
        s = (A[src] * A[dst]).sum(1)
        smax = torch.full((n,), float("-inf")).scatter_reduce(0, dst, s, "amax", include_self=True)
        e = torch.exp(s - smax[dst])
        den = torch.zeros(n).index_add_(0, dst, e)
        agg = torch.zeros(n, H.shape[1]).index_add_(0, dst, H[src] * (e / den[dst]).unsqueeze(1))
    else:
        agg = torch.zeros(n, H.shape[1]).index_add_(0, dst, H[src]) / cnt.unsqueeze(1).float()
    out = torch.cat([F.linear(H[:n], layer.fc_x.weight), F.linear(agg, layer.fc_neib.weight)], dim=1)
    if code == nat.ACT_RELU:
        out = torch.relu(out)
    return post(out) if post is not None else out


# --------------------------------------------------------------------------------------------
# entry point
# --------------------------------------------------------------------------------------------
def _feature_rows(feats, n):
    """The first n rows of the features as a 2-d tensor (a FeatureStore's zero-padded rows, no copy)."""
    if isinstance(feats, FeatureStore):
        if int(feats.data.shape[0]) < n:
            raise ValueError("full-neighbour inference: %d feature rows for an adjacency of %d rows"
                             % (int(feats.data.shape[0]), n))
        if feats.is_fp8:                       # level 0 is decoded ONCE (the FP8 row gather); every layer reads the copy
            feats = feats.decoded(ops.config.compute_dtype if feats.is_cuda else "fp32", n_rows=n)
        return ops.mark_zero_padded(feats.data[:n, :feats.dim])
    if int(feats.shape[0]) < n:
        raise ValueError("full-neighbour inference: %d feature rows for an adjacency of %d rows" % (int(feats.shape[0]), n))
    return feats[:n]


def embeddings(model, feats, adj=None):
    """F.normalize(H^L) of every row of the adjacency, [n_rows, width], by layer-wise full-neighbourhood inference --
    for a GSSupervised (the rows its `fc` classifies) and for a GSUnsupervised (its output).

    feats: a FeatureStore or a tensor; its device decides the route (CUDA: the library's kernels, CPU: host mode).
    adj: a store.DeviceCSR / store.DenseAdj; default: the adjacency evaluation samples from (model.val_sampler).
    The model's current Parameters are read (also when a fused engine trained them).  Raises ValueError for a model
    without a full-neighbourhood form (check_supported)."""
    check_supported(model)
    dev = feats.device
    if adj is None:
        adj = model.val_sampler.csr(dev)
    if _weighted(adj):
        check_supported(model, adj)
    with torch.no_grad():
        settle = getattr(model, "_settle_rows", None)
        if settle is not None:
            settle()
        n = int(adj.n_rows)
        X = _feature_rows(feats, n)
        if dev.type == "cuda":
            H = ops.linear(X, model.prep.fc.weight) if isinstance(model.prep, LinearPrep) else X
            for layer in model.agg_layers.children():
                H = _layer_device(layer, H, adj)
        else:
            H = X.float()
            if isinstance(model.prep, LinearPrep):
                H = F.linear(H, model.prep.fc.weight)
            edges = _edges(adj)
            for layer in model.agg_layers.children():
                H = _layer_host(layer, H, edges)
        return F.normalize(H.float(), dim=1)


def full_neighbour(model, feats, nodes=None, adj=None, embeddings=False, closure=False):
    """Logits of `model` for `nodes` (default: every row of the adjacency) by layer-wise full-neighbourhood inference,
    and, with embeddings=True, also F.normalize(H^L) for every row: returns (logits, emb).  Arguments as for
    embeddings() above, which computes emb; this applies the model's `fc` to it.  closure=True (needs `nodes`): the same
    numbers from the nodes' k-hop closure alone -- query() below, whose emb holds the rows of `nodes` only."""
    if closure:
        if nodes is None:
            raise ValueError("full_neighbour(closure=True) needs the nodes to answer for")
        return query(model, feats, nodes, adj=adj, embeddings=embeddings)
    emb = _embeddings(model, feats, adj=adj)
    dev = feats.device
    with torch.no_grad():
        sel = emb if nodes is None else emb[torch.as_tensor(nodes, device=dev).long().view(-1)]
        if dev.type == "cuda":
            logits = ops.linear(sel, model.fc.weight, model.fc.bias, compute_dtype="fp32")
        else:
            logits = model.fc(sel)
    return (logits, emb) if embeddings else logits


_embeddings = embeddings          # (full_neighbour's keyword of the same name shadows the function inside it)


# --------------------------------------------------------------------------------------------
# a query set: k-hop closure blocks
# --------------------------------------------------------------------------------------------
class Block(object):
    """Block l of a closure: destinations S_l (n_dst rows), sources S_{l-1} (n_src rows, S_l as a prefix).  rowptr
    int64 [n_dst + 1]; col int32: the destinations' stored rows, whole, in stored order, as local indices into the
    source set; edge_cdf: the rows' segments of a weighted adjacency's table, verbatim; dummy: the local index of
    global row 0.  Quacks like an adjacency for plan() and segment_reduce() (n_rows = n_dst); err_flag is the
    adjacency's own."""

    def __init__(self, rowptr, col, n_dst, n_src, dummy, err_flag, edge_cdf=None, buffers=None):
        self.rowptr, self.col, self.edge_cdf = rowptr, col, edge_cdf
        self.n_rows = self.n_dst = int(n_dst)
        self.n_src, self.dummy = int(n_src), int(dummy)
        self.err_flag = err_flag
        # (device blocks: the allocations col / edge_cdf are views of, at least one element each -- a block without
        #  edges, every destination of degree 0, still hands the kernels a pointer)
        self._buffers = buffers if buffers is not None else (col, edge_cdf)

    def col_ptr(self):
        return ops._ptr(self._buffers[0])

    def cdf_ptr(self):
        return ops._ptr(self._buffers[1])

    @property
    def device(self):
        return self.rowptr.device


class Closure(object):
    """closure()'s result for depth L: sets[l] = the global ids of S_l (int64; l = 0 .. L, every S_l a prefix of
    S_0), blocks[l] = Block l for l = 1 .. L (blocks[0] is None), index = the local index in S_L of every query, in the
    caller's order (int64; duplicates repeat)."""

    def __init__(self, sets, blocks, index):
        self.sets, self.blocks, self.index = sets, blocks, index
        self.depth = len(sets) - 1

    def sizes(self):
        return [int(s.shape[0]) for s in self.sets]


def scan_span():
    """Items per workgroup of the closure kernels' scans (bitmap words, set members, queries): 32 x this many rows."""
    return int(nat.lib().gsage_closure_span())


def _closure_state(adj, n, dev):
    """The local map (int32 [n_rows], -1 = absent) and the bitmap of the closure kernels, cached on the adjacency the
    way the plan is; both are back at rest when closure() returns."""
    st = getattr(adj, "_closure_state", None)
    if st is None:
        span = scan_span()
        n_words = (n + 31) // 32
        st = {"local": torch.full((n,), -1, dtype=torch.int32, device=dev),
              "bitmap": torch.zeros(n_words, dtype=torch.int32, device=dev), "span": span,
              "sums_words": torch.empty((n_words + span - 1) // span + 1, dtype=torch.int64, device=dev),
              "counts": torch.zeros(3, dtype=torch.int64, device=dev)}
        adj._closure_state = st
    return st


def _closure_device(adj, nodes, depth):
    rowptr, col, n = _csr(adj)
    cdf = adj.edge_cdf if _weighted(adj) else None
    dev = rowptr.device
    st = _closure_state(adj, n, dev)
    L, span = nat.lib(), st["span"]
    local, bitmap, counts = ops._ptr(st["local"]), ops._ptr(st["bitmap"]), st["counts"]
    err, stream = ops._ptr(adj.err_flag), ops._stream()
    q = nodes.to(device=dev, dtype=torch.int64).contiguous().view(-1)
    nq = int(q.shape[0])

    def i64(k):
        return torch.empty(k, dtype=torch.int64, device=dev)
    try:
        sums_q = i64(nq // span + 2)
        nat.check(L.gsage_closure_seed_count(ops._ptr(q), nq, n, local, ops._ptr(sums_q), ops._ptr(counts), err, stream),
                  "closure_seed_count")
        n_set = int(counts.tolist()[0])                # (the seed level's one readback)
        S, index = i64(n_set), i64(nq)
        nat.check(L.gsage_closure_seed_write(ops._ptr(q), nq, n, local, ops._ptr(sums_q), ops._ptr(S), n_set,
                                             ops._ptr(index), stream), "closure_seed_write")
        if n_set == 0:
            adj.err_flag.zero_()
            raise IndexError("closure: no query id lies inside the adjacency")
        sizes, blocks, lo = [n_set], [None] * (depth + 1), 0
        for l in range(depth, 0, -1):
            hi = int(S.shape[0])
            sums_rows = i64(hi // span + 2)
            nat.check(L.gsage_closure_expand_count(ops._ptr(rowptr), ops._ptr(col), n, ops._ptr(S), lo, hi, local, bitmap,
                                                   ops._ptr(st["sums_words"]), ops._ptr(sums_rows), ops._ptr(counts),
                                                   err, stream), "closure_expand_count")
            n_new, nnz, dummy = (int(v) for v in counts.tolist())          # (the hop's one readback: 24 bytes)
            grown = i64(hi + n_new)
            grown[:hi] = S
            brow = i64(hi + 1)
            colbuf = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
            cdfbuf = i64(max(nnz, 1)) if cdf is not None else None
            nat.check(L.gsage_closure_expand_write(ops._ptr(rowptr), ops._ptr(col), ops._ptr(cdf), n, ops._ptr(grown), hi,
                                                   local, bitmap, ops._ptr(st["sums_words"]), ops._ptr(sums_rows),
                                                   ops._ptr(brow), ops._ptr(colbuf), ops._ptr(cdfbuf), err, stream),
                      "closure_expand_write")
            blocks[l] = Block(brow, colbuf[:nnz], hi, hi + n_new, dummy, adj.err_flag,
                              None if cdfbuf is None else cdfbuf[:nnz], buffers=(colbuf, cdfbuf))
            S, lo = grown, hi
            sizes.append(hi + n_new)
        nat.check(L.gsage_closure_restore(ops._ptr(S), int(S.shape[0]), local, stream), "closure_restore")
    except BaseException:
        adj._closure_state = None          # (left mid-way: the next call starts from a fresh map and bitmap)
        raise
    sizes.reverse()
    return Closure([S[:k] for k in sizes], blocks, index)


def _closure_host(adj, nodes, depth):
    """closure() for CPU tensors: the same definition in numpy.  An id outside the graph raises on the spot."""
    rowptr, col, n = _csr(adj)
    rp, cl = rowptr.numpy(), col.numpy()
    cdf = adj.edge_cdf.numpy() if _weighted(adj) else None
    q = np.asarray(nodes.cpu().numpy() if torch.is_tensor(nodes) else nodes, dtype=np.int64).reshape(-1)
    if q.size and (q.min() < 0 or q.max() >= n):
        raise IndexError("closure: query id out of range of the adjacency")
    if cl.size and (cl.min() < 0 or cl.max() >= n):
        raise IndexError("closure: the adjacency holds ids outside [0, n_rows)")
    _, first = np.unique(q, return_index=True)
    S = q[np.sort(first)]
    local = np.full(n, -1, dtype=np.int64)
    local[S] = np.arange(S.size)
    index = local[q]
    sizes, blocks, lo = [S.size], [None] * (depth + 1), 0
    for l in range(depth, 0, -1):
        hi = S.size
        deg = rp[S + 1] - rp[S]
        brow = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        edge = np.repeat(rp[S] - brow[:-1], deg) + np.arange(int(brow[-1]))    # the stored edges of S, row by row
        nb = cl[edge]
        cand = np.unique(np.concatenate([nb[brow[lo]:], [0]]))                # (older members' rows are inside S already)
        cand = cand[local[cand] < 0]
        local[cand] = hi + np.arange(cand.size)
        S = np.concatenate([S, cand])
        blocks[l] = Block(torch.from_numpy(brow), torch.from_numpy(local[nb].astype(np.int32)), hi, S.size, local[0],
                          adj.err_flag, None if cdf is None else torch.from_numpy(cdf[edge]))
        sizes.append(S.size)
        lo = hi
    sizes.reverse()
    S = torch.from_numpy(S)
    return Closure([S[:k] for k in sizes], blocks, torch.from_numpy(index))


def closure(adj, nodes, depth):
    """The k-hop closure of `nodes` over `adj` (a store.DeviceCSR / store.DenseAdj) for `depth` layers -> Closure.
    S_depth = the nodes, duplicates removed, in order of first appearance; S_{l-1} = S_l, then the nodes of N(S_l) and
    the dummy 0 not yet present, in ascending id; block l = the stored rows of S_l relabelled into S_{l-1}.  A CUDA
    adjacency runs csrc/gsage_block.hip (six launches for the seed level, seven per hop plus torch's copy of the set's
    prefix, one to restore the state, and one readback per level -- whatever the sizes; an id outside
    the graph raises the adjacency's err_flag -- adj.check() -- and is left out), a CPU one the same definition in numpy."""
    depth = int(depth)
    if depth < 1:
        raise ValueError("closure: depth must be at least 1, not %d" % depth)
    nodes = torch.as_tensor(nodes)
    if nodes.dtype.is_floating_point or nodes.dtype == torch.bool:
        raise ValueError("closure: node ids must be integers, not %s" % nodes.dtype)
    if nodes.numel() == 0:
        raise ValueError("closure: no nodes to answer for")
    if _csr(adj)[0].is_cuda:
        return _closure_device(adj, nodes, depth)
    return _closure_host(adj, nodes, depth)


def _gathered_rows(feats, ids, n):
    """The feature rows of `ids` (the closure's S_0) through the row gather: level 0 of a query.  An FP8 store is decoded
    for these rows only."""
    dev = feats.device
    M = int(ids.shape[0])
    rows = int(feats.data.shape[0]) if isinstance(feats, FeatureStore) else int(feats.shape[0])
    if rows < n:
        raise ValueError("full-neighbour inference: %d feature rows for an adjacency of %d rows" % (rows, n))
    if dev.type != "cuda":
        if isinstance(feats, FeatureStore):
            return ops._store_gather(feats, feats.dim, ids, M, 1, torch.float32)
        return feats[ids].float()
    if isinstance(feats, FeatureStore):
        dt = ops.torch_dtype() if feats.is_fp8 else feats.dtype
        ld = _round_up(feats.dim, 64 if dt == torch.bfloat16 else 32)
        return ops.mark_zero_padded(ops._store_gather(feats, feats.dim, ids, M, 1, dt, ld)[:, :feats.dim])
    if feats.dtype not in (torch.float32, torch.bfloat16) or feats.dim() != 2:
        return feats[ids]
    table = feats if feats.stride(1) == 1 else feats.contiguous()
    return ops._gather_mean_raw(table, int(table.shape[1]), ids, M, 1, table.dtype)


def _query(model, feats, nodes, adj, cl=None):
    """(F.normalize(H^L) of the distinct nodes, their Closure -- `cl` when the caller built it already --, the adjacency)"""
    check_supported(model)
    dev = feats.device
    if adj is None:
        adj = model.val_sampler.csr(dev)
    if _weighted(adj):
        check_supported(model, adj)
    layers = list(model.agg_layers.children())
    with torch.no_grad():
        settle = getattr(model, "_settle_rows", None)
        if settle is not None:
            settle()
        if cl is None:
            cl = closure(adj, torch.as_tensor(nodes).to(dev), len(layers))
        elif cl.depth != len(layers) or int(cl.index.shape[0]) != int(torch.as_tensor(nodes).numel()):
            raise ValueError("query: the closure given was not built for these nodes and this model's depth")
        X = _gathered_rows(feats, cl.sets[0], int(adj.n_rows))
        if dev.type == "cuda":
            H = ops.linear(X, model.prep.fc.weight) if isinstance(model.prep, LinearPrep) else X
            for l, layer in enumerate(layers, 1):
                H = _layer_device(layer, H, cl.blocks[l])
        else:
            H = F.linear(X, model.prep.fc.weight) if isinstance(model.prep, LinearPrep) else X
            for l, layer in enumerate(layers, 1):
                H = _layer_host(layer, H, _edges(cl.blocks[l]))
        return F.normalize(H.float(), dim=1), cl, adj


def query_embeddings(model, feats, nodes, adj=None):
    """F.normalize(H^L) of `nodes`, [len(nodes), width], in the caller's order (duplicates repeat), computed from the
    nodes' k-hop closure alone -- the rows embeddings() would give for them.  Arguments as for embeddings()."""
    emb, cl, adj = _query(model, feats, nodes, adj)
    adj.check()
    return emb[cl.index]


def query(model, feats, nodes, adj=None, embeddings=False, closure=None):
    """Logits of `model` for `nodes` by full-neighbourhood inference over their k-hop closure (closure() above): what
    full_neighbour(model, feats, nodes=nodes) returns, at a cost that follows the closure instead of the graph.  Results
    come back in the caller's order, duplicates repeated; embeddings=True: (logits, F.normalize(H^L) of `nodes`).
    Arguments and refusals as for embeddings(); a node id outside the adjacency is an IndexError.  closure: the Closure
    of `nodes` over `adj` at the model's depth, when the caller has built it already (several models, one query set)."""
    emb, cl, adj = _query(model, feats, nodes, adj, cl=closure)
    with torch.no_grad():
        if feats.device.type == "cuda":
            logits = ops.linear(emb, model.fc.weight, model.fc.bias, compute_dtype="fp32")
        else:
            logits = model.fc(emb)
    adj.check()
    logits = logits[cl.index]
    return (logits, emb[cl.index]) if embeddings else logits


# --------------------------------------------------------------------------------------------
# retrieval over the exported embeddings
# --------------------------------------------------------------------------------------------
def nearest(emb, nodes=None, k=10, exclude="self", adj=None):
    """The k rows of `emb` nearest to the rows of `nodes` by inner product -- on the unit rows embeddings() returns,
    the cosine, whose order is the Euclidean one: -> (ids int64 [Q, k], scores fp32 [Q, k]), best first under the total
    order (score descending, row id ascending); ops.topk_ip.

    emb: what embeddings() / query_embeddings() return, or any [N, D] float tensor.  nodes: the node ids whose rows are
    the queries, answered in the caller's order, duplicates repeatedly; None: every row (the k-NN graph).  exclude:
    "none", "self" (a node is not its own neighbour) or "neighbours" (neither itself nor a node it already has an edge
    to in `adj`, a store.DeviceCSR; a WeightedAdj is read as its CSR): link recommendation.  Fewer than k allowed rows:
    id -1, score -inf.  A node id outside the table is an IndexError."""
    if not torch.is_tensor(emb) or emb.dim() != 2 or not emb.is_floating_point():
        raise ValueError("nearest: emb must be a [N, D] float tensor")
    dev = emb.device
    N = int(emb.shape[0])
    if nodes is None:
        ids = torch.arange(N, dtype=torch.int64, device=dev)
        queries = emb
    else:
        ids = torch.as_tensor(nodes)
        if ids.is_floating_point() or ids.dtype == torch.bool:
            raise ValueError("nearest: node ids must be integers, not %s" % ids.dtype)
        ids = ids.to(dev).long().view(-1)
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= N):
            raise IndexError("nearest: node id out of range of the %d embedding rows" % N)
        queries = emb[ids]
    csr = None
    if exclude == "neighbours":
        if adj is None:
            raise ValueError("nearest: exclude='neighbours' needs adj (a store.DeviceCSR)")
        if isinstance(adj, DenseAdj):
            raise ValueError("nearest: exclude='neighbours' reads a CSR; a DenseAdj holds samples, not the edges")
        if isinstance(adj, (WeightedAdj, TemporalAdj)):      # (a TemporalAdj: every stored edge, whatever its time)
            adj = DeviceCSR.from_scipy(adj.adj, dev)
        if not isinstance(adj, DeviceCSR):
            raise ValueError("nearest: adj must be a store.DeviceCSR or a store.WeightedAdj")
        csr = adj
    return ops.topk_ip(emb, queries, k, query_ids=ids, csr=csr, exclude=exclude)


# --------------------------------------------------------------------------------------------
# exact link ranking over the exported embeddings
# --------------------------------------------------------------------------------------------
def _as_csr(adj, dev, who):
    """`adj` as a store.DeviceCSR: a WeightedAdj is read as its CSR, a DenseAdj is refused with nearest()'s sentence."""
    if isinstance(adj, DenseAdj):
        raise ValueError("%s: exclude='neighbours' reads a CSR; a DenseAdj holds samples, not the edges" % who)
    if isinstance(adj, (WeightedAdj, TemporalAdj)):
        got = getattr(adj, "_device_csr", None)
        if got is None or got.device != torch.device(dev):
            got = DeviceCSR.from_scipy(adj.adj, dev)
            adj._device_csr = got
        adj = got
    if not isinstance(adj, DeviceCSR):
        raise ValueError("%s: adj must be a store.DeviceCSR or a store.WeightedAdj" % who)
    return adj


def filter_csr(adj):
    """The stored edges of `adj` (a store.DeviceCSR, columns in any order, duplicates allowed) as the STRICTLY ASCENDING
    CSR ops.rank_ip's filter wants: per row the distinct columns inside [0, n_rows), sorted.  Built once by torch ops on
    the keys row * n_rows + col (sort, unique_consecutive) and cached on the adjacency object the way the closure
    caches its local map; `.keys` keeps the sorted keys (held_out_edges looks edges up in them)."""
    got = getattr(adj, "_rank_filter", None)
    if got is not None:
        return got
    n = int(adj.n_rows)
    rowptr, col = adj.rowptr, adj.col.long()
    row = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=rowptr.device), rowptr[1:] - rowptr[:-1])
    ok = (col >= 0) & (col < n)
    keys = torch.unique_consecutive(torch.sort(row[ok] * n + col[ok]).values)
    counts = torch.bincount(torch.div(keys, n, rounding_mode="floor"), minlength=n)
    new_ptr = torch.zeros(n + 1, dtype=torch.int64, device=rowptr.device)
    torch.cumsum(counts, 0, out=new_ptr[1:])
    got = DeviceCSR(new_ptr, (keys % n).to(torch.int32), n, adj.max_deg)
    got.keys = keys
    adj._rank_filter = got
    return got


def _pair_ids(ids, dev, who, name, N=None):
    ids = torch.as_tensor(ids)
    if ids.is_floating_point() or ids.dtype == torch.bool:
        raise ValueError("%s: %s must be integers, not %s" % (who, name, ids.dtype))
    ids = ids.to(dev).long().view(-1)
    if N is not None and ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= N):
        raise IndexError("%s: %s id out of range of the %d embedding rows" % (who, name, N))
    return ids


def link_rank(emb, src, dst, exclude="neighbours", adj=None):
    """Where does dst[i] rank among ALL rows of `emb` as a neighbour of src[i]?  -> (ranks int64 [P], scores fp32 [P])
    for the pairs in the caller's order, duplicates repeated: rank = 1 + the number of allowed rows that beat dst by
    inner product with emb[src] under the total order (score descending, row id ascending); ops.rank_ip, exact.

    exclude: "none"; "self" (src itself does not count); "neighbours" (the filtered setting of link prediction: neither
    src nor a node src already has an edge to in `adj` counts against dst -- dst itself always stays).  adj: a
    store.DeviceCSR with columns in any order (the strictly ascending filter is built from it once and cached on it);
    a WeightedAdj is read as its CSR.  A pair whose score is NaN is unranked: rank 0.  An id outside the table is an
    IndexError."""
    if not torch.is_tensor(emb) or emb.dim() != 2 or not emb.is_floating_point():
        raise ValueError("link_rank: emb must be a [N, D] float tensor")
    if exclude not in ops.TOPK_EXCLUDE:
        raise ValueError("link_rank: exclude must be one of %s, not %r" % (sorted(ops.TOPK_EXCLUDE), exclude))
    dev, N = emb.device, int(emb.shape[0])
    src = _pair_ids(src, dev, "link_rank", "src", N)
    dst = _pair_ids(dst, dev, "link_rank", "dst", N)
    if int(src.shape[0]) != int(dst.shape[0]):
        raise ValueError("link_rank: %d src for %d dst" % (int(src.shape[0]), int(dst.shape[0])))
    csr = None
    if exclude == "neighbours":
        if adj is None:
            raise ValueError("link_rank: exclude='neighbours' needs adj (a store.DeviceCSR)")
        csr = filter_csr(_as_csr(adj, dev, "link_rank"))
    if src.numel() == 0:
        return torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.float32, device=dev)
    return ops.rank_ip(emb, emb[src], dst, query_ids=src, csr=csr, exclude=exclude)


def link_metrics(ranks, ks=(1, 10, 50)):
    """{"n", "unranked", "mrr", "mean_rank", "hits@k"...} of link_rank's ranks.  An unranked pair (rank 0) counts as
    reciprocal rank 0 and as a miss, and is left out of mean_rank (None when no pair is ranked)."""
    r = np.asarray(ranks.cpu().numpy() if torch.is_tensor(ranks) else ranks, dtype=np.int64).reshape(-1)
    if (r < 0).any():
        raise ValueError("link_metrics: ranks are >= 1, or 0 for unranked")
    n, live = int(r.size), r[r > 0].astype(np.float64)
    out = {"n": n, "unranked": n - int(live.size),
           "mrr": float((1.0 / live).sum() / n) if n else 0.0,
           "mean_rank": float(live.mean()) if live.size else None}
    for k in ks:
        k = int(k)
        if k < 1:
            raise ValueError("link_metrics: ks must be >= 1, not %d" % k)
        out["hits@%d" % k] = float((live <= k).sum() / n) if n else 0.0
    return out


def held_out_edges(adj, train_adj, nodes):
    """The stored edges (u, v) of `adj` with u in `nodes` that `train_adj` does not store -> (src, dst) int64, on the
    adjacency's device: by u in the caller's order (a repeated node repeats its edges), then v ascending; a duplicate
    stored edge counts once.  adj, train_adj: store.DeviceCSR (a WeightedAdj is read as its CSR)."""
    dev = adj.device if isinstance(adj, DeviceCSR) else torch.device("cpu")
    full = filter_csr(_as_csr(adj, dev, "held_out_edges"))
    seen = filter_csr(_as_csr(train_adj, dev, "held_out_edges"))
    n = int(full.n_rows)
    u = _pair_ids(nodes, dev, "held_out_edges", "node")
    if u.numel() and (int(u.min()) < 0 or int(u.max()) >= n):
        raise IndexError("held_out_edges: node id out of range of the adjacency")
    deg = full.rowptr[u + 1] - full.rowptr[u]
    first = torch.cumsum(deg, 0) - deg
    src = torch.repeat_interleave(u, deg)
    pos = torch.arange(int(src.shape[0]), dtype=torch.int64, device=dev) - torch.repeat_interleave(first, deg)
    dst = full.col[torch.repeat_interleave(full.rowptr[u], deg) + pos].long()
    m = int(seen.n_rows)
    if seen.keys.numel():
        key = src * m + dst
        at = torch.searchsorted(seen.keys, key).clamp_(max=int(seen.keys.shape[0]) - 1)
        stored = (seen.keys[at] == key) & (src < m) & (dst < m)
    else:
        stored = torch.zeros_like(src, dtype=torch.bool)
    return src[~stored].contiguous(), dst[~stored].contiguous()


# --------------------------------------------------------------------------------------------
# linear probe over the exported embeddings
# --------------------------------------------------------------------------------------------
PROBE_BETAS, PROBE_EPS = (0.9, 0.999), 1e-8


class LinearProbe(object):
    """A linear classifier fitted on frozen embeddings (linear_probe): W fp32 [C, D], b fp32 [C], the loss of every
    iteration (loss_history fp32 [iters]) and the task it was fitted for."""

    def __init__(self, W, b, loss_history, task):
        self.W, self.b, self.loss_history, self.task = W, b, loss_history, task

    def logits(self, emb, nodes=None):
        """emb[nodes] @ W^T + b (every row when nodes is None), fp32, through ops.linear."""
        x = emb if nodes is None else emb[_pair_ids(nodes, emb.device, "LinearProbe.logits", "node", int(emb.shape[0]))]
        return ops.linear(x, self.W, self.b)

    def predict(self, emb, nodes=None):
        """classification: the arg-max class, int64 [n]; multilabel_classification: the labels whose logit is positive,
        bool [n, C] -- what the F1 metrics of problem.py count."""
        z = self.logits(emb, nodes)
        return z.argmax(dim=1) if self.task == "classification" else z > 0


def linear_probe(emb, targets, nodes, task, n_classes=None, iters=100, lr=0.1, weight_decay=0.0):
    """Fit a linear classifier on the rows `nodes` of the frozen embeddings `emb` [N, D] -> LinearProbe: the GraphSAGE
    paper's judgement of unsupervised embeddings.  targets: one per node of `nodes`, in its order -- int64 class ids
    [n] for task "classification", float [n, C] in [0, 1] for "multilabel_classification".  n_classes: C (default:
    the largest class id + 1, or the targets' columns).

    Zero-initialised W, b; `iters` steps of full-batch Adam (betas 0.9 / 0.999, eps 1e-8, `weight_decay` as Adam's
    L2 term, no clipping).  On CUDA one iteration is ops.probe_pass's kernels (csrc/gsage_probe.hip),
    gsage_finalize_grads and gsage_clip_adam_step, recorded once as a command list and replayed `iters` times
    without a host synchronisation; the loss of iteration t lands in loss_history[t], read back by the caller when it
    wants it.  CPU tensors: the same loop over ops.probe_pass's host definition.  Deterministic: two fits on the same
    inputs are bit-identical.  Refused with a sentence: regression tasks, C > 128, D > 1024, targets of the wrong
    dtype or shape, node ids outside the table, class ids outside [0, C)."""
    ops.probe_task(task)
    if not torch.is_tensor(emb) or emb.dim() != 2 or not emb.is_floating_point():
        raise ValueError("linear_probe: emb must be a [N, D] float tensor")
    iters = int(iters)
    if iters < 1:
        raise ValueError("linear_probe: iters must be at least 1, not %d" % iters)
    dev, N, D = emb.device, int(emb.shape[0]), int(emb.shape[1])
    targets = torch.as_tensor(targets)
    if n_classes is None:
        if task == "classification":
            if targets.is_floating_point() or targets.numel() == 0:
                raise ValueError("linear_probe: classification targets must be integer class ids, not %s" % targets.dtype)
            n_classes = int(targets.max()) + 1
        else:
            if targets.dim() != 2:
                raise ValueError("linear_probe: multilabel targets must have shape [n, C], not %s" % (tuple(targets.shape),))
            n_classes = int(targets.shape[1])
    C = int(n_classes)
    ids, y = ops.probe_check(emb, nodes, targets, C, D, task, who="linear_probe")
    if int(ids.min()) < 0 or int(ids.max()) >= N:
        raise IndexError("linear_probe: node id out of range of the %d embedding rows" % N)
    if task == "classification":
        if int(y.min()) < 0 or int(y.max()) >= C:
            raise ValueError("linear_probe: class id out of range [0, %d)" % C)
    elif float(y[:, :C].min()) < 0.0 or float(y[:, :C].max()) > 1.0:
        raise ValueError("linear_probe: multilabel targets must lie in [0, 1]")
    f32, total = torch.float32, C * D + C
    b1, b2 = PROBE_BETAS
    if not emb.is_cuda:
        # host mode: the same loop over the float64 definition, torch.optim.Adam's arithmetic in fp32
        p = torch.zeros(total, dtype=f32)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        hist = torch.zeros(iters, dtype=f32)
        for t in range(iters):
            loss, dW, db = ops.probe_pass(emb, ids, y, p[:C * D].view(C, D), p[C * D:], task)
            g = torch.cat([dW.reshape(-1), db]) + weight_decay * p
            m = b1 * m + (1 - b1) * g
            v = b2 * v + (1 - b2) * g * g
            step = lr / (1 - b1 ** (t + 1))
            p = p - step * m / (v.sqrt() / (1 - b2 ** (t + 1)) ** 0.5 + PROBE_EPS)
            hist[t] = loss
        return LinearProbe(p[:C * D].view(C, D).clone(), p[C * D:].clone(), hist, task)

    fit = ProbeIteration(emb, ids, y, task, C, iters, lr, weight_decay)
    fit.replay(iters)
    probe = LinearProbe(fit.flat_p[:C * D].view(C, D), fit.flat_p[C * D:], fit.loss_history, task)
    probe._fit = fit                                   # the recorded list and its buffers: alive until the replays ran
    return probe


class ProbeIteration(object):
    """One Adam iteration of the probe on the device -- gsage_probe_pass (two launches), gsage_finalize_grads,
    gsage_clip_adam_step -- recorded once as a command list; replay(k) issues it k times without a host
    synchronisation.  Iteration t (counted on the device) writes its loss to loss_history[t], t < capacity.
    emb, ids, y: as ops.probe_check returns them; the parameters live in flat_p = [W | b], zero-initialised."""

    def __init__(self, emb, ids, y, task, C, capacity, lr, weight_decay):
        from .engine.common import _ReduceDesc
        lib, code = nat.lib(), ops.PROBE_TASKS[task]
        dev, f32 = emb.device, torch.float32
        N, D = int(emb.shape[0]), int(emb.shape[1])
        self.E = E = ops.probe_operand(emb, D)
        self.ids, self.y = ids, y
        n, total = int(ids.shape[0]), C * D + C
        floats, S = ops.probe_scratch(n, C, D, 0)
        self.splits, self.capacity = S, int(capacity)
        self.flat_p = flat_p = torch.zeros(total, dtype=f32, device=dev)
        self.flat_g, self.flat_m, self.flat_v = (torch.zeros_like(flat_p) for _ in range(3))
        self.partial = torch.empty(floats, dtype=f32, device=dev)
        n_sq = int(lib.gsage_finalize_partials(1, total))
        self.sq = torch.zeros(max(n_sq, int(lib.gsage_adam_partials(total))), dtype=f32, device=dev)
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)
        self.lr_t = torch.tensor([float(lr)], dtype=f32, device=dev)
        self.loss_history = torch.zeros(self.capacity, dtype=f32, device=dev)
        desc = _ReduceDesc(self.partial.data_ptr(), total + 1, 0, S, 1, total, total + 1)
        self.descs = torch.frombuffer(bytearray(bytes(desc)), dtype=torch.uint8).to(dev)
        self.issued = 0
        b1, b2 = PROBE_BETAS
        stream = ops._stream()
        with nat.CommandList.record() as cl:
            # the pass reads the step count BEFORE the finalisation ticks it: iteration t writes loss_history[t]
            nat.check(lib.gsage_probe_loss_index_next(self.step.data_ptr()), "probe_loss_index_next")
            nat.check(lib.gsage_probe_pass(ops._ptr(E), ops._code(E.dtype), E.stride(0), N, ops._ptr(ids), n, ops._ptr(y),
                                           code, y.stride(0) if code else 0, flat_p.data_ptr(),
                                           flat_p[C * D:].data_ptr(), C, D, 0, self.partial.data_ptr(),
                                           self.loss_history.data_ptr(), stream), "probe_pass")
            nat.check(lib.gsage_finalize_grads(self.descs.data_ptr(), 1, total, self.flat_g.data_ptr(), self.sq.data_ptr(),
                                               self.step.data_ptr(), None, 0, None, 0, stream), "finalize_grads")
            nat.check(lib.gsage_clip_adam_step(flat_p.data_ptr(), self.flat_g.data_ptr(), self.flat_m.data_ptr(),
                                               self.flat_v.data_ptr(), total, self.sq.data_ptr(), self.lr_t.data_ptr(),
                                               self.step.data_ptr(), b1, b2, PROBE_EPS, float(weight_decay), 3.0e38, None,
                                               1, n_sq, None, 0, None, 0, None, 0, stream), "clip_adam_step")
        self.cl = cl

    def replay(self, k=1):
        if self.issued + k > self.capacity:
            raise ValueError("ProbeIteration: %d iterations asked of a loss history of %d" % (self.issued + k, self.capacity))
        stream = ops._stream()
        for _ in range(k):
            self.cl.replay(stream)
        self.issued += k


def probe_eval(emb, problem, iters=100, lr=0.1, weight_decay=0.0):
    """Fit a linear probe on the embeddings of problem.nodes['train'] and score the val and test folds with the
    problem's F1 metric (on the device for CUDA tensors) ->
    {"task", "iters", "loss_first", "loss_last", "val": {"micro", "macro"}, "test": {...}}."""
    from .problem import batch_metric
    task = problem.task
    ops.probe_task(task)
    dev = emb.device

    def fold(name):
        nodes = np.asarray(problem.nodes[name]).reshape(-1)
        y = torch.as_tensor(np.asarray(problem.targets[nodes]))
        y = y.long().view(-1) if task == "classification" else y.float()
        return torch.as_tensor(nodes).long().to(dev), y.to(dev)

    nodes, y = fold("train")
    C = int(problem.n_classes)
    probe = linear_probe(emb, y, nodes, task, n_classes=C, iters=iters, lr=lr, weight_decay=weight_decay)
    out = {"task": task, "iters": int(iters)}
    for name in ("val", "test"):
        nodes, y = fold(name)
        out[name] = batch_metric(task, y, probe.logits(emb, nodes)) if nodes.numel() else None
    hist = probe.loss_history.cpu()
    out["loss_first"], out["loss_last"] = float(hist[0]), float(hist[-1])
    return out


# --------------------------------------------------------------------------------------------
# k-means over the exported embeddings
# --------------------------------------------------------------------------------------------
KMEANS_CHUNK = 10                                  # iterations between two readbacks of `changed`


class KMeans(object):
    """A k-means fit on frozen embeddings (kmeans): centroids fp32 [k, D]; labels int32 [n], in the order of `nodes`,
    and inertia (fp32 scalar tensor) as the LAST assignment pass saw them -- the centroids are the means of exactly
    these labels; inertia_history fp32 [n_iter] and changed_history int64 [n_iter], one slot per iteration; n_iter."""

    def __init__(self, centroids, bias, labels, inertia_history, changed_history, n_iter, spherical, seed):
        self.centroids, self.bias, self.labels = centroids, bias, labels
        self.inertia_history, self.changed_history = inertia_history, changed_history
        self.inertia = inertia_history[n_iter - 1]
        self.n_iter, self.spherical, self.seed = int(n_iter), bool(spherical), seed

    def predict(self, emb, nodes=None):
        """The nearest centroid of emb[nodes] (every row when nodes is None), int32 [n]: a pass that writes labels only."""
        N = int(emb.shape[0])
        ids = torch.arange(N, device=emb.device) if nodes is None else _pair_ids(nodes, emb.device, "KMeans.predict", "node", N)
        return ops.kmeans_pass(emb, ids, self.centroids, self.bias, accumulate=False)[0]


def _kmeans_init(emb, ids, k, init, seed, spherical):
    """-> (centroids fp32 [k, D], bias fp32 [k]) on emb's device; no host synchronisation for "++"."""
    dev, f32 = emb.device, torch.float32
    n, D = int(ids.shape[0]), int(emb.shape[1])
    bias = torch.zeros(k, dtype=f32, device=dev)
    if torch.is_tensor(init):
        if init.dim() != 2 or tuple(init.shape) != (k, D) or not init.is_floating_point():
            raise ValueError("kmeans: init as a tensor must be float [%d, %d], not %s" % (k, D, tuple(init.shape)))
        cen = init.detach().to(dev).float().contiguous().clone()
    elif init == "random":
        g = torch.Generator().manual_seed(int(seed))
        uniq = torch.unique(ids)
        cen = emb[uniq[torch.randperm(int(uniq.shape[0]), generator=g)[:k].to(dev)]].float().contiguous()
    elif init == "++":
        # k-means++ (Arthur & Vassilvitskii 2007): the first centre a uniform row, centre j a row drawn in proportion to
        # the squared distance to the nearest of the j centres so far -- a pass with k_live = j that writes dist only
        g = torch.Generator().manual_seed(int(seed))
        cen = torch.zeros(k, D, dtype=f32, device=dev)
        first = torch.randint(n, (1,), generator=g).to(dev)
        cen[0] = emb[ids[first]].float()[0]
        ops.kmeans_update(cen, bias)
        for j in range(1, k):
            _, dist = ops.kmeans_pass(emb, ids, cen, bias, k_live=j, want_dist=True, accumulate=False)
            cs = torch.cumsum(dist.double(), dim=0)
            u = torch.rand(1, generator=g, dtype=torch.float64).to(dev)
            at = torch.searchsorted(cs, u * cs[-1], right=True).clamp_(max=n - 1)
            cen[j] = emb[ids[at]].float()[0]
            ops.kmeans_update(cen, bias)
    else:
        raise ValueError('kmeans: init must be "++", "random" or a [k, D] tensor, not %r' % (init,))
    if spherical:
        cen = F.normalize(cen, dim=1).contiguous()
    ops.kmeans_update(cen, bias, spherical=spherical)
    return cen, bias


class KMeansIteration(object):
    """One Lloyd iteration on the device -- gsage_kmeans_pass, gsage_kmeans_update: two launches -- recorded once as a
    command list on two ping-pong label buffers (iteration t reads labels[t % 2] and writes labels[(t + 1) % 2]);
    replay(k) issues k iterations without a host synchronisation.  Iteration t (counted on the device) writes
    inertia_history[t], changed_history[t] and empty_history[t], t < capacity."""

    def __init__(self, emb, ids, centroids, bias, capacity, spherical):
        lib = nat.lib()
        dev, f32 = emb.device, torch.float32
        K, D = int(centroids.shape[0]), int(centroids.shape[1])
        self.E = E = ops.probe_operand(emb, D)
        self.ids, self.centroids, self.bias = ids, centroids, bias
        n = int(ids.shape[0])
        floats, S = ops.kmeans_scratch(n, K, D, 0)
        self.capacity = int(capacity)
        self.partial = torch.empty(floats, dtype=f32, device=dev)
        self.labels = [torch.full((n,), -1, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)]
        self.inertia_history = torch.zeros(self.capacity, dtype=f32, device=dev)
        self.changed_history = torch.zeros(self.capacity, dtype=torch.int64, device=dev)
        self.empty_history = torch.zeros(self.capacity, dtype=torch.int32, device=dev)
        self.index = torch.zeros(1, dtype=torch.int64, device=dev)
        self.issued = 0
        stream = ops._stream()
        self.cl = []
        for a in (0, 1):
            with nat.CommandList.record() as cl:
                nat.check(lib.gsage_kmeans_pass(ops._ptr(E), ops._code(E.dtype), E.stride(0), int(E.shape[0]), ops._ptr(ids),
                                                n, centroids.data_ptr(), bias.data_ptr(), K, D, K,
                                                self.labels[a].data_ptr(), 0, self.partial.data_ptr(),
                                                self.labels[1 - a].data_ptr(), None, stream), "kmeans_pass")
                nat.check(lib.gsage_kmeans_update(self.partial.data_ptr(), S, K, D, ops._code(E.dtype), int(bool(spherical)),
                                                  centroids.data_ptr(), bias.data_ptr(), self.inertia_history.data_ptr(),
                                                  self.changed_history.data_ptr(), self.empty_history.data_ptr(),
                                                  self.index.data_ptr(), self.capacity, stream), "kmeans_update")
            self.cl.append(cl)

    def replay(self, k=1):
        if self.issued + k > self.capacity:
            raise ValueError("KMeansIteration: %d iterations asked of a history of %d" % (self.issued + k, self.capacity))
        stream = ops._stream()
        for _ in range(k):
            self.cl[self.issued % 2].replay(stream)
            self.issued += 1

    def current_labels(self):
        return self.labels[self.issued % 2]


def _kmeans_fit(emb, ids, k, iters, init, seed, spherical):
    cen, bias = _kmeans_init(emb, ids, k, init, seed, spherical)
    n = int(ids.shape[0])
    if emb.is_cuda:
        fit = KMeansIteration(emb, ids, cen, bias, iters, spherical)
        while fit.issued < iters:
            fit.replay(min(KMEANS_CHUNK, iters - fit.issued))
            if int(fit.changed_history[fit.issued - 1]) == 0:        # the chunk's one 8-byte readback
                break
        done = fit.issued
        km = KMeans(cen, bias, fit.current_labels(), fit.inertia_history[:done], fit.changed_history[:done], done,
                    spherical, seed)
        km.empty_history = fit.empty_history[:done]
        km._fit = fit                                  # the recorded lists and their buffers
        return km
    # host mode: the same loop over the float64 definition
    hist = (torch.zeros(iters), torch.zeros(iters, dtype=torch.int64), torch.zeros(iters, dtype=torch.int32),
            torch.zeros(1, dtype=torch.int64))
    labels = torch.full((n,), -1, dtype=torch.int32)
    done = 0
    while done < iters:
        for _ in range(min(KMEANS_CHUNK, iters - done)):
            res = ops.kmeans_pass(emb, ids, cen, bias, labels_in=labels)
            labels = res[4]
            ops.kmeans_update(cen, bias, res.partial, spherical=spherical, history=hist)
            done += 1
        if int(hist[1][done - 1]) == 0:
            break
    km = KMeans(cen, bias, labels, hist[0][:done], hist[1][:done], done, spherical, seed)
    km.empty_history = hist[2][:done]
    return km


def kmeans(emb, k, nodes=None, iters=50, init="++", n_init=1, seed=0, spherical=False):
    """Lloyd's k-means on the rows `nodes` (default: every row) of the frozen embeddings `emb` [N, D] -> KMeans.

    init: "++" (k-means++ on the device, k set-up passes, draws from a CPU torch.Generator seeded with `seed`), "random"
    (k distinct rows of `nodes`) or a [k, D] tensor.  n_init > 1 repeats the fit with seeds seed, seed + 1, .. and keeps
    the lowest final inertia (the lowest seed among equals).  spherical: centroids (the initial ones too) are scaled to
    unit length and the assignment is by inner product.  An empty cluster keeps its centroid.
    On CUDA one iteration is two launches (csrc/gsage_kmeans.hip: pass, update), recorded once as a command list and
    replayed in chunks of 10 iterations; after a chunk ONE 8-byte readback of `changed` ends the loop when no label
    moved -- from then on an iteration reproduces itself bit for bit, so stopping early changes nothing.  CPU tensors:
    the same loop over ops.kmeans_pass's host definition.  Deterministic: two fits on the same inputs are bit-identical.
    Refused with a sentence: k > 128, D > 1024, k larger than the number of distinct ids in `nodes`, a table with
    non-finite values in those rows, ids out of range, iters < 1."""
    if not torch.is_tensor(emb) or emb.dim() != 2 or not emb.is_floating_point():
        raise ValueError("kmeans: emb must be a [N, D] float tensor")
    k, iters, n_init = int(k), int(iters), int(n_init)
    if iters < 1:
        raise ValueError("kmeans: iters must be at least 1, not %d" % iters)
    if n_init < 1:
        raise ValueError("kmeans: n_init must be at least 1, not %d" % n_init)
    N, D = int(emb.shape[0]), int(emb.shape[1])
    ids = ops.kmeans_check(emb, torch.arange(N) if nodes is None else nodes, k, D, who="kmeans")
    if int(ids.min()) < 0 or int(ids.max()) >= N:
        raise IndexError("kmeans: node id out of range of the %d embedding rows" % N)
    distinct = int(torch.unique(ids).shape[0])
    if k > distinct:
        raise ValueError("kmeans: k = %d clusters asked of %d distinct rows" % (k, distinct))
    if not bool(torch.isfinite(emb[ids]).all()):
        raise ValueError("kmeans: the embeddings of the rows to cluster hold non-finite values")
    emb = ops.probe_operand(emb, D)                    # rounded to the compute mode once, not once per fit
    best = _kmeans_fit(emb, ids, k, iters, init, int(seed), spherical)
    for r in range(1, n_init):
        fit = _kmeans_fit(emb, ids, k, iters, init, int(seed) + r, spherical)
        if float(fit.inertia) < float(best.inertia):
            best = fit
    return best


def cluster_metrics(labels, targets, n_classes=None):
    """Agreement of a clustering with class labels -> {"n", "clusters", "nmi", "purity"}: clusters = the non-empty
    ones; NMI = I(U; V) / ((H(U) + H(V)) / 2) in nats (1.0 when both partitions are trivial); purity = (1/n) sum_k max_c
    |cluster k and class c|.  The K x C contingency table is one torch.bincount on the labels' device, evaluated in
    float64 on the host.  A metric, not a hot path.  Multilabel and regression targets are refused."""
    labels, targets = torch.as_tensor(labels), torch.as_tensor(targets)
    if targets.is_floating_point() or targets.dtype == torch.bool:
        raise ValueError("cluster_metrics: targets must be integer class ids (no regression or multilabel targets), not %s"
                         % targets.dtype)
    if targets.dim() > 2 or (targets.dim() == 2 and int(targets.shape[1]) != 1):
        raise ValueError("cluster_metrics: targets must be one class id per row (no multilabel targets), not shape %s"
                         % (tuple(targets.shape),))
    if labels.is_floating_point() or labels.dim() != 1 or labels.numel() != targets.numel() or labels.numel() < 1:
        raise ValueError("cluster_metrics: labels must be integer [n] with one target each")
    u, v = labels.long(), targets.to(labels.device).long().view(-1)
    if int(u.min()) < 0 or int(v.min()) < 0:
        raise ValueError("cluster_metrics: labels and targets must be non-negative")
    C = int(v.max()) + 1 if n_classes is None else int(n_classes)
    if int(v.max()) >= C:
        raise ValueError("cluster_metrics: class id out of range [0, %d)" % C)
    K = int(u.max()) + 1
    T = torch.bincount(u * C + v, minlength=K * C).view(K, C).cpu().double().numpy()
    n = T.sum()
    pu, pv = T.sum(axis=1) / n, T.sum(axis=0) / n

    def H(p):
        p = p[p > 0]
        return float(-(p * np.log(p)).sum())
    nz = T > 0
    mi = float((T[nz] / n * (np.log(T[nz] / n) - np.log(np.outer(pu, pv)[nz]))).sum())
    hu, hv = H(pu), H(pv)
    if hu + hv == 0.0 or (int(nz.sum(axis=1).max()) == 1 and int(nz.sum(axis=0).max()) == 1):
        nmi = 1.0                                      # the same partition under other names: exactly 1, no round-off
    else:
        nmi = max(0.0, mi) / ((hu + hv) / 2.0)
    return {"n": int(n), "clusters": int((pu > 0).sum()), "nmi": min(1.0, nmi), "purity": float(T.max(axis=1).sum() / n)}


def cluster_eval(emb, problem, k=None, iters=50, init="++", n_init=1, seed=0, spherical=False):
    """k-means on the embeddings of every node of the problem's three folds, scored on the val and test folds ->
    {"k", "iters", "inertia", "val": cluster_metrics or None, "test": ..., "nodes", "labels", "centroids"}; k defaults
    to problem.n_classes.  A problem without class labels (multilabel, regression) is clustered all the same and scores
    None."""
    dev = emb.device
    folds = {m: np.asarray(problem.nodes[m], dtype=np.int64).reshape(-1) for m in ("train", "val", "test")}
    nodes = np.concatenate([folds["train"], folds["val"], folds["test"]])
    k = int(problem.n_classes if k is None else k)
    km = kmeans(emb, k, nodes=torch.from_numpy(nodes).to(dev), iters=iters, init=init, n_init=n_init, seed=seed,
                spherical=spherical)
    out = {"k": k, "iters": km.n_iter, "inertia": float(km.inertia), "nodes": nodes, "labels": km.labels,
           "centroids": km.centroids}
    at = len(folds["train"])
    for name in ("val", "test"):
        m = len(folds[name])
        out[name] = None
        if problem.task == "classification" and m:
            y = torch.as_tensor(np.asarray(problem.targets[folds[name]])).long().view(-1)
            out[name] = cluster_metrics(km.labels[at:at + m], y, n_classes=int(problem.n_classes))
        at += m
    return out
