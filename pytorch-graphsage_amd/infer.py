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
"""
import torch
from torch import nn
from torch.nn import functional as F

from . import _native as nat
from . import ops
from .nn_modules import (AttentionAggregator, IdentityPrep, LinearPrep, LSTMAggregator, MeanAggregator,
                         NodeEmbeddingPrep, PoolAggregator, concat_combine, _split_activation)
from .store import DenseAdj, FeatureStore, _round_up

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
    table: [n_rows, D] bf16 / fp32 CUDA tensor whose row stride is a multiple of 16 bytes; out: a (possibly
    strided) fp32 / bf16 [n_rows, D] view; keys (SOFTMAX_WEIGHTED): fp32 [n_rows, 32].  mode SEG_WEIGHTED_MEAN
    (gsage_segment_reduce_weighted) reads the adjacency's edge_cdf."""
    rowptr, col, n = _csr(adj)
    p = plan(adj)
    D = int(table.shape[1])
    assert table.stride(1) == 1 and out.stride(1) == 1 and int(table.shape[0]) >= n and int(out.shape[0]) >= n
    ldp = int(nat.lib().gsage_segment_reduce_ldp(D))
    partials = torch.empty(max(p["n_slices"], 1), ldp, dtype=torch.float32, device=table.device)
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
    code, post = _split_activation(layer.activation)
    cdt = ops.torch_dtype()
    h = layer.output_dim_
    N = int(H.shape[0])
    out = torch.empty(N, 2 * h, dtype=torch.float32, device=H.device)
    out[:, :h] = ops.linear(H, layer.fc_x.weight, None, code)
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
        keys = torch.zeros(N, 32, dtype=torch.float32, device=H.device)
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
    src = torch.cat([col.long()[keep], torch.zeros_like(empty)])
    p = torch.cat([q[keep].float() / T[rows[keep]].float(), torch.ones(empty.numel())])
    order = torch.argsort(dst, stable=True)              # row-major, a row's edges in their stored order
    return src[order], dst[order], p[order], n


def _edges(adj):
    """(src, dst) of every edge of N(v), v = 0..n_rows-1, degree-0 rows reading the dummy 0 (host mode)."""
    if _weighted(adj):
        return _edges_weighted(adj)
    rowptr, col, n = _csr(adj)
    deg = rowptr[1:] - rowptr[:-1]
    dst = torch.repeat_interleave(torch.arange(n, dtype=torch.int64), deg.clamp(min=1))
    src = torch.zeros(dst.numel(), dtype=torch.int64)
    has = torch.repeat_interleave(deg > 0, deg.clamp(min=1))
    src[has] = col.long()
    return src, dst, deg.clamp(min=1), n


def _layer_host(layer, H, edges):
    src, dst, cnt, n = edges
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
    out = torch.cat([F.linear(H, layer.fc_x.weight), F.linear(agg, layer.fc_neib.weight)], dim=1)
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


def full_neighbour(model, feats, nodes=None, adj=None, embeddings=False):
    """Logits of `model` for `nodes` (default: every row of the adjacency) by layer-wise full-neighbourhood inference,
    and, with embeddings=True, also F.normalize(H^L) for every row: returns (logits, emb).  Arguments as for
    embeddings() above, which computes emb; this applies the model's `fc` to it."""
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
