"""Independent float64 restatement of layer-wise full-neighbourhood inference (the definition of infer.py), with
explicit loops over rows and neighbours, and the small graphs / models the full-neighbour tests share."""
import numpy as np
import torch
from scipy import sparse
from torch.nn import functional as F

from conftest import pkg


def neighbours_sparse(indptr, data):
    """N(v) of every row of a CSR in the reference's convention; degree 0 -> the dummy 0."""
    out = []
    for v in range(len(indptr) - 1):
        nb = [int(u) for u in data[indptr[v]:indptr[v + 1]]]
        out.append(nb if nb else [0])
    return out


def neighbours_dense(adj):
    return [[int(u) for u in row] for row in np.asarray(adj)]


def _np(t):
    return t.detach().cpu().double().numpy()


def reference(model, feats, nbrs):
    """(logits [n, C], embeddings [n, 2h]) for every row, float64."""
    gs = pkg()
    X = np.asarray(feats, dtype=np.float64)[:len(nbrs)]
    if isinstance(model.prep, gs.nn_modules.LinearPrep):
        X = X @ _np(model.prep.fc.weight).T
    H = X
    for layer in model.agg_layers.children():
        Wx, Wn = _np(layer.fc_x.weight), _np(layer.fc_neib.weight)
        agg = []
        if isinstance(layer, gs.nn_modules.PoolAggregator):
            Wm, bm = _np(layer.mlp[0].weight), _np(layer.mlp[0].bias)
        if isinstance(layer, gs.nn_modules.AttentionAggregator):
            A0, A2 = _np(layer.att[0].weight), _np(layer.att[2].weight)
            att = lambda h: np.tanh(h @ A0.T) @ A2.T
        for v, nb in enumerate(nbrs):
            if isinstance(layer, gs.nn_modules.PoolAggregator):
                hid = np.maximum(H[nb] @ Wm.T + bm, 0)
                agg.append(hid.max(0) if layer.pool_fn == "max" else hid.mean(0))
            elif isinstance(layer, gs.nn_modules.AttentionAggregator):
                s = np.array([att(H[u]) @ att(H[v]) for u in nb])
                w = np.exp(s - s.max())
                w /= w.sum()
                acc = np.zeros(H.shape[1])
                for wu, u in zip(w, nb):
                    acc += wu * H[u]
                agg.append(acc)
            else:
                acc = np.zeros(H.shape[1])
                for u in nb:
                    acc += H[u]
                agg.append(acc / len(nb))
        out = np.concatenate([H @ Wx.T, np.stack(agg) @ Wn.T], axis=1)
        if layer.activation is F.relu:
            out = np.maximum(out, 0)
        H = out
    emb = H / np.maximum(np.linalg.norm(H, axis=1, keepdims=True), 1e-12)
    return emb @ _np(model.fc.weight).T + _np(model.fc.bias), emb


def sparse_graph(n, rng, max_deg=9, long_row=None):
    """CSR in the reference's convention over n + 1 rows: row 0 the dummy, every 7th row of degree 0, a few of
    degree 1, uneven degrees elsewhere; `long_row` = (row, degree) adds one long row."""
    deg = rng.randint(2, max_deg + 1, size=n + 1)
    deg[0] = 0
    deg[3::7] = 0
    deg[5::11] = 1
    if long_row is not None:
        deg[long_row[0]] = long_row[1]
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    data = rng.randint(1, n + 1, size=int(indptr[-1]))
    cols = np.arange(indptr[-1]) - np.repeat(indptr[:-1], deg)
    adj = sparse.csr_matrix((data, cols, indptr), shape=(n + 1, max(int(deg.max()), 1)))
    return adj, indptr, data


def make_model(agg, prep, adj, D, dims=(16, 16), C=5, sampler="sparse_uniform_neighbor_sampler", n_val=None, seed=0):
    gs = pkg()
    torch.manual_seed(seed)
    specs = []
    for i, h in enumerate(dims):
        last = i == len(dims) - 1
        nv = n_val if n_val is not None else 3
        specs.append({"n_train_samples": nv, "n_val_samples": nv, "output_dim": h,
                      "activation": (lambda x: x) if last else F.relu})
    n_nodes = adj.shape[0] - 1 if sampler == "sparse_uniform_neighbor_sampler" else adj.shape[0] - 1
    return gs.GSSupervised(sampler_class=gs.sampler_lookup[sampler], adj=adj, train_adj=adj,
                           prep_class=gs.prep_lookup[prep], aggregator_class=gs.aggregator_lookup[agg],
                           input_dim=D, n_nodes=n_nodes, n_classes=C, layer_specs=specs)
