"""k-hop closure blocks without a GPU (infer.closure / infer.query in host mode): the sets and blocks against the
restatement of tests/closure_ref.py, integer for integer; query against full_neighbour(nodes=...) on the same CPU
tensors; the argument checks and the refusals."""
import numpy as np
import pytest
import torch

import closure_ref as cr
import segment_reduce_ref as sr
from conftest import pkg
from full_neighbour_ref import make_model, sparse_graph
from util import close

AGGS = ["mean", "max_pool", "mean_pool", "attention"]


def edge_queries(g):
    """Unsorted, with duplicates, a query that is another query's neighbour, the dummy 0, a query of degree 0, and the
    rows the schedule of the reduce turns on: a long row, a row of degree 1."""
    r = g.at[17]
    row = g.col[g.rowptr[r]:g.rowptr[r + 1]]
    nb = next(int(u) for u in row if int(u) not in (0, r))
    zero = 46
    assert g.deg[zero] == 0 and g.deg[0] == 0 and g.deg[1] > g.L
    return np.array([r, zero, 600, 0, nb, r, 1, g.at[1], 3, zero], dtype=np.int64)


def weights_for(g, seed=3):
    """fp32 edge weights; every quantum of row g.at[7] and of the long last row is 0"""
    w = np.random.RandomState(seed).uniform(0.1, 4.0, size=g.col.shape[0]).astype(np.float32)
    for v in (g.at[7], g.n - 1):
        w[g.rowptr[v]:g.rowptr[v + 1]] = 0
    return w


def dense_adj(n=300, K=6, seed=7):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, n, size=(n, K)).astype(np.int64))


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_host_closure_equals_the_restatement(depth):
    gs = pkg()
    g = sr.graph(256)
    q = edge_queries(g)
    ref = cr.closure_ref(g.rowptr, g.col, g.n, q, depth)
    assert not ref.bad and ref.blocks[depth].dummy != 0
    cr.assert_equal(gs.infer.closure(g.csr("cpu"), torch.from_numpy(q), depth), ref, "sparse", n=g.n)
    wadj = g.csr("cpu").with_weights(weights_for(g))
    wq = np.concatenate([q, [g.at[7], g.n - 1]])
    wref = cr.closure_ref(g.rowptr, g.col, g.n, wq, depth, cdf=wadj.edge_cdf.numpy())
    cr.assert_equal(gs.infer.closure(wadj, wq, depth), wref, "weighted", n=g.n, cdf=True)
    d = dense_adj()
    dq = np.array([17, 5, 299, 0, int(d[17, 2]), 17], dtype=np.int64)
    dref = cr.closure_ref(np.arange(d.shape[0] + 1) * d.shape[1], d.numpy().reshape(-1), d.shape[0], dq, depth)
    cr.assert_equal(gs.infer.closure(gs.DenseAdj(d), dq, depth), dref, "dense", n=d.shape[0])


def _problem(seed, n=300, D=20):
    rng = np.random.RandomState(seed)
    adj, indptr, data = sparse_graph(n, rng, max_deg=9, long_row=(17, 280))
    feats = rng.normal(size=(n + 1, D)).astype(np.float32)
    feats[0] = 0
    nodes = torch.from_numpy(np.concatenate([[17, 3, 0, int(data[indptr[17]]), 17], rng.randint(1, n + 1, size=12)]))
    assert indptr[4] == indptr[3]                                       # (row 3 has degree 0)
    return adj, feats, nodes


@pytest.mark.parametrize("prep", ["identity", "linear"])
@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("depth", [2, 3])
def test_host_query_equals_full_neighbour(agg, prep, depth):
    gs = pkg()
    adj, feats, nodes = _problem(depth)
    model = make_model(agg, prep, adj, feats.shape[1], dims=(16,) * depth)
    x = torch.from_numpy(feats)
    want, emb = gs.full_neighbour(model, x, nodes=nodes, embeddings=True)
    got, gemb = gs.infer.query(model, x, nodes, embeddings=True)
    close(got.numpy(), want.numpy(), "logits")
    close(gemb.numpy(), emb[nodes].numpy(), "embeddings")
    assert got.shape[0] == nodes.shape[0] and torch.equal(got[0], got[4])          # caller order, duplicates repeat
    via = gs.full_neighbour(model, x, nodes=nodes, closure=True)
    assert torch.equal(via, got)
    close(gs.infer.query_embeddings(model, x, nodes).numpy(), emb[nodes].numpy(), "query_embeddings")
    store = gs.FeatureStore.from_array(feats, torch.device("cpu"), dtype="fp32")
    assert torch.equal(gs.infer.query(model, store, nodes), got)


@pytest.mark.parametrize("agg", ["mean", "mean_pool"])
def test_host_query_on_a_weighted_adjacency(agg):
    gs = pkg()
    adj, feats, nodes = _problem(5)
    w = np.random.RandomState(1).uniform(0.1, 2.0, size=adj.nnz).astype(np.float32)
    w[adj.indptr[17]:adj.indptr[18]] = 0                                # the long row: no drawable edge
    wadj = gs.DeviceCSR.from_scipy(adj, "cpu", weight=w)
    model = make_model(agg, "identity", adj, feats.shape[1])
    x = torch.from_numpy(feats)
    close(gs.infer.query(model, x, nodes, adj=wadj).numpy(), gs.full_neighbour(model, x, nodes=nodes, adj=wadj).numpy(),
          "weighted")
    with pytest.raises(ValueError, match="weighted adjacency"):
        gs.infer.query(make_model("max_pool", "identity", adj, feats.shape[1]), x, nodes, adj=wadj)


def test_argument_checks_and_refusals():
    gs = pkg()
    adj, feats, nodes = _problem(2)
    x = torch.from_numpy(feats)
    model = make_model("mean", "identity", adj, feats.shape[1])
    csr = model.val_sampler.csr("cpu")
    with pytest.raises(ValueError, match="depth"):
        gs.infer.closure(csr, nodes, 0)
    with pytest.raises(ValueError, match="no nodes"):
        gs.infer.closure(csr, torch.zeros(0, dtype=torch.int64), 2)
    with pytest.raises(ValueError, match="integers"):
        gs.infer.closure(csr, torch.tensor([1.0, 2.0]), 2)
    for bad in (-1, csr.n_rows):
        with pytest.raises(IndexError):
            gs.infer.query(model, x, torch.tensor([1, bad]))
    with pytest.raises(ValueError, match="needs the nodes"):
        gs.full_neighbour(model, x, closure=True)
    with pytest.raises(ValueError, match="feature rows"):
        gs.infer.query(model, x[:50], nodes)
    with pytest.raises(ValueError, match="LSTMAggregator"):
        gs.infer.query(make_model("lstm", "identity", adj, feats.shape[1]), x, nodes)
    with pytest.raises(ValueError, match="NodeEmbeddingPrep"):
        gs.infer.query(make_model("mean", "node_embedding", adj, feats.shape[1]), x, nodes)


def test_bindings_name_the_scan_span():
    gs = pkg()
    span = gs.infer.scan_span()                        # items per workgroup of the closure scans
    assert span > 0 and span % 256 == 0                # (whole 256-thread workgroups, the same items per thread)
    for name in ("gsage_closure_seed_count", "gsage_closure_expand_write", "gsage_segment_reduce_block"):
        assert name in gs._native.SIGNATURES
    L = gs._native.lib()
    assert L.gsage_closure_seed_count(None, 0, 10, None, None, None, None, None) == -1
    assert b"query count" in L.gsage_last_error()
    assert L.gsage_segment_reduce_block(0, None, 1, 8, 8, None, 0, None, None, None, 5, 4, 0, None, 0, None, 0, None, 0,
                                        256, None, 0, None, 0, 8, 0, None, None) == -1
    assert b"n_src" in L.gsage_last_error()
