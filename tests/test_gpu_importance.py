"""Importance neighbourhoods on the GPU (csrc/gsage_importance.hip) against the restatement of tests/importance_ref.py:
all three outputs of the kernel bit for bit over every 64-lane boundary of the walks and every size class of the
sorts, both test graphs, uniform and weighted steps; repeatability, independence of a row from its launch, the error
flag, DeviceCSR.importance against the host-mode build, and the importance-weighted problem through the weighted
module path (the comparisons and tolerances of tests/test_gpu_weighted.py, as they are)."""
import numpy as np
import pytest
import torch

import importance_ref as ir
import weighted_ref as wr
from conftest import pkg
from test_gpu_weighted import _model
from util import close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_ADJ = {}


def _graph(name):
    return wr.graph() if name == "a" else ir.graph_b()


def _csr(name, weighted, device=DEV):
    key = (name, weighted, device)
    if key not in _ADJ:
        gs = pkg()
        g = _graph(name)
        adj = gs.DeviceCSR(torch.from_numpy(g.rowptr).to(device), torch.from_numpy(g.col).to(device), g.n,
                           max(int(g.deg.max()), 1))
        _ADJ[key] = adj.with_weights(torch.from_numpy(g.weight).to(device)) if weighted else adj
    return _ADJ[key]


def _walk(adj, ids, R, L, T, seed=ir.SEED):
    return pkg().ops.importance_walks(adj, torch.as_tensor(ids).to(adj.device), R, L, T, seed)


@pytest.mark.parametrize("name,weighted", [("a", False), ("a", True), ("b", False)])
@pytest.mark.parametrize("case", ir.CASES, ids=lambda c: "R%d-L%d-T%d-M%d" % (c[0] + (c[1],)))
def test_kernel_equals_the_restatement(case, name, weighted):
    gs = pkg()
    (R, L, T), M = case
    g, adj = _graph(name), _csr(name, weighted)
    ids = ir.sources(g, M)
    col, w, deg, err, _ = ir.rows(g, weighted, ids, R, L, T)
    before = gs._native.launch_count()
    got = _walk(adj, ids, R, L, T)
    assert gs._native.launch_count() - before == 1
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32 and got[2].dtype == torch.int32
    assert torch.equal(got[0].cpu(), torch.from_numpy(col))
    assert torch.equal(got[1].cpu(), torch.from_numpy(w))
    assert torch.equal(got[2].cpu(), torch.from_numpy(deg))
    assert int(adj.err_flag.item()) == err
    adj.err_flag.zero_()
    again = _walk(adj, ids, R, L, T)                                   # two launches are bit-equal
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    adj.err_flag.zero_()


def test_the_parameters_produce_their_cases():
    """on the restatement: over graph (a) the parameter set meets every case the comparison above is for"""
    for weighted in (False, True):
        met = set()
        for (R, L, T), M in ir.CASES:
            met |= ir.cases_met(ir.rows(wr.graph(), weighted, ir.sources(wr.graph(), M), R, L, T)[4], T)
        assert met == ir.ALL_CASES, (weighted, ir.ALL_CASES - met)


@pytest.mark.parametrize("name,weighted", [("a", False), ("a", True), ("b", False)])
def test_a_row_does_not_depend_on_its_launch(name, weighted):
    g, adj = _graph(name), _csr(name, weighted)
    ids = ir.sources(g, 72)
    for R, L, T in ((10, 2, 3), (65, 5, 8)):
        whole = _walk(adj, ids, R, L, T)
        parts = [_walk(adj, ids[:29], R, L, T), _walk(adj, ids[29:], R, L, T)]
        rev = _walk(adj, ids[::-1].copy(), R, L, T)
        for k in range(3):
            assert torch.equal(whole[k], torch.cat([parts[0][k], parts[1][k]]))
            assert torch.equal(whole[k], rev[k].flip(0))
    adj.err_flag.zero_()


def test_bad_edge_and_bad_source_raise_the_flag():
    gs = pkg()
    g = ir.graph_b()
    adj = _csr("b", False)
    adj.err_flag.zero_()
    ids = np.array([10, g.n, 5, -1, 20], dtype=np.int64)
    col, w, deg, err, _ = ir.rows(g, False, ids, 10, 2, 3)
    got = _walk(adj, ids, 10, 2, 3)
    assert err == 1 and int(deg[1]) == 0 and int(deg[3]) == 0
    assert torch.equal(got[0].cpu(), torch.from_numpy(col)) and torch.equal(got[1].cpu(), torch.from_numpy(w))
    assert torch.equal(got[2].cpu(), torch.from_numpy(deg))
    with pytest.raises(IndexError):
        adj.check()
    adj.check()
    _walk(adj, np.array([10, 5, 20, 21]), 10, 2, 3)                    # sources that never reach the bad edge
    adj.check()
    _walk(adj, np.array([ir.B_ROWS["leads to the bad edge"]]), 20, 2, 3)
    assert int(adj.err_flag.item()) == 1
    adj.err_flag.zero_()
    with pytest.raises(IndexError):
        adj.importance(n_walks=20, walk_len=2, top=4, seed=1)
    assert int(adj.err_flag.item()) == 0                               # cleared by the check that raised
    good = ir.graph_b(bad=False)
    ok = gs.DeviceCSR(torch.from_numpy(good.rowptr).to(DEV), torch.from_numpy(good.col).to(DEV), good.n, 9)
    assert ok.importance(n_walks=20, walk_len=2, top=4, seed=1).n_rows == good.n


@pytest.mark.parametrize("weighted", [False, True])
def test_importance_equals_the_host_mode_build(weighted):
    gs = pkg()
    dev, host = _csr("a", weighted), _csr("a", weighted, "cpu")
    for kw in (dict(n_walks=10, walk_len=2, top=3), dict(n_walks=63, walk_len=3, top=16, chunk=7), dict()):
        before = gs._native.launch_count()
        a, b = dev.importance(seed=ir.SEED, **kw), host.importance(seed=ir.SEED, **kw)
        chunks = -(-72 // kw.get("chunk", 1 << 20))
        assert gs._native.launch_count() - before == 2 * chunks + 2       # walks + compaction per chunk, the table
        assert a.n_rows == b.n_rows == 72 and a.max_deg == b.max_deg == kw.get("top", 16) and a.rowptr.is_cuda
        assert torch.equal(a.rowptr.cpu(), b.rowptr) and torch.equal(a.col.cpu(), b.col)
        assert torch.equal(a.edge_cdf.cpu(), b.edge_cdf)
    col, w, deg, _, _ = ir.rows(wr.graph(), weighted, np.arange(72), 10, 2, 3)
    a = dev.importance(n_walks=10, walk_len=2, top=3, seed=ir.SEED)
    keep = np.arange(3)[None, :] < deg[:, None]
    assert np.array_equal(a.col.cpu().numpy(), col[keep])
    assert np.array_equal(a.edge_cdf.cpu().numpy().view(np.uint64), wr.build_cdf(a.rowptr.cpu().numpy(), w[keep]))


# ---- downstream: the importance-weighted problem through the weighted paths ---------------------------------------------
_PROBLEM = {}


def _importance_problem():
    """weighted_problem() with its adjacency replaced by importance_adj (R = 20, L = 2, T = 4), built on the GPU and
    checked against the host-mode build"""
    if not _PROBLEM:
        gs = pkg()
        p = dict(wr.weighted_problem())
        wa = gs.importance_adj(p["adj"], n_walks=20, walk_len=2, top=4, seed=ir.SEED, device=torch.device(DEV))
        ref = gs.importance_adj(p["adj"], n_walks=20, walk_len=2, top=4, seed=ir.SEED, device=torch.device("cpu"))
        assert np.array_equal(wa.adj.indptr, ref.adj.indptr) and np.array_equal(wa.adj.data, ref.adj.data)
        assert np.array_equal(wa.weight, ref.weight) and wa.shape == (201, 4)
        from scipy import sparse
        p["adj"] = wa.adj
        p["weight"] = sparse.csr_matrix((wa.weight, wa.adj.indices, wa.adj.indptr), shape=wa.adj.shape)
        p["indptr"], p["data"], p["w"] = wa.adj.indptr.astype(np.int64), wa.adj.data, wa.weight
        _PROBLEM["p"] = p
    return _PROBLEM["p"]


def test_train_step_equals_the_cpu_model():
    """tests/test_gpu_weighted.py::test_train_step_equals_the_cpu_model on the importance-weighted problem: its model
    builder, its steps, its bounds"""
    gs = pkg()
    gs.ops.set_compute_dtype("fp32")
    try:
        p = _importance_problem()
        host, dev = _model(gs, p, "mean"), _model(gs, p, "mean").to(DEV)
        for m in (host, dev):
            m.optimizer = torch.optim.Adam(m.parameters(), lr=0.01)
        store = gs.FeatureStore.from_array(p["feats"], torch.device(DEV), dtype="fp32")
        feats = torch.from_numpy(p["feats"])
        rng = np.random.RandomState(1)
        before = gs._native.launch_count()
        for step in range(2):
            ids = torch.from_numpy(rng.randint(1, 201, size=48))
            tg = torch.from_numpy(p["targets"][ids.numpy()])
            a = host.train_step(ids, feats, tg, gs.ProblemLosses.classification)
            b = dev.train_step(ids.to(DEV), store, tg.to(DEV), gs.ProblemLosses.classification)
            close(b.detach().cpu().numpy(), a.detach().numpy(), ("preds", step), 1e-4, 1e-5)
        assert gs._native.launch_count() - before >= 12
        assert dev.train_sampler.calls == host.train_sampler.calls == 4
        hs = host.state_dict()
        for name, v in dev.state_dict().items():
            close(v.cpu().numpy(), hs[name].numpy(), ("weights", name), 2e-4, 2e-5)
        dev.train_sampler.csr(DEV).check()
    finally:
        gs.ops.set_compute_dtype("bf16")


def test_train_cli_on_the_gpu(capsys, tmp_path):
    """train.py --importance-walks on the GPU: both adjacencies are the ones host mode builds, the run trains on the
    weighted module path and says so, full-neighbour evaluation and the embedding export take the weighted graph"""
    import importlib
    import json
    gs = pkg()
    train = importlib.import_module("pytorch-graphsage_amd.train")
    p = wr.weighted_problem()
    prob = gs.NodeProblem.from_arrays("classification", p["C"], p["adj"], p["adj"].copy(), p["feats"], p["folds"],
                                      p["targets"], cuda=True)
    path = str(tmp_path / "emb.npy")
    try:
        train.main(["--problem-path", "<memory>", "--epochs", "2", "--batch-size", "32", "--sampler-class",
                    "sparse_uniform_neighbor_sampler", "--n-train-samples", "3,2", "--n-val-samples", "3,2",
                    "--output-dims", "8,8", "--show-test", "--importance-walks", "20", "--importance-top", "4",
                    "--importance-seed", "9", "--full-neighbour-eval", "--save-embeddings", path], problem=prob)
        cap = capsys.readouterr()
        assert "becomes sparse_weighted_neighbor_sampler" in cap.err and "on cuda)" in cap.err
        assert "no fused engine covers the weighted sampler" in cap.err and "using the module path" in cap.err
        ref = gs.importance_adj(p["adj"], n_walks=20, walk_len=2, top=4, seed=9, device=torch.device("cpu"))
        for got in (prob.adj, prob.train_adj):
            assert isinstance(got, gs.WeightedAdj) and np.array_equal(got.adj.indptr, ref.adj.indptr)
            assert np.array_equal(got.adj.data, ref.adj.data) and np.array_equal(got.weight, ref.weight)
        lines = [json.loads(l) for l in cap.out.splitlines() if l.startswith("{")]
        assert lines[-1]["test_f1"] is not None and lines[-2]["val_metric"] is not None
        assert np.load(path).shape == (201, 16)
    finally:
        gs.nn_modules.SparseUniformNeighborSampler.rng_default = "compat"
        gs.ops.set_compute_dtype("bf16")


@pytest.mark.parametrize("agg", ["mean", "mean_pool"])
def test_embeddings_equal_host_mode(agg):
    """tests/test_gpu_weighted.py::test_embeddings_equal_host_mode on the importance-weighted problem"""
    gs = pkg()
    gs.ops.set_compute_dtype("fp32")
    try:
        p = _importance_problem()
        host, dev = _model(gs, p, agg, "linear", seed=3), _model(gs, p, agg, "linear", seed=3).to(DEV)
        ref = gs.embeddings(host, torch.from_numpy(p["feats"]))
        got = gs.embeddings(dev, torch.from_numpy(p["feats"]).to(DEV))
        close(got.cpu().numpy(), ref.numpy(), "gpu vs host", 2e-5, 2e-5)
        ref64 = wr.dense_reference(host, p["feats"], p["indptr"], p["data"], p["w"])[1]
        close(got.cpu().numpy(), ref64, "gpu vs float64", 2e-5, 2e-5)
    finally:
        gs.ops.set_compute_dtype("bf16")
