"""Importance neighbourhoods without a GPU: host mode of ops.importance_walks against the restatement of
tests/importance_ref.py (bit for bit, both test graphs, uniform and weighted steps), gs.importance_adj in the
reference's convention, independence of a row from its launch, the seeds, the refusals (Python, C ABI, train.py) and
train.py --importance-walks on the CPU."""
import ctypes
import importlib
import json

import numpy as np
import pytest
import torch

import importance_ref as ir
import weighted_ref as wr
from conftest import pkg


def _csr(g, weighted, device="cpu"):
    gs = pkg()
    adj = gs.DeviceCSR(torch.from_numpy(g.rowptr).to(device), torch.from_numpy(g.col).to(device), g.n,
                       max(int(g.deg.max()), 1))
    return adj.with_weights(torch.from_numpy(g.weight).to(device)) if weighted else adj


GRAPHS = [("a", False), ("a", True), ("b", False)]


def _graph(name):
    return wr.graph() if name == "a" else ir.graph_b()


@pytest.mark.parametrize("name,weighted", GRAPHS)
def test_host_mode_equals_the_restatement(name, weighted):
    gs = pkg()
    g = _graph(name)
    adj = _csr(g, weighted)
    met = set()
    for (R, L, T), M in ir.CASES:
        ids = ir.sources(g, M)
        col, w, deg, err, lists = ir.rows(g, weighted, ids, R, L, T)
        got = gs.ops.importance_walks(adj, torch.from_numpy(ids), R, L, T, ir.SEED)
        assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32 and got[2].dtype == torch.int32
        assert torch.equal(got[0], torch.from_numpy(col)), (R, L, T)
        assert torch.equal(got[1], torch.from_numpy(w)), (R, L, T)
        assert torch.equal(got[2], torch.from_numpy(deg)), (R, L, T)
        assert int(adj.err_flag.item()) == err
        adj.err_flag.zero_()
        met |= ir.cases_met(lists, T)
    # the inputs produce the cases they are for
    if name == "a":
        assert met == ir.ALL_CASES, ir.ALL_CASES - met
    else:
        assert {"distinct = 0", "0 < distinct < T", "tie inside T", "distinct > T"} <= met


def test_the_arranged_graph_holds_its_cases():
    g = ir.graph_b()
    R, L = 10, 5
    hub, _ = ir.ranked(g.rowptr, g.col, None, g.n, ir.B_ROWS["hub"], R, L, ir.SEED)
    assert sum(c for _, c in hub) == R * 3 and {u for u, _ in hub} <= set(range(11, 20))    # steps 1 and 3 land on the hub
    cyc, _ = ir.ranked(g.rowptr, g.col, None, g.n, 5, R, 3, ir.SEED)
    assert cyc == [(1, R), (2, R), (6, R)]                       # equal counts: ascending id
    assert ir.ranked(g.rowptr, g.col, None, g.n, ir.B_ROWS["self loop"], R, L, ir.SEED) == ([], 0)
    assert ir.ranked(g.rowptr, g.col, None, g.n, 21, R, L, ir.SEED) == ([(22, R), (23, R), (24, R)], 0)
    assert ir.ranked(g.rowptr, g.col, None, g.n, ir.B_ROWS["bad edge"], 20, 1, ir.SEED)[1] == 1
    assert ir.ranked(g.rowptr, g.col, None, g.n, g.n, R, L, ir.SEED) == ([], 1)
    assert ir.ranked(ir.graph_b(bad=False).rowptr, ir.graph_b(bad=False).col, None, g.n, 25, 20, 3, ir.SEED)[1] == 0


def test_out_of_range_source_and_bad_edge_raise():
    gs = pkg()
    g = ir.graph_b()
    adj = _csr(g, False)
    ids = np.array([10, g.n, 5, -1], dtype=np.int64)
    col, w, deg, err, _ = ir.rows(g, False, ids, 10, 2, 3)
    got = gs.ops.importance_walks(adj, torch.from_numpy(ids), 10, 2, 3, ir.SEED)
    assert err == 1 and torch.equal(got[0], torch.from_numpy(col)) and torch.equal(got[2], torch.from_numpy(deg))
    assert int(deg[1]) == 0 and int(deg[3]) == 0 and int(deg[0]) == 3
    with pytest.raises(IndexError):
        adj.check()
    adj.check()
    with pytest.raises(IndexError):
        adj.importance(n_walks=20, walk_len=2, top=4, seed=1)
    assert int(adj.err_flag.item()) == 0
    _csr(ir.graph_b(bad=False), False).importance(n_walks=20, walk_len=2, top=4, seed=1)


class _P(object):
    """the weighted problem's adjacency as a graph of the restatement"""

    def __init__(self, p, weighted):
        self.rowptr, self.col, self.n = p["indptr"], p["data"].astype(np.int32), 201
        self.cdf = wr.build_cdf(p["indptr"], p["w"]) if weighted else None


@pytest.mark.parametrize("weighted", [False, True])
def test_importance_adj_is_a_weighted_adj_in_the_reference_convention(weighted):
    gs = pkg()
    p = wr.weighted_problem()
    R, L, T = 20, 2, 4
    wa = gs.importance_adj(gs.WeightedAdj(p["adj"], p["weight"]) if weighted else p["adj"], n_walks=R, walk_len=L,
                           top=T, seed=ir.SEED, device=torch.device("cpu"))
    assert isinstance(wa, gs.WeightedAdj) and wa.shape == (201, T) and wa.weight.dtype == np.float32
    col, w, deg, err, lists = ir.rows(_P(p, weighted), weighted, np.arange(201), R, L, T)
    assert err == 0 and {"distinct > T", "0 < distinct < T", "distinct = 0"} <= ir.cases_met(lists, T)
    assert np.array_equal(np.diff(wa.adj.indptr), deg)
    keep = np.arange(T)[None, :] < deg[:, None]
    assert np.array_equal(wa.adj.data, col[keep]) and np.array_equal(wa.weight, w[keep])
    assert np.array_equal(wa.adj.indices, np.nonzero(keep)[1])               # columns 0 .. k_v - 1
    adj = gs.DeviceCSR.from_scipy(wa.adj, torch.device("cpu"), weight=wa.weight)
    assert adj.max_deg == T and adj.n_rows == 201
    assert np.array_equal(adj.edge_cdf.numpy().view(np.uint64), wr.build_cdf(wa.adj.indptr, wa.weight))
    # the samplers take it as it is
    s = gs.find_sampler("sparse_weighted_neighbor_sampler")(adj=wa, seed=3)
    out = s(torch.arange(1, 50), 5).numpy().reshape(49, 5)
    for i, v in enumerate(range(1, 50)):
        assert set(out[i]) <= ({int(u) for u, _ in lists[v][:T]} or {0})


def test_a_row_does_not_depend_on_its_launch():
    gs = pkg()
    g = wr.graph()
    for weighted in (False, True):
        adj = _csr(g, weighted)
        ids = torch.arange(g.n)
        whole = gs.ops.importance_walks(adj, ids, 10, 2, 3, ir.SEED)
        rev = gs.ops.importance_walks(adj, ids.flip(0), 10, 2, 3, ir.SEED)
        for a, b in zip(whole, rev):
            assert torch.equal(a, b.flip(0))
        for v in (0, wr.ROWS[1000], 71):
            alone = gs.ops.importance_walks(adj, torch.tensor([v]), 10, 2, 3, ir.SEED)
            for a, b in zip(whole, alone):
                assert torch.equal(a[v:v + 1], b)
        a, b = adj.importance(10, 2, 3, seed=ir.SEED), adj.importance(10, 2, 3, seed=ir.SEED, chunk=7)
        assert a.max_deg == 3 and a.n_rows == g.n and a.edge_cdf is not None
        for x, y in ((a.rowptr, b.rowptr), (a.col, b.col), (a.edge_cdf, b.edge_cdf)):
            assert torch.equal(x, y)
        col, w, deg, _, _ = ir.rows(g, weighted, np.arange(g.n), 10, 2, 3)
        keep = np.arange(3)[None, :] < deg[:, None]
        assert np.array_equal(a.rowptr.numpy(), np.concatenate([[0], np.cumsum(deg)]))
        assert np.array_equal(a.col.numpy(), col[keep])
        assert np.array_equal(a.edge_cdf.numpy().view(np.uint64), wr.build_cdf(a.rowptr.numpy(), w[keep]))


def test_seeds():
    gs = pkg()
    adj = _csr(wr.graph(), False)
    ids = torch.arange(72)
    a = gs.ops.importance_walks(adj, ids, 10, 2, 3, 1)
    b = gs.ops.importance_walks(adj, ids, 10, 2, 3, 1)
    c = gs.ops.importance_walks(adj, ids, 10, 2, 3, 2)
    d = gs.ops.importance_walks(adj, ids, 10, 2, 3, 1 + (1 << 32))          # the seed's high word counts
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[0], d[0])


BAD_SIZES = [(10, 0, 4, "walk_len"), (10, 17, 4, "walk_len"), (10, 2, 0, "top"), (10, 2, 65, "top"),
             (4097, 1, 4, "n_walks \\* walk_len = 4097"), (0, 2, 4, "n_walks")]


@pytest.mark.parametrize("R,L,T,what", BAD_SIZES)
def test_bad_sizes_are_refused(R, L, T, what):
    gs = pkg()
    adj = _csr(wr.graph(), False)
    with pytest.raises(ValueError, match=what):
        gs.ops.importance_walks(adj, torch.arange(3), R, L, T, 0)
    with pytest.raises(ValueError, match=what):
        adj.importance(R, L, T)
    # the C entry: GSAGE_EINVAL before any pointer is looked at, without a GPU
    lib = gs._native.lib()
    vp = ctypes.c_void_p
    rc = lib.gsage_importance_walks(vp(16), vp(16), None, 72, vp(16), 3, R, L, T, 0, vp(16), vp(16), vp(16), None, None)
    assert rc == -1 and what.replace("\\", "").encode() in lib.gsage_last_error()


def test_the_c_entries_refuse_more_without_a_gpu():
    lib = pkg()._native.lib()
    vp = ctypes.c_void_p
    assert lib.gsage_importance_walks(None, None, None, 72, None, 3, 10, 2, 4, 0, None, None, None, None, None) == -1
    assert b"null pointer" in lib.gsage_last_error()
    assert lib.gsage_importance_walks(vp(16), vp(16), None, 1 << 31, vp(16), 3, 10, 2, 4, 0, vp(16), vp(16), vp(16),
                                      None, None) == -1
    assert lib.gsage_importance_walks(None, None, None, 72, None, 0, 10, 2, 4, 0, None, None, None, None, None) == 0
    assert lib.gsage_importance_compact(None, None, None, None, 5, 4, None, None, None) == -1
    assert lib.gsage_importance_compact(vp(16), vp(16), vp(16), vp(16), 5, 65, None, None, None) == -1
    assert lib.gsage_importance_compact(None, None, None, None, 0, 4, None, None, None) == 0


# ---- train.py ----------------------------------------------------------------------------------------------------
ARGV = ["--problem-path", "<memory>", "--no-cuda", "--epochs", "2", "--batch-size", "32", "--sampler-class",
        "sparse_uniform_neighbor_sampler", "--n-train-samples", "3,2", "--n-val-samples", "3,2", "--output-dims", "8,8",
        "--show-test"]
IMP = ["--importance-walks", "20", "--importance-top", "4", "--importance-seed", "9"]


def _problem(gs, p, weighted=False):
    kw = dict(adj_weight=p["weight"], train_adj_weight=p["w"]) if weighted else {}
    return gs.NodeProblem.from_arrays("classification", p["C"], p["adj"], p["adj"].copy(), p["feats"], p["folds"],
                                      p["targets"], cuda=False, **kw)


def _with_sampler(name):
    return ARGV[:ARGV.index("--sampler-class") + 1] + [name] + ARGV[ARGV.index("--sampler-class") + 2:]


def test_train_cli_on_the_cpu(capsys):
    gs = pkg()
    train = importlib.import_module("pytorch-graphsage_amd.train")
    p = wr.weighted_problem()
    lines = lambda out: [{k: v for k, v in json.loads(l).items() if k != "time"} for l in out.splitlines()
                         if l.startswith("{")]
    try:
        # without the flag nothing changes: the adjacencies stay the problem's own objects, nothing is said
        prob = _problem(gs, p)
        adj, train_adj = prob.adj, prob.train_adj
        train.main(ARGV, problem=prob)
        cap = capsys.readouterr()
        assert prob.adj is adj and prob.train_adj is train_adj and "importance" not in cap.err
        plain = lines(cap.out)
        # with it: both adjacencies are the importance-weighted ones of themselves, the weighted module path trains
        prob = _problem(gs, p)
        train.main(ARGV + IMP, problem=prob)
        cap = capsys.readouterr()
        assert cap.err.count("becomes sparse_weighted_neighbor_sampler") == 1
        assert "both adjacencies rebuilt from 20 walks of 2 steps per node, top 4" in cap.err
        for got, src in ((prob.adj, adj), (prob.train_adj, train_adj)):
            ref = gs.importance_adj(src, n_walks=20, walk_len=2, top=4, seed=9, device=torch.device("cpu"))
            assert isinstance(got, gs.WeightedAdj) and got.shape == (201, 4)
            assert np.array_equal(got.adj.indptr, ref.adj.indptr) and np.array_equal(got.adj.data, ref.adj.data)
            assert np.array_equal(got.weight, ref.weight)
        imp = lines(cap.out)
        assert len(imp) == len(plain) and imp[-1]["test_f1"] is not None and imp != plain
        # asked for by name, on a problem that carries weights: its walks step by them
        prob = _problem(gs, p, weighted=True)
        train.main(_with_sampler("sparse_weighted_neighbor_sampler") + IMP + ["--full-neighbour-eval"], problem=prob)
        cap = capsys.readouterr()
        assert "becomes" not in cap.err and "both adjacencies rebuilt" in cap.err
        ref = gs.importance_adj(gs.WeightedAdj(p["adj"], p["weight"]), n_walks=20, walk_len=2, top=4, seed=9,
                                device=torch.device("cpu"))
        assert np.array_equal(prob.adj.adj.data, ref.adj.data) and np.array_equal(prob.adj.weight, ref.weight)
        assert lines(cap.out)[-1]["test_f1"] is not None
        # the refusals, one line each
        with pytest.raises(SystemExit, match="--importance-walks: random walks need the stored edges") as e:
            train.main(_with_sampler("uniform_neighbor_sampler") + IMP, problem=_problem(gs, p))
        assert "\n" not in str(e.value)
        with pytest.raises(SystemExit, match="--unsupervised: the weighted sampler") as e:
            train.main(ARGV + IMP + ["--unsupervised"], problem=_problem(gs, p))
        assert "\n" not in str(e.value)
        with pytest.raises(SystemExit, match="--importance-walks: importance_walks: top must be in 1..64") as e:
            train.main(ARGV + ["--importance-walks", "20", "--importance-top", "65"], problem=_problem(gs, p))
        assert "\n" not in str(e.value)
    finally:
        capsys.readouterr()
        gs.nn_modules.SparseUniformNeighborSampler.rng_default = "compat"
        gs.ops.set_compute_dtype("bf16")
