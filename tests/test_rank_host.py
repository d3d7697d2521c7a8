"""Exact link ranking without a GPU: host mode of ops.rank_ip / gs.link_rank against tests/rank_ref.py, link_metrics and
held_out_edges on hand-made data, the filter-CSR builder, every refusal, the workspace arithmetic and EINVAL of the C
entry point, and train.py --link-eval."""
import ctypes
import importlib
import json

import numpy as np
import pytest
import torch

import rank_ref as kr
import retrieve_ref as rr
from conftest import pkg


@pytest.fixture(autouse=True)
def _dtype():
    gs = pkg()
    yield
    gs.ops.set_compute_dtype("bf16")


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("exclude", ["none", "self", "neighbours"])
def test_host_mode_equals_the_reference_on_integer_data(exclude, mode):
    gs = pkg()
    gs.ops.set_compute_dtype(mode)
    N = 50
    E, _ = rr.integer_case(N, 1, 24, seed=4)
    rowptr, col = rr.hub_csr(N)
    ap, ac = kr.ascending_csr(rowptr, col)
    hub = ac[ap[2]:ap[3]]
    src = np.array([2, 2, 5, 9, 9, 2, 7, 31], dtype=np.int64)
    dst = np.array([hub[0], 2, 5, 9, 30, hub[0], 13, 2], dtype=np.int64)      # neighbours, src == dst, a repeated pair
    want_rank, want_sc, _, _ = kr.rank_ref(E, E[src], dst, mode, exclude, src, ap, ac)
    emb = torch.from_numpy(E)
    csr = gs.DeviceCSR(torch.from_numpy(ap), torch.from_numpy(ac), N, 40)
    rank, sc = gs.ops.rank_ip(emb, emb[src], dst, query_ids=src, csr=csr, exclude=exclude)
    assert rank.dtype == torch.int64 and sc.dtype == torch.float32
    assert np.array_equal(rank.numpy(), want_rank) and np.array_equal(sc.numpy(), want_sc.astype(np.float32))
    assert rank[0] == rank[5] and int(rank.min()) >= 1
    # link_rank on the UNSORTED adjacency with its duplicate column builds its own filter
    raw = gs.DeviceCSR(torch.from_numpy(rowptr), torch.from_numpy(col), N, 40)
    rank2, sc2 = gs.link_rank(emb, src, dst, exclude=exclude, adj=raw)
    assert torch.equal(rank2, rank) and torch.equal(sc2, sc)
    if exclude == "neighbours":
        with pytest.raises(ValueError, match="strictly ascending"):
            gs.ops.rank_ip(emb, emb[src], dst, query_ids=src, csr=raw, exclude=exclude)


def test_host_mode_lies_in_the_rank_interval_and_nan_is_unranked():
    gs = pkg()
    gs.ops.set_compute_dtype("fp32")
    E = rr.unit_rows(301, 40, 2)
    E[17] = np.nan
    rng = np.random.RandomState(3)
    src, dst = rng.randint(18, 301, size=40), rng.randint(18, 301, size=40)
    dst[:2] = 17
    rank, sc = gs.link_rank(torch.from_numpy(E), src, dst, exclude="self")
    assert (rank[:2] == 0).all() and torch.isnan(sc[:2]).all() and int(rank[2:].min()) >= 1
    lo, hi, _ = kr.rank_interval(E, E[src[2:]], dst[2:], "fp32", "self", src[2:])
    got = rank[2:].numpy()
    assert ((lo <= got) & (got <= hi)).all()


def test_link_metrics_on_hand_made_ranks():
    gs = pkg()
    m = gs.link_metrics(torch.tensor([1, 2, 0, 11, 50]), ks=(1, 10, 50))
    assert m["n"] == 5 and m["unranked"] == 1
    assert m["mrr"] == pytest.approx((1 + 0.5 + 0 + 1 / 11 + 1 / 50) / 5)
    assert m["mean_rank"] == pytest.approx((1 + 2 + 11 + 50) / 4)
    assert m["hits@1"] == pytest.approx(0.2) and m["hits@10"] == pytest.approx(0.4) and m["hits@50"] == pytest.approx(0.8)
    assert sorted(m) == ["hits@1", "hits@10", "hits@50", "mean_rank", "mrr", "n", "unranked"]
    none = gs.link_metrics(np.array([0, 0]), ks=(3,))
    assert none == {"n": 2, "unranked": 2, "mrr": 0.0, "mean_rank": None, "hits@3": 0.0}
    json.dumps(m), json.dumps(none)
    with pytest.raises(ValueError):
        gs.link_metrics([1, -1])


# a ten-node graph written out by hand: row -> stored neighbours (any order, one duplicate)
FULL = {0: [], 1: [2, 3], 2: [1, 5, 3], 3: [1, 2], 4: [9, 6, 9, 5], 5: [2, 4], 6: [4], 7: [], 8: [9], 9: [4, 8]}
SEEN = {0: [], 1: [2], 2: [1, 3], 3: [2], 4: [6], 5: [], 6: [4], 7: [], 8: [], 9: []}


def _csr_of(gs, rows, n=10):
    rowptr = np.concatenate([[0], np.cumsum([len(rows[v]) for v in range(n)])]).astype(np.int64)
    col = np.array([c for v in range(n) for c in rows[v]], dtype=np.int32)
    return gs.DeviceCSR(torch.from_numpy(rowptr), torch.from_numpy(col), n, 4)


def test_held_out_edges_on_a_ten_node_graph():
    gs = pkg()
    full, seen = _csr_of(gs, FULL), _csr_of(gs, SEEN)
    src, dst = gs.held_out_edges(full, seen, [4, 2, 7, 9, 4, 1])
    assert src.dtype == torch.int64 and dst.dtype == torch.int64
    # by u in the caller's order (4 twice), then v ascending; 4's duplicate 9 once; (4, 6), (2, 1), (2, 3), (1, 2) are kept
    assert src.tolist() == [4, 4, 2, 9, 9, 4, 4, 1]
    assert dst.tolist() == [5, 9, 5, 4, 8, 5, 9, 3]
    e, _ = gs.held_out_edges(full, full, np.arange(10))
    assert e.numel() == 0
    with pytest.raises(IndexError):
        gs.held_out_edges(full, seen, [10])


def test_filter_csr_sorts_and_drops_duplicates_once():
    gs = pkg()
    adj = _csr_of(gs, FULL)
    f = gs.infer.filter_csr(adj)
    assert f.rowptr.tolist() == [0, 0, 2, 5, 7, 10, 12, 13, 13, 14, 16]
    assert f.col.tolist() == [2, 3, 1, 3, 5, 1, 2, 5, 6, 9, 2, 4, 4, 9, 4, 8] and f.col.dtype == torch.int32
    assert gs.infer.filter_csr(adj) is f                                 # cached on the adjacency object
    rowptr, col = rr.hub_csr(50)
    ap, ac = kr.ascending_csr(rowptr, col)
    g = gs.infer.filter_csr(gs.DeviceCSR(torch.from_numpy(rowptr), torch.from_numpy(col), 50, 40))
    assert np.array_equal(g.rowptr.numpy(), ap) and np.array_equal(g.col.numpy(), ac)


def test_refusals():
    gs = pkg()
    E = torch.from_numpy(rr.integer_case(20, 1, 8)[0])
    with pytest.raises(ValueError, match="needs adj"):
        gs.link_rank(E, [1, 2], [3, 4])
    with pytest.raises(ValueError, match="DenseAdj holds samples"):
        gs.link_rank(E, [1, 2], [3, 4], adj=gs.DenseAdj(torch.zeros(20, 4, dtype=torch.int64)))
    with pytest.raises(ValueError, match="DeviceCSR"):
        gs.link_rank(E, [1, 2], [3, 4], adj=object())
    with pytest.raises(IndexError):
        gs.link_rank(E, [1, 20], [3, 4], exclude="self")
    with pytest.raises(IndexError):
        gs.link_rank(E, [1, 2], [3, -1], exclude="self")
    with pytest.raises(ValueError, match="2 src for 1 dst"):
        gs.link_rank(E, [1, 2], [3], exclude="self")
    with pytest.raises(ValueError, match="integers"):
        gs.link_rank(E, [1.0], [3], exclude="self")
    with pytest.raises(ValueError, match="exclude must"):
        gs.link_rank(E, [1], [3], exclude="all")
    with pytest.raises(ValueError, match="emb must"):
        gs.link_rank(E[0], [1], [3], exclude="self")
    with pytest.raises(ValueError, match="query_ids"):
        gs.ops.rank_ip(E, E[:2], [3, 4], exclude="self")
    with pytest.raises(ValueError, match="csr"):
        gs.ops.rank_ip(E, E[:2], [3, 4], query_ids=[0, 1], exclude="neighbours")
    with pytest.raises(ValueError, match="target_ids for 2 queries"):
        gs.ops.rank_ip(E, E[:2], [3])
    with pytest.raises(IndexError, match="target_ids"):
        gs.ops.rank_ip(E, E[:2], [3, 20])
    with pytest.raises(IndexError, match="query_ids"):
        gs.ops.rank_ip(E, E[:2], [3, 4], query_ids=[0, 20], exclude="self")
    with pytest.raises(ValueError, match="share D"):
        gs.ops.rank_ip(E, E[:2, :4], [3, 4])
    with pytest.raises(ValueError, match="splits"):
        gs.ops.rank_ip(E, E[:2], [3, 4], splits=1025)
    with pytest.raises(ValueError, match="D must"):
        gs.ops.rank_ip(torch.zeros(4, 1025), torch.zeros(1, 1025), [0])


def test_bad_arguments_return_einval_without_gpu():
    L = pkg()._native.lib()
    P = ctypes.c_void_p(4096)

    def call(N=100, ldt=16, ldq=16, Q=4, D=16, tg=P, qids=None, rowptr=None, col=None, exclude=0, splits=0, dtype=0):
        return L.gsage_rank_ip(P, dtype, ldt, N, P, 0, ldq, Q, D, tg, qids, rowptr, col, exclude, splits, None, 0, P, P,
                               None, None)

    for kw, name in (({"D": 0}, b"D must"), ({"D": 1025, "ldt": 2048, "ldq": 2048}, b"D must"), ({"ldt": 15}, b"ld ("),
                     ({"ldq": 8}, b"ld ("), ({"N": 0}, b"N must"), ({"N": 2 ** 31}, b"N must"), ({"Q": 0}, b"Q must"),
                     ({"splits": -1}, b"splits"), ({"splits": 1025}, b"splits"), ({"exclude": 3}, b"exclude must"),
                     ({"tg": None}, b"target_ids"), ({"exclude": 1}, b"query_ids"), ({"dtype": 1}, b"dtype"),
                     ({"exclude": 2, "qids": P}, b"rowptr"), ({"exclude": 2, "qids": P, "rowptr": P}, b"col")):
        assert call(**kw) == -1, kw
        assert name in L.gsage_last_error(), (kw, L.gsage_last_error())
    # everything else in order: the workspace is what is missing
    assert call() == -1 and b"workspace" in L.gsage_last_error()


def test_workspace_is_host_arithmetic():
    gs = pkg()
    L = gs._native.lib()
    used = ctypes.c_int64(0)

    def ws(Q, splits, N=232965):
        return int(L.gsage_rank_ip_workspace(Q, N, splits, ctypes.byref(used)))

    assert ws(1, 1) == 8 and used.value == 1
    assert ws(70, 3) == 4 * 70 * 4 and ws(70, 1024) == 4 * 70 * 1025
    for Q in (1, 512, 32768, 262144):
        b0 = ws(Q, 0)
        s = used.value
        assert 1 <= s <= 1024 and b0 == ws(Q, s) == 4 * Q * (s + 1)
        k_used = ctypes.c_int64(0)
        L.gsage_topk_ip_workspace(Q, 232965, 10, 0, ctypes.byref(k_used))
        assert s == k_used.value                                          # the split rule is top-k's
    assert ws(0, 1) == -1 and ws(1, -1) == -1 and ws(1, 1025) == -1 and ws(1, 1, N=0) == -1 and ws(1, 1, N=2 ** 31) == -1
    assert int(L.gsage_rank_ip_workspace(5, 100, 2, None)) == 60
    assert gs.ops.rank_ip_workspace(70, 5003, 3) == (4 * 70 * 4, 3)
    with pytest.raises(ValueError, match="limits"):
        gs.ops.rank_ip_workspace(0, 10)


# ---- train.py --link-eval ------------------------------------------------------------------------------------------------
def _problem(rng, n=120, D=8, C=3):
    from scipy import sparse
    gs = pkg()
    degs = rng.randint(1, 6, size=n + 1)
    degs[0] = 0
    nbrs = [rng.randint(1, n + 1, size=d) for d in degs]
    folds = np.array(["train"] * 80 + ["val"] * 25 + ["test"] * (n + 1 - 105))
    folds[0] = "dummy"
    # the training graph: the edges between training nodes
    kept = [nb[folds[nb] == "train"] if folds[v] == "train" else nb[:0] for v, nb in enumerate(nbrs)]

    def csr(rows):
        deg = np.array([len(r) for r in rows])
        ptr = np.concatenate([[0], np.cumsum(deg)])
        cols = np.arange(ptr[-1]) - np.repeat(ptr[:-1], deg)
        return sparse.csr_matrix((np.concatenate(rows), cols, ptr), shape=(n + 1, 5))
    adj, train_adj = csr(nbrs), csr(kept)
    feats = rng.normal(size=(n + 1, D)).astype(np.float32)
    feats[0] = 0
    return lambda: gs.NodeProblem.from_arrays("classification", C, adj, train_adj, feats, folds,
                                              feats[:, :C].argmax(1).reshape(-1, 1), cuda=False), adj, train_adj


ARGV = ["--problem-path", "<memory>", "--no-cuda", "--epochs", "1", "--batch-size", "32", "--sampler-class",
        "sparse_uniform_neighbor_sampler", "--n-train-samples", "3,2", "--n-val-samples", "3,2", "--output-dims", "8,8"]


@pytest.mark.parametrize("unsup", [False, True])
def test_train_link_eval(unsup, capsys, tmp_path):
    gs = pkg()
    train = importlib.import_module("pytorch-graphsage_amd.train")
    problem, adj, train_adj = _problem(np.random.RandomState(5))
    p = str(tmp_path / "emb.npy")
    calls, embeddings = [], gs.embeddings
    try:
        gs.embeddings = lambda *a, **kw: calls.append(1) or embeddings(*a, **kw)
        train.main(ARGV + ["--link-eval", "--link-eval-ks", "1,5", "--show-test", "--save-embeddings", p] +
                   (["--unsupervised"] if unsup else []), problem=problem())
    finally:
        gs.embeddings = embeddings
    assert len(calls) == 1                                                # one embedding pass for the file and the ranking
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    got = [l["link_eval"] for l in lines if "link_eval" in l]
    assert [g["fold"] for g in got] == ["val", "test"] and lines[-1]["link_eval"] is got[-1]
    gs.ops.set_compute_dtype("bf16")                                      # (train.py's default --precision)
    emb = torch.from_numpy(np.load(p))
    cpu = torch.device("cpu")
    full, seen = gs.DeviceCSR.from_scipy(adj, cpu), gs.DeviceCSR.from_scipy(train_adj, cpu)
    prob = problem()
    for g in got:
        src, dst = gs.held_out_edges(full, seen, prob.nodes[g["fold"]])
        assert g["held_out_edges"] == src.numel() > 20
        ranks, _ = gs.link_rank(emb, src, dst, exclude="neighbours", adj=full)
        want = gs.link_metrics(ranks, ks=(1, 5))
        shown = json.loads(train.dumps(want))                             # (train.py prints five decimals)
        assert {k: v for k, v in g.items() if k not in ("fold", "held_out_edges")} == shown
        assert want["n"] == src.numel() and want["unranked"] == 0 and 0 < want["mrr"] <= 1
    # the cap: a seeded subsample
    train.main(ARGV + ["--link-eval", "--link-eval-edges", "7"], problem=problem())
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert lines[-1]["link_eval"]["n"] == 7 and lines[-1]["link_eval"]["held_out_edges"] > 20


def test_train_link_eval_refusals(monkeypatch):
    gs = pkg()
    train = importlib.import_module("pytorch-graphsage_amd.train")
    rng = np.random.RandomState(1)
    n = 40
    dense = rng.randint(0, n, size=(n + 1, 4))
    folds = np.array(["train"] * 30 + ["val"] * 6 + ["test"] * 5)
    feats = rng.normal(size=(n + 1, 6)).astype(np.float32)
    prob = gs.NodeProblem.from_arrays("classification", 3, dense, dense, feats, folds,
                                      feats[:, :3].argmax(1).reshape(-1, 1), cuda=False)
    with pytest.raises(SystemExit, match="--link-eval: a dense problem"):
        train.main(["--problem-path", "<memory>", "--no-cuda", "--link-eval"], problem=prob)
    with pytest.raises(SystemExit, match="--link-eval-edges must"):
        train.main(["--problem-path", "<memory>", "--no-cuda", "--link-eval", "--link-eval-ks", "1,x"], problem=prob)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="--link-eval: data-parallel"):
        train.main(["--problem-path", "<memory>", "--no-cuda", "--link-eval"], problem=prob)
