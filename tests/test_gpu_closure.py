"""k-hop closure blocks on the MI355X (csrc/gsage_block.hip behind infer.closure, gsage_segment_reduce_block behind
infer.query): the sets and blocks integer for integer against tests/closure_ref.py, the scan carry across workgroups,
the block reduce bit for bit against the whole-graph reduce, query against the float64 reference of full-neighbourhood
inference, the error flag, the restored state, launches per call, and the train.py flags.  No time is asserted."""
import importlib
import json

import numpy as np
import pytest
import torch

import closure_ref as cr
import segment_reduce_ref as sr
from conftest import pkg
from full_neighbour_ref import make_model, neighbours_sparse, reference, sparse_graph
from test_closure_host import dense_adj, edge_queries, weights_for
from util import close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AGGS = ["mean", "max_pool", "mean_pool", "attention"]


@pytest.fixture(autouse=True)
def _dtype():
    gs = pkg()
    yield
    gs.ops.set_compute_dtype("bf16")


def _at_rest(adj):
    st = adj._closure_state
    return bool((st["local"] == -1).all()) and bool((st["bitmap"] == 0).all())


# ---- sets and blocks ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_sets_and_blocks_are_integer_exact(depth):
    gs = pkg()
    g = sr.graph(256)
    assert g.deg.max() > gs.infer.SLICE_LEN and (g.deg == 0).sum() > 2
    q = edge_queries(g)
    adj = g.csr(DEV)
    ref = cr.closure_ref(g.rowptr, g.col, g.n, q, depth)
    got = gs.infer.closure(adj, torch.from_numpy(q), depth)
    cr.assert_equal(got, ref, "sparse", n=g.n)
    assert ref.blocks[depth].dummy != 0 and _at_rest(adj)
    # weighted: the cdf segments verbatim; a row whose quanta sum to 0 (short, and the sliced last row) is a query
    wadj = g.csr(DEV).with_weights(torch.from_numpy(weights_for(g)))
    cdf = wadj.edge_cdf.cpu().numpy()
    assert cdf[g.rowptr[g.at[7] + 1] - 1] == 0
    wq = np.concatenate([q, [g.at[7], g.n - 1]])
    wgot = gs.infer.closure(wadj, torch.from_numpy(wq).to(DEV), depth)
    cr.assert_equal(wgot, cr.closure_ref(g.rowptr, g.col, g.n, wq, depth, cdf=cdf), "weighted", n=g.n, cdf=True)
    b = wgot.blocks[depth]
    for i, v in enumerate(wgot.sets[depth].tolist()):
        assert torch.equal(b.edge_cdf[int(b.rowptr[i]):int(b.rowptr[i + 1])],
                           wadj.edge_cdf[int(g.rowptr[v]):int(g.rowptr[v + 1])])
    # the dense adjacency read as K edges per row
    d = dense_adj()
    dq = np.array([17, 5, 299, 0, int(d[17, 2]), 17], dtype=np.int64)
    dref = cr.closure_ref(np.arange(d.shape[0] + 1) * d.shape[1], d.numpy().reshape(-1), d.shape[0], dq, depth)
    dadj = gs.DenseAdj(d.to(DEV))
    cr.assert_equal(gs.infer.closure(dadj, dq, depth), dref, "dense", n=d.shape[0])
    assert int(adj.err_flag.item()) == 0 and int(wadj.err_flag.item()) == 0 and int(dadj.err_flag.item()) == 0


_BIG = {}


def _big():
    """100 003 rows (no multiple of 32) of degree 4 whose neighbours all lie in the first or in the last scan span of
    the bitmap: whatever a hop marks sits in the first and in the last workgroup of the scan, none in between."""
    if not _BIG:
        gs = pkg()
        span_rows = 32 * gs.infer.scan_span()              # rows per scan workgroup of the bitmap: 32 768
        n = 100003
        n_wg = -(-(-(-n // 32)) // gs.infer.scan_span())
        assert n % 32 != 0 and n_wg >= 4 and (n_wg - 1) * span_rows < n
        rng = np.random.RandomState(11)
        col = np.where(rng.randint(0, 2, size=4 * n) == 0, rng.randint(1, span_rows, size=4 * n),
                       rng.randint((n_wg - 1) * span_rows, n, size=4 * n)).astype(np.int32)
        deg = np.full(n, 4, dtype=np.int64)
        deg[0] = 0
        rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        col = col[:int(rowptr[-1])]
        col[rowptr[12345]] = n - 1                          # the last row: the last bit of the bitmap's last word
        _BIG.update(n=n, span_rows=span_rows, n_wg=n_wg, rowptr=rowptr, col=col, rng=rng,
                    adj=gs.DeviceCSR(torch.from_numpy(rowptr).to(DEV), torch.from_numpy(col).to(DEV), n, 4))
    return _BIG


def test_scan_carry_across_workgroups():
    gs = pkg()
    B = _big()
    n, span_rows, n_wg = B["n"], B["span_rows"], B["n_wg"]
    # queries in every span, the middle ones included: members already, never marked
    q = np.concatenate([np.random.RandomState(5).randint(1, n - 1, size=40), [12345, span_rows + 7, 2 * span_rows + 1]])
    ref = cr.closure_ref(B["rowptr"], B["col"], n, q, 3)
    for l in (3, 2, 1):
        new = ref.sets[l - 1][len(ref.sets[l]):]
        new = new[new != 0]
        assert (new < span_rows).any() and (new >= (n_wg - 1) * span_rows).any()
        assert not ((new >= span_rows) & (new < (n_wg - 1) * span_rows)).any()
    assert n - 1 in ref.sets[2] and n - 1 not in ref.sets[3]
    cr.assert_equal(gs.infer.closure(B["adj"], torch.from_numpy(q).to(DEV), 3), ref, "scan carry", n=n)
    # more queries than one scan span of them, most of them duplicates
    q2 = np.random.RandomState(6).randint(1, 600, size=3 * gs.infer.scan_span() + 5)
    cr.assert_equal(gs.infer.closure(B["adj"], q2, 1), cr.closure_ref(B["rowptr"], B["col"], n, q2, 1), "many queries",
                    n=n)
    assert _at_rest(B["adj"]) and int(B["adj"].err_flag.item()) == 0


def test_launches_and_readbacks_do_not_depend_on_the_query_count(monkeypatch):
    """Depth 2: 6 launches for the seed level, 7 per hop, 1 to restore = 21, and one device-to-host copy per level = 3.
    Copies are counted where a CUDA tensor can reach the host: every Tensor method that hands out host values."""
    gs = pkg()
    B = _big()
    infer = gs.infer
    infer.closure(B["adj"], torch.arange(1, 4), 2)
    seen = []
    for name in ("tolist", "item", "cpu", "numpy", "__int__", "__bool__", "__index__", "__float__"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, _name=name, **k):
            if self.is_cuda:
                seen.append(_name)
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    counts = []
    for k in (3, 300):
        q = torch.from_numpy(np.random.RandomState(k).randint(1, B["n"], size=k)).to(DEV)
        torch.cuda.synchronize()
        c0 = gs._native.launch_count()
        del seen[:]
        infer.closure(B["adj"], q, 2)
        copies = list(seen)
        torch.cuda.synchronize()
        counts.append((gs._native.launch_count() - c0, len(copies)))
    assert counts[0] == counts[1] == (6 + 7 * 2 + 1, 3), counts


# ---- queries without a single edge -------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("weighted", [False, True])
def test_queries_of_degree_zero_only_give_blocks_without_edges(weighted, depth):
    """Every query isolated (and the dummy): every block has 0 edges, every row reads the dummy -- the answer is
    full_neighbour's."""
    gs = pkg()
    gs.ops.set_compute_dtype("fp32")
    adj, nbrs, feats, _ = _problem(2)
    iso = [v for v in range(1, len(nbrs)) if nbrs[v] == [0]][:5]
    assert len(iso) == 5
    model = make_model("mean", "identity", adj, feats.shape[1], dims=(16,) * depth).to(DEV)
    store = gs.FeatureStore.from_array(feats, torch.device(DEV), dtype="fp32")
    csr = model.val_sampler.csr(DEV)
    if weighted:
        w = np.random.RandomState(2).uniform(0.1, 2.0, size=adj.nnz).astype(np.float32)
        csr = gs.DeviceCSR.from_scipy(adj, torch.device(DEV), weight=w)
    for nodes in (iso + [0, iso[1]], [0], iso[:1]):
        ids = torch.tensor(nodes, device=DEV)
        cl = gs.infer.closure(csr, ids, depth)
        assert all(int(b.col.shape[0]) == 0 and int(b.rowptr[-1]) == 0 for b in cl.blocks[1:])
        assert (cl.blocks[depth].edge_cdf is not None) == weighted
        got, emb = gs.infer.query(model, store, ids, adj=csr, embeddings=True)
        want, wemb = gs.full_neighbour(model, store, nodes=ids, adj=csr, embeddings=True)
        close(got.cpu().numpy(), want.cpu().numpy(), "logits", 2e-5, 2e-5)
        close(emb.cpu().numpy(), wemb[ids].cpu().numpy(), "embeddings", 2e-5, 2e-5)
    assert int(csr.err_flag.item()) == 0


# ---- the reduce over a block -------------------------------------------------------------------------------------
@pytest.mark.parametrize("odt", ["fp32", "bf16"])
@pytest.mark.parametrize("tdt", ["bf16", "fp32"])
@pytest.mark.parametrize("mode", ["mean", "max", "softmax", "weighted_mean"])
def test_block_reduce_is_the_whole_graph_reduce_bit_for_bit(mode, tdt, odt):
    gs = pkg()
    nat, infer = gs._native, gs.infer
    g = sr.graph(256)
    adj = g.csr(DEV)
    q = edge_queries(g)
    if mode == "weighted_mean":
        adj = adj.with_weights(torch.from_numpy(weights_for(g)))
        q = np.concatenate([q, [g.at[7], g.n - 1]])
    q = np.concatenate([q, [g.n // 2, g.n - 1, g.at[257], g.at[256], g.at[8]]])        # the sliced rows, the slice edge
    cl = infer.closure(adj, torch.from_numpy(q), 1)
    blk, S0, S1 = cl.blocks[1], cl.sets[0], cl.sets[1]
    assert blk.dummy != 0 and infer.plan(blk)["n_long"] >= 3 and blk.n_src > blk.n_dst
    D = 40
    table, keys = sr.inputs(g.n, D, tdt, seed=77)
    table = torch.tensor(table).to(sr.TORCH_DT[tdt]).to(DEV)
    keys = torch.tensor(keys).to(DEV) if mode == "softmax" else None
    code = {"mean": nat.SEG_MEAN, "max": nat.SEG_MAX, "softmax": nat.SEG_SOFTMAX_WEIGHTED,
            "weighted_mean": nat.SEG_WEIGHTED_MEAN}[mode]
    for act in (nat.ACT_NONE, nat.ACT_RELU):
        whole = torch.full((g.n, D), -7.5, dtype=sr.TORCH_DT[odt], device=DEV)
        infer.segment_reduce(adj, table, code, whole, act, keys=keys)
        part = torch.full((blk.n_dst, D), -7.5, dtype=sr.TORCH_DT[odt], device=DEV)
        infer.segment_reduce(blk, table[S0].contiguous(), code, part, act, keys=None if keys is None else keys[S0].contiguous())
        assert torch.equal(sr.bits(part), sr.bits(whole[S1])), (mode, tdt, odt, act)
    # the empty rows read the dummy's row -- at a local index other than 0
    empty = [i for i, v in enumerate(S1.tolist()) if g.deg[v] == 0]
    assert len(empty) >= 2 and torch.equal(part[empty[0]].float(), torch.relu(table[0].float()).to(sr.TORCH_DT[odt]).float())
    assert int(adj.err_flag.item()) == 0


# ---- query ---------------------------------------------------------------------------------------------------------
_PROBLEMS = {}


def _problem(depth, D=50, n=500):
    if depth not in _PROBLEMS:
        rng = np.random.RandomState(depth)
        adj, indptr, data = sparse_graph(n, rng, max_deg=12, long_row=(17, 300))      # one row above infer.SLICE_LEN
        feats = rng.normal(size=(n + 1, D)).astype(np.float32)
        feats[0] = 0
        nodes = np.concatenate([[17, 3, 0, int(data[indptr[17]]), 17], rng.randint(1, n + 1, size=20)])
        assert indptr[4] == indptr[3]                                                  # (row 3 has degree 0)
        _PROBLEMS[depth] = (adj, neighbours_sparse(indptr, data), feats, nodes)
    return _PROBLEMS[depth]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("prep", ["identity", "linear"])
@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("depth", [2, 3])
def test_query_matches_float64_reference(agg, prep, depth, precision):
    gs = pkg()
    gs.ops.set_compute_dtype(precision)
    adj, nbrs, feats, nodes = _problem(depth)
    model = make_model(agg, prep, adj, feats.shape[1], dims=(16,) * (depth - 1) + (24,)).to(DEV)
    store = gs.FeatureStore.from_array(feats, torch.device(DEV), dtype=precision)
    ids = torch.from_numpy(nodes).to(DEV)
    logits, emb = gs.infer.query(model, store, ids, embeddings=True)
    ref_logits, ref_emb = reference(model, store.dense().cpu().numpy(), nbrs)
    tol = 2e-5 if precision == "fp32" else 3e-2
    assert logits.shape[0] == nodes.shape[0] and emb.shape[0] == nodes.shape[0]
    close(emb.cpu().numpy(), ref_emb[nodes], "embeddings", tol, tol)
    close(logits.cpu().numpy(), ref_logits[nodes], "logits", tol, tol)
    assert torch.equal(logits[0], logits[4])                                           # a duplicate repeats its row
    assert torch.equal(gs.full_neighbour(model, store, nodes=ids, closure=True), logits)
    assert int(model.val_sampler.csr(DEV).err_flag.item()) == 0


def test_query_on_an_fp8_store_decodes_the_closure_rows_only():
    gs = pkg()
    gs.ops.set_compute_dtype("bf16")
    adj, nbrs, feats, nodes = _problem(2)
    model = make_model("mean", "identity", adj, feats.shape[1]).to(DEV)
    store8 = gs.FeatureStore.from_array(feats, torch.device(DEV), dtype="fp8")
    ids = torch.from_numpy(nodes).to(DEV)
    a, ea = gs.infer.query(model, store8, ids, embeddings=True)
    b, eb = gs.infer.query(model, store8.decoded("bf16"), ids, embeddings=True)
    assert torch.equal(a, b) and torch.equal(ea, eb)
    whole = gs.full_neighbour(model, store8, nodes=ids)
    close(a.cpu().numpy(), whole.cpu().numpy(), "fp8 query vs whole graph", 3e-2, 3e-2)


# ---- errors and state ----------------------------------------------------------------------------------------------
def test_out_of_range_neighbour_raises_the_flag_and_is_left_out():
    gs = pkg()
    g0 = sr.graph(256)
    r = g0.at[9]
    g = g0.with_ids([(int(g0.rowptr[r]) + 4, g0.n + 5), (int(g0.rowptr[r]) + 6, -3)])
    adj = g.csr(DEV)
    q = np.array([r, 46, 2], dtype=np.int64)
    ref = cr.closure_ref(g.rowptr, g.col, g.n, q, 2)
    assert ref.bad
    got = gs.infer.closure(adj, torch.from_numpy(q), 2)
    cr.assert_equal(got, ref, "bad neighbour", n=g.n)
    assert all(int(s.max()) < g.n and int(s.min()) >= 0 for s in got.sets)
    b = got.blocks[2]
    assert int(b.col[int(b.rowptr[0]) + 4]) == b.dummy and int(b.col[int(b.rowptr[0]) + 6]) == b.dummy
    with pytest.raises(IndexError):
        adj.check()
    adj.check()                                                                        # (the flag was reset)
    # a query outside the graph: dropped, flagged, and query() refuses to answer
    got = gs.infer.closure(adj, torch.tensor([r, g.n, 2, -1]), 1)
    assert got.sets[1].tolist() == [r, 2] and got.index.tolist() == [0, -1, 1, -1]
    with pytest.raises(IndexError):
        adj.check()
    assert _at_rest(adj)


def test_state_is_restored_between_queries():
    gs = pkg()
    g = sr.graph(256)
    adj = g.csr(DEV)
    q1 = torch.from_numpy(edge_queries(g))
    q2 = torch.tensor([g.n - 1, 7, 7, 300, 0, 46])
    first = gs.infer.closure(adj, q1, 2)
    assert _at_rest(adj) and adj._closure_state["local"].shape[0] == g.n
    state = adj._closure_state
    second = gs.infer.closure(adj, q2, 3)
    assert adj._closure_state is state and _at_rest(adj)                               # cached, not re-allocated
    fresh = gs.infer.closure(g.csr(DEV), q2, 3)
    cr.assert_equal(second, cr.closure_ref(g.rowptr, g.col, g.n, q2.numpy(), 3), "second query", n=g.n)
    for l in range(4):
        assert torch.equal(second.sets[l], fresh.sets[l])
    for l in range(1, 4):
        assert torch.equal(second.blocks[l].col, fresh.blocks[l].col)
    assert first.sets[2].tolist() == cr.closure_ref(g.rowptr, g.col, g.n, q1.numpy(), 2).sets[2].tolist()


# ---- train.py ------------------------------------------------------------------------------------------------------
def test_train_main_closure_flags(capsys, tmp_path, monkeypatch):
    gs = pkg()
    rng = np.random.RandomState(5)
    n, D, C = 300, 16, 4
    adj, _, _ = sparse_graph(n, rng, max_deg=8)
    feats = rng.normal(size=(n + 1, D)).astype(np.float32)
    feats[0] = 0
    folds = np.array(["train"] * 200 + ["val"] * 60 + ["test"] * (n + 1 - 260))
    folds[0] = "dummy"
    prob = gs.NodeProblem.from_arrays("classification", C, adj, adj, feats, folds,
                                      feats[:, :C].argmax(1).reshape(-1, 1), cuda=True)
    p, ids_path = str(tmp_path / "emb.npy"), str(tmp_path / "ids.npy")
    ids = np.array([250, 3, 17, 250, 1, 299])
    np.save(ids_path, ids)
    train = importlib.import_module("pytorch-graphsage_amd.train")
    built, build_model = [], train.build_model
    monkeypatch.setattr(train, "build_model", lambda a, pr: built.append(build_model(a, pr)) or built[-1])
    train.main(["--problem-path", "<memory>", "--epochs", "2", "--batch-size", "64", "--sampler-class",
                "sparse_uniform_neighbor_sampler", "--n-train-samples", "5,3", "--n-val-samples", "5,3",
                "--output-dims", "16,16", "--show-test", "--full-neighbour-eval", "--eval-closure",
                "--save-embeddings", p, "--embed-nodes", ids_path], problem=prob)
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert lines[-1]["test_f1"] is not None and lines[-2]["val_metric"] is not None
    emb = np.load(p)
    assert emb.shape == (ids.shape[0], 32)
    _, want = gs.infer.query(built[0], prob.feats, torch.from_numpy(ids).to(DEV), embeddings=True)
    assert np.array_equal(emb, want.cpu().numpy())
    with pytest.raises(SystemExit):
        train.main(["--problem-path", "<memory>", "--eval-closure"], problem=prob)
    with pytest.raises(SystemExit):
        train.main(["--problem-path", "<memory>", "--embed-nodes", ids_path], problem=prob)
