"""Retrieval over embeddings on the MI355X (csrc/gsage_retrieve.hip behind ops.topk_ip / gs.nearest) against
tests/retrieve_ref.py: exact on integer data with ties everywhere, bit-identical for every split count, tolerance-checked
on random unit rows, the exclusions and the -1 / -inf padding, and the public paths.  No time is asserted."""
import importlib

import numpy as np
import pytest
import torch

import retrieve_ref as rr
from conftest import pkg
from full_neighbour_ref import make_model, sparse_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _dtype():
    gs = pkg()
    yield
    gs.ops.set_compute_dtype("bf16")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


_REF = {}


def _integer(D):
    """The integer case of width D and its reference for k = 128 (a prefix of it is the reference for a smaller k;
    the data are exact in both modes, so one reference serves both)."""
    if D not in _REF:
        E, Qm = rr.integer_case(1001, 33, D, seed=D)
        ids, sc, _, _ = rr.topk_ref(E, Qm, 128, "fp32")
        _REF[D] = (E, Qm, ids, sc.astype(np.float32))
    return _REF[D]


# ---- 1. exact, with ties everywhere ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("D", [40, 48, 256])
def test_exact_on_integer_data_with_ties(D, k, mode):
    gs = pkg()
    gs.ops.set_compute_dtype(mode)
    E, Qm, want_ids, want_sc = _integer(D)
    assert np.unique(want_sc[:, :10]).size < 60                         # a thousand rows share a few dozen scores
    before = gs._native.launch_count()
    ids, sc = gs.ops.topk_ip(_dev(E), _dev(Qm), k)
    assert gs._native.launch_count() - before == 2                      # scan + merge, nothing else
    assert torch.equal(ids.cpu(), torch.from_numpy(want_ids[:, :k].copy()))
    assert torch.equal(sc.cpu(), torch.from_numpy(want_sc[:, :k].copy()))


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_rows_that_are_not_whole_16_byte_chunks(mode):
    """D = 45 (no multiple of a chunk in either mode) out of a wider buffer whose pad columns hold garbage: nothing
    past a row's D columns may be read."""
    gs = pkg()
    gs.ops.set_compute_dtype(mode)
    E, Qm = rr.integer_case(203, 5, 45, seed=8)
    want_ids, want_sc, _, _ = rr.topk_ref(E, Qm, 10, mode)
    dt = gs.ops.torch_dtype()
    for ld in (45, 47, 48):
        Eb = torch.full((203, ld), 7.0, dtype=dt, device=DEV)
        Qb = torch.full((5, ld), -5.0, dtype=dt, device=DEV)
        Eb[:, :45] = _dev(E).to(dt)
        Qb[:, :45] = _dev(Qm).to(dt)
        ids, sc = gs.ops.topk_ip(Eb[:, :45], Qb[:, :45], 10)
        assert torch.equal(ids.cpu(), torch.from_numpy(want_ids)), ld
        assert torch.equal(sc.cpu(), torch.from_numpy(want_sc.astype(np.float32))), ld


# ---- 2. grid independence ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("case", ["integer", "float"])
def test_result_is_bit_identical_for_every_split_count(case, mode):
    gs = pkg()
    gs.ops.set_compute_dtype(mode)
    if case == "integer":
        E, Qm, _, _ = _integer(48)
        k = 10
    else:
        rng = np.random.RandomState(1)
        E = rng.normal(size=(5003, 256)).astype(np.float32)
        Qm = rng.normal(size=(70, 256)).astype(np.float32)
        k = 20
    Ed, Qd = _dev(E), _dev(Qm)
    first = None
    for splits in (1, 3, 7, 0, 0):                                       # (0 twice: two repeated calls)
        ids, sc = gs.ops.topk_ip(Ed, Qd, k, splits=splits)
        if first is None:
            first = (ids, sc)
        assert torch.equal(ids, first[0]) and torch.equal(sc, first[1]), splits
    assert int(first[0].min()) >= 0


def test_recorded_in_a_command_list_with_the_callers_workspace():
    gs = pkg()
    E, Qm, want_ids, want_sc = _integer(48)
    Ed, Qd = _dev(E).to(torch.bfloat16), _dev(Qm).to(torch.bfloat16)
    nbytes, splits = gs.ops.topk_ip_workspace(33, 1001, 10, 3)
    assert splits == 3
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = (torch.zeros(33, 10, dtype=torch.int64, device=DEV), torch.zeros(33, 10, dtype=torch.float32, device=DEV))
    with gs._native.CommandList.record() as cl:
        gs.ops.topk_ip(Ed, Qd, 10, splits=3, workspace=ws, out=out)
    assert len(cl) == 2 and int(out[0].abs().sum()) == 0                 # recorded, not run
    cl.replay(gs.ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(out[0].cpu(), torch.from_numpy(want_ids[:, :10].copy()))
    assert torch.equal(out[1].cpu(), torch.from_numpy(want_sc[:, :10].copy()))


# ---- 3. random unit rows, tolerance-checked --------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("D", [64, 256])
def test_random_unit_rows_within_the_derived_tolerance(D, mode, seed):
    gs = pkg()
    gs.ops.set_compute_dtype(mode)
    N, Q, k = 5003, 70, 20
    E = rr.unit_rows(N, D, seed)
    nodes = np.random.RandomState(100 + seed).randint(0, N, size=Q)
    emb = _dev(E)
    ids, sc = gs.nearest(emb, _dev(nodes), k=k, exclude="self")
    frac = rr.check_tolerance(ids.cpu().numpy(), sc.cpu().numpy(), E, E[nodes], k, mode, "self", nodes,
                              min_unambiguous=0.6)
    print("D=%d %s seed=%d: %.0f %% of the queries have a clear gap at rank k" % (D, mode, seed, 100 * frac))


# ---- 4. exclusion and padding ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("exclude", ["none", "self", "neighbours"])
def test_exclusion_and_padding(exclude, mode):
    gs = pkg()
    gs.ops.set_compute_dtype(mode)
    N, k = 50, 64
    E, _ = rr.integer_case(N, 1, 24, seed=4)
    rowptr, col = rr.hub_csr(N)
    assert rowptr[3] - rowptr[2] == 40 and rowptr[6] == rowptr[5] and 9 in col[rowptr[9]:rowptr[10]]
    hub = col[rowptr[2]:rowptr[3]]
    assert np.unique(hub).size == 39 and (np.diff(hub) < 0).any()         # a duplicate column, unsorted
    nodes = np.array([2, 5, 9, 2, 7], dtype=np.int64)
    adj = gs.DeviceCSR(_dev(rowptr), _dev(col), N, 40)
    ids, sc = gs.nearest(_dev(E), _dev(nodes), k=k, exclude=exclude, adj=adj)
    want_ids, want_sc, _, ok = rr.topk_ref(E, E[nodes], k, mode, exclude, nodes, rowptr, col)
    assert torch.equal(ids.cpu(), torch.from_numpy(want_ids))
    assert torch.equal(sc.cpu(), torch.from_numpy(want_sc.astype(np.float32)))
    pad = (ids.cpu().numpy() == -1).sum(1)
    assert (pad == k - ok.sum(1)).all() and (pad >= 14).all()
    assert np.isneginf(sc.cpu().numpy()[ids.cpu().numpy() == -1]).all()
    if exclude == "neighbours":
        assert pad[0] == k - (N - 1 - 39 + (1 if 2 in hub else 0))       # the hub: itself and its 39 distinct columns


def test_nan_scores_are_never_selected():
    gs = pkg()
    gs.ops.set_compute_dtype("fp32")
    E, Qm = rr.integer_case(100, 3, 16, seed=2)
    E[[4, 40, 77]] = np.nan
    ids, sc = gs.ops.topk_ip(_dev(E), _dev(Qm), 128)
    want_ids, want_sc, _, _ = rr.topk_ref(E, Qm, 128, "fp32")
    assert torch.equal(ids.cpu(), torch.from_numpy(want_ids))
    assert torch.equal(sc.cpu(), torch.from_numpy(want_sc.astype(np.float32)))
    assert (ids.cpu().numpy() == -1).sum() == 3 * (128 - 97)


# ---- 5. public paths -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_nearest_over_a_models_embeddings(mode):
    gs = pkg()
    gs.ops.set_compute_dtype(mode)
    rng = np.random.RandomState(7)
    n, D, C = 699, 24, 5
    adj, _, _ = sparse_graph(n, rng)
    feats = rng.normal(size=(n + 1, D)).astype(np.float32)
    feats[0] = 0
    model = make_model("mean", "identity", adj, D).to(DEV)
    model.optimizer = torch.optim.Adam(model.parameters(), lr=0.01)
    store = gs.FeatureStore.from_array(feats, torch.device(DEV), dtype="fp32")
    ids = rng.randint(1, n + 1, size=64)
    model.train_step(ids=_dev(ids), feats=store, targets=_dev(rng.randint(0, C, size=(64, 1))),
                     loss_fn=gs.ProblemLosses.classification)
    emb = gs.embeddings(model, store)
    assert tuple(emb.shape) == (n + 1, 32)
    E = emb.cpu().numpy()
    live = np.flatnonzero(np.linalg.norm(E, axis=1) > 0.5)              # (the dummy's row is all zero: ties with itself)
    nodes = np.concatenate([live[rng.randint(0, live.size, size=40)], live[:2], live[:1]])
    got_ids, got_sc = gs.nearest(emb, _dev(nodes), k=10)
    assert torch.equal(got_ids[-1], got_ids[-3])                         # a duplicate is answered again
    rr.check_tolerance(got_ids.cpu().numpy(), got_sc.cpu().numpy(), E, E[nodes], 10, mode, "self", nodes)
    all_ids, all_sc = gs.nearest(emb, None, k=10)                        # Q = N = 700: the k-NN graph
    assert tuple(all_ids.shape) == (n + 1, 10)
    rr.check_tolerance(all_ids.cpu().numpy(), all_sc.cpu().numpy(), E, E, 10, mode, "self", np.arange(n + 1))
    assert torch.equal(all_ids[_dev(nodes)], got_ids) and torch.equal(all_sc[_dev(nodes)], got_sc)


@pytest.mark.parametrize("unsup", [False, True])
def test_train_main_save_neighbours(unsup, tmp_path):
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
    p_emb, p_nb, p_ids = str(tmp_path / "emb.npy"), str(tmp_path / "nb.npz"), str(tmp_path / "ids.npy")
    nodes = np.array([250, 3, 17, 250, 1, 299])
    np.save(p_ids, nodes)
    train = importlib.import_module("pytorch-graphsage_amd.train")
    common = ["--problem-path", "<memory>", "--epochs", "1", "--batch-size", "64", "--sampler-class",
              "sparse_uniform_neighbor_sampler", "--n-train-samples", "5,3", "--n-val-samples", "5,3",
              "--output-dims", "16,16"] + (["--unsupervised"] if unsup else [])
    calls, embeddings = [], gs.embeddings
    try:
        gs.embeddings = lambda *a, **kw: calls.append(1) or embeddings(*a, **kw)
        train.main(common + ["--save-embeddings", p_emb, "--save-neighbours", p_nb, "--neighbours-k", "7"], problem=prob)
    finally:
        gs.embeddings = embeddings
    assert len(calls) == 1                                                # one embedding pass for both files
    emb = torch.from_numpy(np.load(p_emb)).to(DEV)
    got = np.load(p_nb)
    assert sorted(got.files) == ["ids", "scores"] and got["ids"].shape == (n + 1, 7)
    ids, sc = gs.nearest(emb, None, k=7)
    assert np.array_equal(got["ids"], ids.cpu().numpy()) and np.array_equal(got["scores"], sc.cpu().numpy())
    if not unsup:
        train.main(common + ["--save-neighbours", p_nb, "--neighbour-nodes", p_ids, "--neighbours-exclude", "neighbours",
                             "--neighbours-k", "4"], problem=prob)
        got = np.load(p_nb)
        assert got["ids"].shape == (nodes.size, 4) and np.array_equal(got["ids"][0], got["ids"][3])
        rowptr, col = np.asarray(adj.indptr), np.asarray(adj.data)
        for q, v in enumerate(nodes):
            assert v not in got["ids"][q] and not np.isin(got["ids"][q], col[rowptr[v]:rowptr[v + 1]]).any()
