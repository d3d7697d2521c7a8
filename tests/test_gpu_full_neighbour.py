"""Layer-wise full-neighbourhood inference on the MI355X (csrc/gsage_fullgraph.hip behind infer.full_neighbour):
against the float64 restatement of the definition, against the sampled forward where the two coincide, bitwise
determinism across split rows, GPU == host mode, the live weights of a fused engine, launches per call independent
of the node count, and the train.py flags."""
import importlib
import json

import numpy as np
import pytest
import torch
from scipy import sparse

from conftest import pkg
from full_neighbour_ref import make_model, neighbours_dense, neighbours_sparse, reference, sparse_graph
from util import close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AGGS = ["mean", "max_pool", "mean_pool", "attention"]
LONG = (17, 20500)                  # one row far above the split threshold (infer.SLICE_LEN)


@pytest.fixture(autouse=True)
def _dtype():
    gs = pkg()
    yield
    gs.ops.set_compute_dtype("bf16")


def _graph(seed, n=1500, D=602):
    rng = np.random.RandomState(seed)
    adj, indptr, data = sparse_graph(n, rng, max_deg=40, long_row=LONG)
    feats = rng.normal(size=(n + 1, D)).astype(np.float32)
    feats[0] = 0
    return rng, adj, indptr, data, feats


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("depth,D,dims", [
    pytest.param(2, 602, None, id="2-602"), pytest.param(3, 50, None, id="3-50"),
    # widths 18 and 10: no multiple of the 16-byte chunk in either precision, so infer._table's padding copy runs
    pytest.param(2, 50, (18, 10), id="2-50-dims18x10")])
def test_gpu_matches_float64_reference(agg, depth, D, dims, precision):
    gs = pkg()
    gs.ops.set_compute_dtype(precision)
    rng, adj, indptr, data, feats = _graph(depth, D=D)
    model = make_model(agg, "identity", adj, D, dims=dims or (16,) * (depth - 1) + (24,)).to(DEV)
    store = gs.FeatureStore.from_array(feats, torch.device(DEV), dtype=precision)
    logits, emb = gs.full_neighbour(model, store, embeddings=True)
    ref_logits, ref_emb = reference(model, store.dense().cpu().numpy(), neighbours_sparse(indptr, data))
    tol = 2e-5 if precision == "fp32" else 3e-2
    close(emb.cpu().numpy(), ref_emb, "embeddings", tol, tol)
    close(logits.cpu().numpy(), ref_logits, "logits", tol, tol)
    assert int(model.val_sampler.csr(DEV).err_flag.item()) == 0


@pytest.mark.parametrize("agg", AGGS)
def test_gpu_dense_sampler_anchor(agg):
    """fp32, dense sampler, n_val_samples == K: the sampled forward on the GPU IS the full-neighbourhood inference."""
    gs = pkg()
    gs.ops.set_compute_dtype("fp32")
    rng = np.random.RandomState(7)
    n, D, K = 300, 50, 6
    adj = torch.from_numpy(rng.randint(0, n + 1, size=(n + 1, K)).astype(np.int64))
    feats = rng.normal(size=(n + 1, D)).astype(np.float32)
    feats[n] = 0
    model = make_model(agg, "identity", adj, D, sampler="uniform_neighbor_sampler", n_val=K).to(DEV)
    store = gs.FeatureStore.from_array(feats, torch.device(DEV), dtype="fp32")
    ids = torch.arange(0, n, 5, device=DEV)
    with torch.no_grad():
        sampled = model(ids, store, train=False)
    full = gs.full_neighbour(model, store, nodes=ids)
    close(full.cpu().numpy(), sampled.cpu().numpy(), "dense anchor", 2e-5, 2e-5)
    ref, _ = reference(model, feats, neighbours_dense(adj.numpy()))
    close(full.cpu().numpy(), ref[ids.cpu().numpy()], "dense vs float64", 2e-5, 2e-5)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("agg", AGGS)
def test_gpu_bitwise_deterministic_with_split_rows(agg, precision):
    gs = pkg()
    gs.ops.set_compute_dtype(precision)
    _, adj, _, _, feats = _graph(11, D=128)
    model = make_model(agg, "linear", adj, 128, dims=(32, 32)).to(DEV)
    store = gs.FeatureStore.from_array(feats, torch.device(DEV), dtype=precision)
    a, ea = gs.full_neighbour(model, store, embeddings=True)
    b, eb = gs.full_neighbour(model, store, embeddings=True)
    assert gs.infer.plan(model.val_sampler.csr(DEV))["n_long"] == 1
    assert torch.equal(a, b) and torch.equal(ea, eb)


@pytest.mark.parametrize("agg", AGGS)
def test_gpu_equals_host_mode(agg):
    gs = pkg()
    gs.ops.set_compute_dtype("fp32")
    _, adj, _, _, feats = _graph(12, n=800, D=50)
    host = make_model(agg, "linear", adj, 50, seed=3)
    dev = make_model(agg, "linear", adj, 50, seed=3).to(DEV)
    ref = gs.full_neighbour(host, torch.from_numpy(feats))
    got = gs.full_neighbour(dev, torch.from_numpy(feats).to(DEV))
    close(got.cpu().numpy(), ref.numpy(), "gpu vs host", 2e-5, 2e-5)


def test_gpu_reads_the_weights_a_fused_engine_trained():
    gs = pkg()
    gs.ops.set_compute_dtype("bf16")
    rng, adj, _, _, feats = _graph(13, n=1000, D=64)
    model = make_model("mean", "identity", adj, 64, dims=(128, 128)).to(DEV)
    store = gs.FeatureStore.from_array(feats, torch.device(DEV), dtype="bf16")
    B, C = 40, 5
    batches = [(torch.from_numpy(rng.randint(1, 1001, size=B)).to(DEV),
                torch.from_numpy(rng.randint(0, C, size=(B, 1))).to(DEV)) for _ in range(3)]
    before = gs.full_neighbour(model, store)
    eng = gs.engine.FusedMeanTrainStep(model, store, gs.ProblemLosses.classification, batches[0][0], batches[0][1],
                                       capture=False)
    for ids, tg in batches:
        eng(ids, tg)
    torch.cuda.synchronize()
    after = gs.full_neighbour(model, store)
    assert not torch.equal(before, after)
    host = make_model("mean", "identity", adj, 64, dims=(128, 128))
    with torch.no_grad():
        for (k, p), (k2, q) in zip(host.named_parameters(), model.named_parameters()):
            assert k == k2
            p.copy_(q.detach().cpu())
    ref = gs.full_neighbour(host, store.dense().cpu())
    close(after.cpu().numpy(), ref.numpy(), "engine-trained weights", 3e-2, 3e-2)


def test_gpu_launches_per_call_do_not_depend_on_node_count():
    gs = pkg()
    gs.ops.set_compute_dtype("bf16")
    dev = torch.device(DEV)
    counts = []
    for n in (10000, 200000):
        csr = gs.DeviceCSR.synthetic(n, 1, 12, dev, empty_every=9, seed=1)
        store = gs.FeatureStore.synthetic(n, 50, dev)
        placeholder, _, _ = sparse_graph(10, np.random.RandomState(0))
        model = make_model("max_pool", "identity", placeholder, 50).to(DEV)
        gs.full_neighbour(model, store, adj=csr)                 # builds (and caches) the plan
        torch.cuda.synchronize()
        c0 = gs._native.launch_count()
        gs.full_neighbour(model, store, adj=csr)
        torch.cuda.synchronize()
        counts.append(gs._native.launch_count() - c0)
    assert counts[0] == counts[1] and counts[0] >= 4


def test_gpu_train_main_flags(capsys, tmp_path):
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
    p = str(tmp_path / "emb.npy")
    train = importlib.import_module("pytorch-graphsage_amd.train")
    train.main(["--problem-path", "<memory>", "--epochs", "2", "--batch-size", "64", "--sampler-class",
                "sparse_uniform_neighbor_sampler", "--n-train-samples", "5,3", "--n-val-samples", "5,3",
                "--output-dims", "16,16", "--show-test", "--full-neighbour-eval", "--save-embeddings", p],
               problem=prob)
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert lines[-1]["test_f1"] is not None and lines[-2]["val_metric"] is not None
    emb = np.load(p)
    assert emb.shape == (n + 1, 32)
    assert np.allclose(np.linalg.norm(emb[1:], axis=1), 1.0, atol=1e-4)
