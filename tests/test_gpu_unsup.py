"""-m gpu: unsupervised GraphSAGE on the MI355X -- the batch builder bit-exact against the restatement of
tests/unsup_ref.py, the skip-gram head against float64 autograd (bound: the project's fp32 head bound, 1e-5 of each
tensor's max-abs, as test_head_ce_forward_backward_vs_torch), ops.skipgram_loss under autograd, GSUnsupervised,
infer.embeddings and the command line.  Measured errors go to GSAGE_PARITY_LOG (profiles/unsup_parity.jsonl)."""
import importlib
import json

import numpy as np
import pytest
import torch

import unsup_ref
from conftest import pkg
from test_unsup_host import _specs, make_unsup_model
from util import close_rel, note_parity

pytestmark = pytest.mark.gpu
gs = pkg()
ops = gs.ops
nat = gs._native
DEV = "cuda"
HEAD_BOUND = 1e-5


@pytest.fixture(autouse=True)
def _warm():
    ops.warmup(torch.device(DEV))
    yield
    ops.set_compute_dtype("bf16")


# ---- 1. builder ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walk():
    rowptr, col = unsup_ref.walk_graph()
    csr = gs.DeviceCSR(torch.from_numpy(rowptr).to(DEV), torch.from_numpy(col).to(DEV), 60, int(np.diff(rowptr).max()))
    return rowptr, col, csr, ops.neg_cdf(csr)


def _seeds(B):
    seeds = np.random.RandomState(B).randint(0, 60, size=B)
    seeds[0] = 7                                           # a seed without edges
    if B > 2:
        seeds[1], seeds[2] = 5, 10                         # the self-loop, the chain
    return seeds


SEED = 0x1234567887654321


@pytest.mark.parametrize("Q", [1, 20, 64])
@pytest.mark.parametrize("walk_len", [1, 5, 16])
@pytest.mark.parametrize("B", [1, 37, 256])
def test_builder_bit_exact(walk, B, walk_len, Q):
    rowptr, col, csr, cdf = walk
    # (the table is the builder's INPUT: the device's pow and parallel running sum round differently from numpy's)
    assert np.allclose(cdf.cpu().numpy(), unsup_ref.degree_cdf(rowptr), rtol=1e-12, atol=0)
    seeds = _seeds(B)
    ids, pw = ops.unsup_batch(csr, torch.from_numpy(seeds).to(DEV), walk_len, Q, cdf, {"seed": SEED, "call_base": 2})
    rid, rpw, err = unsup_ref.build_batch(rowptr, col, 60, seeds, walk_len, Q, cdf.cpu().numpy(), SEED, 2)
    assert err == 0 and int(csr.err_flag.item()) == 0
    assert ids.dtype == torch.int64 and pw.dtype == torch.float32
    assert torch.equal(ids.cpu(), torch.from_numpy(rid)) and torch.equal(pw.cpu(), torch.from_numpy(rpw))
    assert int(ids[B]) == 7 and float(pw[0]) == 0
    if B > 2:
        assert int(ids[B + 1]) == 5 and float(pw[1]) == 0
    assert (np.diff(rowptr)[ids[2 * B:].cpu().numpy()] > 0).all()          # no negative of degree 0


def test_builder_shards_counter_and_errors(walk):
    rowptr, col, csr, cdf = walk
    B, wl, Q = 64, 5, 20
    seeds = torch.from_numpy(_seeds(B)).to(DEV)
    ph = {"seed": SEED, "call_base": 4}
    ids, pw = ops.unsup_batch(csr, seeds, wl, Q, cdf, ph)
    # the shard [13, 37) of the batch draws what the whole batch draws (and the same negatives)
    sid, spw = ops.unsup_batch(csr, seeds[13:37], wl, Q, cdf, dict(ph, g0=13))
    assert torch.equal(sid[:24], ids[13:37]) and torch.equal(sid[24:48], ids[B + 13:B + 37])
    assert torch.equal(sid[48:], ids[2 * B:]) and torch.equal(spw, pw[13:37])
    # a device word advances the stream: call_base 3 + *ctr 1 is call 4, *ctr 2 is another draw
    ctr = torch.ones(1, dtype=torch.int64, device=DEV)
    cid, cpw = ops.unsup_batch(csr, seeds, wl, Q, cdf, {"seed": SEED, "call_base": 3, "call_ctr": ctr})
    assert torch.equal(cid, ids) and torch.equal(cpw, pw)
    ctr.fill_(2)
    nid, _ = ops.unsup_batch(csr, seeds, wl, Q, cdf, {"seed": SEED, "call_base": 3, "call_ctr": ctr})
    assert not torch.equal(nid[B:], ids[B:])
    rid, _, _ = unsup_ref.build_batch(rowptr, col, 60, seeds.cpu().numpy(), wl, Q, cdf.cpu().numpy(), SEED, 5)
    assert torch.equal(nid.cpu(), torch.from_numpy(rid))
    # an id outside the graph raises the flag and yields 0
    bad = seeds.clone()
    bad[3] = 60
    bid, bpw = ops.unsup_batch(csr, bad, wl, Q, cdf, ph)
    rid, rpw, err = unsup_ref.build_batch(rowptr, col, 60, bad.cpu().numpy(), wl, Q, cdf.cpu().numpy(), SEED, 4)
    assert err == 1 and int(csr.err_flag.item()) == 1
    csr.err_flag.zero_()
    assert torch.equal(bid.cpu(), torch.from_numpy(rid)) and torch.equal(bpw.cpu(), torch.from_numpy(rpw))
    assert int(bid[3]) == 0 and int(bid[B + 3]) == 0 and float(bpw[3]) == 0
    # an all-zero table is refused before anything is launched
    zero = torch.zeros(60, dtype=torch.float64, device=DEV)
    out, w = torch.zeros(2 * B + Q, dtype=torch.int64, device=DEV), torch.zeros(B, device=DEV)
    before = nat.launch_count()
    L = nat.lib()
    args = lambda total, wlen=wl: (csr.rowptr.data_ptr(), csr.col.data_ptr(), 60, seeds.data_ptr(), B, wlen, Q,   # noqa: E731
                                   zero.data_ptr(), total, SEED, None, 0, 0, out.data_ptr(), w.data_ptr(), None, None)
    assert L.gsage_unsup_batch(*args(0.0)) == -1 and b"weight" in L.gsage_last_error()
    assert L.gsage_unsup_batch(*args(float("nan"))) == -1
    assert L.gsage_unsup_batch(*args(1.0, 0)) == -1 and L.gsage_unsup_batch(*args(1.0, 17)) == -1
    assert nat.launch_count() == before
    with pytest.raises(RuntimeError):
        ops.unsup_batch(csr, seeds, wl, Q, zero, ph)


# ---- 2. head -------------------------------------------------------------------------------------------------------
def _head_inputs(B, Q, D):
    rng = np.random.RandomState(1000 * B + 10 * Q + D)
    E = rng.normal(size=(2 * B + Q, D)).astype(np.float32)
    zero_row = (0, B, 2 * B)[(B + Q + D) % 3]              # a seed, a positive or a negative: the 1e-12 clamp
    E[zero_row] = 0
    E[2 * B + Q - 1] *= 1e3
    E[B - 1 if B - 1 != zero_row else 2 * B - 1] *= 1e-3
    pw = np.ones(B, dtype=np.float32)
    dead = [0, B // 2] if B > 1 else [0]                   # pairs whose walk ended on the seed
    pw[dead] = 0
    return E, pw, dead


def _run_head(E, B, Q, D, pw, nw, dtype, lde, ldd):
    Ed = torch.zeros(2 * B + Q, lde, device=DEV)
    Ed[:, :D] = torch.from_numpy(E)
    Ed[:, D:] = 7.0                                        # the padding columns must not be read as data
    dE = torch.full((2 * B + Q, ldd), 3.0, dtype=dtype, device=DEV)
    loss, aff = torch.empty(1, device=DEV), torch.empty(B, 1 + Q, device=DEV)
    L = nat.lib()
    scratch = torch.empty(L.gsage_head_skipgram_scratch(B, Q, D), device=DEV)
    nat.check(L.gsage_head_skipgram(Ed.data_ptr(), lde, B, Q, D, pw.data_ptr(), nw, dE.data_ptr(), ops._code(dtype), ldd,
                                    loss.data_ptr(), aff.data_ptr(), scratch.data_ptr(), None), "head_skipgram")
    assert bool((dE[:, D:] == 3.0).all())                  # nothing stored past the width
    return loss, aff, dE[:, :D]


@pytest.mark.parametrize("D", [8, 256, 1000])
@pytest.mark.parametrize("Q", [1, 20, 64])
@pytest.mark.parametrize("B", [1, 16, 17, 37])
def test_head_vs_float64(B, Q, D):
    E, pw, dead = _head_inputs(B, Q, D)
    pwd = torch.from_numpy(pw).to(DEV)
    for nw in (1.0, 0.25):
        loss, aff, dE = _run_head(E, B, Q, D, pwd, nw, torch.float32, D + 3, D + 5)
        rl, raff, rdE = unsup_ref.head(torch.from_numpy(E), B, Q, torch.from_numpy(pw), nw)
        errs = {"loss": abs(float(loss) - float(rl)) / abs(float(rl)),
                "aff": float((aff.cpu().double() - raff).abs().max() / raff.abs().max()),
                "dE": float((dE.cpu().double() - rdE).abs().max() / rdE.abs().max())}
        print("head B=%d Q=%d D=%d nw=%g: %r" % (B, Q, D, nw, errs))
        note_parity("head/B%d_Q%d_D%d_nw%g" % (B, Q, D, nw), **errs)
        assert np.isfinite(float(loss))
        assert errs["loss"] <= HEAD_BOUND, errs
        close_rel(aff.cpu().numpy(), raff.numpy(), "aff", HEAD_BOUND)
        close_rel(dE.cpu().numpy(), rdE.numpy(), "dE", HEAD_BOUND)
        for i in dead:                                     # pair_w == 0: the positive's row gets no gradient at all
            assert bool((dE[B + i] == 0).all()) and bool((rdE[B + i] == 0).all())
        # bf16 gradient = the fp32 gradient rounded to bf16, bit for bit
        l16, a16, d16 = _run_head(E, B, Q, D, pwd, nw, torch.bfloat16, D + 3, D + 5)
        assert torch.equal(d16, dE.to(torch.bfloat16)) and torch.equal(l16, loss) and torch.equal(a16, aff)
        # deterministic: same inputs, same bits
        l2, a2, d2 = _run_head(E, B, Q, D, pwd, nw, torch.float32, D + 3, D + 5)
        assert torch.equal(d2, dE) and torch.equal(l2, loss)


def test_head_envelope():
    L = nat.lib()
    B, Q, D = 4, 3, 8
    E, pw = torch.randn(2 * B + Q, D, device=DEV), torch.ones(B, device=DEV)
    dE, loss = torch.empty(2 * B + Q, D, device=DEV), torch.empty(1, device=DEV)
    scratch = torch.empty(1 << 20, device=DEV)
    call = lambda B=B, Q=Q, D=D, lde=D, ldd=D, dt=nat.F32: L.gsage_head_skipgram(        # noqa: E731
        E.data_ptr(), lde, B, Q, D, pw.data_ptr(), 1.0, dE.data_ptr(), dt, ldd, loss.data_ptr(), None, scratch.data_ptr(),
        None)
    before = nat.launch_count()
    for kw in ({"Q": 65}, {"Q": 0}, {"D": 1025}, {"D": 0}, {"B": 0}, {"lde": 7}, {"ldd": 7}, {"dt": nat.FP8}):
        assert call(**kw) == -1, kw
    assert nat.launch_count() == before
    assert L.gsage_head_skipgram_scratch(37, 20, 256) == 3 * (20 * 256 + 1)
    assert call() == 0                                     # aff == NULL is allowed
    torch.cuda.synchronize()
    assert np.isfinite(float(loss))


# ---- 3. autograd ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Q,D", [(37, 20, 64), (64, 5, 300)])
def test_skipgram_loss_autograd_equals_host_mode(B, Q, D):
    torch.manual_seed(B)
    E = torch.randn(2 * B + Q, D)
    pw = (torch.rand(B) > 0.2).float()
    Eh = E.clone().requires_grad_(True)
    lh = ops.skipgram_loss(Eh, B, Q, pw, 0.5)
    (3.0 * lh).backward()
    Ed = E.to(DEV).requires_grad_(True)
    ld = ops.skipgram_loss(Ed, B, Q, pw.to(DEV), 0.5)
    assert ld.shape == () and ld.requires_grad
    (3.0 * ld).backward()
    assert abs(float(ld.detach()) - float(lh.detach())) <= HEAD_BOUND * abs(float(lh.detach()))
    close_rel(Ed.grad.cpu().numpy(), Eh.grad.numpy(), "dE", HEAD_BOUND)


# ---- 4. model ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prob():
    return unsup_ref.model_problem()


def test_model_overfits_evaluates_and_exports(prob):
    model = make_unsup_model(gs, prob, DEV)
    assert not any(k.startswith("fc.") for k in model.state_dict())
    store = gs.FeatureStore.from_array(prob["feats"], torch.device(DEV), dtype=ops.config.compute_dtype)
    batch = (torch.from_numpy(prob["batch_ids"]).to(DEV), torch.from_numpy(prob["pair_w"]).to(DEV))
    before = nat.launch_count()
    losses = [float(model.train_step(None, store, batch=batch)) for _ in range(40)]
    print("device overfit: first %.5f last %.5f" % (losses[0], losses[-1]))
    assert nat.launch_count() - before >= 40 * 4, "HIP kernels did not run"
    assert isinstance(model.optimizer, gs.optim.FlatAdam)
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    seeds = batch[0][:64]
    l0 = float(model.train_step(seeds, store))             # a batch built on the device
    assert np.isfinite(l0)
    res = model.evaluate(seeds, store)
    assert set(res) == {"loss", "mrr"} and np.isfinite(res["loss"]) and 0 < res["mrr"] <= 1
    for s in (model.train_sampler, model.val_sampler):
        for csr in s._dev.values():
            csr.check()
    out = model(seeds, store, train=False)
    assert out.shape == (64, 64) and torch.allclose(out.norm(dim=1), torch.ones(64, device=DEV), atol=1e-4)
    emb = gs.embeddings(model, store)
    assert emb.shape == (200, 64)
    assert torch.allclose(emb[1:].norm(dim=1), torch.ones(199, device=DEV), atol=1e-4)


def test_full_neighbour_is_embeddings_then_fc(prob):
    torch.manual_seed(0)
    model = gs.GSSupervised(
        sampler_class=gs.sampler_lookup["sparse_uniform_neighbor_sampler"], adj=prob["adj"], train_adj=prob["adj"],
        prep_class=gs.prep_lookup["identity"], aggregator_class=gs.aggregator_lookup["mean"], input_dim=16, n_nodes=200,
        n_classes=3, layer_specs=_specs()).to(DEV)
    store = gs.FeatureStore.from_array(prob["feats"], torch.device(DEV), dtype=ops.config.compute_dtype)
    nodes = torch.arange(5, 60, device=DEV)
    logits, emb = gs.full_neighbour(model, store, nodes=nodes, embeddings=True)
    emb2 = gs.embeddings(model, store)
    assert torch.equal(emb, emb2)
    want = ops.linear(emb2[nodes], model.fc.weight, model.fc.bias, compute_dtype="fp32")
    assert torch.equal(logits, want)
    assert torch.equal(gs.full_neighbour(model, store, nodes=nodes), logits)


# ---- 5. command line -----------------------------------------------------------------------------------------------
def test_train_main_unsupervised(prob, capsys, tmp_path, monkeypatch):
    problem = gs.NodeProblem.from_arrays("classification", 3, prob["adj"], prob["adj"], prob["feats"], prob["folds"],
                                         prob["targets"], cuda=True)
    path = str(tmp_path / "emb.npy")
    train = importlib.import_module("pytorch-graphsage_amd.train")
    argv = ["--problem-path", "<memory>", "--epochs", "2", "--batch-size", "64", "--sampler-class",
            "sparse_uniform_neighbor_sampler", "--n-train-samples", "5,3", "--n-val-samples", "5,3", "--output-dims",
            "32,32", "--unsupervised", "--walk-len", "5", "--n-negatives", "20", "--save-embeddings", path]
    train.main(argv, problem=problem)
    cap = capsys.readouterr()
    assert "unsupervised model: module path" in cap.err
    lines = [json.loads(l) for l in cap.out.splitlines() if l.startswith("{")]
    batches = [l for l in lines if "epoch_progress" in l]
    epochs = [l for l in lines if "mrr" in l and "epoch_progress" not in l]
    assert len(batches) == 2 * (140 // 64 + 1) and all(np.isfinite(l["loss"]) for l in batches)
    assert len(epochs) == 3 and all(0 < l["mrr"] <= 1 for l in epochs)         # one per epoch and the final line
    emb = np.load(path)
    assert emb.shape == (200, 64) and np.allclose(np.linalg.norm(emb[1:], axis=1), 1.0, atol=1e-4)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="data-parallel"):
        train.main(argv, problem=problem)
