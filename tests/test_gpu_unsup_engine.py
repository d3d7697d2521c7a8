"""-m gpu: the fused unsupervised engine (engine/unsup.py) on the MI355X -- the skip-gram head with a live-seed count
against float64 autograd of the masked loss (tests/unsup_engine_ref.py; bound: the project's fp32 head bound), the
engine's batches against GSUnsupervised.build_batch bit for bit, its steps against GSUnsupervised.train_step from
identical weights (tolerances of test_gpu_engine.py in bf16, 2e-4 with an fp32 store), short batches against autograd
of the masked loss, the handover back to the module path and the command line.
Measured errors go to GSAGE_PARITY_LOG (profiles/unsup_parity.jsonl)."""
import importlib
import json

import numpy as np
import pytest
import torch

import unsup_engine_ref as uref
import unsup_ref
from conftest import pkg
from test_gpu_unsup import _head_inputs
from util import close_fro, close_rel, note_parity

pytestmark = pytest.mark.gpu
gs = pkg()
ops = gs.ops
nat = gs._native
DEV = "cuda"
HEAD_BOUND = 1e-5
FP32_BOUND = 2e-4


@pytest.fixture(autouse=True)
def _warm():
    ops.set_compute_dtype("bf16")
    ops.warmup(torch.device(DEV))
    yield
    ops.set_compute_dtype("bf16")


# ---- 1. head, direct -----------------------------------------------------------------------------------------------
def _run_live(E, B, Q, D, pw, nw, dtype, lde, ldd, b, entry="live"):
    """entry: "live" (n_valid = a device word holding b), "null" (the live entry, n_valid == NULL), "plain" (the
    existing entry point)"""
    Ed = torch.zeros(2 * B + Q, lde, device=DEV)
    Ed[:, :D] = torch.from_numpy(E)
    Ed[:, D:] = 7.0                                        # the padding columns must not be read as data
    dE = torch.full((2 * B + Q, ldd), 3.0, dtype=dtype, device=DEV)        # stale: padded rows must be WRITTEN
    loss, aff = torch.empty(1, device=DEV), torch.full((B, 1 + Q), 9.0, device=DEV)
    L = nat.lib()
    scratch = torch.empty(L.gsage_head_skipgram_scratch(B, Q, D), device=DEV)
    nv = torch.tensor([b], dtype=torch.int32, device=DEV)
    if entry == "plain":
        nat.check(L.gsage_head_skipgram(Ed.data_ptr(), lde, B, Q, D, pw.data_ptr(), nw, dE.data_ptr(), ops._code(dtype),
                                        ldd, loss.data_ptr(), aff.data_ptr(), scratch.data_ptr(), None), "head_skipgram")
    else:
        nat.check(L.gsage_head_skipgram_live(Ed.data_ptr(), lde, B, Q, D, pw.data_ptr(), nw,
                                             nv.data_ptr() if entry == "live" else None, dE.data_ptr(), ops._code(dtype),
                                             ldd, loss.data_ptr(), aff.data_ptr(), scratch.data_ptr(), None),
                  "head_skipgram_live")
    assert bool((dE[:, D:] == 3.0).all())                  # nothing stored past the width
    return loss, aff, dE[:, :D]


@pytest.mark.parametrize("D", [8, 256, 1000])
@pytest.mark.parametrize("Q", [1, 20, 64])
@pytest.mark.parametrize("B", [1, 16, 17, 37])
def test_live_head_vs_float64(B, Q, D):
    E, pw, dead = _head_inputs(B, Q, D)
    pwd = torch.from_numpy(pw).to(DEV)
    f32 = torch.float32
    for nw in (1.0, 0.25):
        for b in sorted({B, max(B - 1, 1), 1}, reverse=True):
            loss, aff, dE = _run_live(E, B, Q, D, pwd, nw, f32, D + 3, D + 5, b)
            rl, raff, rdE = uref.masked_head(torch.from_numpy(E), B, Q, torch.from_numpy(pw), nw, b)
            errs = {"loss": abs(float(loss) - float(rl)) / max(abs(float(rl)), 1e-300),
                    "aff": float((aff[:b].cpu().double() - raff[:b]).abs().max() / raff[:b].abs().max()),
                    "dE": float((dE.cpu().double() - rdE).abs().max() / rdE.abs().max())}
            print("live head B=%d b=%d Q=%d D=%d nw=%g: %r" % (B, b, Q, D, nw, errs))
            note_parity("live_head/B%d_b%d_Q%d_D%d_nw%g" % (B, b, Q, D, nw), **errs)
            assert np.isfinite(float(loss))
            assert errs["loss"] <= HEAD_BOUND, errs
            close_rel(aff[:b].cpu().numpy(), raff[:b].numpy(), "aff", HEAD_BOUND)
            close_rel(dE.cpu().numpy(), rdE.numpy(), "dE", HEAD_BOUND)
            # padded seeds: rows i and B + i are exact zeros (written, not left stale), aff is not touched
            assert bool((dE[b:B] == 0).all()) and bool((dE[B + b:2 * B] == 0).all())
            assert bool((rdE[b:B] == 0).all()) and bool((rdE[B + b:2 * B] == 0).all())
            assert bool((aff[b:] == 9.0).all())
            # bf16 gradient = the fp32 gradient rounded to bf16, bit for bit
            l16, a16, d16 = _run_live(E, B, Q, D, pwd, nw, torch.bfloat16, D + 3, D + 5, b)
            assert torch.equal(d16, dE.to(torch.bfloat16)) and torch.equal(l16, loss) and torch.equal(a16, aff)
            # deterministic: same inputs, same bits
            l2, a2, d2 = _run_live(E, B, Q, D, pwd, nw, f32, D + 3, D + 5, b)
            assert torch.equal(d2, dE) and torch.equal(l2, loss) and torch.equal(a2, aff)
            if b == B:                                     # every seed live, or no count at all: the existing entry's bits
                for entry, nv in (("plain", B), ("null", B), ("live", B + 5)):
                    l0, a0, d0 = _run_live(E, B, Q, D, pwd, nw, f32, D + 3, D + 5, nv, entry=entry)
                    assert torch.equal(l0, loss) and torch.equal(a0, aff) and torch.equal(d0, dE), entry


def test_live_head_through_ops_and_envelope():
    B, Q, D = 17, 5, 24
    torch.manual_seed(3)
    E, pw = torch.randn(2 * B + Q, D, device=DEV), (torch.rand(B, device=DEV) > 0.2).float()
    l0, a0, d0 = ops.skipgram_head(E, B, Q, pw, 0.5)
    l1, a1, d1 = ops.skipgram_head(E, B, Q, pw, 0.5, n_valid=None)
    l2, a2, d2 = ops.skipgram_head(E, B, Q, pw, 0.5, n_valid=B)
    assert torch.equal(l0, l1) and torch.equal(d0, d1) and torch.equal(l0, l2) and torch.equal(d0, d2) and \
        torch.equal(a0, a2)
    l3, a3, d3 = ops.skipgram_head(E, B, Q, pw, 0.5, n_valid=torch.tensor([2], dtype=torch.int32, device=DEV))
    rl, raff, rdE = uref.masked_head(E.cpu(), B, Q, pw.cpu(), 0.5, 2)
    assert abs(float(l3) - float(rl)) <= HEAD_BOUND * abs(float(rl))
    close_rel(d3.cpu().numpy(), rdE.numpy(), "dE", HEAD_BOUND)
    assert bool((a3[2:] == 0).all()) and bool((d3[2:B] == 0).all())
    # bad arguments: EINVAL before any launch, as the existing entry point
    L = nat.lib()
    dE, loss = torch.empty(2 * B + Q, D, device=DEV), torch.empty(1, device=DEV)
    scratch = torch.empty(1 << 16, device=DEV)
    nv = torch.tensor([3], dtype=torch.int32, device=DEV)
    call = lambda B=B, Q=Q, D=D, lde=D, ldd=D, dt=nat.F32: L.gsage_head_skipgram_live(        # noqa: E731
        E.data_ptr(), lde, B, Q, D, pw.data_ptr(), 1.0, nv.data_ptr(), dE.data_ptr(), dt, ldd, loss.data_ptr(), None,
        scratch.data_ptr(), None)
    before = nat.launch_count()
    for kw in ({"Q": 65}, {"Q": 0}, {"D": 1025}, {"D": 0}, {"B": 0}, {"lde": D - 1}, {"ldd": D - 1}, {"dt": nat.FP8}):
        assert call(**kw) == -1, kw
    assert nat.launch_count() == before
    assert call() == 0
    torch.cuda.synchronize()
    assert np.isfinite(float(loss))


# ---- the engine ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prob():
    adj, feats, _ = uref.problem()
    return adj, feats


def _twins(prob, dims, fans, Q, nw, dtype="bf16"):
    adj, feats = prob
    store = gs.FeatureStore.from_array(feats, torch.device(DEV), dtype=dtype)
    mk = lambda: uref.make_model(gs, adj, feats.shape[1], dims, fans, Q, nw, DEV)       # noqa: E731
    ref_model, eng_model = mk(), mk()
    eng_model.load_state_dict(ref_model.state_dict())
    return store, ref_model, eng_model


def _seed_batches(adj, B, n, seed=1):
    rng = np.random.RandomState(seed)
    return [torch.from_numpy(rng.randint(1, adj.shape[0], size=B)).to(DEV) for _ in range(n)]


# ---- 2. same batch as the module path ------------------------------------------------------------------------------
@pytest.mark.parametrize("capture", [False, "cmdlist"])
def test_engine_builds_the_module_paths_batches(prob, capture):
    B, Q = 17, 5
    store, ref_model, eng_model = _twins(prob, (16, 8), (5, 3), Q, 1.0)
    batches = _seed_batches(prob[0], B, 4)
    # the models' stream does not start at 0: one batch each before the engine exists
    ref_model.build_batch(batches[3])
    eng_model.build_batch(batches[3])
    eng = gs.engine.FusedUnsupMeanTrainStep(eng_model, store, batches[0], capture=capture)
    R = 2 * B + Q
    assert eng.B == R and eng.size[0] == R and eng.off[1] == R
    torch.cuda.synchronize()
    # the warm-up inside the constructor has advanced nothing
    assert eng_model._batch_calls == [0, 1] and int(eng.batch_ctr.item()) == 0 and int(eng.counter.item()) == 0
    assert int(eng.step.item()) == 0
    for t, seeds in enumerate(batches[:3]):
        eng(seeds)
        rid, rpw = ref_model.build_batch(seeds)
        assert torch.equal(eng.ids_set[0][:R], rid) and torch.equal(eng.pair_w, rpw), t
        assert int(eng.batch_ctr.item()) == t + 1
    assert eng_model._batch_calls[1] == ref_model._batch_calls[1] == 4
    a, b = eng_model.build_batch(batches[3]), ref_model.build_batch(batches[3])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # ... and the engine follows a stream that moved without it (the module-path build_batch above)
    eng(batches[0])
    rid, rpw = ref_model.build_batch(batches[0])
    assert torch.equal(eng.ids_set[0][:R], rid) and torch.equal(eng.pair_w, rpw)
    eng_model.train_sampler.csr(DEV).check()
    with pytest.raises(ValueError):
        eng.load_epoch(None, None)
    with pytest.raises(ValueError):
        eng.step_queue()


# ---- 3. step parity ------------------------------------------------------------------------------------------------
SHAPES = [((128, 128), (25, 10), 16, 20), ((16, 8), (5, 3), 17, 5), ((32, 16, 8), (4, 3, 2), 8, 3)]


def _parity_run(prob, dims, fans, B, Q, nw, capture, dtype):
    """three steps, each from identical weights -> [(loss error, {name: gradient error}, {name: weight error})]"""
    store, ref_model, eng_model = _twins(prob, dims, fans, Q, nw, dtype)
    ref_model.optimizer = torch.optim.Adam(ref_model.parameters(), lr=0.01, weight_decay=1e-4)
    batches = _seed_batches(prob[0], B, 3)
    assert gs.engine.FusedUnsupMeanTrainStep.supports(eng_model, store)
    eng = gs.engine.FusedUnsupMeanTrainStep(eng_model, store, batches[0], capture=capture)
    assert eng.capture_mode == (capture or None)
    out = []
    for seeds in batches:
        ref_model.load_state_dict(eng_model.state_dict())
        l_ref = float(ref_model.train_step(seeds, store))
        l_eng = float(eng(seeds))
        fro = lambda a, b: float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-12))       # noqa: E731
        grads, wts = {}, {}
        for (k, a), (_, b) in zip(eng_model.named_parameters(), ref_model.named_parameters()):
            grads[k] = fro(a.grad.double().cpu().numpy(), b.grad.double().cpu().numpy())
            wts[k] = fro(a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy())
        out.append((abs(l_eng - l_ref) / max(1.0, abs(l_ref)), grads, wts, l_eng, l_ref))
    eng_model.train_sampler.csr(DEV).check()
    return out


@pytest.mark.parametrize("nw", [1.0, 2.0])
@pytest.mark.parametrize("dims,fans,B,Q", SHAPES)
@pytest.mark.parametrize("capture", [False, "cmdlist"])
def test_engine_step_matches_train_step(prob, capture, dims, fans, B, Q, nw):
    res = _parity_run(prob, dims, fans, B, Q, nw, capture, "bf16")
    for step, (le, grads, wts, l_eng, l_ref) in enumerate(res):
        print("bf16 step %d: loss %.6f vs %.6f, worst grad %.3g, worst weight %.3g"
              % (step, l_eng, l_ref, max(grads.values()), max(wts.values())))
    for step, (le, grads, wts, l_eng, l_ref) in enumerate(res):
        assert np.isfinite(l_eng) and le <= 3e-2, (step, l_eng, l_ref)
        for k, e in grads.items():
            assert e <= 0.1, ("grad", step, k, e)
        if step == 0:
            for k, e in wts.items():
                assert e <= 0.05, ("weight", k, e)


@pytest.mark.parametrize("nw", [1.0, 2.0])
@pytest.mark.parametrize("dims,fans,B,Q", SHAPES)
@pytest.mark.parametrize("capture", [False, "cmdlist"])
def test_engine_step_matches_train_step_fp32(prob, capture, dims, fans, B, Q, nw):
    ops.set_compute_dtype("fp32")
    res = _parity_run(prob, dims, fans, B, Q, nw, capture, "fp32")
    worst = 0.0
    for step, (le, grads, wts, l_eng, l_ref) in enumerate(res):
        print("fp32 step %d: loss %.8f vs %.8f (%.3g), worst grad %.3g" % (step, l_eng, l_ref, le, max(grads.values())))
        worst = max(worst, abs(l_eng - l_ref) / abs(l_ref), max(grads.values()))
    note_parity("unsup_engine_fp32/%s_B%d_Q%d_nw%g_%s" % ("x".join(map(str, dims)), B, Q, nw, capture or "eager"),
                worst=worst)
    for step, (le, grads, wts, l_eng, l_ref) in enumerate(res):
        assert abs(l_eng - l_ref) <= FP32_BOUND * abs(l_ref), (step, l_eng, l_ref)
        for k, e in grads.items():
            assert e <= FP32_BOUND, ("grad", step, k, e)


# ---- 4. short batches ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_short_batches_take_the_masked_loss(prob, dtype):
    ops.set_compute_dtype(dtype)
    dims, fans, B, Q, nw = (16, 8), (5, 3), 17, 5, 1.0
    store, ref_model, eng_model = _twins(prob, dims, fans, Q, nw, dtype)
    full = _seed_batches(prob[0], B, 3, seed=2)
    eng = gs.engine.FusedUnsupMeanTrainStep(eng_model, store, full[0], capture="cmdlist")
    R = 2 * B + Q
    ltol, gtol = (3e-2, 0.1) if dtype == "bf16" else (FP32_BOUND, FP32_BOUND)
    for seeds, b in ((full[0], B), (full[1][:B - 1], B - 1), (full[2][:2], 2), (full[0], B)):
        ref_model.load_state_dict(eng_model.state_dict())
        l_eng = float(eng(seeds))
        padded = torch.cat([seeds, seeds[:1].expand(B - b)])
        all_ids, pair_w = ref_model.build_batch(padded)
        assert torch.equal(eng.ids_set[0][:R], all_ids) and torch.equal(eng.pair_w, pair_w)
        for p in ref_model.parameters():
            p.grad = None
        E = ref_model._encode(all_ids, store, train=True)
        loss, _ = uref.masked_loss(E, B, Q, pair_w, nw, b)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(ref_model.parameters(), 5)
        with torch.no_grad():
            over_B = float(uref.masked_loss(E, B, Q, pair_w, nw, b)[0]) * b / B        # the 1/B normalisation
        l_ref = float(loss)
        print("short %s b=%d: loss %.6f vs %.6f (1/B: %.6f)" % (dtype, b, l_eng, l_ref, over_B))
        assert abs(l_eng - l_ref) <= ltol * max(1.0, abs(l_ref)), (b, l_eng, l_ref)
        if b == 2:
            assert abs(l_ref - over_B) > 10 * ltol * max(1.0, abs(l_ref))
            assert abs(l_eng - over_B) > 5 * ltol * max(1.0, abs(l_ref))
        for (k, a), (_, r) in zip(eng_model.named_parameters(), ref_model.named_parameters()):
            close_fro(a.grad.cpu().numpy(), r.grad.cpu().numpy(), ("grad", b, k), gtol)
    with pytest.raises(ValueError):
        eng(full[0][:1])
    with pytest.raises(ValueError):
        eng(torch.cat([full[0], full[1]]))
    eng_model.train_sampler.csr(DEV).check()


# ---- 5. handover ---------------------------------------------------------------------------------------------------
def test_engine_hands_over_to_the_module_path(prob):
    adj, feats = prob
    B, Q = 32, 20
    store = gs.FeatureStore.from_array(feats, torch.device(DEV), dtype="bf16")
    model = uref.make_model(gs, adj, feats.shape[1], (16, 8), (5, 3), Q, 1.0, DEV)
    batches = _seed_batches(adj, B, 4, seed=5)
    eng = gs.engine.FusedUnsupMeanTrainStep(model, store, batches[0], capture="cmdlist")
    losses = [float(eng(s)) for s in batches[:3]]
    torch.cuda.synchronize()
    assert np.isfinite(losses).all() and eng.holds_parameters()
    assert not any(k.startswith("fc.") for k in model.state_dict())
    res = model.evaluate(batches[3], store)
    assert np.isfinite(res["loss"]) and 0 < res["mrr"] <= 1
    emb = gs.embeddings(model, store)
    assert emb.shape == (adj.shape[0], 16)
    live = emb.norm(dim=1) > 0.5                            # (rows without edges and features embed to zero)
    assert int(live.sum()) >= adj.shape[0] - 1
    assert torch.allclose(emb[live].norm(dim=1), torch.ones(int(live.sum()), device=DEV), atol=1e-4)
    sd = model.optimizer_state_dict()
    assert int(sd["state"][0]["step"]) == 3 and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    m3, v3 = eng.flat_m.clone(), eng.flat_v.clone()
    assert float(m3.abs().max()) > 0
    l4 = float(model.train_step(batches[3], store))
    torch.cuda.synchronize()
    opt = model.optimizer
    assert np.isfinite(l4) and isinstance(opt, gs.optim.FlatAdam) and not eng.holds_parameters()
    assert int(opt.step_count.item()) == 4 and model._batch_calls[1] == 4
    wd_g = opt.flat_g + 1e-4 * opt.flat_p                   # m4 = 0.9 m3 + 0.1 g4 (weight decay folded into g)
    assert torch.allclose(opt.flat_m, 0.9 * m3 + 0.1 * wd_g, rtol=0, atol=2e-4 * float(1 + wd_g.abs().max()))
    assert float((opt.flat_v - 0.999 * v3).min()) >= -1e-12
    for s in (model.train_sampler, model.val_sampler):
        for csr in s._dev.values():
            csr.check()
    import pickle
    pickle.dumps(model.state_dict())


# ---- 6. command line -----------------------------------------------------------------------------------------------
def test_train_main_unsupervised_fused(capsys, tmp_path):
    p = unsup_ref.model_problem()
    problem = gs.NodeProblem.from_arrays("classification", 3, p["adj"], p["adj"], p["feats"], p["folds"], p["targets"],
                                         cuda=True)
    path = str(tmp_path / "emb.npy")
    train = importlib.import_module("pytorch-graphsage_amd.train")
    base = ["--problem-path", "<memory>", "--epochs", "2", "--batch-size", "64", "--sampler-class",
            "sparse_uniform_neighbor_sampler", "--n-train-samples", "5,3", "--n-val-samples", "5,3", "--output-dims",
            "32,32", "--unsupervised", "--walk-len", "5", "--n-negatives", "20", "--save-embeddings", path]
    train.main(base + ["--engine", "fused", "--rng", "philox"], problem=problem)
    cap = capsys.readouterr()
    assert "FusedUnsupMeanTrainStep" in cap.err and "module path" not in cap.err
    lines = [json.loads(l) for l in cap.out.splitlines() if l.startswith("{")]
    batches = [l for l in lines if "epoch_progress" in l]
    epochs = [l for l in lines if "mrr" in l and "epoch_progress" not in l]
    assert len(batches) == 2 * (140 // 64 + 1) and all(np.isfinite(l["loss"]) for l in batches)
    assert len(epochs) == 3 and all(0 < l["mrr"] <= 1 for l in epochs)
    emb = np.load(path)
    assert emb.shape == (200, 64) and np.allclose(np.linalg.norm(emb[1:], axis=1), 1.0, atol=1e-4)
    with pytest.raises(SystemExit, match="philox"):
        train.main(base + ["--engine", "fused"], problem=problem)
    with pytest.raises(SystemExit, match="aggregators other than mean"):
        train.main(base + ["--engine", "fused", "--rng", "philox", "--aggregator-class", "max_pool"], problem=problem)
    capsys.readouterr()
    train.main(base + ["--engine", "auto"], problem=problem)
    assert "unsupervised model: module path" in capsys.readouterr().err
