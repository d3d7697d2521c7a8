"""-m gpu: FusedTemporalMeanTrainStep.  Its frontier and the frontier's times against the serial restatement of
tests/temporal_ref.py and against the module path's sampler calls (torch.equal), with explicit query times and with the
node_time default; the step against GSSupervised.train_step under the same sampler and times at the bounds
tests/test_gpu_distinct.py applies (same samples, same kernels behind the sampler); queue mode against per-call steps
bit for bit under a time queue with a different time per seed; the evaluation engine on the validation adjacency; the
refusals; and train.py --engine fused."""
import importlib
import json
import math

import numpy as np
import pytest
import torch

import temporal_engine_ref as ter
import temporal_ref as tr
from conftest import pkg
from util import close, close_fro

pytestmark = pytest.mark.gpu
gs = pkg()
ops, nat = gs.ops, gs._native
DEV = "cuda"
LOSS = gs.ProblemLosses.classification
CLS = gs.engine.FusedTemporalMeanTrainStep
TRAIN_SEED, VAL_SEED = ter.TRAIN_SEED, ter.VAL_SEED


@pytest.fixture(autouse=True)
def _setup():
    ops.set_compute_dtype("bf16")
    ops.warmup(torch.device(DEV))
    yield
    ops.set_compute_dtype("bf16")


def _model(p, dims, fans, strategy="uniform", inherit="seed", val=None):
    return ter.model(p, dims, fans, strategy=strategy, inherit=inherit, val=val).to(DEV)


def _store(p, dtype="bf16"):
    return gs.FeatureStore.from_array(p["feats"], torch.device(DEV), dtype=dtype)


def _batches(p, rng, B, n):
    """-> (ids [n, B], targets [n, B, 1], times [n, B]: a different query time per seed, on either side of T_SNAP)"""
    ids = rng.randint(1, p["n"] + 1, size=(n, B))
    tg = p["targets"][ids.reshape(-1)].reshape(n, B, 1)
    tm = rng.randint(-60, tr.T_SNAP + 60, size=(n, B)).astype(np.int64)
    return torch.from_numpy(ids).to(DEV), torch.from_numpy(tg).to(DEV), torch.from_numpy(tm).to(DEV)


def _ref(p, ids, times, fans, seed, call0, strategy, inherit, val=False):
    pre = "val_" if val else ""
    return ter.frontier(p[pre + "indptr"], p[pre + "data"], p[pre + "etime"], p["n"] + 1, ids, times, fans, seed, call0,
                        strategy, inherit)


def _eq(got, ref):
    return torch.equal(got.cpu(), torch.from_numpy(ref))


@pytest.mark.parametrize("strategy,inherit", [("uniform", "seed"), ("recent", "edge")])
@pytest.mark.parametrize("capture", [False, "cmdlist"])
def test_engine_frontier_equals_the_restatement_and_the_module_path(capture, strategy, inherit):
    p = ter.problem()
    dims, fans, B, L = (16, 8), (5, 3), 33, 2
    store = _store(p)
    ids, tg, tm = _batches(p, np.random.RandomState(5), B, 3)
    for explicit in (True, False):
        model, twin = _model(p, dims, fans, strategy, inherit), _model(p, dims, fans, strategy, inherit)
        eng = CLS(model, store, LOSS, ids[0], tg[0], capture=capture, keep_times=True,
                  example_times=tm[0] if explicit else None)
        for t in range(3):
            eng(ids[t], tg[t], times=tm[t] if explicit else None)
            want = tm[t].cpu().numpy() if explicit else p["node_time"][ids[t].cpu().numpy()]
            ref, ref_t, err = _ref(p, ids[t].cpu().numpy(), want, fans, TRAIN_SEED, L * t, strategy, inherit)
            assert err == 0 and _eq(eng.ids_set[0], ref) and _eq(eng.times_set[0], ref_t), ("step", t, explicit)
            cur, cur_t = ids[t], tm[t] if explicit else None
            hops, hops_t = [cur], [torch.from_numpy(want).to(DEV)]
            for fn in twin.train_sample_fns:                    # what GSSupervised._encode asks its sampler for
                cur, cur_t = fn(ids=cur, times=cur_t)
                hops.append(cur.view(-1))
                hops_t.append(cur_t.view(-1))
            assert torch.equal(eng.ids_set[0], torch.cat(hops)) and torch.equal(eng.times_set[0], torch.cat(hops_t)), \
                ("module path, step", t, explicit)
        assert int(eng.counter.item()) == 3 * L and twin.train_sampler.calls == 3 * L
        eng.csr.check()


@pytest.mark.parametrize("dims,fans,B", [((128, 128), (25, 10), 16), ((16, 8), (5, 3), 33), ((32, 16, 8), (4, 3, 2), 20)])
@pytest.mark.parametrize("capture", [False, "cmdlist"])
def test_step_matches_the_module_path(dims, fans, B, capture):
    """tests/test_gpu_distinct.py::test_step_matches_the_module_path over the temporal sampler, its comparisons and
    bounds as they are: the two paths draw the same frontier, and every kernel behind the sampler is the uniform
    engine's.  The module path is called with the same times."""
    p = ter.problem()
    store = _store(p)
    ref_model, eng_model = _model(p, dims, fans), _model(p, dims, fans)
    eng_model.load_state_dict(ref_model.state_dict())
    ref_model.optimizer = torch.optim.Adam(ref_model.parameters(), lr=0.01, weight_decay=1e-4)
    ids, tg, tm = _batches(p, np.random.RandomState(6), B, 3)
    eng = CLS(eng_model, store, LOSS, ids[0], tg[0], capture=capture, example_times=tm[0])
    assert eng.fused_tail == (dims == (128, 128))               # the first shape takes the fused seed level
    for step in range(3):
        ref_model.load_state_dict(eng_model.state_dict())       # every step from identical weights
        p_ref = ref_model.train_step(ids=ids[step], feats=store, targets=tg[step], loss_fn=LOSS, times=tm[step])
        p_ref = p_ref.detach().float().cpu().numpy()
        p_eng = eng(ids[step], tg[step], times=tm[step]).detach().float().cpu().numpy()
        close(p_eng, p_ref, ("preds", step), 3e-2, 3e-2)
        for (k, a), (_, b) in zip(eng_model.named_parameters(), ref_model.named_parameters()):
            close_fro(a.grad.cpu().numpy(), b.grad.cpu().numpy(), ("grad", step, k), 0.1)
            if step == 0:
                close_fro(a.detach().cpu().numpy(), b.detach().cpu().numpy(), ("weight", k), 0.05)
    eng.csr.check()


@pytest.mark.parametrize("B,fans", [(24, (5, 3)), (40, (25, 10))])
@pytest.mark.parametrize("capture", [False, "cmdlist"])
def test_queue_mode_equals_per_call_steps(B, fans, capture):
    """7 steps across a 3-batch queue, batch 1 one seed short, a different query time per seed (a queue that read batch
    i's times for batch i + 2's seeds would differ): preds and weights bit for bit"""
    p = ter.problem()
    store = _store(p)
    ids, tg, tm = _batches(p, np.random.RandomState(7), B, 3)
    live = [B, B - 1, B]
    ids[1, B - 1], tg[1, B - 1], tm[1, B - 1] = ids[1, 0], tg[1, 0], tm[1, 0]     # the padding the per-call engine adds
    res = []
    for queued in (False, True):
        eng = CLS(_model(p, (128, 128), fans, "uniform", "edge"), store, LOSS, ids[0], tg[0], capture=capture,
                  example_times=tm[0], keep_times=True)
        preds, fronts = [], []
        if queued:
            eng.load_epoch(ids, tg, n_valid=live, times_epoch=tm)
            for k in range(7):
                preds.append(eng.step_queue().clone())
            assert eng.P == 2
            with pytest.raises(ValueError, match="sel_epoch"):
                eng.load_epoch(ids, tg, sel_epoch=torch.zeros(3, 8, dtype=torch.int32), times_epoch=tm)
        else:
            for k in range(7):
                nv = live[k % 3]
                preds.append(eng(ids[k % 3, :nv], tg[k % 3, :nv], times=tm[k % 3, :nv]).clone())
        res.append((torch.stack(preds), eng.flat_p.clone()))
        eng.csr.check()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_queue_mode_defaults_to_node_time():
    """times_epoch=None: the frontiers the queue samples ahead are the restatement's under node_time[ids], with their
    kept times.  When step t returns, the ring holds the frontiers of steps t + 1 and t + 2 (the latter sampled ahead of
    the counters into the buffer step t has just left)."""
    p = ter.problem()
    store = _store(p)
    B, fans, L = 24, (5, 3), 2
    ids, tg, _ = _batches(p, np.random.RandomState(11), B, 3)
    eng = CLS(_model(p, (16, 8), fans, "uniform", "edge"), store, LOSS, ids[0], tg[0], keep_times=True)
    eng.load_epoch(ids, tg)
    for t in range(4):
        eng.step_queue()
        torch.cuda.synchronize()
        assert eng.P == 2
        for u in (t + 1, t + 2):
            seeds = ids[u % 3].cpu().numpy()
            ref, ref_t, err = _ref(p, seeds, p["node_time"][seeds], fans, TRAIN_SEED, L * u, "uniform", "edge")
            assert err == 0 and _eq(eng.ids_q[u % 2], ref) and _eq(eng.times_q[u % 2], ref_t), ("step", t, "holds", u)
    eng.csr.check()


def test_two_engines_are_bit_equal():
    p = ter.problem()
    store = _store(p)
    ids, tg, tm = _batches(p, np.random.RandomState(8), 20, 4)
    outs = []
    for _ in range(2):
        eng = CLS(_model(p, (32, 16), (6, 4), "recent", "edge"), store, LOSS, ids[0], tg[0], example_times=tm[0])
        preds = torch.stack([eng(ids[t], tg[t], times=tm[t]).clone() for t in range(4)])
        outs.append((preds, eng.flat_p.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_eval_only_walks_the_validation_adjacency():
    """the validation sampler's adjacency, seed, strategy and rule (they differ from the train sampler's here)"""
    p = ter.problem()
    store = _store(p)
    dims, fans, L = (16, 8), (5, 3), 2
    nodes = np.arange(1, 41)
    chunks = np.array_split(np.arange(nodes.shape[0]), nodes.shape[0] // 16 + 1)
    B, live = max(len(c) for c in chunks), [len(c) for c in chunks]
    assert B <= 16 and len(chunks) == 3 and min(live) < B
    pad = lambda a: np.stack([np.concatenate([a[c], np.repeat(a[c[:1]], B - len(c))]) for c in chunks])    # noqa: E731
    mids = pad(nodes)
    mtm = pad(np.random.RandomState(13).randint(-60, tr.T_SNAP + 60, size=nodes.shape[0]).astype(np.int64))
    ids, tm = torch.from_numpy(mids).to(DEV), torch.from_numpy(mtm).to(DEV)
    tg = torch.zeros(B, 1, dtype=torch.int64, device=DEV)
    val = ("recent", "edge")
    model = _model(p, dims, fans, val=val)
    whole = CLS(model, store, LOSS, ids[0], tg, eval_only=True, example_times=tm[0]).evaluate_fold(ids, live, times=tm)
    assert tuple(whole.shape) == (sum(live), p["C"])
    # batch by batch on a second engine: the frontier of batch b, and the same predictions
    eng = CLS(model, store, LOSS, ids[0], tg, eval_only=True, keep_times=True)
    twin = _model(p, dims, fans, val=val)
    twin.load_state_dict(model.state_dict())
    row = 0
    for b in range(len(chunks)):
        got = eng.evaluate_fold(ids[b:b + 1], live[b:b + 1], times=tm[b:b + 1])
        ref, ref_t, err = _ref(p, mids[b], mtm[b], fans, VAL_SEED, L * b, *val, val=True)
        assert err == 0 and _eq(eng.ids_set[0], ref) and _eq(eng.times_set[0], ref_t), ("batch", b)
        assert torch.equal(got, whole[row:row + live[b]])
        with torch.no_grad():
            want = twin(ids[b, :live[b]], store, train=False, times=tm[b, :live[b]])
        close(got.cpu().numpy(), want.float().cpu().numpy(), ("preds", b), 3e-2, 3e-2)
        row += live[b]
    # times=None: the validation sampler's node_time
    got = eng.evaluate_fold(ids[:1], live[:1])
    ref, ref_t, err = _ref(p, mids[0], p["node_time"][mids[0]], fans, VAL_SEED, L * 3, *val, val=True)
    assert err == 0 and _eq(eng.ids_set[0], ref) and _eq(eng.times_set[0], ref_t)
    eng.csr.check()


def test_constructor_refuses_with_the_sentence():
    p = ter.problem()
    store = _store(p)
    ids, tg, tm = _batches(p, np.random.RandomState(9), 8, 1)
    old = gs.nn_modules.SparseUniformNeighborSampler.rng_default
    gs.nn_modules.SparseUniformNeighborSampler.rng_default = "philox"
    try:
        uniform = tr.model(p, (16, 8), (5, 3), sampler="sparse_uniform_neighbor_sampler", adj=p["adj"]).to(DEV)
    finally:
        gs.nn_modules.SparseUniformNeighborSampler.rng_default = old
    why = CLS.why_not(uniform, store)
    assert "SparseUniformNeighborSampler" in why
    with pytest.raises(ValueError) as e:
        CLS(uniform, store, LOSS, ids[0], tg[0])
    assert why in str(e.value)
    model = _model(p, (16, 8), (5, 3))
    assert CLS.why_not(model, store) is None
    why = CLS.why_not(model, store, pipelined=True)
    assert "pipelined=True" in why
    with pytest.raises(ValueError) as e:
        CLS(model, store, LOSS, ids[0], tg[0], pipelined=True)
    assert why in str(e.value)
    fp8 = store.quantize()
    why = CLS.why_not(model, fp8)
    assert "FP8" in why
    with pytest.raises(ValueError) as e:
        CLS(model, fp8, LOSS, ids[0], tg[0])
    assert why in str(e.value)
    # the registry answers as without the class; the uniform engine does not take the model
    assert "SparseTemporalNeighborSampler" in gs.engine.why_no_fused_engine(model, store)["FusedMeanTrainStep"]
    assert gs.engine.fused_engine_for(model, store) is None


def test_train_cli_engine_fused(capsys):
    train = importlib.import_module("pytorch-graphsage_amd.train")
    p = tr.problem()
    folds = np.array(["train"] * 40 + ["val"] * 11 + ["test"] * 10)
    problem = gs.NodeProblem.from_arrays("classification", p["C"], p["adj"], p["adj"], p["feats"], folds, p["targets"],
                                         cuda=True, adj_time=p["time"], train_adj_time=p["time"],
                                         node_time=np.full(p["n"] + 1, tr.T_SNAP))
    try:
        train.main(["--problem-path", "<memory>", "--epochs", "2", "--batch-size", "16", "--n-train-samples", "3,2",
                    "--n-val-samples", "3,2", "--output-dims", "8,8", "--show-test", "--rng", "philox", "--sampler-class",
                    "sparse_temporal_neighbor_sampler", "--temporal-inherit", "edge", "--engine", "fused",
                    "--log-interval", "1"], problem=problem)
        cap = capsys.readouterr()
        assert "train_step runs on FusedTemporalMeanTrainStep" in cap.err
        assert "using the module path" not in cap.err and "on the module path" not in cap.err     # training, evaluation
        assert "falls back to the module path" not in cap.err
        lines = [json.loads(l) for l in cap.out.splitlines() if l.startswith("{")]
        steps = [l for l in lines if "train_metric" in l and l.get("epoch_progress") is not None]
        assert len(steps) >= 3 and {l["epoch"] for l in steps} == {0, 1}
        assert all(math.isfinite(v) for l in steps for v in l["train_metric"].values())
        assert lines[-1]["test_f1"] is not None
    finally:
        gs.nn_modules.SparseUniformNeighborSampler.rng_default = "compat"
        gs.nn_modules.SparseTemporalNeighborSampler.strategy_default = "uniform"
        gs.nn_modules.SparseTemporalNeighborSampler.inherit_default = "seed"
        ops.set_compute_dtype("bf16")
