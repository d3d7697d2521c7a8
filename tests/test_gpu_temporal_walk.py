"""-m gpu: temporal walks (include/gsage.h, "Temporal walks").  gsage_unsup_batch_temporal against the restatement of
tests/temporal_walk_ref.py bit for bit over the host tests' grid (one wave holds rows of 3, 300, 4097 and 0 edges, walks
of different lengths, walks that end early beside walks of 16 steps; B is mostly no multiple of 16), ids outside the
graph, the launch in a command list, GSUnsupervised(temporal_walks=True) against host mode, and
FusedUnsupTemporalMeanTrainStep against the module path."""
import importlib
import json

import numpy as np
import pytest
import torch

import temporal_ref as tr
import temporal_walk_ref as twr
from conftest import pkg
from test_gpu_unsup import HEAD_BOUND                      # the bound of that file's device-against-host-mode comparison

pytestmark = pytest.mark.gpu
gs = pkg()
ops, nat = gs.ops, gs._native
DEV = "cuda"
INT64_MAX = tr.INT64_MAX
FP32_BOUND = 2e-4                                          # tests/test_gpu_unsup_engine.py: engine against module path


@pytest.fixture(autouse=True)
def _setup():
    ops.set_compute_dtype("bf16")
    ops.warmup(torch.device(DEV))
    old = gs.nn_modules.SparseUniformNeighborSampler.rng_default
    gs.nn_modules.SparseUniformNeighborSampler.rng_default = "philox"
    yield
    gs.nn_modules.SparseUniformNeighborSampler.rng_default = old
    ops.set_compute_dtype("bf16")


def _dev(a):
    return torch.from_numpy(np.asarray(a, dtype=np.int64)).to(DEV)


_ADJ = {}


def _graph():
    """(the test graph, its device CSR, the negatives' table on the device), built once"""
    if not _ADJ:
        g = tr.graph()
        _ADJ["g"] = (g, g.csr(DEV), twr.table(DEV))
    return _ADJ["g"]


def _philox(**kw):
    ph = {"seed": twr.SEED, "call_base": twr.CALL_BASE, "g0": twr.G0,
          "call_ctr": torch.tensor([twr.CALL_CTR], dtype=torch.int64, device=DEV)}
    ph.update(kw)
    return ph


def _same(got, ref, what=""):
    for a, r, name in zip(got, ref[:3], ("ids", "pair_w", "times")):
        assert np.array_equal(a.cpu().numpy(), r), (what, name)


# ---- the kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", twr.RULES)
@pytest.mark.parametrize("M", twr.MS)
def test_kernel_equals_the_restatement(M, rule):
    g, adj, cdf = _graph()
    seeds, times = tr.parents(M)
    d_seeds, d_times = _dev(seeds), _dev(times)
    for walk_len in twr.WALK_LENS:
        for Q in twr.QS:
            before = nat.launch_count()
            got = ops.unsup_batch_temporal(adj, d_seeds, d_times, walk_len, Q, cdf, _philox(), inherit=rule)
            assert nat.launch_count() - before == 1
            assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[2].dtype == torch.int64
            _same(got, twr.reference(M, walk_len, Q, rule), (walk_len, Q))
            nv = twr.n_valid_of(M, walk_len, Q, rule)
            word = torch.tensor([nv], dtype=torch.int32, device=DEV)
            _same(ops.unsup_batch_temporal(adj, d_seeds, d_times, walk_len, Q, cdf, _philox(), inherit=rule, n_valid=word),
                  twr.reference(M, walk_len, Q, rule, nv), (walk_len, Q, nv))
    assert int(adj.err_flag.item()) == 0


@pytest.mark.parametrize("rule", twr.RULES)
def test_every_live_count_and_two_launches(rule):
    g, adj, cdf = _graph()
    M, Q = 17, 20
    seeds, times = tr.parents(M)
    for nv in (None, 1, 2, M - 1, M, M + 5, 0, -3):
        got = ops.unsup_batch_temporal(adj, _dev(seeds), _dev(times), 5, Q, cdf, _philox(), inherit=rule, n_valid=nv)
        _same(got, twr.reference(M, 5, Q, rule, nv), nv)
    a = ops.unsup_batch_temporal(adj, _dev(seeds), _dev(times), 16, 64, cdf, _philox(), inherit=rule)
    b = ops.unsup_batch_temporal(adj, _dev(seeds), _dev(times), 16, 64, cdf, _philox(), inherit=rule)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert int(adj.err_flag.item()) == 0


@pytest.mark.parametrize("rule", twr.RULES)
def test_ids_outside_the_graph(rule):
    g, adj, cdf = _graph()
    B, Q = 37, 20
    seeds, times = tr.parents(B)
    bad = seeds.copy()
    bad[[1, 18, 35]] = [g.n, -1, 1 << 40]                   # between good seeds of the same waves
    got = ops.unsup_batch_temporal(adj, _dev(bad), _dev(times), 16, Q, cdf, _philox(), inherit=rule)
    ref = twr.build_batch(g.rowptr, g.col, g.etime, g.n, bad, times, 16, Q, twr.degree_cdf(), twr.SEED,
                          twr.CALL_BASE + twr.CALL_CTR, twr.G0, rule, None, twr._COUNTS)
    assert ref[3] == 1
    _same(got, ref)
    ids, pw, ot = [t.cpu().numpy() for t in got]
    for i in (1, 18, 35):
        assert ids[i] == 0 and ids[B + i] == 0 and pw[i] == 0.0 and ot[i] == ot[B + i] == times[i]
    good = np.setdiff1d(np.arange(B), [1, 18, 35])
    whole = twr.reference(B, 16, Q, rule)                    # the seeds around them: what the clean batch gives
    assert np.array_equal(ids[good], whole[0][good]) and np.array_equal(ids[B + good], whole[0][B + good])
    assert np.array_equal(pw[good], whole[1][good])
    with pytest.raises(IndexError):
        adj.check()
    assert int(adj.err_flag.item()) == 0                     # check() cleared it
    # a node the walk REACHES outside the graph: 0, and the flag
    rowptr = np.asarray([0, 2, 3, 3], dtype=np.int64)
    col = np.asarray([1, 99, 2], dtype=np.int32)
    etime = np.asarray([0, 1, 0], dtype=np.int64)
    small = gs.DeviceCSR(torch.from_numpy(rowptr).to(DEV), torch.from_numpy(col).to(DEV), 3, 2,
                         etime=torch.from_numpy(etime).to(DEV))
    s = np.asarray([0] * 20 + [1, 2], dtype=np.int64)
    t = np.full(22, 5, dtype=np.int64)
    tab = np.asarray([1.0, 2.0, 2.0])
    dtab = torch.from_numpy(tab).to(DEV)
    dtab._gsage_total = 2.0
    got = ops.unsup_batch_temporal(small, _dev(s), _dev(t), 4, 3, dtab, {"seed": 9}, inherit=rule)
    ref = twr.build_batch(rowptr, col, etime, 3, s, t, 4, 3, tab, 9, 0, 0, rule)
    assert ref[3] == 1 and int(small.err_flag.item()) == 1 and 0 < int((ref[0][22:42] == 0).sum()) < 20
    small.err_flag.zero_()
    _same(got, ref)


def test_einval_returns_without_a_launch():
    g, adj, cdf = _graph()
    L = nat.lib()
    seeds, times = _dev([1, 2, 3]), _dev([5, 5, 5])
    ids, ot = torch.zeros(9, dtype=torch.int64, device=DEV), torch.zeros(9, dtype=torch.int64, device=DEV)
    pw = torch.zeros(3, device=DEV)
    torch.cuda.synchronize()

    def call(B=3, walk_len=5, Q=3, total=cdf._gsage_total, inherit=0, etime=adj.etime.data_ptr(), times=times.data_ptr()):
        return L.gsage_unsup_batch_temporal(adj.rowptr.data_ptr(), adj.col.data_ptr(), etime, adj.n_rows, seeds.data_ptr(),
                                            times, B, walk_len, Q, cdf.data_ptr(), total, 7, None, 0, 0, inherit, None,
                                            ids.data_ptr(), ot.data_ptr(), pw.data_ptr(), None, None)
    before = nat.launch_count()
    for kw in ({"B": 0}, {"B": 1 << 31}, {"Q": 0}, {"walk_len": 0}, {"walk_len": 17}, {"inherit": 2}, {"total": 0.0},
               {"total": float("nan")}, {"etime": None}, {"times": None}):
        assert call(**kw) == -1, kw
    assert nat.launch_count() == before and not ids.any().item()
    assert call() == 0 and nat.launch_count() == before + 1
    torch.cuda.synchronize()
    assert ids[:3].cpu().tolist() == [1, 2, 3] and ot.cpu().tolist() == [5] * 9


def test_the_recorded_launch_replays_under_a_device_call_counter():
    """recorded once with a device counter, replayed three times with the counter advanced between: three separate calls"""
    g, adj, cdf = _graph()
    B, Q, wl, c = 84, 20, 16, 4
    seeds, times = tr.parents(B)
    d_seeds, d_times = _dev(seeds), _dev(times)
    ctr = torch.tensor([c], dtype=torch.int64, device=DEV)
    live = torch.tensor([B - 3], dtype=torch.int32, device=DEV)
    ids = torch.zeros(2 * B + Q, dtype=torch.int64, device=DEV)
    ot, pw = torch.zeros_like(ids), torch.zeros(B, device=DEV)
    with nat.CommandList.record() as cl:
        nat.check(nat.lib().gsage_unsup_batch_temporal(
            adj.rowptr.data_ptr(), adj.col.data_ptr(), adj.etime.data_ptr(), adj.n_rows, d_seeds.data_ptr(),
            d_times.data_ptr(), B, wl, Q, cdf.data_ptr(), cdf._gsage_total, twr.SEED, ctr.data_ptr(), 2, twr.G0, 1,
            live.data_ptr(), ids.data_ptr(), ot.data_ptr(), pw.data_ptr(), adj.err_flag.data_ptr(), None),
            "unsup_batch_temporal")
        nat.check(nat.lib().gsage_counter_add(ctr.data_ptr(), 1, None), "counter_add")
    assert len(cl) == 2 and not ids.any().item()              # recorded, not launched
    for k in range(3):
        cl.replay(ops._stream())
        sep = ops.unsup_batch_temporal(adj, d_seeds, d_times, wl, Q, cdf, {"seed": twr.SEED, "call_base": 2 + c + k,
                                                                          "g0": twr.G0}, inherit="edge", n_valid=B - 3)
        assert torch.equal(ids, sep[0]) and torch.equal(pw, sep[1]) and torch.equal(ot, sep[2]), k
        if k == 0:
            first = ids.clone()
    assert int(ctr.item()) == c + 3 and not torch.equal(first[B:2 * B], ids[B:2 * B])
    adj.check()


# ---- the model -------------------------------------------------------------------------------------------------------
IDS = [5, 9, 32, 1, 60, 17, 44, 23, 2]
TIMES = [tr.T_SNAP, tr.T_SNAP + 20, 0, -60, INT64_MAX, tr.T_SNAP, 500, tr.T_SNAP + 1, 999]


@pytest.mark.parametrize("rule", twr.RULES)
def test_model_on_the_device_against_host_mode(rule):
    """train_step and evaluate of GSUnsupervised(temporal_walks=True), device against host mode, fp32 compute over an fp32
    store, from identical weights: the batches and frontiers are equal bit for bit (integers), the losses within the
    bound tests/test_gpu_unsup.py holds the device's skip-gram loss to against host mode (HEAD_BOUND, relative)."""
    ops.set_compute_dtype("fp32")
    p = tr.problem()
    dev_model, host_model = twr.model(p, inherit=rule, temporal_walks=True).to(DEV), twr.model(p, inherit=rule,
                                                                                               temporal_walks=True)
    for m in (dev_model, host_model):
        m.train_sampler.seed = m.val_sampler.seed = 77
    ids, times = torch.tensor(IDS, dtype=torch.int64), torch.tensor(TIMES, dtype=torch.int64)
    a, b = dev_model.build_batch(ids.to(DEV), times=times.to(DEV)), host_model.build_batch(ids, times=times)
    assert all(torch.equal(x.cpu(), y) for x, y in zip(a, b))
    store = gs.FeatureStore.from_array(p["feats"], torch.device(DEV), dtype="fp32")
    feats = torch.from_numpy(p["feats"])
    l_dev = float(dev_model.train_step(ids.to(DEV), store, times=times.to(DEV)))
    l_host = float(host_model.train_step(ids, feats, times=times))
    print("train_step %s: device %.8f host %.8f (%.3g)" % (rule, l_dev, l_host, abs(l_dev - l_host) / abs(l_host)))
    e_dev = dev_model.evaluate(ids.to(DEV), store, times=times.to(DEV))
    e_host = host_model.evaluate(ids, feats, times=times)
    print("evaluate %s: device %r host %r" % (rule, e_dev, e_host))
    assert abs(l_dev - l_host) <= HEAD_BOUND * abs(l_host)
    assert abs(e_dev["loss"] - e_host["loss"]) <= HEAD_BOUND * abs(e_host["loss"])
    assert abs(e_dev["mrr"] - e_host["mrr"]) <= HEAD_BOUND * abs(e_host["mrr"])
    assert dev_model._batch_calls == host_model._batch_calls == [1, 2]
    for s in (dev_model.train_sampler, dev_model.val_sampler):
        s.csr(DEV).check()


# ---- the engine ------------------------------------------------------------------------------------------------------
def _twins(rule, dtype, dims=(16, 8), fans=(3, 2), Q=5, strategy="uniform"):
    p = tr.problem()
    store = gs.FeatureStore.from_array(p["feats"], torch.device(DEV), dtype=dtype)
    mk = lambda: twr.model(p, dims=dims, fans=fans, inherit=rule, strategy=strategy, n_negatives=Q,       # noqa: E731
                           temporal_walks=True, lr_init=0.01, weight_decay=1e-4).to(DEV)
    ref_model, eng_model = mk(), mk()
    for m in (ref_model, eng_model):
        m.train_sampler.seed = 77
    return p, store, ref_model, eng_model


def _batches(B, n, seed=1):
    rng = np.random.RandomState(seed)
    pool = np.asarray([tr.T_SNAP, tr.T_SNAP + 1, tr.T_SNAP + 30, 0, 400, -60, INT64_MAX], dtype=np.int64)
    return [(torch.from_numpy(rng.randint(0, 61, size=B)).to(DEV), torch.from_numpy(pool[rng.randint(0, 7, size=B)]).to(DEV))
            for _ in range(n)]


def _module_frontier(model, seeds, times, Bs):
    """[ids of every hop], [times of every hop], pair_w of the module path for a batch padded to Bs seeds with its first
    seed (the live count = len(seeds) given to the builder, as the engine gives it)"""
    b = int(seeds.shape[0])
    ps, pt = torch.cat([seeds, seeds[:1].expand(Bs - b)]), torch.cat([times, times[:1].expand(Bs - b)])
    csr, cdf = model._walk_graph(True, DEV)
    ph = {"seed": model.train_sampler.seed, "call_base": model._batch_calls[1], "g0": 0}
    model._batch_calls[1] += 1
    ids, pw, tm = ops.unsup_batch_temporal(csr, ps, pt, model.walk_len, model.n_negatives, cdf, ph,
                                           inherit=model.train_sampler.inherit, n_valid=b)
    if b == Bs:                                              # a full batch: this IS build_batch
        model._batch_calls[1] -= 1
        again = model.build_batch(seeds, times=times)
        assert all(torch.equal(x, y) for x, y in zip(again, (ids, pw, tm)))
    all_ids, all_times = [ids], [tm]
    for fn in model.train_sample_fns:
        ids, tm = fn(ids=ids, times=tm)
        all_ids.append(ids)
        all_times.append(tm)
    return torch.cat(all_ids), torch.cat(all_times), pw


@pytest.mark.parametrize("capture", [False, "cmdlist"])
@pytest.mark.parametrize("rule,strategy", [("seed", "uniform"), ("edge", "uniform"), ("edge", "recent")])
def test_engine_builds_the_module_paths_batches_and_frontiers(rule, strategy, capture):
    Bs, Q = 17, 5
    p, store, ref_model, eng_model = _twins(rule, "bf16", strategy=strategy)
    batches = _batches(Bs, 4)
    cls = gs.engine.FusedUnsupTemporalMeanTrainStep
    assert cls.supports(eng_model, store) and cls not in gs.engine.ENGINES
    eng = cls(eng_model, store, batches[0][0], capture=capture, example_times=batches[0][1], keep_times=True)
    R = 2 * Bs + Q
    assert eng.B == R and eng.capture_mode == (capture or None)
    torch.cuda.synchronize()
    assert eng_model._batch_calls == [0, 0] and int(eng.batch_ctr.item()) == 0 and int(eng.counter.item()) == 0
    steps = [batches[0], (batches[1][0][:Bs - 1], batches[1][1][:Bs - 1]), (batches[2][0][:2], batches[2][1][:2]),
             batches[3]]
    for t, (seeds, times) in enumerate(steps):
        loss = float(eng(seeds, times))
        assert np.isfinite(loss), t
        ids, tm, pw = _module_frontier(ref_model, seeds, times, Bs)
        assert torch.equal(eng.ids_set[0][:R], ids[:R]) and torch.equal(eng.times_in, tm[:R]), t
        assert torch.equal(eng.pair_w, pw), t
        assert torch.equal(eng.ids_set[0], ids) and torch.equal(eng.times_set[0], tm), t
        assert int(eng.batch_ctr.item()) == t + 1 and eng_model._batch_calls[1] == ref_model._batch_calls[1] == t + 1
    # times=None: the sampler's default_times
    eng(batches[0][0])
    ids, tm, pw = _module_frontier(ref_model, batches[0][0], eng_model.train_sampler.default_times(batches[0][0]), Bs)
    assert torch.equal(eng.ids_set[0], ids) and torch.equal(eng.times_set[0], tm) and bool((tm[:R] == INT64_MAX).all())
    eng_model.train_sampler.csr(DEV).check()
    for bad in (batches[0][0][:1], torch.cat([batches[0][0], batches[1][0]])):
        with pytest.raises(ValueError):
            eng(bad)
    with pytest.raises(ValueError):
        eng(batches[0][0], batches[0][1][:3])
    with pytest.raises(ValueError, match="no queue mode"):
        eng.load_epoch(None, None)
    with pytest.raises(ValueError, match="no queue mode"):
        eng.step_queue()


def _parity_run(rule, dtype, capture):
    """three steps, each from identical weights -> [(loss error, gradient errors, weight errors, losses)]"""
    Bs = 17
    p, store, ref_model, eng_model = _twins(rule, dtype)
    ref_model.optimizer = torch.optim.Adam(ref_model.parameters(), lr=0.01, weight_decay=1e-4)
    batches = _batches(Bs, 3, seed=4)
    eng = gs.engine.FusedUnsupTemporalMeanTrainStep(eng_model, store, batches[0][0], capture=capture,
                                                    example_times=batches[0][1])
    out = []
    for seeds, times in batches:
        ref_model.load_state_dict(eng_model.state_dict())
        l_ref = float(ref_model.train_step(seeds, store, times=times))
        l_eng = float(eng(seeds, times))
        fro = lambda a, b: float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-12))       # noqa: E731
        grads, wts = {}, {}
        for (k, a), (_, b) in zip(eng_model.named_parameters(), ref_model.named_parameters()):
            grads[k] = fro(a.grad.double().cpu().numpy(), b.grad.double().cpu().numpy())
            wts[k] = fro(a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy())
        out.append((abs(l_eng - l_ref) / max(1.0, abs(l_ref)), grads, wts, l_eng, l_ref))
    eng_model.train_sampler.csr(DEV).check()
    return out


@pytest.mark.parametrize("capture", [False, "cmdlist"])
@pytest.mark.parametrize("rule", twr.RULES)
def test_engine_step_matches_train_step(rule, capture):
    """the bounds tests/test_gpu_unsup_engine.py holds FusedUnsupMeanTrainStep to against the module path (bf16)"""
    res = _parity_run(rule, "bf16", capture)
    for step, (le, grads, wts, l_eng, l_ref) in enumerate(res):
        print("bf16 step %d: loss %.6f vs %.6f, worst grad %.3g, worst weight %.3g"
              % (step, l_eng, l_ref, max(grads.values()), max(wts.values())))
    for step, (le, grads, wts, l_eng, l_ref) in enumerate(res):
        assert np.isfinite(l_eng) and le <= 3e-2, (step, l_eng, l_ref)
        for k, e in grads.items():
            assert e <= 0.1, ("grad", step, k, e)
        for k, e in wts.items():
            assert e <= 0.05, ("weight", step, k, e)


@pytest.mark.parametrize("rule", twr.RULES)
def test_engine_step_matches_train_step_fp32(rule):
    """... and with an fp32 store and fp32 compute (that file's FP32_BOUND on the loss and on every gradient)"""
    ops.set_compute_dtype("fp32")
    res = _parity_run(rule, "fp32", "cmdlist")
    for step, (le, grads, wts, l_eng, l_ref) in enumerate(res):
        print("fp32 step %d: loss %.8f vs %.8f (%.3g), worst grad %.3g, worst weight %.3g"
              % (step, l_eng, l_ref, le, max(grads.values()), max(wts.values())))
    for step, (le, grads, wts, l_eng, l_ref) in enumerate(res):
        assert abs(l_eng - l_ref) <= FP32_BOUND * abs(l_ref), (step, l_eng, l_ref)
        for k, e in grads.items():
            assert e <= FP32_BOUND, ("grad", step, k, e)


def test_why_not_sentences():
    p = tr.problem()
    store = gs.FeatureStore.from_array(p["feats"], torch.device(DEV), dtype="bf16")
    cls = gs.engine.FusedUnsupTemporalMeanTrainStep
    good = twr.model(p, temporal_walks=True).to(DEV)
    assert cls.why_not(good, store) is None
    sup = tr.model(p, (8, 8), (3, 2)).to(DEV)
    cases = [
        (sup, {}, "not GSUnsupervised"),
        (twr.model(p).to(DEV), {}, "temporal_walks=False"),
        (good, {"ddp": object()}, "data-parallel"),
        (good, {"pipelined": True}, "pipelined=True"),
        (good, {"eval_only": True}, "eval_only=True"),
        (twr.model(p, dims=(16, 12), temporal_walks=True).to(DEV), {}, "multiples of 8"),
    ]
    for model, kw, words in cases:
        why = cls.why_not(model, store, **kw)
        assert why is not None and words in why and "\n" not in why, (words, why)
    pool = gs.GSUnsupervised(sampler_class=gs.find_sampler("sparse_temporal_neighbor_sampler"), adj=p["tadj"],
                             train_adj=p["tadj"], prep_class=gs.prep_lookup["identity"],
                             aggregator_class=gs.aggregator_lookup["max_pool"], input_dim=16, n_nodes=61,
                             layer_specs=[{"n_train_samples": 3, "n_val_samples": 3, "output_dim": 8,
                                           "activation": lambda x: x}], temporal_walks=True).to(DEV)
    assert "aggregators other than mean" in cls.why_not(pool, store)
    assert "FP8" in cls.why_not(good, store.quantize())
    with pytest.raises(ValueError, match="does not cover"):
        cls(twr.model(p).to(DEV), store, torch.arange(1, 9, device=DEV))
    # the plain unsupervised engine still refuses the temporal sampler
    assert gs.engine.FusedUnsupMeanTrainStep.why_not(good, store) is not None


def test_engine_hands_over_to_the_module_path():
    Bs = 16
    p, store, _, model = _twins("edge", "bf16")
    batches = _batches(Bs, 4, seed=5)
    eng = gs.engine.FusedUnsupTemporalMeanTrainStep(model, store, batches[0][0], capture="cmdlist",
                                                    example_times=batches[0][1])
    losses = [float(eng(s, t)) for s, t in batches[:3]]
    torch.cuda.synchronize()
    assert np.isfinite(losses).all() and eng.holds_parameters() and model._batch_calls == [0, 3]
    res = model.evaluate(batches[3][0], store, times=batches[3][1])
    assert np.isfinite(res["loss"]) and 0 < res["mrr"] <= 1
    snap = model.val_sampler.csr(DEV).snapshot(tr.T_SNAP)
    emb = gs.embeddings(model, store, adj=snap)
    assert emb.shape == (61, 16) and bool(torch.isfinite(emb).all())
    assert torch.allclose(emb.norm(dim=1), torch.ones(61, device=DEV), atol=1e-4)
    l4 = float(model.train_step(batches[3][0], store, times=batches[3][1]))
    torch.cuda.synchronize()
    assert np.isfinite(l4) and not eng.holds_parameters() and model._batch_calls == [1, 4]
    assert int(model.optimizer.step_count.item()) == 4
    for s in (model.train_sampler, model.val_sampler):
        for csr in s._dev.values():
            csr.check()


# ---- train.py --------------------------------------------------------------------------------------------------------
def test_train_cli_engine_fused(capsys):
    train = importlib.import_module("pytorch-graphsage_amd.train")
    p = tr.problem()
    folds = np.array(["train"] * 40 + ["val"] * 11 + ["test"] * 10)
    problem = gs.NodeProblem.from_arrays("classification", p["C"], p["adj"], p["adj"], p["feats"], folds, p["targets"],
                                         cuda=True, adj_time=p["time"], train_adj_time=p["time"],
                                         node_time=np.full(p["n"] + 1, tr.T_SNAP))
    base = ["--problem-path", "<memory>", "--epochs", "1", "--batch-size", "16", "--n-train-samples", "3,2",
            "--n-val-samples", "3,2", "--output-dims", "8,8", "--sampler-class", "sparse_temporal_neighbor_sampler",
            "--temporal-inherit", "edge", "--unsupervised", "--temporal-walks", "--walk-len", "3", "--n-negatives", "5",
            "--engine", "fused"]
    try:
        train.main(base + ["--rng", "philox"], problem=problem)
        cap = capsys.readouterr()
        assert "train_step runs on FusedUnsupTemporalMeanTrainStep" in cap.err and "module path" not in cap.err
        lines = [json.loads(l) for l in cap.out.splitlines() if l.startswith("{")]
        batches = [l for l in lines if "epoch_progress" in l]
        assert len(batches) == 40 // 16 + 1 and all(np.isfinite(l["loss"]) for l in batches)
        assert any("mrr" in l and "epoch_progress" not in l and 0 < l["mrr"] <= 1 for l in lines)
        with pytest.raises(SystemExit, match="FusedUnsupTemporalMeanTrainStep: aggregators other than mean"):
            train.main(base + ["--rng", "philox", "--aggregator-class", "max_pool"], problem=problem)
    finally:
        gs.nn_modules.SparseUniformNeighborSampler.rng_default = "compat"
        gs.nn_modules.SparseTemporalNeighborSampler.inherit_default = "seed"
        ops.set_compute_dtype("bf16")
