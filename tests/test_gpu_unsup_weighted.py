"""-m gpu: weighted walks for unsupervised training on the MI355X.  gsage_unsup_batch_weighted against the restatement of
tests/unsup_weighted_ref.py bit for bit (every arranged row of weighted_ref.graph(), the deep rows, shards, the counter,
the error flag) and against a permutation graph that needs no restatement; GSUnsupervised(weighted_walks=True);
FusedUnsupWeightedMeanTrainStep's batches and frontiers against the module path bit for bit and its steps against
GSUnsupervised.train_step from identical weights at the bounds tests/test_gpu_unsup_engine.py applies to the unweighted
engine (bf16: loss 3e-2, gradients 0.1, first-step weights 0.05; fp32 store and compute: 2e-4); the command line.
Measured errors go to GSAGE_PARITY_LOG."""
import importlib
import json

import numpy as np
import pytest
import torch

import unsup_engine_ref as uref
import unsup_ref
import unsup_weighted_ref as ur
import weighted_ref as wr
from conftest import pkg
from util import close_fro, note_parity

pytestmark = pytest.mark.gpu
gs = pkg()
ops = gs.ops
nat = gs._native
DEV = "cuda"
SEED = 0x1234567887654321
FP32_BOUND = 2e-4


@pytest.fixture(autouse=True)
def _warm():
    ops.set_compute_dtype("bf16")
    ops.warmup(torch.device(DEV))
    yield
    ops.set_compute_dtype("bf16")


# ---- 1. the builder on the arranged rows ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arranged():
    g = wr.graph()
    csr = g.csr(DEV)
    assert torch.equal(csr.edge_cdf.cpu(), torch.from_numpy(g.cdf.view(np.int64)))
    return g, csr, ops.neg_cdf(csr, weighted=True)


def _seeds(g, B):
    if B == 1:
        return np.asarray([wr.ROWS[1000]], dtype=np.int64)
    seeds = ur.seeds_on_rows(g, B, np.random.RandomState(B))
    assert set(wr.ROWS.values()) <= set(seeds.tolist())       # a walk starts on every arranged row
    return seeds


_REF = {}


def _reference(B, walk_len, Q, call, cdf):
    """the restatement over the DEVICE's negatives' table (an input of the builder), computed once per case"""
    key = (B, walk_len, Q, call)
    if key not in _REF:
        g = wr.graph()
        _REF[key] = ur.build_batch(g.rowptr, g.col, g.cdf, g.n, _seeds(g, B), walk_len, Q, cdf.cpu().numpy(), SEED, call)
    return _REF[key]


@pytest.mark.parametrize("Q", [1, 20])
@pytest.mark.parametrize("walk_len", [1, 5, 16])
@pytest.mark.parametrize("B", [1, 37, 256])
def test_builder_bit_exact(arranged, B, walk_len, Q):
    g, csr, cdf = arranged
    # (the table is the builder's INPUT; the device's pow and running sum round differently from numpy's)
    assert np.allclose(cdf.cpu().numpy(), ur.neg_table(g.rowptr, g.cdf), rtol=1e-12, atol=0)
    seeds = torch.from_numpy(_seeds(g, B)).to(DEV)
    before = nat.launch_count()
    ids, pw = ops.unsup_batch(csr, seeds, walk_len, Q, cdf, {"seed": SEED, "call_base": 2}, weighted=True)
    assert nat.launch_count() - before == 1
    rid, rpw, err = _reference(B, walk_len, Q, 2, cdf)
    assert err == 0 and int(csr.err_flag.item()) == 0
    assert ids.dtype == torch.int64 and pw.dtype == torch.float32
    assert torch.equal(ids.cpu(), torch.from_numpy(rid)) and torch.equal(pw.cpu(), torch.from_numpy(rpw))
    # the negatives: those of the unweighted builder for the same table and call
    plain, _ = ops.unsup_batch(csr, seeds, walk_len, Q, cdf, {"seed": SEED, "call_base": 2})
    assert torch.equal(ids[2 * B:], plain[2 * B:])
    host, _ = ops.unsup_batch(g.csr("cpu"), seeds.cpu(), walk_len, Q, cdf.cpu(), {"seed": SEED, "call_base": 2},
                              weighted=True)
    assert torch.equal(ids.cpu(), host)                        # host mode on the device's table: every bit
    dead = {wr.ROWS[k] for k in ("degree 0", "degree 0 again", "all zero", "all zero, 12 edges", "all zero, 300 edges")}
    assert not set(ids[2 * B:].tolist()) & dead                # no negative without a drawable edge
    for name in ("degree 0", "all zero", "all zero, 300 edges"):
        for i in np.flatnonzero(seeds.cpu().numpy() == wr.ROWS[name]):
            assert int(ids[B + i]) == wr.ROWS[name] and float(pw[i]) == 0.0


# ---- 2. deep rows ----------------------------------------------------------------------------------------------------------
def test_builder_deep_rows():
    g = ur.deep_graph()
    csr = g.csr(DEV)
    assert torch.equal(csr.edge_cdf.cpu(), torch.from_numpy(g.cdf.view(np.int64)))
    cdf = ops.neg_cdf(csr, weighted=True)
    B, wl, Q = 64, 16, 20
    seeds = np.arange(B, dtype=np.int64) % g.n
    ids, pw = ops.unsup_batch(csr, torch.from_numpy(seeds).to(DEV), wl, Q, cdf, {"seed": SEED, "call_base": 1},
                              weighted=True)
    trace = []
    rid, rpw, err = ur.build_batch(g.rowptr, g.col, g.cdf, g.n, seeds, wl, Q, cdf.cpu().numpy(), SEED, 1, trace=trace)
    assert err == 0 and int(csr.err_flag.item()) == 0
    assert torch.equal(ids.cpu(), torch.from_numpy(rid)) and torch.equal(pw.cpu(), torch.from_numpy(rpw))
    # the walks did take the longest searches and the ordinary ones: steps through the heavy first edges of every deep
    # row (four rounds at degree 262 145, three at 4097) and steps far behind them
    for deg in (4096, 4097, 262145):
        at = [k for d, k in trace if d == deg]
        assert sum(k <= 1 for k in at) >= 3 and sum(k > deg // 64 + 1 for k in at) >= 3, (deg, len(at))


# ---- 3. independent of the restatement -------------------------------------------------------------------------------------
def test_builder_walks_a_permutation():
    """every row: one drawable edge among zero-weight ones, to perm[row]; so the positive of seed s is perm^t_s(s)"""
    rng = np.random.RandomState(9)
    n, fixed, two = 97, 10, (20, 21)                           # a fixed point, a 2-cycle, one cycle through the rest
    perm = np.arange(n)
    perm[two[0]], perm[two[1]] = two[1], two[0]
    rest = rng.permutation([v for v in range(n) if v != fixed and v not in two])
    perm[rest] = np.roll(rest, -1)
    assert sorted(perm.tolist()) == list(range(n)) and perm[fixed] == fixed
    deg = rng.randint(1, 140, size=n)                          # both sides of 64
    deg[:4] = [1, 64, 65, 139]
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.randint(0, n, size=int(rowptr[-1])).astype(np.int32)
    weight = np.zeros(int(rowptr[-1]), dtype=np.float32)
    for v in range(n):
        e = rowptr[v] + rng.randint(deg[v])
        col[e], weight[e] = perm[v], rng.uniform(0.1, 10.0)
    csr = gs.DeviceCSR(torch.from_numpy(rowptr).to(DEV), torch.from_numpy(col).to(DEV), n, int(deg.max()))
    csr = csr.with_weights(torch.from_numpy(weight).to(DEV))
    cdf = ops.neg_cdf(csr, weighted=True)
    B, wl, call = 97, 16, 6
    seeds = np.arange(n, dtype=np.int64)
    ids, pw = ops.unsup_batch(csr, torch.from_numpy(seeds).to(DEV), wl, 4, cdf, {"seed": SEED, "call_base": call},
                              weighted=True)
    ids, pw = ids.cpu().numpy(), pw.cpu().numpy()
    lens = set()
    for s in range(n):
        t = 1 + ((unsup_ref._P(s, call, SEED, unsup_ref.TAG_LEN)[0] * wl) >> 32)      # the lengths of the unweighted batch
        lens.add(t)
        v = s
        for _ in range(t):
            v = int(perm[v])
        assert ids[s] == s and ids[B + s] == v, (s, t)
        assert pw[s] == (0.0 if v == s else 1.0)
    assert len(lens) >= 8 and pw[fixed] == 0.0 and (pw == 1).sum() >= n - 3
    assert int(csr.err_flag.item()) == 0


# ---- 4. shards, counter, errors --------------------------------------------------------------------------------------------
def test_builder_shards_counter_and_errors(arranged):
    g, csr, cdf = arranged
    B, wl, Q = 37, 5, 20
    seeds = torch.from_numpy(_seeds(g, B)).to(DEV)
    ph = {"seed": SEED, "call_base": 4}
    ids, pw = ops.unsup_batch(csr, seeds, wl, Q, cdf, ph, weighted=True)
    # the shard [13, 37) of the batch draws what the whole batch draws (and the same negatives)
    sid, spw = ops.unsup_batch(csr, seeds[13:37], wl, Q, cdf, dict(ph, g0=13), weighted=True)
    assert torch.equal(sid[:24], ids[13:37]) and torch.equal(sid[24:48], ids[B + 13:B + 37])
    assert torch.equal(sid[48:], ids[2 * B:]) and torch.equal(spw, pw[13:37])
    # a device word advances the stream: call_base 3 + *ctr 1 is call 4, *ctr 2 is another draw
    ctr = torch.ones(1, dtype=torch.int64, device=DEV)
    cid, cpw = ops.unsup_batch(csr, seeds, wl, Q, cdf, {"seed": SEED, "call_base": 3, "call_ctr": ctr}, weighted=True)
    assert torch.equal(cid, ids) and torch.equal(cpw, pw)
    ctr.fill_(2)
    nid, _ = ops.unsup_batch(csr, seeds, wl, Q, cdf, {"seed": SEED, "call_base": 3, "call_ctr": ctr}, weighted=True)
    assert not torch.equal(nid[B:2 * B], ids[B:2 * B])
    rid, _, _ = _reference(B, wl, Q, 5, cdf)
    assert torch.equal(nid.cpu(), torch.from_numpy(rid))
    # a seed outside the graph raises the flag and yields 0
    for outside in (g.n, -1):
        bad = seeds.clone()
        bad[3] = outside
        bid, bpw = ops.unsup_batch(csr, bad, wl, Q, cdf, ph, weighted=True)
        rid, rpw, err = ur.build_batch(g.rowptr, g.col, g.cdf, g.n, bad.cpu().numpy(), wl, Q, cdf.cpu().numpy(), SEED, 4)
        assert err == 1 and int(csr.err_flag.item()) == 1
        csr.err_flag.zero_()
        assert torch.equal(bid.cpu(), torch.from_numpy(rid)) and torch.equal(bpw.cpu(), torch.from_numpy(rpw))
        assert int(bid[3]) == 0 and int(bid[B + 3]) == 0 and float(bpw[3]) == 0
    # a stored column outside the graph: the walk that reaches it ends at 0, the seed stays
    col = g.col.copy()
    row = wr.ROWS["degree 1"]
    col[g.rowptr[row]] = g.n
    col[g.rowptr[wr.ROWS["one drawable of 20"]] + 13] = -5
    broken = gs.DeviceCSR(torch.from_numpy(g.rowptr).to(DEV), torch.from_numpy(col).to(DEV), g.n, int(g.deg.max()))
    broken = broken.with_weights(torch.from_numpy(g.weight).to(DEV))
    assert torch.equal(broken.edge_cdf, csr.edge_cdf)
    bid, bpw = ops.unsup_batch(broken, seeds, wl, Q, cdf, ph, weighted=True)
    rid, rpw, err = ur.build_batch(g.rowptr, col, g.cdf, g.n, seeds.cpu().numpy(), wl, Q, cdf.cpu().numpy(), SEED, 4)
    assert err == 1 and int(broken.err_flag.item()) == 1 and int(csr.err_flag.item()) == 0
    broken.err_flag.zero_()
    assert torch.equal(bid.cpu(), torch.from_numpy(rid)) and torch.equal(bpw.cpu(), torch.from_numpy(rpw))
    for name in ("degree 1", "one drawable of 20"):
        i = int(np.flatnonzero(seeds.cpu().numpy() == wr.ROWS[name])[0])
        assert int(bid[i]) == wr.ROWS[name] and int(bid[B + i]) == 0 and float(bpw[i]) == 1.0
    # refusals before anything is launched
    out, w = torch.zeros(2 * B + Q, dtype=torch.int64, device=DEV), torch.zeros(B, device=DEV)
    L = nat.lib()
    args = lambda total=1.0, wlen=wl, ecdf=csr.edge_cdf.data_ptr(): (                                    # noqa: E731
        csr.rowptr.data_ptr(), csr.col.data_ptr(), ecdf, g.n, seeds.data_ptr(), B, wlen, Q, cdf.data_ptr(), total, SEED,
        None, 0, 0, out.data_ptr(), w.data_ptr(), None, None)
    torch.cuda.synchronize()
    before = nat.launch_count()
    assert L.gsage_unsup_batch_weighted(*args(ecdf=None)) == -1 and b"edge_cdf" in L.gsage_last_error()
    assert L.gsage_unsup_batch_weighted(*args(0.0)) == -1 and b"weight" in L.gsage_last_error()
    assert L.gsage_unsup_batch_weighted(*args(float("nan"))) == -1
    assert L.gsage_unsup_batch_weighted(*args(1.0, 0)) == -1 and L.gsage_unsup_batch_weighted(*args(1.0, 17)) == -1
    assert nat.launch_count() == before
    with pytest.raises(ValueError, match="edge weights"):
        ops.unsup_batch(g.csr(DEV, weighted=False), seeds, wl, Q, cdf, ph, weighted=True)


# ---- the model and the engine ----------------------------------------------------------------------------------------------
TRAIN_SEED, VAL_SEED = 77, 78
_PROBLEM = []
CLS = gs.engine.FusedUnsupWeightedMeanTrainStep


def _problem():
    """weighted_ref.weighted_problem() plus a validation adjacency of the same structure and OTHER weights"""
    if not _PROBLEM:
        p = dict(wr.weighted_problem())
        rng = np.random.RandomState(11)
        w2 = np.exp(rng.normal(size=p["w"].shape[0]) * 1.5).astype(np.float32)
        w2[rng.rand(w2.shape[0]) < 0.1] = 0.0
        p["w_val"] = w2
        _PROBLEM.append(p)
    return _PROBLEM[0]


def _model(dims, fans, Q=20, nw=1.0, weighted_walks=True, seed=3):
    p = _problem()
    torch.manual_seed(seed)
    m = gs.GSUnsupervised(sampler_class=gs.find_sampler("sparse_weighted_neighbor_sampler"),
                          adj=gs.WeightedAdj(p["adj"], p["w_val"]), train_adj=gs.WeightedAdj(p["adj"], p["w"]),
                          prep_class=gs.prep_lookup["identity"], aggregator_class=gs.aggregator_lookup["mean"],
                          input_dim=p["feats"].shape[1], n_nodes=201, layer_specs=uref.specs(dims, fans), n_negatives=Q,
                          walk_len=5, neg_weight=nw, lr_init=0.01, weight_decay=1e-4, weighted_walks=weighted_walks)
    m.train_sampler.seed, m.val_sampler.seed = TRAIN_SEED, VAL_SEED
    return m.to(DEV)


def _twins(dims, fans, Q, nw, dtype="bf16"):
    store = gs.FeatureStore.from_array(_problem()["feats"], torch.device(DEV), dtype=dtype)
    ref_model, eng_model = _model(dims, fans, Q, nw), _model(dims, fans, Q, nw)
    eng_model.load_state_dict(ref_model.state_dict())
    return store, ref_model, eng_model


def _seed_batches(B, n, seed=1):
    rng = np.random.RandomState(seed)
    ids = rng.randint(1, 201, size=(n, B))
    ids[0, :2] = [5, 9]                                        # the all-zero row, a row of degree 0
    return [torch.from_numpy(ids[k]).to(DEV) for k in range(n)]


# ---- 5. the model ------------------------------------------------------------------------------------------------------------
def test_model_builds_evaluates_and_learns():
    p = _problem()
    model = _model((16, 8), (5, 3))
    assert "weighted_walks=True" in repr(model)
    store = gs.FeatureStore.from_array(p["feats"], torch.device(DEV), dtype="bf16")
    seeds = _seed_batches(64, 2)
    model.build_batch(seeds[1])
    ids, pw = model.build_batch(seeds[0])                      # the model's call index is 1 now
    csr = model.train_sampler.csr(DEV)
    want = ops.unsup_batch(csr, seeds[0], 5, 20, ops.neg_cdf(csr, weighted=True), {"seed": TRAIN_SEED, "call_base": 1},
                           weighted=True)
    assert torch.equal(ids, want[0]) and torch.equal(pw, want[1]) and model._batch_calls == [0, 2]
    cdf = wr.build_cdf(p["indptr"], p["w"])
    rid, rpw, err = ur.build_batch(p["indptr"], p["data"], cdf, 201, seeds[0].cpu().numpy(), 5, 20,
                                   model._walk_graph(True, torch.device(DEV))[1].cpu().numpy(), TRAIN_SEED, 1)
    assert err == 0 and torch.equal(ids.cpu(), torch.from_numpy(rid)) and torch.equal(pw.cpu(), torch.from_numpy(rpw))
    # evaluation walks the evaluation graph by ITS weights
    res = model.evaluate(seeds[0], store)
    assert np.isfinite(res["loss"]) and 0 < res["mrr"] <= 1 and model._batch_calls == [1, 2]
    vcsr = model.val_sampler.csr(DEV)
    assert model._walk_graph(False, torch.device(DEV))[0] is vcsr and not torch.equal(vcsr.edge_cdf, csr.edge_cdf)
    losses = [float(model.train_step(None, store, batch=(ids, pw))) for _ in range(40)]
    print("weighted walks, one fixed batch: first %.5f last %.5f" % (losses[0], losses[-1]))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    # weighted_walks=False over the weighted sampler: the uniform builder, as before
    plain = _model((16, 8), (5, 3), weighted_walks=False)
    a = plain.build_batch(seeds[0])
    b = ops.unsup_batch(csr, seeds[0], 5, 20, ops.neg_cdf(csr), {"seed": TRAIN_SEED, "call_base": 0})
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for s in (model.train_sampler, model.val_sampler):
        for c in s._dev.values():
            c.check()


# ---- 6. the engine's batches ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capture", [False, "cmdlist"])
def test_engine_builds_the_module_paths_batches_and_frontiers(capture):
    B, Q, dims, fans = 17, 5, (16, 8), (5, 3)
    L = len(fans)
    store, ref_model, eng_model = _twins(dims, fans, Q, 1.0)
    assert CLS.why_not(eng_model, store) is None and CLS.supports(eng_model, store)
    assert "the fused K1 draws uniformly" in gs.engine.FusedUnsupMeanTrainStep.why_not(eng_model, store)
    batches = _seed_batches(B, 4)
    # the models' stream does not start at 0: one batch each before the engine exists
    ref_model.build_batch(batches[3])
    eng_model.build_batch(batches[3])
    before = nat.launch_count()
    eng = CLS(eng_model, store, batches[0], capture=capture)
    assert nat.launch_count() > before
    R = 2 * B + Q
    assert eng.B == R and eng.size[0] == R and eng.off[1] == R and eng._k1_own_launch()
    torch.cuda.synchronize()
    assert eng_model._batch_calls == [0, 1] and int(eng.batch_ctr.item()) == 0 and int(eng.counter.item()) == 0
    csr = eng_model.train_sampler.csr(DEV)
    assert eng.csr is csr and eng.walk_csr is csr

    def check(t, seeds):
        rid, rpw = ref_model.build_batch(seeds)
        assert torch.equal(eng.ids_set[0][:R], rid) and torch.equal(eng.pair_w, rpw), t
        # the frontier: what the module path's sampler draws for those R rows at its call indices L t .. L t + L - 1
        buf = torch.zeros_like(eng.ids_set[0])
        buf[:R] = rid
        ops.sample_hops_weighted(csr, buf, R, fans, {"seed": TRAIN_SEED, "call_base": L * t})
        assert torch.equal(eng.ids_set[0], buf), ("frontier", t)
        cur, hops = rid, [rid]
        for n in fans:
            cur = ops.sample_csr_weighted(csr, cur, n, {"seed": TRAIN_SEED, "call_base": L * t + len(hops) - 1})
            hops.append(cur)
        assert torch.equal(eng.ids_set[0], torch.cat(hops)), ("per-hop launches", t)

    for t, seeds in enumerate(batches[:3]):
        eng(seeds)
        check(t, seeds)
        assert int(eng.batch_ctr.item()) == t + 1 and int(eng.counter.item()) == L * (t + 1)
    assert eng_model._batch_calls[1] == ref_model._batch_calls[1] == 4
    a, b = eng_model.build_batch(batches[3]), ref_model.build_batch(batches[3])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # ... and the engine follows a stream that moved without it (the module-path build_batch above)
    eng(batches[0])
    check(3, batches[0])
    csr.check()
    with pytest.raises(ValueError):
        eng.load_epoch(None, None)
    with pytest.raises(ValueError):
        eng.step_queue()


# ---- 7. step parity ------------------------------------------------------------------------------------------------------------
SHAPES = [((16, 8), (5, 3), 17, 5), ((32, 16, 8), (4, 3, 2), 8, 3), ((128, 128), (25, 10), 16, 20)]


def _parity_run(dims, fans, B, Q, nw, capture, dtype):
    """three steps, each from identical weights -> [(loss error, {name: gradient error}, {name: weight error}, ..)]"""
    store, ref_model, eng_model = _twins(dims, fans, Q, nw, dtype)
    ref_model.optimizer = torch.optim.Adam(ref_model.parameters(), lr=0.01, weight_decay=1e-4)
    batches = _seed_batches(B, 3)
    eng = CLS(eng_model, store, batches[0], capture=capture)
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
    assert ref_model.train_sampler.calls == 3 * len(fans) == int(eng.counter.item())
    eng_model.train_sampler.csr(DEV).check()
    return out


@pytest.mark.parametrize("nw", [1.0, 2.0])
@pytest.mark.parametrize("dims,fans,B,Q", SHAPES)
@pytest.mark.parametrize("capture", [False, "cmdlist"])
def test_engine_step_matches_train_step(capture, dims, fans, B, Q, nw):
    res = _parity_run(dims, fans, B, Q, nw, capture, "bf16")
    for step, (le, grads, wts, l_eng, l_ref) in enumerate(res):
        print("bf16 step %d: loss %.6f vs %.6f, worst grad %.3g, worst weight %.3g"
              % (step, l_eng, l_ref, max(grads.values()), max(wts.values())))
    note_parity("unsup_weighted_engine_bf16/%s_B%d_Q%d_nw%g_%s" % ("x".join(map(str, dims)), B, Q, nw, capture or "eager"),
                loss=max(r[0] for r in res), grad=max(max(r[1].values()) for r in res), weight=max(res[0][2].values()))
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
def test_engine_step_matches_train_step_fp32(capture, dims, fans, B, Q, nw):
    ops.set_compute_dtype("fp32")
    res = _parity_run(dims, fans, B, Q, nw, capture, "fp32")
    worst = 0.0
    for step, (le, grads, wts, l_eng, l_ref) in enumerate(res):
        print("fp32 step %d: loss %.8f vs %.8f (%.3g), worst grad %.3g" % (step, l_eng, l_ref, le, max(grads.values())))
        worst = max(worst, abs(l_eng - l_ref) / abs(l_ref), max(grads.values()))
    note_parity("unsup_weighted_engine_fp32/%s_B%d_Q%d_nw%g_%s" % ("x".join(map(str, dims)), B, Q, nw, capture or "eager"),
                worst=worst)
    for step, (le, grads, wts, l_eng, l_ref) in enumerate(res):
        assert abs(l_eng - l_ref) <= FP32_BOUND * abs(l_ref), (step, l_eng, l_ref)
        for k, e in grads.items():
            assert e <= FP32_BOUND, ("grad", step, k, e)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_short_batches_take_the_masked_loss(dtype):
    ops.set_compute_dtype(dtype)
    dims, fans, B, Q, nw = (16, 8), (5, 3), 17, 5, 1.0
    store, ref_model, eng_model = _twins(dims, fans, Q, nw, dtype)
    full = _seed_batches(B, 3, seed=2)
    eng = CLS(eng_model, store, full[0], capture="cmdlist")
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
        assert torch.equal(eng.ids_set[0][R:R + R * fans[0]],
                           ops.sample_csr_weighted(eng.csr, all_ids, fans[0],
                                                   {"seed": TRAIN_SEED, "call_base": ref_model.train_sampler.calls - 2}))
        loss, _ = uref.masked_loss(E, B, Q, pair_w, nw, b)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(ref_model.parameters(), 5)
        with torch.no_grad():
            over_B = float(uref.masked_loss(E, B, Q, pair_w, nw, b)[0]) * b / B        # the 1/B normalisation
        l_ref = float(loss.detach())
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


def test_engine_hands_over_to_the_module_path():
    B, Q = 32, 20
    store = gs.FeatureStore.from_array(_problem()["feats"], torch.device(DEV), dtype="bf16")
    model = _model((16, 8), (5, 3), Q)
    batches = _seed_batches(B, 4, seed=5)
    eng = CLS(model, store, batches[0], capture="cmdlist")
    losses = [float(eng(s)) for s in batches[:3]]
    torch.cuda.synchronize()
    assert np.isfinite(losses).all() and eng.holds_parameters()
    res = model.evaluate(batches[3], store)
    assert np.isfinite(res["loss"]) and 0 < res["mrr"] <= 1
    sd = model.optimizer_state_dict()
    assert int(sd["state"][0]["step"]) == 3
    l4 = float(model.train_step(batches[3], store))
    torch.cuda.synchronize()
    assert np.isfinite(l4) and isinstance(model.optimizer, gs.optim.FlatAdam) and not eng.holds_parameters()
    assert int(model.optimizer.step_count.item()) == 4 and model._batch_calls[1] == 4
    for s in (model.train_sampler, model.val_sampler):
        for csr in s._dev.values():
            csr.check()


# ---- 8. the command line -------------------------------------------------------------------------------------------------------
def test_train_main_weighted_walks_fused(capsys, tmp_path):
    p = wr.weighted_problem()
    problem = gs.NodeProblem.from_arrays("classification", p["C"], p["adj"], p["adj"].copy(), p["feats"], p["folds"],
                                         p["targets"], cuda=True)
    path = str(tmp_path / "emb.npy")
    train = importlib.import_module("pytorch-graphsage_amd.train")
    argv = ["--problem-path", "<memory>", "--epochs", "2", "--batch-size", "32", "--sampler-class",
            "sparse_uniform_neighbor_sampler", "--n-train-samples", "5,3", "--n-val-samples", "5,3", "--output-dims",
            "32,32", "--unsupervised", "--weighted-walks", "--engine", "fused", "--rng", "philox", "--importance-walks",
            "20", "--save-embeddings", path]
    try:
        train.main(argv, problem=problem)
        cap = capsys.readouterr()
        assert "train_step runs on FusedUnsupWeightedMeanTrainStep" in cap.err and "module path" not in cap.err
        assert "weighted_walks=True" in cap.err
        lines = [json.loads(l) for l in cap.out.splitlines() if l.startswith("{")]
        batches = [l for l in lines if "epoch_progress" in l]
        epochs = [l for l in lines if "mrr" in l and "epoch_progress" not in l]
        assert len(batches) == 2 * (130 // 32 + 1) and all(np.isfinite(l["loss"]) for l in batches)
        assert len(epochs) == 3 and all(0 < l["mrr"] <= 1 for l in epochs)
        emb = np.load(path)
        assert emb.shape == (201, 64) and np.isfinite(emb).all()
        norms = np.linalg.norm(emb, axis=1)
        assert ((np.abs(norms - 1.0) <= 1e-4) | (norms <= 1e-4)).all() and (norms > 0.5).sum() >= 190
        with pytest.raises(SystemExit, match="FusedUnsupWeightedMeanTrainStep: aggregators other than mean"):
            train.main(argv[:-2] + ["--aggregator-class", "max_pool"], problem=problem)      # (without the export)
        with pytest.raises(SystemExit, match="max-pool and attention"):
            train.main(argv + ["--aggregator-class", "max_pool"], problem=problem)
    finally:
        gs.nn_modules.SparseUniformNeighborSampler.rng_default = "compat"
