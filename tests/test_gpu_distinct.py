"""-m gpu: the distinct-draw sampler.  gsage_sample_csr_distinct and gsage_sample_hops_distinct against the serial
restatement of tests/distinct_ref.py, against each other and against host mode (torch.equal: the frontier is defined bit
for bit); FusedDistinctMeanTrainStep against GSSupervised.train_step on the module path under the same sampler at the
bounds tests/test_gpu_weighted_engine.py applies to the weighted engine (same samples, same kernels behind the sampler),
queue mode against per-call steps bit for bit, the evaluation engine, the refusals; the other aggregators on the module
path; exactness against full-neighbourhood inference where the degrees divide the fan-out; and train.py."""
import ctypes
import importlib
import json
import math

import numpy as np
import pytest
import torch

import distinct_ref as dr
from conftest import pkg
from full_neighbour_ref import neighbours_sparse, reference
from util import close, close_fro

pytestmark = pytest.mark.gpu
gs = pkg()
ops, nat = gs.ops, gs._native
DEV = "cuda"
SEED = 0x0123456789ABCDEF
EINVAL = -1                         # GSAGE_EINVAL (include/gsage.h)


@pytest.fixture(autouse=True)
def _setup():
    ops.set_compute_dtype("bf16")
    ops.warmup(torch.device(DEV))
    yield
    ops.set_compute_dtype("bf16")


def _dev(a):
    return torch.from_numpy(np.asarray(a, dtype=np.int64)).to(DEV)


# ---- the per-hop kernel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,n", [(1, 1), (7, 3), (257, 10), (600, 25), (5, 64), (3, 256)])
def test_per_hop_kernel_equals_the_restatement_and_host_mode(M, n):
    g = dr.graph(n)
    adj, host = g.csr(DEV), g.csr("cpu")
    ids = dr.parents(M, n, np.random.RandomState(M))
    ctr = torch.tensor([6], dtype=torch.int64, device=DEV)
    for g0, base, c in ((0, 0, None), (21 * n, 5, None), (21 * n, 2, ctr)):
        ph = {"seed": SEED, "call_base": base, "g0": g0}
        if c is not None:
            ph["call_ctr"] = c
        before = nat.launch_count()
        got = ops.sample_csr_distinct(adj, _dev(ids), n, ph)
        assert nat.launch_count() - before == 1
        ref, err = dr.sample(g.rowptr, g.col, g.n, ids, n, SEED, base + (6 if c is not None else 0), g0)
        assert err == 0 and torch.equal(got.cpu(), torch.from_numpy(ref)), (g0, base)
        if c is not None:
            ph["call_ctr"] = c.cpu()
        assert torch.equal(got.cpu(), ops.sample_csr_distinct(host, torch.from_numpy(ids), n, ph))
    assert int(ctr.item()) == 6                               # read, not advanced
    adj.check()


def test_per_hop_kernel_beyond_one_trip_per_workgroup():
    """more groups of parents than the launch has workgroups (8192): every workgroup takes a second trip through its
    alternate t buffer.  n = 128: two parents per trip.  Against host mode (which the host tests hold to the
    restatement), and against the restatement itself on parents of the second trip."""
    n, M = 128, 2 * 8192 + 37
    g = dr.graph(n)
    adj = g.csr(DEV)
    ids = np.random.RandomState(9).randint(0, g.n, size=M).astype(np.int64)
    ids[-4:] = [dr.ROWS["n + 1"], dr.ROWS[1000], dr.ROWS["n"], dr.ROWS["degree 0"]]
    ph = {"seed": SEED, "call_base": 3, "g0": 2}
    got = ops.sample_csr_distinct(adj, _dev(ids), n, ph).cpu()
    assert torch.equal(got, ops.sample_csr_distinct(g.csr("cpu"), torch.from_numpy(ids), n, ph))
    for i in (2 * 8192, M - 4, M - 3, M - 2, M - 1):
        ref, _ = dr.sample(g.rowptr, g.col, g.n, ids[i:i + 1], n, SEED, 3, 2 + i * n)
        assert torch.equal(got[i * n:(i + 1) * n], torch.from_numpy(ref)), i
    adj.check()


def test_per_hop_kernel_out_of_range_ids_raise_the_flag():
    n = 3
    g = dr.graph(n)
    adj = g.csr(DEV)
    ids = np.asarray([dr.ROWS[300], g.n, 33, -1, dr.ROWS["last"], 1 << 40], dtype=np.int64)
    got = ops.sample_csr_distinct(adj, _dev(ids), n, {"seed": SEED}).cpu()
    ref, err = dr.sample(g.rowptr, g.col, g.n, ids, n, SEED, 0, 0)
    assert err == 1 and torch.equal(got, torch.from_numpy(ref))
    assert not got.view(-1, n)[[1, 3, 5]].any() and int(adj.err_flag.item()) == 1
    adj.err_flag.zero_()


# ---- the all-hops kernel -----------------------------------------------------------------------------------------
def _sizes(B, fans):
    out = [B]
    for n in fans:
        out.append(out[-1] * n)
    return out


def _buffer(seeds, fans):
    B = len(seeds)
    ids = torch.full((sum(_sizes(B, fans)),), -7, dtype=torch.int64, device=DEV)
    ids[:B] = _dev(seeds)
    return ids


def _ref(g, seeds, fans, call0=0, rank=0):
    return dr.sample_hops(g.rowptr, g.col, g.n, seeds, fans, SEED, call0, rank)


# (2, (25, 25)): hop 2 takes three trips of ten parents -- the alternate t buffers inside one hop
SHAPES = [(1, (3,)), (5, (25, 10)), (33, (5, 3)), (20, (4, 3, 2)), (3, (2, 2, 2, 2, 2)), (2, (64, 4)), (2, (25, 25))]


@pytest.mark.parametrize("B,fans", SHAPES)
def test_all_hops_equal_the_per_hop_launches_and_the_restatement(B, fans):
    g = dr.graph(fans[0])
    adj = g.csr(DEV)
    seeds = dr.parents(B, fans[0], np.random.RandomState(B))
    before = nat.launch_count()
    ids = ops.sample_hops_distinct(adj, _buffer(seeds, fans), B, fans, {"seed": SEED, "call_base": 3})
    assert nat.launch_count() - before == 1                   # every hop in one launch
    ref, err = _ref(g, seeds, fans, call0=3)
    assert err == 0 and torch.equal(ids.cpu(), torch.from_numpy(np.concatenate(ref)))
    cur, off = ids[:B], B
    for k, n in enumerate(fans):
        nxt = ops.sample_csr_distinct(adj, cur, n, {"seed": SEED, "call_base": 3 + k, "g0": 0})
        assert torch.equal(nxt, ids[off:off + nxt.numel()]), ("hop", k + 1)
        cur, off = nxt, off + nxt.numel()
    assert off == ids.numel()
    adj.check()


def test_all_hops_call_counter_and_base():
    g = dr.graph(5)
    adj = g.csr(DEV)
    B, fans = 3, (5, 3)
    seeds = dr.parents(B, 5, np.random.RandomState(2))
    ctr = torch.tensor([6], dtype=torch.int64, device=DEV)
    ids = ops.sample_hops_distinct(adj, _buffer(seeds, fans), B, fans, {"seed": SEED, "call_base": 2, "call_ctr": ctr})
    ref, _ = _ref(g, seeds, fans, call0=8)
    assert torch.equal(ids.cpu(), torch.from_numpy(np.concatenate(ref))) and int(ctr.item()) == 6


def test_all_hops_rank_offsets_the_global_sample_index():
    """rank 1 with B seeds = rows [B, 2B) of every hop of a rank-0 run over 2B seeds whose second half they are"""
    g = dr.graph(4)
    adj = g.csr(DEV)
    B, fans = 6, (4, 3, 2)
    rng = np.random.RandomState(3)
    mine, other = dr.parents(B, 4, rng), rng.randint(0, g.n, size=B)
    one = ops.sample_hops_distinct(adj, _buffer(mine, fans), B, fans, {"seed": SEED, "rank": 1})
    two = ops.sample_hops_distinct(adj, _buffer(np.concatenate([other, mine]), fans), 2 * B, fans, {"seed": SEED})
    o1 = o2 = 0
    for s in _sizes(B, fans):
        assert torch.equal(one[o1:o1 + s], two[o2 + s:o2 + 2 * s])
        o1, o2 = o1 + s, o2 + 2 * s
    ref, _ = _ref(g, mine, fans, rank=1)
    assert torch.equal(one.cpu(), torch.from_numpy(np.concatenate(ref)))


def _desc(adj, ids, B, fans):
    d = nat.HopsDesc()
    d.rowptr, d.col, d.n_rows = adj.rowptr.data_ptr(), adj.col.data_ptr(), adj.n_rows
    d.ids, d.B, d.n_hops = ids.data_ptr(), B, len(fans)
    for k in range(5):
        d.fan[k] = fans[k] if k < len(fans) else 1
    d.max_deg, d.seed, d.err_flag = 0, SEED, adj.err_flag.data_ptr()          # (max_deg is ignored)
    return d


def test_all_hops_seed_queue():
    """n_batches = 3, *batch_idx = 4, batch_base = 1: batch (4 + 1) % 3 = 2 becomes hop 0, its sub-trees follow"""
    g = dr.graph(4)
    adj = g.csr(DEV)
    B, fans = 5, (4, 3)
    rng = np.random.RandomState(4)
    queue = _dev(np.stack([dr.parents(B, 4, rng)[::-1].copy(), rng.randint(0, g.n, size=B), dr.parents(B, 4, rng)]))
    bidx = torch.tensor([4], dtype=torch.int64, device=DEV)
    ids = torch.full((sum(_sizes(B, fans)),), -7, dtype=torch.int64, device=DEV)
    d = _desc(adj, ids, B, fans)
    d.seed_queue, d.batch_idx, d.batch_base, d.n_batches = queue.data_ptr(), bidx.data_ptr(), 1, 3
    nat.check(nat.lib().gsage_sample_hops_distinct(ctypes.addressof(d), None), "hops")
    ref, err = _ref(g, queue[2].cpu().numpy(), fans)
    assert err == 0 and torch.equal(ids.cpu(), torch.from_numpy(np.concatenate(ref)))
    assert int(bidx.item()) == 4
    adj.check()


def test_all_hops_out_of_range_seeds_and_no_seeds():
    g = dr.graph(4)
    adj = g.csr(DEV)
    B, fans = 5, (4, 3)
    seeds = np.asarray([dr.ROWS[300], g.n, 33, -1, dr.ROWS[1000]], dtype=np.int64)
    ids = ops.sample_hops_distinct(adj, _buffer(seeds, fans), B, fans, {"seed": SEED})
    ref, err = _ref(g, seeds, fans)
    assert err == 1 and torch.equal(ids.cpu(), torch.from_numpy(np.concatenate(ref)))
    h1 = ids[B:B + 20].view(B, 4).cpu()                        # (their hop 2 is drawn from row 0, an ordinary row here)
    assert not h1[1].any() and not h1[3].any()
    assert int(adj.err_flag.item()) == 1
    adj.err_flag.zero_()
    torch.cuda.synchronize()
    before = nat.launch_count()
    d = _desc(adj, ids, 0, fans)                              # B = 0: OK, nothing is launched
    assert nat.lib().gsage_sample_hops_distinct(ctypes.addressof(d), None) == 0
    d.B, d.n_hops = B, 6
    assert nat.lib().gsage_sample_hops_distinct(ctypes.addressof(d), None) == EINVAL
    assert nat.launch_count() == before


# ---- the engine --------------------------------------------------------------------------------------------------
TRAIN_SEED, VAL_SEED = 77, 78
_PROBLEM = []


def _problem():
    """a 500-node problem with rows of degree 0, and a validation adjacency of ANOTHER structure (so that an
    evaluation engine walking the training graph would be seen)"""
    if not _PROBLEM:
        p = dict(dr.problem(n=500))
        q = dr.problem(n=500, seed=8)
        p["val_adj"], p["val_indptr"], p["val_data"] = q["adj"], q["indptr"], q["data"]
        _PROBLEM.append(p)
    return _PROBLEM[0]


def _model(p, dims, fans, seed=3, sampler="sparse_distinct_neighbor_sampler", agg="mean"):
    m = dr.model(p, dims, fans, agg=agg, sampler=sampler, seed=seed, adj=p["val_adj"], train_adj=p["adj"],
                 lr_init=0.01, weight_decay=1e-4)
    m.train_sampler.seed, m.val_sampler.seed = TRAIN_SEED, VAL_SEED
    return m.to(DEV)


def _store(p, dtype="bf16"):
    return gs.FeatureStore.from_array(p["feats"], torch.device(DEV), dtype=dtype)


def _batches(p, rng, B, n):
    ids = rng.randint(1, p["n"] + 1, size=(n, B))
    ids[0, :2] = [9, 32]                                       # two rows of degree 0
    tg = p["targets"][ids.reshape(-1)].reshape(n, B, 1)
    return torch.from_numpy(ids).to(DEV), torch.from_numpy(tg).to(DEV)


LOSS = gs.ProblemLosses.classification
CLS = gs.engine.FusedDistinctMeanTrainStep


@pytest.mark.parametrize("capture", [False, "cmdlist"])
def test_engine_frontier_equals_the_restatement_and_the_module_path(capture):
    p = _problem()
    dims, fans, B, L = (16, 8), (5, 3), 33, 2
    store = _store(p)
    ids, tg = _batches(p, np.random.RandomState(5), B, 3)
    model, twin = _model(p, dims, fans), _model(p, dims, fans)
    eng = CLS(model, store, LOSS, ids[0], tg[0], capture=capture)
    for t in range(3):
        eng(ids[t], tg[t])
        ref, err = dr.sample_hops(p["indptr"], p["data"], p["n"] + 1, ids[t].cpu().numpy(), fans, TRAIN_SEED, L * t)
        assert err == 0 and torch.equal(eng.ids_set[0].cpu(), torch.from_numpy(np.concatenate(ref))), ("step", t)
        cur, hops = ids[t], [ids[t]]
        for fn in twin.train_sample_fns:                        # what GSSupervised._encode asks its sampler for
            cur = fn(ids=cur)
            hops.append(cur.view(-1))
        assert torch.equal(eng.ids_set[0], torch.cat(hops)), ("module path, step", t)
    assert int(eng.counter.item()) == 3 * L and twin.train_sampler.calls == 3 * L
    eng.csr.check()


@pytest.mark.parametrize("dims,fans,B", [((128, 128), (25, 10), 16), ((16, 8), (5, 3), 33), ((32, 16, 8), (4, 3, 2), 20)])
@pytest.mark.parametrize("capture", [False, "cmdlist"])
def test_step_matches_the_module_path(dims, fans, B, capture):
    """tests/test_gpu_weighted_engine.py::test_step_matches_the_weighted_module_path over the distinct sampler, its
    comparisons and bounds as they are: the two paths draw the same frontier, and every kernel behind the sampler is
    the uniform engine's"""
    p = _problem()
    store = _store(p)
    ref_model, eng_model = _model(p, dims, fans), _model(p, dims, fans)
    eng_model.load_state_dict(ref_model.state_dict())
    ref_model.optimizer = torch.optim.Adam(ref_model.parameters(), lr=0.01, weight_decay=1e-4)
    ids, tg = _batches(p, np.random.RandomState(6), B, 3)
    eng = CLS(eng_model, store, LOSS, ids[0], tg[0], capture=capture)
    assert eng.fused_tail == (dims == (128, 128))               # the first shape takes the fused seed level
    for step in range(3):
        ref_model.load_state_dict(eng_model.state_dict())       # every step from identical weights
        p_ref = ref_model.train_step(ids=ids[step], feats=store, targets=tg[step], loss_fn=LOSS)
        p_ref = p_ref.detach().float().cpu().numpy()
        p_eng = eng(ids[step], tg[step]).detach().float().cpu().numpy()
        close(p_eng, p_ref, ("preds", step), 3e-2, 3e-2)
        for (k, a), (_, b) in zip(eng_model.named_parameters(), ref_model.named_parameters()):
            close_fro(a.grad.cpu().numpy(), b.grad.cpu().numpy(), ("grad", step, k), 0.1)
            if step == 0:
                close_fro(a.detach().cpu().numpy(), b.detach().cpu().numpy(), ("weight", k), 0.05)
    eng.csr.check()


@pytest.mark.parametrize("B,fans", [(24, (5, 3)), (40, (25, 10))])
@pytest.mark.parametrize("capture", [False, "cmdlist"])
def test_queue_mode_equals_per_call_steps(B, fans, capture):
    """7 steps across a 3-batch queue, batch 1 one seed short: preds and weights bit for bit"""
    p = _problem()
    store = _store(p)
    ids, tg = _batches(p, np.random.RandomState(7), B, 3)
    live = [B, B - 1, B]
    ids[1, B - 1], tg[1, B - 1] = ids[1, 0], tg[1, 0]           # the padding the per-call engine adds itself
    res = []
    for queued in (False, True):
        eng = CLS(_model(p, (128, 128), fans), store, LOSS, ids[0], tg[0], capture=capture)
        preds = []
        if queued:
            eng.load_epoch(ids, tg, n_valid=live)
            for k in range(7):
                preds.append(eng.step_queue().clone())
            assert eng.P == 2
        else:
            for k in range(7):
                nv = live[k % 3]
                preds.append(eng(ids[k % 3, :nv], tg[k % 3, :nv]).clone())
        res.append((torch.stack(preds), eng.flat_p.clone()))
        eng.csr.check()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_two_engines_are_bit_equal():
    p = _problem()
    store = _store(p)
    ids, tg = _batches(p, np.random.RandomState(8), 20, 4)
    outs = []
    for _ in range(2):
        eng = CLS(_model(p, (32, 16), (6, 4)), store, LOSS, ids[0], tg[0])
        preds = torch.stack([eng(ids[t], tg[t]).clone() for t in range(4)])
        outs.append((preds, eng.flat_p.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_eval_only_walks_the_validation_adjacency():
    p = _problem()
    store = _store(p)
    dims, fans, L = (16, 8), (5, 3), 2
    nodes = np.flatnonzero(p["folds"] == "val")[:40]
    chunks = np.array_split(np.arange(nodes.shape[0]), nodes.shape[0] // 16 + 1)
    B, live = max(len(c) for c in chunks), [len(c) for c in chunks]
    assert B <= 16 and len(chunks) == 3 and min(live) < B
    mids = np.stack([np.concatenate([nodes[c], np.repeat(nodes[c[:1]], B - len(c))]) for c in chunks])
    ids = torch.from_numpy(mids).to(DEV)
    tg = torch.zeros(B, 1, dtype=torch.int64, device=DEV)
    model = _model(p, dims, fans)
    whole = CLS(model, store, LOSS, ids[0], tg, eval_only=True).evaluate_fold(ids, live)
    assert tuple(whole.shape) == (sum(live), p["C"])
    # batch by batch on a second engine: the frontier of batch b, and the same predictions
    eng = CLS(model, store, LOSS, ids[0], tg, eval_only=True)
    twin = _model(p, dims, fans)
    twin.load_state_dict(model.state_dict())
    row = 0
    for b in range(len(chunks)):
        got = eng.evaluate_fold(ids[b:b + 1], live[b:b + 1])
        ref, err = dr.sample_hops(p["val_indptr"], p["val_data"], p["n"] + 1, mids[b], fans, VAL_SEED, L * b)
        assert err == 0 and torch.equal(eng.ids_set[0].cpu(), torch.from_numpy(np.concatenate(ref))), ("batch", b)
        assert torch.equal(got, whole[row:row + live[b]])
        with torch.no_grad():
            want = twin(ids[b, :live[b]], store, train=False)
        close(got.cpu().numpy(), want.float().cpu().numpy(), ("preds", b), 3e-2, 3e-2)
        row += live[b]
    eng.csr.check()


def test_constructor_refuses_with_the_sentence():
    p = _problem()
    store = _store(p)
    ids, tg = _batches(p, np.random.RandomState(9), 8, 1)
    old = gs.nn_modules.SparseUniformNeighborSampler.rng_default
    gs.nn_modules.SparseUniformNeighborSampler.rng_default = "philox"
    try:
        uniform = _model(p, (16, 8), (5, 3), sampler="sparse_uniform_neighbor_sampler")
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
    assert "SparseDistinctNeighborSampler" in gs.engine.why_no_fused_engine(model, store)["FusedMeanTrainStep"]
    assert gs.engine.fused_engine_for(model, store) is None


# ---- the module path under the other aggregators ---------------------------------------------------------------------
@pytest.mark.parametrize("agg", ["max_pool", "attention", "lstm"])
def test_module_path_runs_the_other_aggregators(agg):
    p = _problem()
    store = _store(p)
    fans = (5, 3)
    ids, tg = _batches(p, np.random.RandomState(10), 12, 1)
    model, twin = _model(p, (16, 8), fans, agg=agg), _model(p, (16, 8), fans, agg=agg)
    preds = model.train_step(ids=ids[0], feats=store, targets=tg[0], loss_fn=LOSS)
    assert tuple(preds.shape) == (12, p["C"]) and bool(torch.isfinite(preds.float()).all())
    assert model.train_sampler.calls == 2
    cur, hops = ids[0], [ids[0]]
    for fn in twin.train_sample_fns:
        cur = fn(ids=cur)
        hops.append(cur.view(-1))
    ref, err = dr.sample_hops(p["indptr"], p["data"], p["n"] + 1, ids[0].cpu().numpy(), fans, TRAIN_SEED, 0)
    assert err == 0 and torch.equal(torch.cat(hops).cpu(), torch.from_numpy(np.concatenate(ref)))
    model.train_sampler.csr(DEV).check()


# ---- exactness -----------------------------------------------------------------------------------------------------
def test_sampled_forward_is_exact_where_degrees_divide_the_fanout():
    """degrees in {1, 2, 5, 10}, fan-outs (10, 10), fp32: the sampled forward under the distinct sampler equals
    full-neighbourhood inference and the float64 restatement of it, at the bound tests/test_gpu_full_neighbour.py
    applies between a sampled anchor and the full path; the uniform sampler's does not"""
    ops.set_compute_dtype("fp32")
    p = dr.problem(n=120, degrees=(1, 2, 5, 10), seed=11)
    store = _store(p, "fp32")
    ids = torch.arange(0, 121, 3, device=DEV)
    model = dr.model(p, (16, 8), (10, 10)).to(DEV)
    with torch.no_grad():
        sampled = model(ids, store, train=False)
    full = gs.full_neighbour(model, store, nodes=ids)
    close(sampled.cpu().numpy(), full.cpu().numpy(), "distinct sampler vs full neighbourhood", 2e-5, 2e-5)
    ref, _ = reference(model, p["feats"], neighbours_sparse(p["indptr"], p["data"]))
    close(sampled.cpu().numpy(), ref[ids.cpu().numpy()], "distinct sampler vs float64", 2e-5, 2e-5)
    old = gs.nn_modules.SparseUniformNeighborSampler.rng_default
    gs.nn_modules.SparseUniformNeighborSampler.rng_default = "philox"
    try:
        uniform = dr.model(p, (16, 8), (10, 10), sampler="sparse_uniform_neighbor_sampler").to(DEV)
    finally:
        gs.nn_modules.SparseUniformNeighborSampler.rng_default = old
    uniform.load_state_dict(model.state_dict())
    with torch.no_grad():
        noisy = uniform(ids, store, train=False)
    with pytest.raises(AssertionError):
        close(noisy.cpu().numpy(), full.cpu().numpy(), "uniform sampler vs full neighbourhood", 2e-5, 2e-5)


# ---- train.py ------------------------------------------------------------------------------------------------------
CLI = ["--problem-path", "<memory>", "--epochs", "2", "--batch-size", "32", "--n-train-samples", "3,2",
       "--n-val-samples", "3,2", "--output-dims", "8,8", "--show-test", "--sampler-class",
       "sparse_distinct_neighbor_sampler", "--rng", "philox"]


def _cli_problem():
    p = dr.problem(n=200)
    return gs.NodeProblem.from_arrays("classification", p["C"], p["adj"], p["adj"], p["feats"], p["folds"],
                                      p["targets"], cuda=True)


def test_train_cli_engine_fused(capsys):
    train = importlib.import_module("pytorch-graphsage_amd.train")
    try:
        train.main(CLI + ["--engine", "fused"], problem=_cli_problem())
        cap = capsys.readouterr()
        assert "train_step runs on FusedDistinctMeanTrainStep" in cap.err
        assert "using the module path" not in cap.err and "on the module path" not in cap.err     # training, evaluation
        assert "falls back to the module path" not in cap.err
        lines = [json.loads(l) for l in cap.out.splitlines() if l.startswith("{")]
        steps = lines[:-1]                                      # (--engine fused prints every --log-interval batches)
        assert len(steps) >= 3 and {l["epoch"] for l in steps} == {0, 1}
        assert all(math.isfinite(v) for l in steps for v in l["train_metric"].values())
        assert lines[-2]["val_metric"] is not None and lines[-1]["test_f1"] is not None
    finally:
        gs.nn_modules.SparseUniformNeighborSampler.rng_default = "compat"
        ops.set_compute_dtype("bf16")


def test_train_cli_engine_auto_takes_the_module_path(capsys):
    train = importlib.import_module("pytorch-graphsage_amd.train")
    try:
        train.main(CLI + ["--engine", "auto"], problem=_cli_problem())
        cap = capsys.readouterr()
        said = [l for l in cap.err.splitlines() if "using the module path" in l]
        assert len(said) == 1 and "SparseDistinctNeighborSampler" in said[0]
        assert "FusedDistinctMeanTrainStep" in said[0] and "train_step runs on" not in cap.err
        lines = [json.loads(l) for l in cap.out.splitlines() if l.startswith("{")]
        assert lines and lines[-1]["test_f1"] is not None
    finally:
        gs.nn_modules.SparseUniformNeighborSampler.rng_default = "compat"
        ops.set_compute_dtype("bf16")


def test_train_cli_refuses_importance_walks():
    train = importlib.import_module("pytorch-graphsage_amd.train")
    try:
        with pytest.raises(SystemExit) as e:
            train.main(CLI + ["--engine", "auto", "--importance-walks", "5"], problem=_cli_problem())
        msg = str(e.value)
        assert "--importance-walks" in msg and "sparse_distinct_neighbor_sampler" in msg and "\n" not in msg
    finally:
        gs.nn_modules.SparseUniformNeighborSampler.rng_default = "compat"
        ops.set_compute_dtype("bf16")
