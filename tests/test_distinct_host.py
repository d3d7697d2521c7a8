"""The distinct-draw sampler without a GPU: host mode of ops.sample_csr_distinct against the serial restatement of
tests/distinct_ref.py (bit for bit), the definition's properties and its uniformity, the entry points' refusals, the
registry, the engine's refusals, the module path's frontier, and the point of it all -- on a graph whose degrees divide
the fan-out the sampled forward IS full-neighbourhood inference, which the uniform sampler's is not."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import distinct_ref as dr
from conftest import pkg
from util import close

SEED = 0x0123456789ABCDEF
EINVAL = -1                         # GSAGE_EINVAL (include/gsage.h)
NS = [1, 2, 3, 10, 25]


# ---- host mode against the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_host_mode_equals_the_restatement(n):
    gs = pkg()
    g = dr.graph(n)
    adj = g.csr("cpu")
    ids = np.concatenate([dr.arranged(n), np.random.RandomState(n).randint(0, g.n, size=9)]).astype(np.int64)
    for g0, base, ctr in ((0, 0, None), (21 * n, 5, None), (21 * n, 2, torch.tensor([6], dtype=torch.int64))):
        ph = {"seed": SEED, "call_base": base, "g0": g0}
        if ctr is not None:
            ph["call_ctr"] = ctr
        got = gs.ops.sample_csr_distinct(adj, torch.from_numpy(ids), n, ph)
        ref, err = dr.sample(g.rowptr, g.col, g.n, ids, n, SEED, base + (6 if ctr is not None else 0), g0)
        assert err == 0 and got.dtype == torch.int64 and np.array_equal(got.numpy(), ref), (n, g0, base)
    # the key tag is the sampler's own: neither the uniform nor the weighted stream
    assert gs.ops.DISTINCT_TAG == dr.TAG == 0x44000000 != gs.ops.WEIGHTED_TAG
    with pytest.raises(IndexError):
        gs.ops.sample_csr_distinct(adj, torch.tensor([0, g.n]), n, {"seed": SEED})
    with pytest.raises(IndexError):
        gs.ops.sample_csr_distinct(adj, torch.tensor([-1]), n, {"seed": SEED})


@pytest.mark.parametrize("n", NS)
def test_properties_of_the_definition(n):
    g = dr.graph(n)
    ids = np.arange(g.n, dtype=np.int64)
    for call in (0, 3):
        for i, v in enumerate(ids):
            deg = int(g.deg[v])
            if deg == 0:
                out, _ = dr.sample(g.rowptr, g.col, g.n, [v], n, SEED, call, i * n)
                assert not out.any()
                continue
            off = dr.offsets(deg, n, [dr.word(SEED, call, i * n + j) for j in range(n)])
            assert all(0 <= o < deg for o in off)
            if deg > n:
                assert len(set(off)) == n, (v, deg, off)
            else:
                counts = np.bincount(off, minlength=deg)
                assert counts.min() >= 1 and counts.max() - counts.min() <= 1 and counts.sum() == n, (v, deg, off)


def test_uniform_over_ordered_triples():
    """deg = 5, n = 3: each of the 60 ordered triples within +-10 % of 2 000 over 120 000 parents (a condition, not a
    measurement: 4.5 standard deviations at 2 000)"""
    gs = pkg()
    rowptr = torch.tensor([0, 5], dtype=torch.int64)
    col = torch.arange(5, dtype=torch.int32)
    adj = gs.DeviceCSR(rowptr, col, 1, 5)
    out = gs.ops.sample_csr_distinct(adj, torch.zeros(120000, dtype=torch.int64), 3, {"seed": 20240607}).view(-1, 3).numpy()
    code = out[:, 0] * 25 + out[:, 1] * 5 + out[:, 2]
    counts = np.bincount(code, minlength=125)
    triples = [a * 25 + b * 5 + c for a, b, c in itertools.permutations(range(5), 3)]
    assert len(triples) == 60 and counts.sum() == counts[triples].sum() == 120000
    assert counts[triples].min() >= 1800 and counts[triples].max() <= 2200, (counts[triples].min(), counts[triples].max())


# ---- the entry points' refusals ------------------------------------------------------------------------------------
def _desc(gs, adj, ids, B=3, n_hops=2, fan=5):
    d = gs._native.HopsDesc()
    d.rowptr, d.col, d.n_rows = adj.rowptr.data_ptr(), adj.col.data_ptr(), adj.n_rows
    d.ids, d.B, d.n_hops = ids.data_ptr(), B, n_hops
    for k in range(5):
        d.fan[k] = fan
    d.max_deg, d.seed = 0, SEED                             # (max_deg is ignored)
    return d


def test_refusals_without_a_gpu():
    gs = pkg()
    nat = gs._native
    lib = nat.lib()
    adj = dr.graph(3).csr("cpu")
    ids = torch.zeros(3 * (1 + 5 + 25 + 125 + 625 + 3125), dtype=torch.int64)
    out = torch.zeros(64, dtype=torch.int64)
    rp, col, idp, op = adj.rowptr.data_ptr(), adj.col.data_ptr(), ids.data_ptr(), out.data_ptr()
    before = nat.launch_count()
    for n in (0, 257):
        assert lib.gsage_sample_csr_distinct(rp, col, adj.n_rows, idp, 4, n, SEED, None, 0, 0, op, None, None) == EINVAL
        assert b"n (samples per parent)" in lib.gsage_last_error() and b"1..256" in lib.gsage_last_error()
    assert lib.gsage_sample_csr_distinct(None, col, adj.n_rows, idp, 4, 3, SEED, None, 0, 0, op, None, None) == EINVAL
    assert b"rowptr" in lib.gsage_last_error()
    assert lib.gsage_sample_csr_distinct(rp, col, adj.n_rows, idp, 0, 3, SEED, None, 0, 0, op, None, None) == 0

    assert lib.gsage_sample_hops_distinct(None, None) == EINVAL and b"hops" in lib.gsage_last_error()
    d = _desc(gs, adj, ids)
    keep = torch.zeros(64, dtype=torch.int32)
    dense = torch.zeros(adj.n_rows, 4, dtype=torch.int64)
    d.sel = keep.data_ptr()
    assert lib.gsage_sample_hops_distinct(ctypes.addressof(d), None) == EINVAL and b"sel" in lib.gsage_last_error()
    d.sel = None
    d.dense_adj, d.dense_ld = dense.data_ptr(), 4
    assert lib.gsage_sample_hops_distinct(ctypes.addressof(d), None) == EINVAL and b"dense_adj" in lib.gsage_last_error()
    d.dense_adj, d.dense_ld = None, 0
    for n_hops in (0, 6):
        d.n_hops = n_hops
        assert lib.gsage_sample_hops_distinct(ctypes.addressof(d), None) == EINVAL
        assert b"n_hops" in lib.gsage_last_error()
    d.n_hops = 2
    for fan in (0, 257):
        d.fan[1] = fan
        assert lib.gsage_sample_hops_distinct(ctypes.addressof(d), None) == EINVAL
        assert b"fan[1]" in lib.gsage_last_error()
    d.n_hops = 3
    for k in range(3):
        d.fan[k] = 25                                      # 15 625 ids of one seed: 244 KiB of frontier
    assert lib.gsage_sample_hops_distinct(ctypes.addressof(d), None) == EINVAL
    assert b"fan[]" in lib.gsage_last_error() and b"LDS" in lib.gsage_last_error()
    d.n_hops, d.B = 2, 0                                   # no seeds: OK, and nothing is launched
    d.fan[0] = d.fan[1] = 5
    assert lib.gsage_sample_hops_distinct(ctypes.addressof(d), None) == 0
    assert nat.launch_count() == before
    with pytest.raises(AssertionError):
        gs.ops.sample_csr_distinct(adj, ids[:4], 257, {"seed": SEED})


@pytest.mark.parametrize("rank", [0, 1])
@pytest.mark.parametrize("B,fans", [(3, (5, 3)), (17, (4, 3, 2))])
def test_host_hops_equal_the_restatement_hop_after_hop(B, fans, rank):
    gs = pkg()
    g = dr.graph(fans[0])
    seeds = dr.parents(B, fans[0], np.random.RandomState(B))
    total = B + sum(B * int(np.prod(fans[:k])) for k in range(1, len(fans) + 1))
    ids = torch.zeros(total, dtype=torch.int64)
    ids[:B] = torch.from_numpy(seeds)
    got = gs.ops.sample_hops_distinct(g.csr("cpu"), ids, B, fans, {"seed": SEED, "call_base": 2, "rank": rank})
    ref, err = dr.sample_hops(g.rowptr, g.col, g.n, seeds, fans, SEED, 2, rank)
    assert got is ids and err == 0 and np.array_equal(got.numpy(), np.concatenate(ref))


# ---- registry, engine refusals -------------------------------------------------------------------------------------
def test_the_name_resolves_and_the_reference_table_is_unchanged():
    gs = pkg()
    cls = gs.find_sampler("sparse_distinct_neighbor_sampler")
    assert cls is gs.nn_modules.SparseDistinctNeighborSampler is gs.sampler_extensions["sparse_distinct_neighbor_sampler"]
    assert sorted(gs.sampler_lookup) == ["sparse_uniform_neighbor_sampler", "uniform_neighbor_sampler"]
    assert not issubclass(cls, gs.nn_modules.SparseUniformNeighborSampler)
    p = dr.problem(n=60)
    s = cls(p["adj"], seed=5)
    assert s.rng == "philox" and s.shard == (0, 1) and np.array_equal(s.degrees, np.diff(p["indptr"]))
    w = cls(gs.WeightedAdj(p["adj"], np.ones(p["adj"].nnz, dtype=np.float32)), seed=5)      # weights are ignored
    ids = torch.arange(0, 61, 3)
    assert torch.equal(s(ids, 4), w(ids, 4)) and s.calls == 1
    s.begin_capture(torch.tensor([3], dtype=torch.int64))
    a = s(ids, 4)
    assert s.calls_in_capture() == 1
    ref, _ = dr.sample(p["indptr"], p["data"], 61, ids.numpy(), 4, 5, 3, 0)
    assert np.array_equal(a.numpy(), ref)


def test_registry_and_engine_refusals():
    gs = pkg()
    p = dr.problem(n=60)
    cls = gs.engine.FusedDistinctMeanTrainStep
    assert cls not in gs.engine.ENGINES and issubclass(cls, gs.engine.FusedMeanTrainStep)
    assert cls.TIMED["sampler"] == (10, 11)
    model = dr.model(p, (16, 16), (4, 3))
    assert gs.engine.fused_engine_for(model, None) is None
    why = gs.engine.why_no_fused_engine(model, None)
    assert "SparseDistinctNeighborSampler" in why["FusedMeanTrainStep"]

    def sentence(m, **kw):
        s = cls.why_not(m, None, **kw)
        assert isinstance(s, str) and "\n" not in s
        return s

    assert "SparseUniformNeighborSampler" in sentence(dr.model(p, (16, 16), (4, 3), sampler="sparse_uniform_neighbor_sampler"))
    assert "not all mean aggregators" in sentence(dr.model(p, (16, 16), (4, 3), agg="max_pool"))
    assert "node_embedding" in sentence(dr.model(p, (16, 16), (4, 3), prep="node_embedding"))
    assert "pipelined=True" in sentence(model, pipelined=True)
    assert "data-parallel" in sentence(model, ddp=object())
    assert "FeatureStore" in sentence(model)              # the model alone passes: what is left is the feature store
    store = gs.FeatureStore.from_array(p["feats"], torch.device("cpu"), dtype="fp32").quantize()
    assert store.is_fp8 and "FP8" in cls.why_not(model, store)
    # the unsupervised engine answers with the sentence it has for a sampler it does not know
    specs = [{"n_train_samples": f, "n_val_samples": f, "output_dim": 16, "activation": a}
             for f, a in ((4, torch.nn.functional.relu), (3, lambda x: x))]
    unsup = gs.GSUnsupervised(sampler_class=cls_s(gs), adj=p["adj"], train_adj=p["adj"],
                              prep_class=gs.prep_lookup["identity"], aggregator_class=gs.aggregator_lookup["mean"],
                              input_dim=p["feats"].shape[1], n_nodes=61, layer_specs=specs)
    assert "SparseDistinctNeighborSampler" in gs.engine.FusedUnsupMeanTrainStep.why_not(unsup, None)
    loss = unsup.train_step(ids=torch.arange(1, 9), feats=torch.from_numpy(p["feats"]))       # the module path runs it
    assert np.isfinite(float(loss))


def cls_s(gs):
    return gs.find_sampler("sparse_distinct_neighbor_sampler")


# ---- the module path -----------------------------------------------------------------------------------------------
def test_cpu_train_step_draws_the_restatements_frontier():
    gs = pkg()
    gs.ops.set_compute_dtype("fp32")
    try:
        p = dr.problem(n=60)
        fans = (4, 3)
        model = dr.model(p, (8, 8), fans)
        model.train_sampler.seed = 77
        ids = torch.tensor([5, 9, 32, 1, 60, 17], dtype=torch.int64)
        cur, hops = ids, [ids]
        for fn in model.train_sample_fns:                       # what GSSupervised._encode asks its sampler for
            cur = fn(ids=cur)
            hops.append(cur.view(-1))
        ref, err = dr.sample_hops(p["indptr"], p["data"], 61, ids.numpy(), fans, 77, 0)
        assert err == 0 and np.array_equal(torch.cat(hops).numpy(), np.concatenate(ref))
        tg = torch.from_numpy(p["targets"][ids.numpy()])
        preds = model.train_step(ids=ids, feats=torch.from_numpy(p["feats"]), targets=tg,
                                 loss_fn=gs.ProblemLosses.classification)
        assert tuple(preds.shape) == (6, p["C"]) and bool(torch.isfinite(preds).all())
        assert model.train_sampler.calls == 4                   # two hops drawn above, two by the step
    finally:
        gs.ops.set_compute_dtype("bf16")


def test_sampled_forward_is_exact_where_degrees_divide_the_fanout():
    """degrees in {1, 2, 5, 10}, fan-outs (10, 10), fp32: the sampled forward under the distinct sampler equals
    full-neighbourhood inference at the bound tests/test_gpu_full_neighbour.py applies between a sampled anchor and
    the full path; under the uniform sampler it does not (the test bites)"""
    gs = pkg()
    gs.ops.set_compute_dtype("fp32")
    old = gs.nn_modules.SparseUniformNeighborSampler.rng_default
    gs.nn_modules.SparseUniformNeighborSampler.rng_default = "philox"
    try:
        p = dr.problem(n=120, degrees=(1, 2, 5, 10), seed=11)
        assert set(np.diff(p["indptr"])) == {1, 2, 5, 10}
        feats = torch.from_numpy(p["feats"])
        ids = torch.arange(0, 121, 3)
        model = dr.model(p, (16, 8), (10, 10))
        with torch.no_grad():
            sampled = model(ids, feats, train=False)
        full = gs.full_neighbour(model, feats, nodes=ids)
        close(sampled.numpy(), full.numpy(), "distinct sampler vs full neighbourhood", 2e-5, 2e-5)
        uniform = dr.model(p, (16, 8), (10, 10), sampler="sparse_uniform_neighbor_sampler")
        uniform.load_state_dict(model.state_dict())
        with torch.no_grad():
            noisy = uniform(ids, feats, train=False)
        with pytest.raises(AssertionError):
            close(noisy.numpy(), full.numpy(), "uniform sampler vs full neighbourhood", 2e-5, 2e-5)
    finally:
        gs.nn_modules.SparseUniformNeighborSampler.rng_default = old
        gs.ops.set_compute_dtype("bf16")
