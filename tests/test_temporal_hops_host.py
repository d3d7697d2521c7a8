"""Without a GPU: ops.sample_hops_temporal in host mode against the serial restatement of tests/temporal_ref.py (ids and
times, torch.equal), its call counter / base / rank arithmetic, every GSAGE_EINVAL of gsage_sample_hops_temporal through
ctypes, what FusedTemporalMeanTrainStep.why_not can say without a device, and train.py --no-cuda --engine fused."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import temporal_engine_ref as ter
import temporal_ref as tr
from conftest import pkg

SEED = ter.SEED
EINVAL = -1                         # GSAGE_EINVAL (include/gsage.h)
SHAPES = [(1, (3,)), (5, (25, 10)), (33, (5, 3)), (3, (2, 2, 2, 2, 2))]


def _buffer(seeds, fans):
    ids = torch.full((sum(ter.sizes(len(seeds), fans)),), -7, dtype=torch.int64)
    ids[:len(seeds)] = torch.from_numpy(np.asarray(seeds, dtype=np.int64))
    return ids


# ---- host mode against the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("strategy,inherit", ter.PAIRS)
@pytest.mark.parametrize("B,fans", SHAPES)
def test_host_mode_equals_the_restatement(B, fans, strategy, inherit):
    gs = pkg()
    adj = tr.graph().csr("cpu")
    seeds, times = tr.parents(B)
    ids, out_t = gs.ops.sample_hops_temporal(adj, _buffer(seeds, fans), torch.from_numpy(times), B, fans,
                                             {"seed": SEED, "call_base": 3}, strategy=strategy, inherit=inherit)
    ref, ref_t, err = ter.graph_frontier(seeds, times, fans, 3, strategy, inherit)
    assert err == 0 and ids.dtype == out_t.dtype == torch.int64
    assert torch.equal(ids, torch.from_numpy(ref)) and torch.equal(out_t, torch.from_numpy(ref_t))
    # a buffer of the caller's for the times is the one that comes back
    mine = torch.zeros_like(ids)
    _, again = gs.ops.sample_hops_temporal(adj, _buffer(seeds, fans), torch.from_numpy(times), B, fans,
                                           {"seed": SEED, "call_base": 3}, strategy=strategy, inherit=inherit, out_times=mine)
    assert again is mine and torch.equal(mine, out_t)


def test_call_counter_and_base():
    gs = pkg()
    adj = tr.graph().csr("cpu")
    B, fans = 3, (5, 3)
    seeds, times = tr.parents(B)
    ctr = torch.tensor([6], dtype=torch.int64)
    ids, out_t = gs.ops.sample_hops_temporal(adj, _buffer(seeds, fans), torch.from_numpy(times), B, fans,
                                             {"seed": SEED, "call_base": 2, "call_ctr": ctr}, inherit="edge")
    ref, ref_t, _ = ter.graph_frontier(seeds, times, fans, 8, "uniform", "edge")
    assert torch.equal(ids, torch.from_numpy(ref)) and torch.equal(out_t, torch.from_numpy(ref_t)) and int(ctr.item()) == 6


def test_rank_offsets_the_global_sample_index():
    """rank 1 with B seeds = rows [B, 2B) of every hop of a rank-0 run over 2B seeds whose second half they are"""
    gs = pkg()
    adj = tr.graph().csr("cpu")
    B, fans = 6, (4, 3, 2)
    ids2, times2 = (a[56:56 + 2 * B] for a in tr.parents())   # times above every edge: the draws decide the children
    tm2 = torch.from_numpy(times2)
    one, one_t = gs.ops.sample_hops_temporal(adj, _buffer(ids2[B:], fans), tm2[B:], B, fans, {"seed": SEED, "rank": 1},
                                             inherit="edge")
    two, two_t = gs.ops.sample_hops_temporal(adj, _buffer(ids2, fans), tm2, 2 * B, fans, {"seed": SEED}, inherit="edge")
    o1 = o2 = 0
    for s in ter.sizes(B, fans):
        assert torch.equal(one[o1:o1 + s], two[o2 + s:o2 + 2 * s]) and torch.equal(one_t[o1:o1 + s], two_t[o2 + s:o2 + 2 * s])
        o1, o2 = o1 + s, o2 + 2 * s
    zero, _ = gs.ops.sample_hops_temporal(adj, _buffer(ids2[B:], fans), tm2[B:], B, fans, {"seed": SEED}, inherit="edge")
    assert not torch.equal(zero, one)                         # (the rank does reach the words)


def test_ops_refusals():
    gs = pkg()
    adj = tr.graph().csr("cpu")
    seeds, times = tr.parents(2)
    args = (_buffer(seeds, (3,)), torch.from_numpy(times), 2, (3,), {"seed": SEED})
    with pytest.raises(ValueError, match=r"unknown strategy 'latest' \(known: uniform, recent\)"):
        gs.ops.sample_hops_temporal(adj, *args, strategy="latest")
    with pytest.raises(ValueError, match=r"unknown inherit rule 'parent' \(known: seed, edge\)"):
        gs.ops.sample_hops_temporal(adj, *args, inherit="parent")
    plain = gs.DeviceCSR(adj.rowptr, adj.col, adj.n_rows, adj.max_deg)
    with pytest.raises(ValueError, match="no edge times"):
        gs.ops.sample_hops_temporal(plain, *args)


# ---- the C entry's refusals ------------------------------------------------------------------------------------------
def test_entry_refusals_without_a_gpu():
    gs = pkg()
    nat = gs._native
    lib = nat.lib()
    adj = tr.graph().csr("cpu")
    B, fans = 2, (3, 2)
    ids = _buffer([1, 2], fans)
    tm = torch.zeros(B, dtype=torch.int64)
    tq = torch.zeros(3, B, dtype=torch.int64)
    sq = torch.zeros(3, B, dtype=torch.int64)
    bidx = torch.zeros(1, dtype=torch.int64)
    sel = torch.zeros(64, dtype=torch.int32)
    out_t = torch.zeros_like(ids)
    et = adj.etime.data_ptr()

    def desc(**kw):
        d = nat.HopsDesc()
        d.rowptr, d.col, d.n_rows = adj.rowptr.data_ptr(), adj.col.data_ptr(), adj.n_rows
        d.ids, d.B, d.n_hops = ids.data_ptr(), B, len(fans)
        for k in range(5):
            d.fan[k] = fans[k] if k < len(fans) else 1
        d.max_deg, d.seed = 0, SEED                            # (max_deg is ignored)
        for k, v in kw.items():
            if k == "fan":
                for i, n in enumerate(v):
                    d.fan[i] = n
            else:
                setattr(d, k, v)
        return d

    def call(d, etime=et, times=tm.data_ptr(), time_queue=None, strategy=0, inherit=0, null_desc=False):
        return lib.gsage_sample_hops_temporal(None if null_desc else ctypes.addressof(d), etime, times, time_queue,
                                              strategy, inherit, out_t.data_ptr(), None)

    queue = dict(seed_queue=sq.data_ptr(), batch_idx=bidx.data_ptr(), n_batches=3)
    before = nat.launch_count()
    cases = [
        (desc(), dict(null_desc=True), b"hops"),
        (desc(), dict(etime=None), b"etime"),
        (desc(rowptr=None), {}, b"rowptr"),
        (desc(col=None), {}, b"col"),
        (desc(ids=None), {}, b"ids"),
        (desc(sel=sel.data_ptr()), {}, b"sel"),
        (desc(dense_adj=sq.data_ptr(), dense_ld=2), {}, b"dense_adj"),
        (desc(n_hops=0), {}, b"n_hops"),
        (desc(n_hops=6), {}, b"n_hops"),
        (desc(fan=(3, 0)), {}, b"fan[1]"),
        (desc(fan=(-1, 2)), {}, b"fan[0]"),
        (desc(), dict(strategy=2), b"strategy"),
        (desc(), dict(strategy=-1), b"strategy"),
        (desc(), dict(inherit=2), b"inherit"),
        (desc(), dict(times=None), b"times"),
        (desc(), dict(time_queue=tq.data_ptr()), b"time_queue"),
        (desc(**queue), dict(time_queue=None), b"time_queue"),
        (desc(n_hops=3, fan=(100, 100, 100)), {}, b"does not fit the LDS"),
    ]
    for d, kw, word in cases:
        assert call(d, **kw) == EINVAL and word in lib.gsage_last_error() and \
            b"sample_hops_temporal" in lib.gsage_last_error(), (kw, word, lib.gsage_last_error())
    assert call(desc(B=0)) == 0                               # B == 0: OK, nothing is launched
    assert call(desc(B=0, **queue), times=None, time_queue=tq.data_ptr()) == 0
    assert nat.launch_count() == before


# ---- the engine's refusals that need no device -------------------------------------------------------------------------
def test_why_not_without_a_device():
    gs = pkg()
    CLS = gs.engine.FusedTemporalMeanTrainStep
    assert CLS not in gs.engine.ENGINES and CLS.TIMED["sampler"] == (10, 11)
    p = ter.problem()
    model = ter.model(p, (16, 8), (5, 3))
    store = gs.FeatureStore.from_array(p["feats"], torch.device("cpu"), dtype="fp32")
    old = gs.nn_modules.SparseUniformNeighborSampler.rng_default
    gs.nn_modules.SparseUniformNeighborSampler.rng_default = "philox"
    try:
        uniform = tr.model(p, (16, 8), (5, 3), sampler="sparse_uniform_neighbor_sampler", adj=p["adj"])
    finally:
        gs.nn_modules.SparseUniformNeighborSampler.rng_default = old
    why = CLS.why_not(uniform, store)
    assert "SparseUniformNeighborSampler" in why and "not SparseTemporalNeighborSampler" in why and "\n" not in why
    why = CLS.why_not(model, store, pipelined=True)
    assert "pipelined=True" in why and "temporal engine" in why
    why = CLS.why_not(model, store, ddp=object())
    assert "data-parallel" in why and "temporal engine" in why
    why = CLS.why_not(model, store.quantize())
    assert "FP8" in why and "temporal engine" in why
    # what is left is the mean engine's own word on a store that is not in HBM: said last, after the model's
    assert "HBM" in CLS.why_not(model, store)
    # the two samplers may differ in strategy and rule: each launch reads its own sampler's
    assert CLS.why_not(ter.model(p, (16, 8), (5, 3), val=("recent", "edge")), store) == CLS.why_not(model, store)
    with pytest.raises(ValueError) as e:
        CLS(uniform, store, gs.ProblemLosses.classification, torch.zeros(4, dtype=torch.int64),
            torch.zeros(4, 1, dtype=torch.int64))
    assert CLS.why_not(uniform, store) in str(e.value)
    assert gs.engine.fused_engine_for(model, store) is None


# ---- train.py ------------------------------------------------------------------------------------------------------
def test_train_cli_no_cuda_engine_fused_keeps_its_words():
    gs = pkg()
    train = importlib.import_module("pytorch-graphsage_amd.train")
    p = tr.problem()
    folds = np.array(["train"] * 40 + ["val"] * 11 + ["test"] * 10)
    problem = gs.NodeProblem.from_arrays("classification", p["C"], p["adj"], p["adj"], p["feats"], folds, p["targets"],
                                         cuda=False, adj_time=p["time"], train_adj_time=p["time"],
                                         node_time=np.full(p["n"] + 1, tr.T_SNAP))
    try:
        with pytest.raises(SystemExit) as e:
            train.main(["--problem-path", "<memory>", "--no-cuda", "--epochs", "1", "--batch-size", "16",
                        "--n-train-samples", "3,2", "--n-val-samples", "3,2", "--output-dims", "8,8", "--rng", "philox",
                        "--precision", "fp32", "--sampler-class", "sparse_temporal_neighbor_sampler", "--engine", "fused"],
                       problem=problem)
        msg = str(e.value)
        assert "sparse_temporal_neighbor_sampler" in msg and "--engine fused" in msg and "no fused engine covers" in msg
        assert "--no-cuda" in msg and "\n" not in msg
    finally:
        gs.nn_modules.SparseUniformNeighborSampler.rng_default = "compat"
        gs.nn_modules.SparseTemporalNeighborSampler.strategy_default = "uniform"
        gs.nn_modules.SparseTemporalNeighborSampler.inherit_default = "seed"
        gs.ops.set_compute_dtype("bf16")
