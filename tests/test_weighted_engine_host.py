"""The fused engine over weighted adjacencies, without a GPU: the entry point's symbol and refusals, host mode of
ops.sample_hops_weighted against the restatement of tests/weighted_ref.py applied hop after hop (bit for bit), the
registry (the engine is opt-in) and the engine's refusals, one sentence each."""
import ctypes

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import weighted_ref as wr
from conftest import pkg

SEED = 0x0123456789ABCDEF
EINVAL = -1                         # GSAGE_EINVAL (include/gsage.h)


def _desc(gs, g, n_hops=2, B=3):
    nat = gs._native
    adj = g.csr("cpu")
    ids = torch.zeros(B * (1 + 5 + 25 + 125 + 625 + 3125), dtype=torch.int64)
    d = nat.HopsDesc()
    d.rowptr, d.col, d.n_rows = adj.rowptr.data_ptr(), adj.col.data_ptr(), adj.n_rows
    d.ids, d.B, d.n_hops = ids.data_ptr(), B, n_hops
    for k in range(5):
        d.fan[k] = 5
    d.max_deg, d.seed = 1, SEED
    return d, adj, ids


def test_symbol_and_refusals():
    gs = pkg()
    nat = gs._native
    lib = nat.lib()
    assert hasattr(lib, "gsage_sample_hops_weighted")
    g = wr.graph()
    d, adj, ids = _desc(gs, g)
    cdf = adj.edge_cdf.data_ptr()
    keep = torch.zeros(64, dtype=torch.int32)
    dense = torch.zeros(g.n, 4, dtype=torch.int64)
    before = nat.launch_count()
    assert lib.gsage_sample_hops_weighted(None, cdf, None) == EINVAL
    assert lib.gsage_sample_hops_weighted(ctypes.addressof(d), None, None) == EINVAL
    d.sel = keep.data_ptr()
    assert lib.gsage_sample_hops_weighted(ctypes.addressof(d), cdf, None) == EINVAL
    d.sel = None
    d.dense_adj, d.dense_ld = dense.data_ptr(), 4
    assert lib.gsage_sample_hops_weighted(ctypes.addressof(d), cdf, None) == EINVAL
    d.dense_adj, d.dense_ld = None, 0
    for n_hops in (0, 6):
        d.n_hops = n_hops
        assert lib.gsage_sample_hops_weighted(ctypes.addressof(d), cdf, None) == EINVAL
    d.n_hops, d.B = 2, 0                                   # no seeds: OK, and nothing is launched
    assert lib.gsage_sample_hops_weighted(ctypes.addressof(d), cdf, None) == 0
    assert nat.launch_count() == before


def _restatement(g, seeds, fans, seed, call_base, rank):
    hops = [np.asarray(seeds, dtype=np.int64)]
    for k, n in enumerate(fans, 1):
        out, err = wr.sample(g.rowptr, g.col, g.cdf, g.n, hops[-1], n, seed, call_base + k - 1,
                             rank * len(hops[-1]) * n)
        assert err == 0
        hops.append(out)
    return np.concatenate(hops)


@pytest.mark.parametrize("rank", [0, 1])
@pytest.mark.parametrize("B,fans", [(3, (5, 3)), (17, (4, 3, 2))])
def test_host_mode_equals_the_restatement_hop_after_hop(B, fans, rank):
    gs = pkg()
    g = wr.graph()
    adj = g.csr("cpu")
    rng = np.random.RandomState(B)
    seeds = rng.randint(0, g.n, size=B)
    seeds[:3] = [wr.ROWS[1000], wr.ROWS["degree 0"], wr.ROWS["all zero, 300 edges"]]
    total = B + sum(B * int(np.prod(fans[:k])) for k in range(1, len(fans) + 1))
    for base, ctr in ((0, None), (2, torch.tensor([6], dtype=torch.int64))):
        ids = torch.zeros(total, dtype=torch.int64)
        ids[:B] = torch.from_numpy(seeds)
        ph = {"seed": SEED, "call_base": base, "rank": rank}
        if ctr is not None:
            ph["call_ctr"] = ctr
        got = gs.ops.sample_hops_weighted(adj, ids, B, fans, ph)
        assert got is ids
        ref = _restatement(g, seeds, fans, SEED, base + (6 if ctr is not None else 0), rank)
        assert np.array_equal(got.numpy(), ref)
    with pytest.raises(ValueError, match="no edge weights"):
        gs.ops.sample_hops_weighted(g.csr("cpu", weighted=False), ids, B, fans, {"seed": SEED})


def _model(gs, p, agg="mean", prep="identity", sampler="sparse_weighted_neighbor_sampler", dims=(16, 16), fan=(4, 3)):
    torch.manual_seed(0)
    specs = [{"n_train_samples": f, "n_val_samples": f, "output_dim": h,
              "activation": (lambda x: x) if i == len(dims) - 1 else F.relu} for i, (f, h) in enumerate(zip(fan, dims))]
    wa = gs.WeightedAdj(p["adj"], p["weight"])
    return gs.GSSupervised(sampler_class=gs.find_sampler(sampler), adj=wa, train_adj=wa,
                           prep_class=gs.prep_lookup[prep], aggregator_class=gs.aggregator_lookup[agg],
                           input_dim=p["feats"].shape[1] if prep == "identity" else None, n_nodes=201,
                           n_classes=p["C"], layer_specs=specs)


def test_registry_and_refusals():
    gs = pkg()
    p = wr.weighted_problem()
    cls = gs.engine.FusedWeightedMeanTrainStep
    assert cls not in gs.engine.ENGINES and issubclass(cls, gs.engine.FusedMeanTrainStep)
    model = _model(gs, p)
    why = gs.engine.why_no_fused_engine(model, None)
    assert "SparseWeightedNeighborSampler" in why["FusedMeanTrainStep"]
    assert gs.engine.fused_engine_for(model, None) is None

    def sentence(m, **kw):
        s = cls.why_not(m, None, **kw)
        assert isinstance(s, str) and "\n" not in s
        return s

    assert "SparseUniformNeighborSampler" in sentence(_model(gs, p, sampler="sparse_uniform_neighbor_sampler"))
    assert "not all mean aggregators" in sentence(_model(gs, p, agg="max_pool"))
    assert "node_embedding" in sentence(_model(gs, p, prep="node_embedding"))
    assert "pipelined=True" in sentence(model, pipelined=True)
    assert "data-parallel" in sentence(model, ddp=object())
    # the model alone passes: what is left to say is about the feature store
    assert "FeatureStore" in sentence(model)
