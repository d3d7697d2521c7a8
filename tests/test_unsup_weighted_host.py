"""Without a GPU: weighted walks for unsupervised training -- ops.unsup_batch(weighted=True) in host mode against the
restatement of tests/unsup_weighted_ref.py bit for bit, the negatives' table of a weighted adjacency, the new entry
point's refusals before any launch, every sentence of FusedUnsupWeightedMeanTrainStep.why_not, and the command line:
--unsupervised --weighted-walks on the CPU, its refusals, and the refusal that stays without the flag."""
import importlib
import json
import math

import numpy as np
import pytest
import torch

import unsup_engine_ref as uref
import unsup_weighted_ref as ur
import weighted_ref as wr
from conftest import pkg

SEED = 0x1234567890ABCDEF


# ---- host mode -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk_len", [1, 5, 16])
@pytest.mark.parametrize("B", [1, 37])
def test_host_mode_equals_the_restatement(B, walk_len):
    gs = pkg()
    g = wr.graph()
    csr = g.csr("cpu")
    assert torch.equal(csr.edge_cdf, torch.from_numpy(g.cdf.view(np.int64)))
    cdf = gs.ops.neg_cdf(csr, weighted=True)
    Q, call = 20, 3
    seeds = ur.seeds_on_rows(g, B, np.random.RandomState(B + walk_len)) if B > 1 else np.asarray([wr.ROWS[1000]])
    ids, pw = gs.ops.unsup_batch(csr, torch.from_numpy(seeds), walk_len, Q, cdf, {"seed": SEED, "call_base": call},
                                 weighted=True)
    rid, rpw, err = ur.build_batch(g.rowptr, g.col, g.cdf, g.n, seeds, walk_len, Q, cdf.numpy(), SEED, call)
    assert err == 0
    assert torch.equal(ids, torch.from_numpy(rid)) and torch.equal(pw, torch.from_numpy(rpw))
    # a walk that starts on a row without a drawable edge stays there, whatever its length
    for name in ("degree 0", "all zero", "all zero, 300 edges"):
        for i in np.flatnonzero(seeds == wr.ROWS[name]):
            assert int(ids[B + i]) == wr.ROWS[name] and float(pw[i]) == 0.0
    # the steps are weighted ones: the unweighted builder over the same structure draws other positives
    if B > 1 and walk_len > 1:
        plain, _ = gs.ops.unsup_batch(csr, torch.from_numpy(seeds), walk_len, Q, cdf, {"seed": SEED, "call_base": call})
        assert not torch.equal(plain[B:2 * B], ids[B:2 * B]) and torch.equal(plain[2 * B:], ids[2 * B:])
    # shards concatenate, the counter adds to the base
    if B == 37:
        ph = {"seed": SEED, "call_base": 1, "g0": 13, "call_ctr": torch.tensor([2])}
        part, ppw = gs.ops.unsup_batch(csr, torch.from_numpy(seeds[13:]), walk_len, Q, cdf, ph, weighted=True)
        assert torch.equal(part[:24], ids[13:37]) and torch.equal(part[24:48], ids[B + 13:2 * B])
        assert torch.equal(ppw, pw[13:]) and torch.equal(part[48:], ids[2 * B:])


def test_host_mode_refusals():
    gs = pkg()
    g = wr.graph()
    plain = g.csr("cpu", weighted=False)
    seeds = torch.arange(4)
    with pytest.raises(ValueError, match="weighted=True needs an adjacency with edge weights"):
        gs.ops.unsup_batch(plain, seeds, 5, 3, gs.ops.neg_cdf(plain), {"seed": 0}, weighted=True)
    with pytest.raises(ValueError, match="weighted=True needs an adjacency with edge weights"):
        gs.ops.neg_cdf(plain, weighted=True)
    csr = g.csr("cpu")
    cdf = gs.ops.neg_cdf(csr, weighted=True)
    with pytest.raises(ValueError, match="walk_len"):
        gs.ops.unsup_batch(csr, seeds, 17, 3, cdf, {"seed": 0}, weighted=True)
    with pytest.raises(IndexError):
        gs.ops.unsup_batch(csr, torch.tensor([g.n]), 5, 3, cdf, {"seed": 0}, weighted=True)


def test_neg_cdf_weighted_zeroes_exactly_the_rows_without_a_drawable_edge():
    gs = pkg()
    g = wr.graph()
    csr = g.csr("cpu")
    plain, weighted = gs.ops.neg_cdf(csr), gs.ops.neg_cdf(csr, weighted=True)
    w_plain = np.diff(np.concatenate([[0.0], plain.numpy()]))
    w_weighted = np.diff(np.concatenate([[0.0], weighted.numpy()]))
    T = np.array([int(g.cdf[g.rowptr[v + 1] - 1]) if g.deg[v] else 0 for v in range(g.n)])
    dead = (g.deg > 0) & (T == 0)
    assert set(np.flatnonzero(dead)) == {wr.ROWS["all zero"], wr.ROWS["all zero, 12 edges"],
                                         wr.ROWS["all zero, 300 edges"]}
    assert (w_plain[dead] > 0).all() and (w_weighted[dead] == 0).all()
    assert np.allclose(w_weighted[~dead], g.deg[~dead].astype(np.float64) ** 0.75, rtol=1e-12, atol=0)
    assert np.array_equal(weighted.numpy(), ur.neg_table(g.rowptr, g.cdf))
    assert weighted._gsage_total == float(weighted[-1]) and torch.equal(gs.ops.neg_cdf(csr), plain)
    # so such a row is never a negative
    ids, _ = gs.ops.unsup_batch(csr, torch.arange(4), 1, 64, weighted, {"seed": 5}, weighted=True)
    assert not set(ids[8:].tolist()) & set(np.flatnonzero(dead)) and not set(ids[8:].tolist()) & {0, 11}


# ---- the entry point's refusals ----------------------------------------------------------------------------------------
def test_bad_arguments_return_einval_without_gpu():
    gs = pkg()
    nat = gs._native
    L = nat.lib()
    assert "gsage_unsup_batch_weighted" in nat.SIGNATURES and L.gsage_abi_version() == 6
    buf = np.zeros(4096, dtype=np.int64).ctypes.data
    call = lambda ecdf=buf, walk_len=5, Q=3, B=4, total=1.0, rowptr=buf: L.gsage_unsup_batch_weighted(      # noqa: E731
        rowptr, buf, ecdf, 10, buf, B, walk_len, Q, buf, total, 0, None, 0, 0, buf, buf, None, None)
    before = nat.launch_count()
    assert call(ecdf=None) == -1 and b"edge_cdf" in L.gsage_last_error()
    assert call(rowptr=None) == -1 and b"null pointer" in L.gsage_last_error()
    for wl in (0, 17):
        assert call(walk_len=wl) == -1 and b"walk_len" in L.gsage_last_error(), wl
    for total in (0.0, float("nan"), float("inf"), -1.0):
        assert call(total=total) == -1 and b"weights sum" in L.gsage_last_error(), total
    for kw in ({"Q": 0}, {"B": 0}, {"B": 1 << 31}):
        assert call(**kw) == -1 and b"bad sizes" in L.gsage_last_error(), kw
    assert nat.launch_count() == before


# ---- the model and the engine, without a device ------------------------------------------------------------------------
def _make(gs, p, weighted_walks, sampler="sparse_weighted_neighbor_sampler", agg="mean", prep="identity"):
    torch.manual_seed(3)
    wa = gs.WeightedAdj(p["adj"], p["weight"]) if "weighted" in sampler else p["adj"]
    return gs.GSUnsupervised(sampler_class=gs.find_sampler(sampler), adj=wa, train_adj=wa,
                             prep_class=gs.prep_lookup[prep], aggregator_class=gs.aggregator_lookup[agg],
                             input_dim=p["feats"].shape[1], n_nodes=201, layer_specs=uref.specs((32, 32), (5, 3)),
                             n_negatives=20, walk_len=5, weighted_walks=weighted_walks)


def test_model_builds_weighted_batches_on_the_host():
    gs = pkg()
    p = wr.weighted_problem()
    try:
        model, plain = _make(gs, p, True), _make(gs, p, False)
        assert "weighted_walks=True" in repr(model) and "weighted_walks" not in repr(plain)
        seeds = torch.arange(1, 41)
        csr = model.train_sampler.csr("cpu")
        ids, pw = model.build_batch(seeds)
        want = gs.ops.unsup_batch(csr, seeds, 5, 20, gs.ops.neg_cdf(csr, weighted=True), {"seed": 0, "call_base": 0},
                                  weighted=True)
        assert torch.equal(ids, want[0]) and torch.equal(pw, want[1]) and model._batch_calls == [0, 1]
        cdf = wr.build_cdf(p["indptr"], p["weight"].data.astype(np.float32))
        rid, rpw, err = ur.build_batch(p["indptr"], p["data"], cdf, 201, seeds.numpy(), 5, 20,
                                       ur.neg_table(p["indptr"], cdf), 0, 0)
        assert err == 0 and torch.equal(ids, torch.from_numpy(rid)) and torch.equal(pw, torch.from_numpy(rpw))
        # weighted_walks=False over the weighted sampler: today's uniform steps
        a = plain.build_batch(seeds)
        b = gs.ops.unsup_batch(csr, seeds, 5, 20, gs.ops.neg_cdf(csr), {"seed": 0, "call_base": 0})
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], ids)
        res = model.evaluate(seeds, torch.from_numpy(p["feats"]))
        assert math.isfinite(res["loss"]) and 0 < res["mrr"] <= 1 and model._batch_calls == [1, 1]
        # a sampler without a table
        with pytest.raises(ValueError, match="weighted_walks"):
            _make(gs, p, True, sampler="sparse_uniform_neighbor_sampler")
    finally:
        gs.nn_modules.SparseUniformNeighborSampler.rng_default = "compat"


def test_why_not_says_every_refusal_without_a_device():
    gs = pkg()
    cls = gs.engine.FusedUnsupWeightedMeanTrainStep
    assert issubclass(cls, gs.engine.FusedUnsupMeanTrainStep) and cls not in gs.engine.ENGINES
    p = wr.weighted_problem()
    store = gs.FeatureStore.from_array(p["feats"], torch.device("cpu"), dtype="bf16")
    ok = _make(gs, p, True)
    assert "HBM" in cls.why_not(ok, store) and not cls.supports(ok, store)        # only the device is missing
    # the parent keeps its sentence for the weighted sampler
    assert "the fused K1 draws uniformly" in gs.engine.FusedUnsupMeanTrainStep.why_not(ok, store)
    sup = gs.GSSupervised(sampler_class=gs.find_sampler("sparse_weighted_neighbor_sampler"),
                          adj=gs.WeightedAdj(p["adj"], p["weight"]), train_adj=gs.WeightedAdj(p["adj"], p["weight"]),
                          prep_class=gs.prep_lookup["identity"], aggregator_class=gs.aggregator_lookup["mean"],
                          input_dim=p["feats"].shape[1], n_nodes=201, n_classes=3, layer_specs=uref.specs((32, 32), (5, 3)))
    assert "not GSUnsupervised" in cls.why_not(sup, store)
    assert "weighted_walks=False" in cls.why_not(_make(gs, p, False), store)
    for agg in ("max_pool", "mean_pool", "attention", "lstm"):
        assert "aggregators other than mean" in cls.why_not(_make(gs, p, True, agg=agg), store), agg
    assert "node_embedding" in cls.why_not(_make(gs, p, True, prep="node_embedding"), store)
    uni = _make(gs, p, False, sampler="sparse_uniform_neighbor_sampler")
    uni.weighted_walks = True                                  # (the constructor refuses this pair: only why_not is asked)
    why = cls.why_not(uni, store)
    assert "not SparseWeightedNeighborSampler" in why and "SparseUniformNeighborSampler" in why
    mixed = _make(gs, p, True)
    mixed.val_sampler = uni.val_sampler
    assert "not SparseWeightedNeighborSampler" in cls.why_not(mixed, store)
    assert "data-parallel" in cls.why_not(ok, store, ddp=object())
    assert "pipelined" in cls.why_not(ok, store, pipelined=True)
    assert "eval_only" in cls.why_not(ok, store, eval_only=True)
    fp8 = gs.FeatureStore.from_array(p["feats"], torch.device("cpu"), dtype="fp8")
    assert "FP8" in cls.why_not(ok, fp8)
    assert "not a FeatureStore" in cls.why_not(ok, torch.from_numpy(p["feats"]))
    odd = _make(gs, p, True)
    odd.agg_layers[0].output_dim_ = 12
    assert "multiples of 8" in cls.why_not(odd, store)
    relu = _make(gs, p, True)
    relu.agg_layers[-1].activation = torch.nn.functional.relu
    assert "activations other than ReLU" in cls.why_not(relu, store)
    many = _make(gs, p, True)
    many.n_negatives = 65
    assert "64 negatives" in cls.why_not(many, store)
    # model reasons come before device reasons, and the constructor raises the same sentence
    assert "aggregators other than mean" in cls.why_not(_make(gs, p, True, agg="max_pool"), torch.from_numpy(p["feats"]))
    with pytest.raises(ValueError, match="weighted_walks=False"):
        cls(_make(gs, p, False), store, torch.arange(1, 9))
    with pytest.raises(ValueError, match="pipelined"):
        cls(ok, store, torch.arange(1, 9), pipelined=True)
    gs.nn_modules.SparseUniformNeighborSampler.rng_default = "compat"


# ---- the command line --------------------------------------------------------------------------------------------------
ARGV = ["--problem-path", "<memory>", "--no-cuda", "--epochs", "2", "--batch-size", "32", "--sampler-class",
        "sparse_weighted_neighbor_sampler", "--n-train-samples", "3,2", "--n-val-samples", "3,2", "--output-dims", "8,8",
        "--show-test", "--unsupervised"]


def _problem(gs, p, weighted=True):
    kw = dict(adj_weight=p["weight"], train_adj_weight=p["w"]) if weighted else {}
    return gs.NodeProblem.from_arrays("classification", p["C"], p["adj"], p["adj"].copy(), p["feats"], p["folds"],
                                      p["targets"], cuda=False, **kw)


def test_train_cli_on_the_cpu(capsys, tmp_path):
    gs = pkg()
    train = importlib.import_module("pytorch-graphsage_amd.train")
    p = wr.weighted_problem()

    def run(extra, argv=ARGV, weighted=True):
        train.main(argv + extra, problem=_problem(gs, p, weighted))
        cap = capsys.readouterr()
        return [json.loads(l) for l in cap.out.splitlines() if l.startswith("{")], cap.err

    uniform = ARGV[:ARGV.index("--sampler-class") + 1] + ["sparse_uniform_neighbor_sampler"] + \
        ARGV[ARGV.index("--sampler-class") + 2:]
    try:
        base, err = run(["--weighted-walks"])
        assert "weighted_walks=True" in err and "unsupervised model: module path" in err
        steps = [l for l in base if "epoch_progress" in l]
        assert len(steps) == 2 * (130 // 32 + 1) and all(math.isfinite(l["loss"]) for l in steps)
        assert 0 < base[-2]["mrr"] <= 1 and math.isfinite(base[-1]["test"]["loss"])
        strip = lambda ls: [{k: v for k, v in l.items() if k != "time"} for l in ls]       # noqa: E731
        assert strip(run(["--weighted-walks"])[0]) == strip(base)          # Philox from the seed: the run repeats itself
        # importance neighbourhoods reach the weighted sampler by the switch
        imp, err = run(["--weighted-walks", "--importance-walks", "20", "--importance-top", "4"], argv=uniform,
                       weighted=False)
        assert "becomes sparse_weighted_neighbor_sampler" in err and "weighted_walks=True" in err
        assert all(math.isfinite(l["loss"]) for l in imp if "epoch_progress" in l) and 0 < imp[-2]["mrr"] <= 1
        # the exports go through the weight-normalised mean: a max-pool model is refused with the existing sentence
        path = str(tmp_path / "emb.npy")
        run(["--weighted-walks", "--save-embeddings", path])
        assert np.load(path).shape == (201, 16)
        with pytest.raises(SystemExit, match="max-pool and attention") as e:
            run(["--weighted-walks", "--save-embeddings", path, "--aggregator-class", "max_pool"])
        assert "\n" not in str(e.value)
        # the new refusals, one line each
        with pytest.raises(SystemExit, match="--weighted-walks: the walks belong to --unsupervised") as e:
            run(["--weighted-walks"], argv=[a for a in ARGV if a != "--unsupervised"])
        assert "\n" not in str(e.value)
        with pytest.raises(SystemExit, match="--weighted-walks: needs the weighted sampler") as e:
            run(["--weighted-walks"], argv=uniform)
        assert "\n" not in str(e.value) and "sparse_uniform_neighbor_sampler" in str(e.value)
        with pytest.raises(SystemExit, match="--engine fused: FusedUnsupWeightedMeanTrainStep: features that are not") as e:
            run(["--weighted-walks", "--engine", "fused"])
        assert "\n" not in str(e.value)
        # without the flag: the pinned refusal, still one line, now with the hint
        with pytest.raises(SystemExit, match="^gsage: --unsupervised: the weighted sampler") as e:
            run([])
        assert "\n" not in str(e.value) and "--weighted-walks" in str(e.value)
        with pytest.raises(SystemExit, match="^gsage: --unsupervised: the weighted sampler") as e:
            run(["--importance-walks", "20", "--importance-top", "4"], argv=uniform, weighted=False)
        assert "\n" not in str(e.value)
    finally:
        gs.nn_modules.SparseUniformNeighborSampler.rng_default = "compat"
        gs.ops.set_compute_dtype("bf16")
