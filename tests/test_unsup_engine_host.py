"""Without a GPU: what the fused unsupervised engine (engine/unsup.py) can say of a model before a device is involved --
the masked skip-gram loss it trains under, every refusal of `why_not`, the new entry point's argument checks and the
command line's refusals."""
import importlib

import numpy as np
import pytest
import torch

import unsup_engine_ref as uref
import unsup_ref
import weighted_ref as wr
from conftest import pkg


def test_masked_loss_is_the_head_at_full_batches_and_the_live_mean_below():
    gs = pkg()
    torch.manual_seed(1)
    B, Q, D, nw = 17, 5, 24, 0.25
    E = torch.randn(2 * B + Q, D)
    pw = (torch.rand(B) > 0.2).float()
    host, haff = gs.ops._skipgram_host(E, B, Q, pw, nw)
    full, aff = uref.masked_loss(E.double(), B, Q, pw, nw, B)
    assert abs(float(full) - float(host)) <= 1e-6 * abs(float(host))
    assert float((aff - haff.double()).abs().max()) <= 1e-6
    rl, _, rdE = unsup_ref.head(E, B, Q, pw, nw)
    ml, _, mdE = uref.masked_head(E, B, Q, pw, nw, B)
    assert abs(float(ml) - float(rl)) <= 1e-12 and float((mdE - rdE).abs().max()) <= 1e-12
    for b in (B - 1, 2, 1):
        # the live seeds alone, as a batch of their own: [seeds[:b] | positives[:b] | negatives]
        sub = torch.cat([E[:b], E[B:B + b], E[2 * B:]])
        want, _ = gs.ops._skipgram_host(sub, b, Q, pw[:b], nw)
        got, _, dE = uref.masked_head(E, B, Q, pw, nw, b)
        assert abs(float(got) - float(want)) <= 1e-6 * abs(float(want))
        assert bool((dE[b:B] == 0).all()) and bool((dE[B + b:2 * B] == 0).all())
        # ... which is not the 1/B-normalised sum over the live seeds
        assert abs(float(got) * b / B - float(want)) > 1e-3 * abs(float(want))


def _dense_adj(n, K=6):
    rng = np.random.RandomState(0)
    return torch.from_numpy(rng.randint(1, n, size=(n, K))).long()


def test_why_not_says_every_refusal_without_a_device():
    gs = pkg()
    cls = gs.engine.FusedUnsupMeanTrainStep
    adj, feats, _ = uref.problem()
    D = feats.shape[1]
    store = gs.FeatureStore.from_array(feats, torch.device("cpu"), dtype="bf16")
    ok = uref.make_model(gs, adj, D)
    # a model the engine covers: only the device is missing, and that is said last
    assert "HBM" in cls.why_not(ok, store)
    assert not cls.supports(ok, store)
    # not a GSUnsupervised
    sup = gs.GSSupervised(sampler_class=lambda adj: gs.nn_modules.SparseUniformNeighborSampler(adj, rng="philox"), adj=adj,
                          train_adj=adj, prep_class=gs.prep_lookup["identity"],
                          aggregator_class=gs.aggregator_lookup["mean"], input_dim=D, n_nodes=adj.shape[0], n_classes=3,
                          layer_specs=uref.specs((32, 32), (5, 3)))
    assert "not GSUnsupervised" in cls.why_not(sup, store)
    # aggregators
    for agg in ("max_pool", "mean_pool", "attention", "lstm"):
        why = cls.why_not(uref.make_model(gs, adj, D, agg=agg), store)
        assert "aggregators other than mean" in why, (agg, why)
    # prep
    why = cls.why_not(uref.make_model(gs, adj, D, prep="node_embedding"), store)
    assert "node_embedding" in why
    # the FP8 store
    fp8 = gs.FeatureStore.from_array(feats, torch.device("cpu"), dtype="fp8")
    assert "FP8" in cls.why_not(ok, fp8)
    # samplers: dense, weighted, compat
    n = adj.shape[0]
    dense = uref.make_model(gs, _dense_adj(n), D, sampler=gs.sampler_lookup["uniform_neighbor_sampler"], n_nodes=n)
    assert "dense sampler" in cls.why_not(dense, store)
    p = wr.weighted_problem()
    wa = gs.WeightedAdj(p["adj"], p["weight"])
    weighted = uref.make_model(gs, wa, p["feats"].shape[1], sampler=gs.find_sampler("sparse_weighted_neighbor_sampler"),
                               n_nodes=201)
    assert "weighted sampler" in cls.why_not(weighted, store)
    why = cls.why_not(uref.make_model(gs, adj, D, rng="compat"), store)
    assert "philox" in why and "padded rows" in why
    # modes
    assert "data-parallel" in cls.why_not(ok, store, ddp=object())
    assert "pipelined" in cls.why_not(ok, store, pipelined=True)
    assert "eval_only" in cls.why_not(ok, store, eval_only=True)
    # model reasons come before device reasons: a CPU store does not hide them
    assert "philox" in cls.why_not(uref.make_model(gs, adj, D, rng="compat"), torch.from_numpy(feats))
    # the constructor raises the same sentence
    with pytest.raises(ValueError, match="aggregators other than mean"):
        cls(uref.make_model(gs, adj, D, agg="max_pool"), store, torch.arange(1, 9))
    with pytest.raises(ValueError, match="pipelined"):
        cls(ok, store, torch.arange(1, 9), pipelined=True)
    # the supervised engines keep their answers for the models they cover (head hooks only moved)
    assert gs.engine.FusedMeanTrainStep.head_why_not(sup, gs.ProblemLosses.classification, torch.zeros(1).long(), 64,
                                                     True) is None
    assert cls.head_why_not(ok, None, None, 64, True) is None


def test_live_head_bad_arguments_return_einval_without_gpu():
    gs = pkg()
    L = gs._native.lib()
    nat = gs._native
    assert "gsage_head_skipgram_live" in nat.SIGNATURES and L.gsage_abi_version() == 6
    buf = (np.zeros(4096, dtype=np.float32)).ctypes.data
    call = lambda E=buf, B=4, Q=3, D=8, lde=8, ldd=8, dt=nat.F32, pw=buf, dE=buf, loss=buf, scr=buf: \
        L.gsage_head_skipgram_live(E, lde, B, Q, D, pw, 1.0, None, dE, dt, ldd, loss, None, scr, None)        # noqa: E731
    before = nat.launch_count()
    for kw in ({"E": None}, {"pw": None}, {"dE": None}, {"loss": None}, {"scr": None}):
        assert call(**kw) == -1 and b"null pointer" in L.gsage_last_error(), kw
    for kw in ({"Q": 65}, {"Q": 0}, {"D": 1025}, {"D": 0}, {"B": 0}):
        assert call(**kw) == -1 and b"n_negatives" in L.gsage_last_error(), kw
    for kw in ({"lde": 7}, {"ldd": 7}):
        assert call(**kw) == -1 and b"leading" in L.gsage_last_error(), kw
    assert call(dt=nat.FP8) == -1 and b"dtype" in L.gsage_last_error()
    assert nat.launch_count() == before


def _specs_argv():
    return ["--problem-path", "<memory>", "--no-cuda", "--epochs", "1", "--batch-size", "64", "--sampler-class",
            "sparse_uniform_neighbor_sampler", "--n-train-samples", "5,3", "--n-val-samples", "5,3", "--output-dims",
            "32,32", "--unsupervised", "--engine", "fused"]


def test_train_refuses_the_fused_unsupervised_run_with_the_engines_sentence():
    gs = pkg()
    p = unsup_ref.model_problem()
    problem = gs.NodeProblem.from_arrays("classification", 3, p["adj"], p["adj"], p["feats"], p["folds"], p["targets"],
                                         cuda=False)
    train = importlib.import_module("pytorch-graphsage_amd.train")
    with pytest.raises(SystemExit, match=r"--engine fused: .*--rng philox"):
        train.main(_specs_argv(), problem=problem)                      # the default --rng compat
    with pytest.raises(SystemExit, match="--engine fused: aggregators other than mean"):
        train.main(_specs_argv() + ["--rng", "philox", "--aggregator-class", "max_pool"], problem=problem)
    with pytest.raises(SystemExit, match="--engine fused: features that are not a FeatureStore"):
        train.main(_specs_argv() + ["--rng", "philox"], problem=problem)     # everything but the device
