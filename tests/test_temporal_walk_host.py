"""Temporal walks without a GPU (include/gsage.h, "Temporal walks"): host-mode ops.unsup_batch_temporal against the
restatement of tests/temporal_walk_ref.py bit for bit, the properties of the definition, the snapshot equivalence, the
negatives, padding and shards; GSUnsupervised(temporal_walks=True) in host mode; train.py's new flags."""
import importlib
import json

import numpy as np
import pytest
import torch

import temporal_ref as tr
import temporal_walk_ref as twr
from conftest import pkg

INT64_MAX = tr.INT64_MAX


def _philox(**kw):
    ph = {"seed": twr.SEED, "call_base": twr.CALL_BASE, "g0": twr.G0,
          "call_ctr": torch.tensor([twr.CALL_CTR], dtype=torch.int64)}
    ph.update(kw)
    return ph


def _host(M, walk_len, Q, rule, n_valid=None, csr=None, seeds=None, times=None, **ph):
    gs = pkg()
    if seeds is None:
        seeds, times = tr.parents(M)
    csr = tr.graph().csr() if csr is None else csr
    return gs.ops.unsup_batch_temporal(csr, torch.from_numpy(np.asarray(seeds)), torch.from_numpy(np.asarray(times)),
                                       walk_len, Q, twr.table(), _philox(**ph), inherit=rule, n_valid=n_valid)


def _same(got, ref):
    ids, pw, ot = got
    assert ids.dtype == torch.int64 and pw.dtype == torch.float32 and ot.dtype == torch.int64
    assert np.array_equal(ids.numpy(), ref[0]) and np.array_equal(pw.numpy(), ref[1]) and np.array_equal(ot.numpy(), ref[2])


# ---- the definition -------------------------------------------------------------------------------------------------
def test_the_tag_is_new_and_the_table_is_the_timeless_one():
    gs = pkg()
    assert gs.ops.UNSUP_TAG_TSTEP == twr.TAG_TSTEP == 0x56000000
    others = {gs.ops.UNSUP_TAG_LEN, gs.ops.UNSUP_TAG_STEP, gs.ops.UNSUP_TAG_NEG, gs.ops.UNSUP_TAG_WSTEP, gs.ops.TEMPORAL_TAG,
              gs.ops.WEIGHTED_TAG, gs.ops.DISTINCT_TAG, gs.ops.IMPORTANCE_TAG, gs.ops.WALK_BIAS_TAG}
    assert all((t >> 24) != 0x56 for t in others)
    cdf = gs.ops.neg_cdf(tr.graph().csr())                  # degree^0.75 of the timeless degrees
    assert np.allclose(cdf.numpy(), twr.degree_cdf(), rtol=1e-12, atol=0)


@pytest.mark.parametrize("rule", twr.RULES)
@pytest.mark.parametrize("Q", twr.QS)
@pytest.mark.parametrize("walk_len", twr.WALK_LENS)
@pytest.mark.parametrize("M", twr.MS)
def test_host_mode_equals_the_restatement(M, walk_len, Q, rule):
    ref = twr.reference(M, walk_len, Q, rule)
    assert ref[3] == 0
    _same(_host(M, walk_len, Q, rule), ref)
    nv = twr.n_valid_of(M, walk_len, Q, rule)
    _same(_host(M, walk_len, Q, rule, n_valid=nv), twr.reference(M, walk_len, Q, rule, nv))


@pytest.mark.parametrize("rule", twr.RULES)
def test_every_live_count(rule):
    M, Q = 17, 20
    _, times = tr.parents(M)
    for nv in (None, 1, 2, M - 1, M, M + 5, 0, -3):
        got = _host(M, 5, Q, rule, n_valid=nv)
        _same(got, twr.reference(M, 5, Q, rule, nv))
        b = M if nv is None else min(max(nv, 1), M)
        assert np.array_equal(got[2][2 * M:].numpy(), times[np.arange(Q) % b])
    # a tensor of one element is the device word's host form
    _same(_host(M, 5, Q, rule, n_valid=torch.tensor([2], dtype=torch.int32)), twr.reference(M, 5, Q, rule, 2))


@pytest.mark.parametrize("rule", twr.RULES)
def test_properties_of_the_trace(rule):
    g = tr.graph()
    early = steps = 0
    for M in (84, 257):
        ids, pw, ot, err, traces = twr.reference(M, 16, 20, rule)
        seeds, times = tr.parents(M)
        assert len(traces) == M
        for i, trace in enumerate(traces):
            assert 1 <= len(trace) <= 16 and trace[0][0] == seeds[i] and trace[0][1] == times[i]
            for k, (v, tau, cnt, off) in enumerate(trace):
                beg = int(g.rowptr[v])
                if cnt == 0:                                 # cnt == 0 ends the walk, at v
                    assert k == len(trace) - 1 and off is None and ids[M + i] == v
                    early += k > 0 or len(trace) == 1
                    continue
                steps += 1
                assert 0 <= off < cnt and int(g.etime[beg + off]) < tau       # every walked edge happened before tau
                if k + 1 < len(trace):
                    nxt = trace[k + 1]
                    assert nxt[0] == int(g.col[beg + off])
                    if rule == "edge":                       # times strictly decrease along the walk
                        assert nxt[1] == int(g.etime[beg + off]) < tau
                    else:
                        assert nxt[1] == times[i]
            assert ot[i] == ot[M + i] == times[i]
            assert pw[i] == (0.0 if ids[M + i] == seeds[i] else 1.0)
    assert early > 10 and steps > 100                        # the grid holds both walks that end early and long ones


@pytest.mark.parametrize("rule", twr.RULES)
def test_properties_of_one_step_on_the_outputs_alone(rule):
    g = tr.graph()
    M = 257
    seeds, times = tr.parents(M)
    ids, pw, ot = [t.numpy() for t in _host(M, 1, 20, rule)]
    empty = 0
    for i in range(M):
        v, t = int(seeds[i]), int(times[i])
        beg, end = int(g.rowptr[v]), int(g.rowptr[v + 1])
        cnt = tr.count(g.etime, beg, end, t)
        if cnt == 0:
            empty += 1
            assert ids[M + i] == v and pw[i] == 0.0
        else:
            assert int(ids[M + i]) in set(int(c) for c in g.col[beg:beg + cnt])
        assert ids[i] == v and ot[i] == ot[M + i] == t
    assert 0 < empty < M


def test_snapshot_equivalence():
    """rule seed, every time = T on the full graph == times INT64_MAX on snapshot(T), the same table for both"""
    g = tr.graph()
    seeds, _ = tr.parents(84)
    for T in (-10, 2, 150):
        snap = g.csr().snapshot(T)
        assert 0 < snap.nnz < len(g.col)
        a = _host(84, 5, 20, "seed", seeds=seeds, times=np.full(84, T, dtype=np.int64))
        b = _host(84, 5, 20, "seed", seeds=seeds, times=np.full(84, INT64_MAX, dtype=np.int64), csr=snap)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert float(a[1].sum()) > 0


def test_negatives_are_the_plain_builders():
    gs = pkg()
    M, Q = 17, 64
    seeds, _ = tr.parents(M)
    plain, _ = gs.ops.unsup_batch(tr.graph().csr(), torch.from_numpy(seeds), 5, Q, twr.table(), _philox())
    for rule in twr.RULES:
        assert torch.equal(_host(M, 5, Q, rule)[0][2 * M:], plain[2 * M:])
    assert torch.equal(_host(M, 5, Q, "seed", g0=77)[0][2 * M:], plain[2 * M:])        # g0 does not enter


@pytest.mark.parametrize("rule", twr.RULES)
def test_padding_and_shards(rule):
    seeds, times = tr.parents(84)
    b, B, Q = 7, 16, 20                                      # (Q > b: the negatives' times wrap round the live seeds)
    short = _host(b, 5, Q, rule, seeds=seeds[:b], times=times[:b])
    ps = np.concatenate([seeds[:b], np.repeat(seeds[:1], B - b)])
    pt = np.concatenate([times[:b], np.repeat(times[:1], B - b)])
    padded = _host(B, 5, Q, rule, seeds=ps, times=pt, n_valid=b)
    for k in (0, 2):
        assert torch.equal(short[k][:b], padded[k][:b]) and torch.equal(short[k][b:2 * b], padded[k][B:B + b])
        assert torch.equal(short[k][2 * b:], padded[k][2 * B:])
    assert torch.equal(short[1], padded[1][:b])
    # without the live count the padded batch's negatives would take other times
    assert not torch.equal(_host(B, 5, Q, rule, seeds=ps, times=pt)[2][2 * B:], short[2][2 * b:])
    # two halves with g0 = G0 and g0 = G0 + B / 2 reproduce the whole's seeds, positives, their times and pair_w
    B = 48
    whole = _host(B, 5, Q, rule, seeds=seeds[:B], times=times[:B])
    h = B // 2
    for lo, g0 in ((0, twr.G0), (h, twr.G0 + h)):
        half = _host(h, 5, Q, rule, seeds=seeds[lo:lo + h], times=times[lo:lo + h], g0=g0)
        for k in (0, 2):
            assert torch.equal(half[k][:h], whole[k][lo:lo + h]) and torch.equal(half[k][h:2 * h], whole[k][B + lo:B + lo + h])
        assert torch.equal(half[1], whole[1][lo:lo + h]) and torch.equal(half[0][2 * h:], whole[0][2 * B:])


def test_refusals_of_the_op():
    gs = pkg()
    seeds, times = tr.parents(4)
    plain = gs.DeviceCSR(torch.from_numpy(tr.graph().rowptr), torch.from_numpy(tr.graph().col), tr.graph().n, 4097)
    args = (torch.from_numpy(seeds), torch.from_numpy(times), 5, 3, twr.table(), _philox())
    with pytest.raises(ValueError, match="no edge times"):
        gs.ops.unsup_batch_temporal(plain, *args)
    with pytest.raises(ValueError, match="unknown inherit rule"):
        gs.ops.unsup_batch_temporal(tr.graph().csr(), *args, inherit="walk")
    with pytest.raises(ValueError):
        _host(4, 17, 3, "seed")
    with pytest.raises(IndexError):
        _host(4, 5, 3, "seed", seeds=np.array([1, 2, 14, 3]), times=times)


def test_entry_validates_without_a_launch():
    """every refusal is GSAGE_EINVAL before any launch (so: without a GPU), the message naming the argument"""
    nat = pkg()._native
    L = nat.lib()
    P = 16                                                   # a non-null address that is never read

    def call(**kw):
        a = dict(rowptr=P, col=P, etime=P, n_rows=14, seeds=P, times=P, B=4, walk_len=5, Q=3, cdf=P, total=1.0,
                 inherit=0, ids=P, out_times=P, pair_w=P)
        a.update(kw)
        rc = L.gsage_unsup_batch_temporal(a["rowptr"], a["col"], a["etime"], a["n_rows"], a["seeds"], a["times"], a["B"],
                                          a["walk_len"], a["Q"], a["cdf"], a["total"], 7, None, 0, 0, a["inherit"], None,
                                          a["ids"], a["out_times"], a["pair_w"], None, None)
        return rc, L.gsage_last_error().decode()
    before = nat.launch_count()
    for kw, word in (({"rowptr": None}, "rowptr"), ({"col": None}, "col"), ({"etime": None}, "etime"),
                     ({"seeds": None}, "seeds"), ({"times": None}, "times"), ({"cdf": None}, "cdf"), ({"ids": None}, "ids"),
                     ({"out_times": None}, "out_times"), ({"pair_w": None}, "pair_w"), ({"B": 0}, "B"),
                     ({"B": 1 << 31}, "B"), ({"Q": 0}, "Q"), ({"walk_len": 0}, "walk_len"), ({"walk_len": 17}, "walk_len"),
                     ({"inherit": 2}, "inherit"), ({"total": 0.0}, "cdf_total"), ({"total": float("nan")}, "cdf_total"),
                     ({"total": float("inf")}, "cdf_total"), ({"total": -1.0}, "cdf_total")):
        rc, msg = call(**kw)
        assert rc == -1 and "unsup_batch_temporal" in msg and word in msg, (kw, msg)
    assert nat.launch_count() == before


# ---- the model ------------------------------------------------------------------------------------------------------
@pytest.fixture()
def fp32():
    gs = pkg()
    gs.ops.set_compute_dtype("fp32")
    old = gs.nn_modules.SparseUniformNeighborSampler.rng_default
    gs.nn_modules.SparseUniformNeighborSampler.rng_default = "philox"
    yield gs
    gs.nn_modules.SparseUniformNeighborSampler.rng_default = old
    gs.ops.set_compute_dtype("bf16")


def test_model_constructor_refusals_and_the_unchanged_default(fp32):
    gs = fp32
    p = tr.problem()
    with pytest.raises(ValueError, match="temporal_walks=True needs the temporal sampler"):
        twr.model(p, sampler="sparse_uniform_neighbor_sampler", temporal_walks=True)
    with pytest.raises(ValueError, match="weighted_walks"):
        twr.model(p, temporal_walks=True, weighted_walks=True)
    for kw in ({"walk_p": 2.0}, {"walk_q": 0.5}):
        with pytest.raises(ValueError, match="walk_p / walk_q"):
            twr.model(p, temporal_walks=True, **kw)
    ids = torch.tensor([5, 9, 32, 1, 60, 17], dtype=torch.int64)
    plain = twr.model(p)                                     # temporal_walks=False: the 2-tuple, the timeless walks
    assert not plain.temporal_walks and "temporal_walks" not in repr(plain)
    out = plain.build_batch(ids)
    assert len(out) == 2
    csr = plain.train_sampler.csr("cpu")
    ref = gs.ops.unsup_batch(csr, ids, 3, 5, gs.ops.neg_cdf(csr), {"seed": 0, "call_base": 0})
    assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1])
    with pytest.raises(ValueError, match="not temporal"):
        plain.build_batch(ids, times=torch.zeros(6, dtype=torch.int64))
    feats = torch.from_numpy(p["feats"])
    assert np.isfinite(float(plain.train_step(ids, feats)))


@pytest.mark.parametrize("rule", twr.RULES)
def test_model_builds_trains_and_evaluates(fp32, rule):
    p = tr.problem()
    feats = torch.from_numpy(p["feats"])
    m = twr.model(p, inherit=rule, temporal_walks=True)
    assert "temporal_walks=True" in repr(m)
    m.train_sampler.seed = 77
    ids = torch.tensor([5, 9, 32, 1, 60, 17], dtype=torch.int64)
    times = torch.tensor([tr.T_SNAP, tr.T_SNAP + 20, 0, -60, INT64_MAX, tr.T_SNAP], dtype=torch.int64)
    all_ids, pair_w, all_times = m.build_batch(ids, times=times)
    ref = twr.build_batch(p["indptr"], p["data"], p["etime"], 61, ids.numpy(), times.numpy(), 3, 5,
                          np.cumsum(np.diff(p["indptr"]).astype(np.float64) ** 0.75), 77, 0, 0, rule)
    assert ref[3] == 0 and np.array_equal(all_ids.numpy(), ref[0]) and np.array_equal(pair_w.numpy(), ref[1])
    assert np.array_equal(all_times.numpy(), ref[2])
    assert float(pair_w[3]) == 0.0 and int(all_ids[6 + 3]) == 1          # no edge before -60: its own positive
    assert m._batch_calls == [0, 1]
    # times=None: the sampler's default_times (INT64_MAX without a node_time)
    d_ids, _, d_times = m.build_batch(ids)
    assert bool((d_times == INT64_MAX).all()) and m._batch_calls == [0, 2]
    loss = float(m.train_step(ids, feats, times=times))
    assert np.isfinite(loss) and m._batch_calls == [0, 3] and m.train_sampler.calls == 2
    loss2 = float(m.train_step(None, feats, batch=(all_ids, pair_w, all_times)))
    assert np.isfinite(loss2) and m._batch_calls == [0, 3]
    res = m.evaluate(ids, feats, times=times)
    assert set(res) == {"loss", "mrr"} and np.isfinite(res["loss"]) and 0 < res["mrr"] <= 1 and m._batch_calls == [1, 3]
    with pytest.raises(ValueError, match="carries its own times"):
        m.train_step(None, feats, batch=(all_ids, pair_w, all_times), times=times)
    with pytest.raises(ValueError, match="temporal_walks=True a batch is"):
        m.train_step(None, feats, batch=(all_ids, pair_w))
    # the frontier of the step is drawn before the batch's times: hop 1 of the encoder, from the restatement
    m2 = twr.model(p, inherit=rule, temporal_walks=True)
    m2.train_sampler.seed = 77
    a_ids, _, a_times = m2.build_batch(ids, times=times)
    hop, hop_t = m2.train_sample_fns[0](ids=a_ids, times=a_times)
    r_hop, r_t, err = tr.sample(p["indptr"], p["data"], p["etime"], 61, a_ids.numpy(), a_times.numpy(), 3, 77, 0, 0,
                                "uniform", rule)
    assert err == 0 and np.array_equal(hop.numpy(), r_hop) and np.array_equal(hop_t.numpy(), r_t)


def _toy_run(steps=40):
    p = tr.problem()
    feats = torch.from_numpy(p["feats"])
    m = twr.model(p, dims=(16, 16), fans=(3, 2), walk_len=2, n_negatives=10, temporal_walks=True, lr_init=0.01)
    rng = np.random.RandomState(1)
    times = torch.full((32,), tr.T_SNAP, dtype=torch.int64)
    fixed_seeds = torch.from_numpy(rng.permutation(np.arange(1, 61))[:32])
    fixed = m.build_batch(fixed_seeds, train=False, times=times)

    def score():
        m.val_sampler.calls = 0                              # the same frontier draws before and after
        return m.evaluate(None, feats, batch=fixed)["loss"]
    before = score()
    for _ in range(steps):
        seeds = torch.from_numpy(rng.permutation(np.arange(1, 61))[:32])
        m.train_step(seeds, feats, times=times)
    return before, score()


def test_training_lowers_a_fixed_evaluation_batchs_loss(fp32):
    """GSUnsupervised(temporal_walks=True) on temporal_ref.problem(), host mode, fp32: 40 steps of 32 seeds as of T_SNAP,
    walks of at most 2 steps, 10 negatives, lr 0.01.  The loss of one fixed evaluation batch (32 seeds, the same frontier
    draws both times) was observed as 9.5053 before and 7.9891 after training (asserted: a drop of more than 5 %)."""
    before, after = _toy_run()
    print("fixed evaluation batch: loss %.4f before, %.4f after" % (before, after))
    assert np.isfinite([before, after]).all() and after < before - 0.05 * before


# ---- train.py -------------------------------------------------------------------------------------------------------
CLI = ["--problem-path", "<memory>", "--no-cuda", "--epochs", "1", "--batch-size", "16", "--n-train-samples", "3,2",
       "--n-val-samples", "3,2", "--output-dims", "8,8", "--rng", "philox", "--precision", "fp32", "--sampler-class",
       "sparse_temporal_neighbor_sampler", "--walk-len", "3", "--n-negatives", "5"]


def _cli_problem(temporal=True):
    gs = pkg()
    p = tr.problem()
    folds = np.array(["train"] * 40 + ["val"] * 11 + ["test"] * 10)
    kw = dict(adj_time=p["time"], train_adj_time=p["time"], node_time=np.full(p["n"] + 1, tr.T_SNAP)) if temporal else {}
    return gs.NodeProblem.from_arrays("classification", p["C"], p["adj"], p["adj"], p["feats"], folds, p["targets"],
                                      cuda=False, **kw)


def _restore():
    gs = pkg()
    gs.nn_modules.SparseUniformNeighborSampler.rng_default = "compat"
    gs.nn_modules.SparseTemporalNeighborSampler.strategy_default = "uniform"
    gs.nn_modules.SparseTemporalNeighborSampler.inherit_default = "seed"
    gs.ops.set_compute_dtype("bf16")


@pytest.mark.parametrize("engine", ["auto", "eager"])
@pytest.mark.parametrize("rule", twr.RULES)
def test_train_cli_runs_on_the_module_path(capsys, engine, rule):
    train = importlib.import_module("pytorch-graphsage_amd.train")
    try:
        train.main(CLI + ["--unsupervised", "--temporal-walks", "--engine", engine, "--temporal-inherit", rule, "--show-test"],
                   problem=_cli_problem())
        cap = capsys.readouterr()
        assert "temporal_walks=True" in cap.err and "module path" in cap.err
        lines = [json.loads(l) for l in cap.out.splitlines() if l.startswith("{")]
        batches = [l for l in lines if "epoch_progress" in l]
        assert len(batches) == 40 // 16 + 1 and all(np.isfinite(l["loss"]) for l in batches)
        assert any("mrr" in l and "epoch_progress" not in l and 0 < l["mrr"] <= 1 for l in lines)
        assert any("test" in l and np.isfinite(l["test"]["loss"]) for l in lines)
    finally:
        _restore()


UNIFORM = [a if a != "sparse_temporal_neighbor_sampler" else "sparse_uniform_neighbor_sampler" for a in CLI]


@pytest.mark.parametrize("argv,words", [
    (CLI + ["--temporal-walks"], ("--temporal-walks", "--unsupervised")),
    (UNIFORM + ["--unsupervised", "--temporal-walks"], ("--temporal-walks", "needs the temporal sampler")),
    (CLI + ["--unsupervised", "--temporal-walks", "--weighted-walks"], ("--temporal-walks", "--weighted-walks")),
    (CLI + ["--unsupervised", "--temporal-walks", "--walk-p", "2"], ("--temporal-walks", "--walk-p")),
    (CLI + ["--unsupervised", "--temporal-walks", "--walk-q", "0.5"], ("--temporal-walks", "--walk-q")),
    (CLI + ["--unsupervised", "--temporal-walks", "--importance-walks", "5"], ("--temporal-walks", "--importance-walks")),
    (CLI + ["--unsupervised", "--temporal-walks", "--engine", "fused"], ("--engine fused", "without a GPU")),
    (CLI + ["--unsupervised"], ("--unsupervised is not supported (the random walks are not temporal",)),
    (CLI + ["--link-eval-future"], ("--link-eval-future", "--link-eval", "--eval-as-of")),
    (CLI + ["--link-eval", "--link-eval-future"], ("--link-eval-future", "--eval-as-of")),
    (CLI + ["--link-eval-future", "--eval-as-of", "5", "--save-embeddings", "x.npy"], ("--link-eval-future", "--link-eval")),
])
def test_train_cli_refuses_with_a_sentence(argv, words):
    train = importlib.import_module("pytorch-graphsage_amd.train")
    try:
        with pytest.raises(SystemExit) as e:
            train.main(argv, problem=_cli_problem())
        msg = str(e.value)
        assert msg.startswith("gsage: ") and "\n" not in msg and all(w in msg for w in words), msg
    finally:
        _restore()


def test_link_eval_future_ranks_the_edges_at_or_after_T(capsys):
    gs = pkg()
    train = importlib.import_module("pytorch-graphsage_amd.train")
    T = tr.T_SNAP
    base = CLI + ["--unsupervised", "--temporal-walks", "--link-eval", "--eval-as-of", str(T), "--show-test"]
    try:
        problem = _cli_problem()
        train.main(base + ["--link-eval-future"], problem=problem)
        cap = capsys.readouterr()
        lines = [json.loads(l)["link_eval"] for l in cap.out.splitlines() if l.startswith('{"link_eval"')]
        assert [l["fold"] for l in lines] == ["val", "test"]
        full = gs.DeviceCSR.from_scipy(problem.adj, torch.device("cpu"))
        for l in lines:
            assert l["future"] is True and l["as_of"] == T and 0 < l["mrr"] <= 1
            src, dst = gs.held_out_edges(full, full.snapshot(T), torch.from_numpy(np.asarray(problem.nodes[l["fold"]])))
            assert l["held_out_edges"] == int(src.shape[0]) > 0
        # every ranked edge first happens at or after T
        p = tr.problem()
        first = {}
        for v in range(61):
            for e in range(int(p["indptr"][v]), int(p["indptr"][v + 1])):
                key = (v, int(p["data"][e]))
                first[key] = min(first.get(key, INT64_MAX), int(p["etime"][e]))
        src, dst = gs.held_out_edges(full, full.snapshot(T), torch.from_numpy(np.asarray(problem.nodes["val"])))
        assert all(first[(int(u), int(v))] >= T for u, v in zip(src, dst))
        # without the switch the line is today's: adj == train_adj holds nothing out, and no new keys
        train.main(base, problem=_cli_problem())
        cap = capsys.readouterr()
        lines = [json.loads(l)["link_eval"] for l in cap.out.splitlines() if l.startswith('{"link_eval"')]
        assert len(lines) == 2 and all("future" not in l and "as_of" not in l and l["held_out_edges"] == 0 for l in lines)
    finally:
        _restore()
