"""The temporal sampler without a GPU: host mode of ops.sample_csr_temporal against the serial restatement of
tests/temporal_ref.py (bit for bit), the definition's properties and its uniformity, TemporalAdj / with_times /
snapshot, the registry, the refusals, a problem's round trip with its times, and the point of it all -- with the
`recent` strategy on a graph whose eligible counts divide the fan-outs, the sampled forward as of T IS
full-neighbourhood inference over snapshot(T), which the uniform sampler on the timeless graph is not."""
import importlib

import numpy as np
import pytest
import torch
from scipy import sparse

import temporal_ref as tr
from conftest import pkg
from util import close

SEED = 0x0123456789ABCDEF
EINVAL = -1                         # GSAGE_EINVAL (include/gsage.h)
NS = [1, 3, 10, 25]
INT64_MAX = tr.INT64_MAX
COUNTS = {}                         # (row, t) -> cnt of the restatement, shared by the tests of this file


def _triples():
    return ((0, 0, None), (21, 5, None), (21, 2, torch.tensor([6], dtype=torch.int64)))


# ---- host mode against the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("inherit", tr.RULES)
@pytest.mark.parametrize("strategy", tr.STRATEGIES)
@pytest.mark.parametrize("n", NS)
def test_host_mode_equals_the_restatement(n, strategy, inherit):
    gs = pkg()
    g = tr.graph()
    adj = g.csr("cpu")
    ids, times = tr.parents()
    for g0, base, ctr in _triples():
        ph = {"seed": SEED, "call_base": base, "g0": g0 * n}
        if ctr is not None:
            ph["call_ctr"] = ctr
        got, got_t = gs.ops.sample_csr_temporal(adj, torch.from_numpy(ids), torch.from_numpy(times), n, ph,
                                                strategy=strategy, inherit=inherit)
        ref, ref_t, err = tr.sample(g.rowptr, g.col, g.etime, g.n, ids, times, n, SEED,
                                    base + (6 if ctr is not None else 0), g0 * n, strategy, inherit, COUNTS)
        assert err == 0 and got.dtype == got_t.dtype == torch.int64
        assert np.array_equal(got.numpy(), ref) and np.array_equal(got_t.numpy(), ref_t), (n, g0, base)
    assert gs.ops.TEMPORAL_TAG == tr.TAG == 0x54000000
    assert tr.TAG not in (gs.ops.DISTINCT_TAG, gs.ops.WEIGHTED_TAG, gs.ops.IMPORTANCE_TAG, gs.ops.WALK_BIAS_TAG)
    for bad in ([0, g.n], [-1]):
        with pytest.raises(IndexError):
            gs.ops.sample_csr_temporal(adj, torch.tensor(bad), torch.zeros(len(bad), dtype=torch.int64), n, {"seed": SEED})


def test_the_graph_is_what_the_tests_need():
    """every kind of query time gives the count the definition says, on every row; the PAIRED rows' last two times
    differ only above bit 32, and the time between them sees all but the last edge"""
    g = tr.graph()
    assert sorted(g.deg) == sorted(tr.DEGREES) and list(g.deg[:4]) == [3, 300, 4097, 0]
    assert (g.etime < 0).any() and int(g.etime.max()) < INT64_MAX
    for v in range(g.n):
        beg, d = int(g.rowptr[v]), int(g.deg[v])
        qt = tr.query_times(g, v)
        cnt = [tr.count(g.etime, beg, beg + d, t) for t in qt]
        if d == 0:
            assert cnt == [0] * 6
            continue
        assert cnt[0] == 0 and cnt[1] == 0 and cnt[4] == d and cnt[5] == d
        row = [int(x) for x in g.etime[beg:beg + d]]
        assert cnt[2] == row.index(qt[2]) and (d < 5 or d in (16, 17) or row.count(qt[2]) > 1)
        assert 0 < cnt[3] <= d and (cnt[3] == d or row[cnt[3] - 1] < qt[3] < row[cnt[3]]) or d < 3
        if d in tr.PAIRED:
            assert cnt[3] == d - 1 and (row[-1] ^ row[-2]) & 0xFFFFFFFF == 0 and (row[0] ^ row[1]) & 0xFFFFFFFF == 0


@pytest.mark.parametrize("inherit", tr.RULES)
@pytest.mark.parametrize("strategy", tr.STRATEGIES)
def test_properties_of_the_definition(strategy, inherit):
    """a 3-hop frontier in host mode: every non-dummy output is an edge of its parent that happened before the parent's
    time; under `edge` the times strictly decrease along every path, under `seed` they are constant"""
    gs = pkg()
    g = tr.graph()
    adj = g.csr("cpu")
    ids, times = tr.parents()
    fans = (3, 2, 2)
    cur, cur_t = torch.from_numpy(ids), torch.from_numpy(times)
    for k, n in enumerate(fans):
        nxt, nxt_t = gs.ops.sample_csr_temporal(adj, cur, cur_t, n, {"seed": SEED, "call_base": k}, strategy=strategy,
                                                inherit=inherit)
        par, par_t = cur.numpy().repeat(n), cur_t.numpy().repeat(n)
        o, ot = nxt.numpy(), nxt_t.numpy()
        for i in range(o.shape[0]):
            v, t = int(par[i]), int(par_t[i])
            beg, end = int(g.rowptr[v]), int(g.rowptr[v + 1])
            cnt = COUNTS.setdefault((v, t), tr.count(g.etime, beg, end, t))
            if cnt == 0:
                assert o[i] == 0 and ot[i] == t
                continue
            assert o[i] != 0 and o[i] in g.col[beg:beg + cnt]              # an edge among the first cnt: etime < t
            if inherit == "edge":
                assert ot[i] < t and ot[i] in g.etime[beg:beg + cnt][g.col[beg:beg + cnt] == o[i]]
            else:
                assert ot[i] == t
        cur, cur_t = nxt, nxt_t


@pytest.mark.parametrize("n", NS)
def test_recent_returns_the_latest_edges_balanced(n):
    gs = pkg()
    g = tr.graph()
    ids, times = tr.parents()
    out, out_t = gs.ops.sample_csr_temporal(g.csr("cpu"), torch.from_numpy(ids), torch.from_numpy(times), n,
                                            {"seed": SEED}, strategy="recent", inherit="edge")
    out, out_t = out.view(-1, n).numpy(), out_t.view(-1, n).numpy()
    for i, (v, t) in enumerate(zip(ids, times)):
        beg, end = int(g.rowptr[v]), int(g.rowptr[v + 1])
        cnt = COUNTS.setdefault((int(v), int(t)), tr.count(g.etime, beg, end, int(t)))
        if cnt == 0:
            continue
        k = min(n, cnt)
        latest = list(range(beg + cnt - 1, beg + cnt - 1 - k, -1))        # most recent first
        assert list(out[i, :k]) == [int(g.col[e]) for e in latest]
        assert list(out_t[i, :k]) == [int(g.etime[e]) for e in latest]
        offs = [cnt - 1 - (j % cnt) for j in range(n)]
        times_used = np.bincount(offs, minlength=cnt)[cnt - k:]
        assert set(times_used) <= {n // cnt, -(-n // cnt)} and times_used.sum() == n
        assert list(out[i]) == [int(g.col[beg + o]) for o in offs]


def test_uniform_over_the_eligible_edges():
    """one row of 7 edges, 5 of them before t: 120 000 parents, n = 1, seed 20240607, call 0.  Each of the 5 offsets
    within +-5 % of 24 000 (a condition, not a measurement: 8.6 standard deviations at 139 draws each; the definition
    alone stays within 0.6 % on these words), the two later edges never"""
    gs = pkg()
    rowptr = torch.tensor([0, 7], dtype=torch.int64)
    col = torch.arange(1, 8, dtype=torch.int32)
    adj = gs.DeviceCSR(rowptr, col, 1, 7).with_times(torch.tensor([1, 2, 3, 4, 5, 6, 7]))
    M = 120000
    out, out_t = gs.ops.sample_csr_temporal(adj, torch.zeros(M, dtype=torch.int64), torch.full((M,), 6), 1,
                                            {"seed": 20240607})
    counts = np.bincount(out.numpy(), minlength=8)
    assert counts[0] == counts[6] == counts[7] == 0 and counts.sum() == M
    assert counts[1:6].min() >= 22800 and counts[1:6].max() <= 25200, counts
    assert bool((out_t == 6).all())


# ---- TemporalAdj, with_times, snapshot ---------------------------------------------------------------------------
def _small():
    """3 rows in the reference's convention: row 0 of 4 edges with a tie, row 1 empty, row 2 of 3 edges"""
    indptr = np.asarray([0, 4, 4, 7])
    data = np.asarray([5, 6, 7, 8, 1, 2, 3])
    cols = np.asarray([0, 1, 2, 3, 0, 1, 2])
    adj = sparse.csr_matrix((data, cols, indptr), shape=(3, 4))
    time = np.asarray([30, 10, 30, -20, 9, 9, 1], dtype=np.int64)
    return adj, time


def test_temporal_adj_reorders_rows_stably():
    gs = pkg()
    adj, time = _small()
    t = gs.TemporalAdj(adj, time, node_time=np.asarray([5, 6, 7]))
    assert t.shape == (3, 4) and t.adj.has_sorted_indices
    assert list(t.adj.data) == [8, 6, 5, 7, 3, 1, 2]              # ties (30, 30 and 9, 9) keep their stored order
    assert list(t.time) == [-20, 10, 30, 30, 1, 9, 9] and t.time.dtype == np.int64
    assert list(t.adj.indices) == [0, 1, 2, 3, 0, 1, 2] and list(t.adj.indptr) == [0, 4, 4, 7]
    assert list(t.node_time) == [5, 6, 7]
    as_matrix = sparse.csr_matrix((time, adj.indices, adj.indptr), shape=adj.shape)
    u = gs.TemporalAdj(adj, as_matrix)
    assert list(u.adj.data) == list(t.adj.data) and list(u.time) == list(t.time) and u.node_time is None
    csr = gs.DeviceCSR.from_scipy(t, torch.device("cpu"))        # the times ride along
    assert csr.etime is not None and list(csr.etime.numpy()) == list(t.time)


def test_temporal_adj_refuses():
    gs = pkg()
    adj, time = _small()
    with pytest.raises(ValueError, match="7 stored edges"):
        gs.TemporalAdj(adj, time[:-1])
    other = sparse.csr_matrix((np.ones(7, dtype=np.int64), np.asarray([0, 1, 2, 0, 1, 2, 3]), np.asarray([0, 3, 3, 7])),
                              shape=(3, 4))
    with pytest.raises(ValueError, match="structure"):
        gs.TemporalAdj(adj, other)
    bad = time.copy()
    bad[3] = INT64_MAX
    with pytest.raises(ValueError, match="INT64_MAX"):
        gs.TemporalAdj(adj, bad)
    with pytest.raises(ValueError, match="integers"):
        gs.TemporalAdj(adj, time.astype(np.float64))
    with pytest.raises(ValueError, match="scipy sparse"):
        gs.TemporalAdj(adj.toarray(), time)
    with pytest.raises(ValueError, match="node_time"):
        gs.TemporalAdj(adj, time, node_time=np.zeros(2, dtype=np.int64))


def test_with_times_refuses_unsorted_rows():
    gs = pkg()
    adj, time = _small()
    csr = gs.DeviceCSR.from_scipy(adj, torch.device("cpu"))
    with pytest.raises(ValueError, match="TemporalAdj"):
        csr.with_times(torch.from_numpy(time))
    assert csr.etime is None
    with pytest.raises(ValueError, match="7 stored edges"):
        csr.with_times(torch.zeros(6, dtype=torch.int64))
    with pytest.raises(ValueError, match="INT64_MAX"):
        csr.with_times(torch.tensor([1, 2, 3, INT64_MAX, 1, 2, 3]))
    # a step down where a row begins is no disorder
    assert csr.with_times(torch.tensor([1, 2, 3, 4, -9, -9, 0])) is csr and csr.etime.dtype == torch.int64
    for fn in (lambda: gs.ops.temporal_count(gs.DeviceCSR.from_scipy(adj, torch.device("cpu")), t=3),
               lambda: gs.DeviceCSR.from_scipy(adj, torch.device("cpu")).snapshot(3)):
        with pytest.raises(ValueError, match="no edge times"):
            fn()


def test_snapshot_equals_the_restatement():
    gs = pkg()
    g = tr.graph()
    adj = g.csr("cpu")
    for t in (-tr.BIG - 5, -41, -40, -37, 0, 11, 12, 2000, tr.BIG, tr.BIG + 1, tr.BIG + (1 << 32), INT64_MAX - 1):
        snap = adj.snapshot(t)
        rp, col, et = tr.snapshot(g.rowptr, g.col, g.etime, t)
        assert snap.n_rows == adj.n_rows and snap.max_deg == adj.max_deg and snap.edge_cdf is None
        assert np.array_equal(snap.rowptr.numpy(), rp) and np.array_equal(snap.col.numpy(), col), t
        assert np.array_equal(snap.etime.numpy(), et) and snap.col.dtype == torch.int32
        cnt = gs.ops.temporal_count(adj, t=t)
        assert np.array_equal(cnt.numpy(), np.diff(rp))
    whole = adj.snapshot(INT64_MAX)
    assert torch.equal(whole.rowptr, adj.rowptr) and torch.equal(whole.col, adj.col) and torch.equal(whole.etime, adj.etime)
    assert adj.snapshot(-tr.BIG - (1 << 32)).nnz == 0


def test_temporal_count_per_row_times():
    gs = pkg()
    g = tr.graph()
    adj = g.csr("cpu")
    ids, times = tr.parents()
    cnt = gs.ops.temporal_count(adj, torch.from_numpy(ids), torch.from_numpy(times))
    ref = [COUNTS.setdefault((int(v), int(t)), tr.count(g.etime, int(g.rowptr[v]), int(g.rowptr[v + 1]), int(t)))
           for v, t in zip(ids, times)]
    assert cnt.dtype == torch.int64 and list(cnt.numpy()) == ref
    every = gs.ops.temporal_count(adj, times=torch.from_numpy(times[:g.n]))
    assert list(every.numpy()) == ref[:g.n]
    with pytest.raises(ValueError, match="exactly one"):
        gs.ops.temporal_count(adj)
    with pytest.raises(IndexError):
        gs.ops.temporal_count(adj, torch.tensor([g.n]), t=0)


# ---- the entry points' refusals ------------------------------------------------------------------------------------
def test_refusals_without_a_gpu():
    gs = pkg()
    nat = gs._native
    lib = nat.lib()
    adj = tr.graph().csr("cpu")
    ids = torch.zeros(4, dtype=torch.int64)
    tm = torch.zeros(4, dtype=torch.int64)
    out, out_t = torch.zeros(64, dtype=torch.int64), torch.zeros(64, dtype=torch.int64)
    cnt = torch.zeros(adj.n_rows, dtype=torch.int64)
    rp, col, et = adj.rowptr.data_ptr(), adj.col.data_ptr(), adj.etime.data_ptr()
    idp, tp, op, otp = ids.data_ptr(), tm.data_ptr(), out.data_ptr(), out_t.data_ptr()
    before = nat.launch_count()

    def hop(rowptr=rp, etime=et, times=tp, M=4, n=3, strategy=0, inherit=0, out_time=otp, n_rows=adj.n_rows):
        return lib.gsage_sample_csr_temporal(rowptr, col, etime, n_rows, idp, times, M, n, strategy, inherit, SEED, None,
                                             0, 0, op, out_time, None, None)

    for kw, word in (({"n": 0}, b"n (samples per parent)"), ({"strategy": 2}, b"strategy"), ({"strategy": -1}, b"strategy"),
                     ({"inherit": 2}, b"inherit"), ({"M": -1}, b"negative size"), ({"n_rows": -1}, b"negative size"),
                     ({"rowptr": None}, b"rowptr"), ({"etime": None}, b"etime"), ({"times": None}, b"times"),
                     ({"out_time": None}, b"out_time")):
        assert hop(**kw) == EINVAL and word in lib.gsage_last_error(), kw
    assert hop(M=0) == 0 and hop(M=0, rowptr=None) == 0

    assert lib.gsage_temporal_count(None, et, adj.n_rows, idp, 4, tp, 0, cnt.data_ptr(), None, None) == EINVAL
    assert b"rowptr" in lib.gsage_last_error()
    assert lib.gsage_temporal_count(rp, et, adj.n_rows, idp, -1, tp, 0, cnt.data_ptr(), None, None) == EINVAL
    assert b"negative size" in lib.gsage_last_error()
    assert lib.gsage_temporal_count(rp, et, adj.n_rows, None, adj.n_rows + 1, None, 0, cnt.data_ptr(), None, None) == EINVAL
    assert b"ids is NULL" in lib.gsage_last_error()
    assert lib.gsage_temporal_count(rp, et, adj.n_rows, idp, 4, tp, 0, None, None, None) == EINVAL
    assert b"cnt" in lib.gsage_last_error()
    assert lib.gsage_temporal_count(rp, et, adj.n_rows, idp, 0, tp, 0, cnt.data_ptr(), None, None) == 0

    oc, oe = torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int64)
    assert lib.gsage_temporal_compact(rp, col, et, adj.n_rows, None, cnt.data_ptr(), oc.data_ptr(), oe.data_ptr(), 8,
                                      None) == EINVAL and b"cnt" in lib.gsage_last_error()
    assert lib.gsage_temporal_compact(rp, col, et, adj.n_rows, cnt.data_ptr(), cnt.data_ptr(), None, oe.data_ptr(), 8,
                                      None) == EINVAL and b"out_col" in lib.gsage_last_error()
    assert lib.gsage_temporal_compact(rp, col, et, adj.n_rows, cnt.data_ptr(), cnt.data_ptr(), oc.data_ptr(),
                                      oe.data_ptr(), -1, None) == EINVAL and b"negative size" in lib.gsage_last_error()
    assert lib.gsage_temporal_compact(rp, col, et, 0, cnt.data_ptr(), cnt.data_ptr(), oc.data_ptr(), oe.data_ptr(), 8,
                                      None) == 0
    assert nat.launch_count() == before
    for kw in ({"strategy": "latest"}, {"inherit": "parent"}):
        with pytest.raises(ValueError, match="unknown"):
            gs.ops.sample_csr_temporal(adj, ids, tm, 3, {"seed": SEED}, **kw)
    plain = gs.DeviceCSR(adj.rowptr, adj.col, adj.n_rows, adj.max_deg)
    with pytest.raises(ValueError, match="no edge times"):
        gs.ops.sample_csr_temporal(plain, ids, tm, 3, {"seed": SEED})


# ---- registry, sampler class ---------------------------------------------------------------------------------------
def test_the_name_resolves_and_the_reference_table_is_unchanged():
    gs = pkg()
    cls = gs.find_sampler("sparse_temporal_neighbor_sampler")
    assert cls is gs.nn_modules.SparseTemporalNeighborSampler is gs.sampler_extensions["sparse_temporal_neighbor_sampler"]
    assert sorted(gs.sampler_lookup) == ["sparse_uniform_neighbor_sampler", "uniform_neighbor_sampler"]
    assert not issubclass(cls, gs.nn_modules.SparseUniformNeighborSampler)
    p = tr.problem()
    with pytest.raises(ValueError, match="no edge times"):
        cls(p["adj"])
    with pytest.raises(ValueError, match="unknown strategy"):
        cls(p["tadj"], strategy="latest")
    with pytest.raises(ValueError, match="unknown inherit"):
        cls(p["tadj"], inherit="parent")
    s = cls(p["tadj"], seed=5)
    assert s.rng == "philox" and s.shard == (0, 1) and (s.strategy, s.inherit) == ("uniform", "seed")
    assert np.array_equal(s.degrees, np.diff(p["indptr"]))
    ids = torch.arange(0, 61, 3)
    times = torch.full((21,), tr.T_SNAP)
    a, at = s(ids, times, 4)
    ref, ref_t, _ = tr.sample(p["indptr"], p["data"], p["etime"], 61, ids.numpy(), times.numpy(), 4, 5, 0, 0, "uniform",
                              "seed")
    assert s.calls == 1 and np.array_equal(a.numpy(), ref) and np.array_equal(at.numpy(), ref_t)
    s.begin_capture(torch.tensor([3], dtype=torch.int64))
    b, bt = s(ids=ids, times=times, n_samples=4)
    assert s.calls_in_capture() == 1
    ref, _, _ = tr.sample(p["indptr"], p["data"], p["etime"], 61, ids.numpy(), times.numpy(), 4, 5, 3, 0, "uniform", "seed")
    assert np.array_equal(b.numpy(), ref)
    # class-wide defaults, as rng_default; no node_time: a seed without a time sees its whole row
    try:
        cls.strategy_default, cls.inherit_default = "recent", "edge"
        r = cls(p["tadj"])
        assert (r.strategy, r.inherit) == ("recent", "edge")
    finally:
        cls.strategy_default, cls.inherit_default = "uniform", "seed"
    assert bool((s.default_times(ids) == INT64_MAX).all())
    nt = np.arange(61, dtype=np.int64) * 7
    with_nt = cls(gs.TemporalAdj(p["adj"], p["time"], node_time=nt))
    assert list(with_nt.default_times(ids).numpy()) == list(nt[ids.numpy()])
    # the other samplers read a TemporalAdj as its adjacency: the times are ignored
    gs.nn_modules.SparseUniformNeighborSampler.rng_default = "philox"
    try:
        for name in ("sparse_uniform_neighbor_sampler", "sparse_distinct_neighbor_sampler"):
            other = gs.find_sampler(name)
            assert torch.equal(other(p["tadj"], seed=2)(ids, 4), other(p["tadj"].adj, seed=2)(ids, 4))
    finally:
        gs.nn_modules.SparseUniformNeighborSampler.rng_default = "compat"


def test_models_take_times_only_with_a_temporal_sampler():
    gs = pkg()
    gs.ops.set_compute_dtype("fp32")
    gs.nn_modules.SparseUniformNeighborSampler.rng_default = "philox"
    try:
        p = tr.problem()
        feats = torch.from_numpy(p["feats"])
        ids = torch.tensor([5, 9, 32, 1, 60, 17], dtype=torch.int64)
        times = torch.full((6,), tr.T_SNAP)
        uniform = tr.model(p, (8, 8), (3, 2), sampler="sparse_uniform_neighbor_sampler")
        with pytest.raises(ValueError, match="not a temporal sampler"):
            uniform(ids, feats, train=False, times=times)
        assert tuple(uniform(ids, feats, train=False).shape) == (6, p["C"])
        # the module path's frontier is the restatement's, hop by hop beside the times
        fans = (3, 2)
        m = tr.model(p, (8, 8), fans, strategy="uniform", inherit="edge")
        m.train_sampler.seed = 77
        cur, cur_t, hops = ids, times, []
        for fn in m.train_sample_fns:
            cur, cur_t = fn(ids=cur, times=cur_t)
            hops.append((cur, cur_t))
        ref, err = tr.sample_hops(p["indptr"], p["data"], p["etime"], 61, ids.numpy(), times.numpy(), fans, 77, 0,
                                  "uniform", "edge")
        assert err == 0
        for (a, at), (r, rt) in zip(hops, ref[1:]):
            assert np.array_equal(a.numpy(), r) and np.array_equal(at.numpy(), rt)
        tg = torch.from_numpy(p["targets"][ids.numpy()])
        preds = m.train_step(ids=ids, feats=feats, targets=tg, loss_fn=gs.ProblemLosses.classification, times=times)
        assert tuple(preds.shape) == (6, p["C"]) and bool(torch.isfinite(preds).all())
        assert m.train_sampler.calls == 4                       # two hops drawn above, two by the step
        with torch.no_grad():                                   # no times: INT64_MAX without a node_time
            whole = m(ids, feats, train=False)
        assert tuple(whole.shape) == (6, p["C"]) and m.val_sampler.calls == 2
    finally:
        gs.nn_modules.SparseUniformNeighborSampler.rng_default = "compat"
        gs.ops.set_compute_dtype("bf16")


# ---- problem files -------------------------------------------------------------------------------------------------
def test_a_problem_round_trips_with_its_times(tmp_path, capsys):
    gs = pkg()
    p = tr.problem()
    n = p["n"]
    folds = np.array(["train"] * 40 + ["val"] * 11 + ["test"] * 10)
    nt = np.arange(n + 1, dtype=np.int64) + 990
    prob = gs.NodeProblem.from_arrays("classification", p["C"], p["adj"], p["adj"], p["feats"], folds, p["targets"],
                                      cuda=False, adj_time=p["time"], train_adj_time=p["time"], node_time=nt)
    assert isinstance(prob.adj, gs.TemporalAdj) and isinstance(prob.train_adj, gs.TemporalAdj)
    assert gs.problem._is_sparse(prob.adj) and list(prob.adj.node_time) == list(nt)
    path = str(tmp_path / "temporal.npz")
    gs.problem.save_problem_npz(path, {"task": "classification", "n_classes": p["C"], "sparse": True, "adj": prob.adj,
                                       "train_adj": prob.train_adj, "feats": p["feats"], "folds": folds,
                                       "targets": p["targets"]})
    with np.load(path) as f:
        assert {"adj_time", "train_adj_time", "node_time"} <= set(f.files) and f["adj_time"].dtype == np.int64
    back = gs.NodeProblem(path, cuda=False)
    for a, b in ((back.adj, prob.adj), (back.train_adj, prob.train_adj)):
        assert isinstance(a, gs.TemporalAdj) and np.array_equal(a.time, b.time) and np.array_equal(a.node_time, nt)
        assert np.array_equal(a.adj.data, b.adj.data) and np.array_equal(a.adj.indptr, b.adj.indptr)
    assert np.array_equal(back.adj.time, p["etime"]) and np.array_equal(back.adj.adj.data, p["data"])
    assert np.array_equal(back.node_time, nt)
    capsys.readouterr()
    # without the keys a file loads as before; with weights AND times it is temporal, said once
    gs.problem.save_problem_npz(path, {"task": "classification", "n_classes": p["C"], "sparse": True, "adj": p["adj"],
                                       "train_adj": p["adj"], "feats": p["feats"], "folds": folds, "targets": p["targets"]})
    plain = gs.NodeProblem(path, cuda=False)
    assert sparse.issparse(plain.adj) and plain.node_time is None
    capsys.readouterr()
    w = np.ones(p["adj"].nnz, dtype=np.float32)
    both = gs.NodeProblem.from_arrays("classification", p["C"], p["adj"], p["adj"], p["feats"], folds, p["targets"],
                                      cuda=False, adj_weight=w, train_adj_weight=w, adj_time=p["time"],
                                      train_adj_time=p["time"])
    err = capsys.readouterr().err
    assert isinstance(both.adj, gs.TemporalAdj) and isinstance(both.train_adj, gs.TemporalAdj)
    assert len([l for l in err.splitlines() if "weights are ignored" in l]) == 1


# ---- train.py's refusals -------------------------------------------------------------------------------------------
CLI = ["--problem-path", "<memory>", "--no-cuda", "--epochs", "1", "--batch-size", "16", "--n-train-samples", "3,2",
       "--n-val-samples", "3,2", "--output-dims", "8,8", "--rng", "philox", "--precision", "fp32", "--sampler-class",
       "sparse_temporal_neighbor_sampler"]


def _cli_problem(temporal=True, dense=False):
    gs = pkg()
    p = tr.problem()
    folds = np.array(["train"] * 40 + ["val"] * 11 + ["test"] * 10)
    if dense:
        adj = np.random.RandomState(0).randint(1, p["n"] + 1, size=(p["n"] + 1, 4))
        return gs.NodeProblem.from_arrays("classification", p["C"], adj, adj, p["feats"], folds, p["targets"], cuda=False)
    kw = dict(adj_time=p["time"], train_adj_time=p["time"], node_time=np.full(p["n"] + 1, tr.T_SNAP)) if temporal else {}
    return gs.NodeProblem.from_arrays("classification", p["C"], p["adj"], p["adj"], p["feats"], folds, p["targets"],
                                      cuda=False, **kw)


def _restore():
    gs = pkg()
    gs.nn_modules.SparseUniformNeighborSampler.rng_default = "compat"
    gs.nn_modules.SparseTemporalNeighborSampler.strategy_default = "uniform"
    gs.nn_modules.SparseTemporalNeighborSampler.inherit_default = "seed"
    gs.ops.set_compute_dtype("bf16")


@pytest.mark.parametrize("extra,problem,words", [
    ([], dict(temporal=False), ("no edge times", "adj_time")),
    ([], dict(dense=True), ("sparse problem",)),
    (["--unsupervised"], {}, ("--unsupervised", "not temporal")),
    (["--importance-walks", "5"], {}, ("--importance-walks",)),
    (["--engine", "fused"], {}, ("--engine fused", "no fused engine covers")),
])
def test_train_cli_refuses_with_a_sentence(extra, problem, words):
    train = importlib.import_module("pytorch-graphsage_amd.train")
    try:
        with pytest.raises(SystemExit) as e:
            train.main(CLI + extra, problem=_cli_problem(**problem))
        msg = str(e.value)
        assert "sparse_temporal_neighbor_sampler" in msg and "\n" not in msg and all(w in msg for w in words), msg
    finally:
        _restore()


def test_train_cli_other_refusals():
    train = importlib.import_module("pytorch-graphsage_amd.train")
    base = [a if a != "sparse_temporal_neighbor_sampler" else "sparse_uniform_neighbor_sampler" for a in CLI]
    try:
        with pytest.raises(SystemExit, match="--temporal-strategy"):
            train.main(base + ["--temporal-strategy", "recent"], problem=_cli_problem())
        with pytest.raises(SystemExit, match="--eval-as-of"):
            train.main(base + ["--eval-as-of", "5", "--full-neighbour-eval"], problem=_cli_problem(temporal=False))
        with pytest.raises(SystemExit, match="--eval-as-of goes with"):
            train.main(CLI + ["--eval-as-of", "5"], problem=_cli_problem())
    finally:
        _restore()


def test_train_cli_runs_on_the_module_path(capsys, tmp_path):
    """one epoch on the CPU with the recent / edge sampler, evaluated and exported as of T_SNAP"""
    gs = pkg()
    train = importlib.import_module("pytorch-graphsage_amd.train")
    emb = str(tmp_path / "emb.npy")
    try:
        train.main(CLI + ["--temporal-strategy", "recent", "--temporal-inherit", "edge", "--show-test", "--eval-as-of",
                          str(tr.T_SNAP), "--full-neighbour-eval", "--save-embeddings", emb], problem=_cli_problem())
        cap = capsys.readouterr()
        assert "--eval-as-of %d" % tr.T_SNAP in cap.err
        assert gs.nn_modules.SparseTemporalNeighborSampler.strategy_default == "recent"
        assert np.load(emb).shape == (61, 16)                   # (the mean aggregator concatenates self and neighbours)
        assert '"test_f1"' in cap.out
    finally:
        _restore()


# ---- the point of the feature --------------------------------------------------------------------------------------
def test_sampled_forward_as_of_T_is_full_neighbour_inference_over_the_snapshot():
    """every row has 1, 2, 3 or 6 edges before T and up to four at or after it; fan-outs (6, 6), fp32: the sampled
    forward with recent / seed and every seed time = T equals full-neighbourhood inference over snapshot(T), at the
    bound the distinct sampler's test of the same shape uses; the uniform sampler on the timeless graph does not"""
    gs = pkg()
    gs.ops.set_compute_dtype("fp32")
    old = gs.nn_modules.SparseUniformNeighborSampler.rng_default
    gs.nn_modules.SparseUniformNeighborSampler.rng_default = "philox"
    try:
        p = tr.problem()
        assert set(p["early"]) == {1, 2, 3, 6}
        feats = torch.from_numpy(p["feats"])
        ids = torch.arange(0, 61)
        times = torch.full((61,), tr.T_SNAP)
        model = tr.model(p, (16, 8), (6, 6), strategy="recent", inherit="seed")
        csr = model.val_sampler.csr("cpu")
        snap = csr.snapshot(tr.T_SNAP)
        assert np.array_equal(np.diff(snap.rowptr.numpy()), p["early"]) and snap.nnz < csr.nnz
        with torch.no_grad():
            sampled = model(ids, feats, train=False, times=times)
        full = gs.full_neighbour(model, feats, adj=snap)
        close(sampled.numpy(), full.numpy(), "temporal sampler vs full neighbourhood over the snapshot", 2e-5, 2e-5)
        uniform = tr.model(p, (16, 8), (6, 6), sampler="sparse_uniform_neighbor_sampler", adj=p["adj"])
        uniform.load_state_dict(model.state_dict())
        with torch.no_grad():
            noisy = uniform(ids, feats, train=False)
        with pytest.raises(AssertionError):
            close(noisy.numpy(), full.numpy(), "uniform sampler on the timeless graph vs the snapshot", 2e-5, 2e-5)
    finally:
        gs.nn_modules.SparseUniformNeighborSampler.rng_default = old
        gs.ops.set_compute_dtype("bf16")
