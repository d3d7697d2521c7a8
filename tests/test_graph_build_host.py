"""Graph construction without a GPU (include/gsage.h, "Graph construction"): host mode of ops.edges_to_csr /
ops.csr_transpose against the serial restatement of tests/graph_build_ref.py and, where the definition is the
reference, against convert.graph_from_edgelist + make_sparse_adjacency -- every comparison exact -- then the public
surface (gs.graph_from_edges, gs.problem_from_edges, `convert edges`) and every refusal."""
import numpy as np
import pytest
import torch

import graph_build_ref as gb
from conftest import pkg

N, E = 40, 300
CPU = torch.device("cpu")
# (weight?, time?, order, duplicates): every combination the definition has
COMBOS = [(False, False, o, d) for o in ("insertion", "id") for d in ("first", "all")] + \
         [(True, False, o, d) for o in ("insertion", "id") for d in ("first", "sum", "all")] + \
         [(False, True, "time", "all")]
_EDGES = {}


def _edges(seed=3):
    if seed not in _EDGES:
        e = gb.edge_list(N, E, seed)
        rng = np.random.RandomState(seed + 100)
        w = rng.rand(E).astype(np.float32) * 3
        w[::17] = 0
        t = rng.randint(-50, 50, size=E).astype(np.int64)            # few distinct values: equal times inside a row
        sel = rng.rand(N) < 0.6
        sel[[0, N - 1]] = True, False
        _EDGES[seed] = (e, w, t, sel)
    return _EDGES[seed]


def _host(e, n, **kw):
    ops = pkg().ops
    for k in ("weight", "time", "sel"):
        if kw.get(k) is not None:
            kw[k] = torch.from_numpy(kw[k])
    return ops.edges_to_csr(torch.from_numpy(e[:, 0].copy()), torch.from_numpy(e[:, 1].copy()), n, **kw)


def _same(got, ref):
    rowptr, col, max_deg, pay = got
    assert rowptr.dtype == torch.int64 and col.dtype == torch.int32
    assert np.array_equal(rowptr.numpy(), ref[0]) and np.array_equal(col.numpy(), ref[1]) and max_deg == ref[2]
    assert (pay is None) == (ref[3] is None)
    if pay is not None:
        assert pay.numpy().dtype == ref[3].dtype and np.array_equal(pay.numpy(), ref[3])


def test_the_list_is_what_the_tests_need():
    e, w, t, sel = _edges()
    assert (e[:, 0] == e[:, 1]).sum() >= 2 and e.max() == N - 4 and not (e == 1).any()
    pairs = [tuple(x) for x in e]
    assert pairs.count(pairs[2]) >= 2 and pairs[2][::-1] in pairs
    assert len(set(t)) < E


@pytest.mark.parametrize("with_sel", [False, True])
def test_the_default_build_is_the_reference(with_sel):
    e, _, _, sel = _edges()
    sel = sel if with_sel else None
    indptr, data, width = gb.reference(e, N, sel)
    rowptr, col, max_deg, pay = _host(e, N, sel=sel)
    assert pay is None and np.array_equal(rowptr.numpy(), indptr) and max_deg == width
    assert np.array_equal(col.numpy().astype(np.int64), data)
    _same((rowptr, col, max_deg, pay), gb.build(e, N, sel=sel))


@pytest.mark.parametrize("with_sel", [False, True])
@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "%s%s-%s-%s" % ("w" if c[0] else "", "t" if c[1] else "", c[2], c[3]))
def test_host_mode_equals_the_restatement(combo, directed, with_sel):
    e, w, t, sel = _edges()
    kw = dict(weight=w if combo[0] else None, time=t if combo[1] else None, sel=sel if with_sel else None,
              directed=directed, order=combo[2], duplicates=combo[3])
    _same(_host(e, N, **kw), gb.build(e, N, **kw))


def test_sum_adds_in_record_order():
    """a run of 40 duplicates whose fp32 sum depends on the order of the additions"""
    e = np.array([[0, 1]] * 40 + [[1, 0]] * 3, dtype=np.int64)
    w = (np.float32(1e8) * (np.arange(43) % 3 == 0) + np.arange(43)).astype(np.float32)
    ref = gb.build(e, 3, weight=w, duplicates="sum")
    _same(_host(e, 3, weight=w, duplicates="sum"), ref)
    assert ref[3][0] != np.float32(np.sum(w.astype(np.float64)))


def test_empty_and_single_edge():
    z = np.zeros((0, 2), dtype=np.int64)
    rowptr, col, max_deg, pay = _host(z, 5)
    assert col.numel() == 0 and max_deg == 1 and pay is None and rowptr.tolist() == [0] * 7
    rowptr, col, max_deg, pay = _host(z, 5, weight=np.zeros(0, dtype=np.float32))
    assert col.numel() == 0 and pay.numel() == 0
    _same(_host(np.array([[3, 1]]), 5), gb.build(np.array([[3, 1]]), 5))
    gs = pkg()
    csr = gs.DeviceCSR.from_edges(z[:, 0], z[:, 1], 5, CPU)
    assert csr.nnz == 0 and csr.max_deg == 1 and csr.n_rows == 6
    assert csr.transpose().nnz == 0 and csr.symmetrized().max_deg == 1


def test_a_temporal_build_is_temporaladj_of_the_timeless_builds():
    """Ties go by record index: the temporal build IS TemporalAdj (a stable lexsort) over the record-ordered build
    with every duplicate kept.  Over the "id"-ordered build TemporalAdj breaks ties by neighbour id instead, so there
    the rows agree as far as that allows: the same row lengths, the same times, and inside every (row, time) group
    the same neighbours."""
    gs = pkg()
    e, _, t, _ = _edges()
    got = gs.graph_from_edges(e, N, time=t, device=CPU)
    assert isinstance(got, gs.TemporalAdj)
    refs = {}
    for order in ("insertion", "id"):
        # (the timeless builds carry the times as fp32 weights: |t| < 2^24, so they come back exactly)
        rowptr, col, max_deg, pay = _host(e, N, weight=t.astype(np.float32), order=order, duplicates="all")
        refs[order] = gs.TemporalAdj(gs.DeviceCSR(rowptr, col, N + 1, max_deg).to_scipy(), pay.numpy().astype(np.int64))
    ref = refs["insertion"]
    assert got.adj.shape == ref.adj.shape
    assert np.array_equal(got.adj.indptr, ref.adj.indptr) and np.array_equal(got.adj.indices, ref.adj.indices)
    assert np.array_equal(got.adj.data, ref.adj.data) and np.array_equal(got.time, ref.time)
    csr = gs.DeviceCSR.from_edges(e[:, 0], e[:, 1], N, CPU, time=t)
    assert np.array_equal(csr.etime.numpy(), ref.time) and np.array_equal(csr.col.numpy(), ref.adj.data)
    by_id = refs["id"]
    assert np.array_equal(got.adj.indptr, by_id.adj.indptr) and np.array_equal(got.time, by_id.time)
    rows = np.repeat(np.arange(N + 1), np.diff(got.adj.indptr))
    assert not np.array_equal(got.adj.data, by_id.adj.data)              # (the list has such ties)
    assert np.array_equal(got.adj.data[np.lexsort((got.adj.data, got.time, rows))], by_id.adj.data)


@pytest.mark.parametrize("directed", [False, True])
def test_transpose_twice_is_the_id_build_with_duplicates(directed):
    gs = pkg()
    e = _edges()[0]
    a = gs.DeviceCSR.from_edges(e[:, 0], e[:, 1], N, CPU, directed=directed, duplicates="all")
    at = a.transpose()
    ref = gb.transpose(a.rowptr.numpy(), a.col.numpy(), a.n_rows)
    assert np.array_equal(at.rowptr.numpy(), ref[0]) and np.array_equal(at.col.numpy(), ref[1])
    assert at.max_deg == ref[2] and at.n_rows == a.n_rows
    att = at.transpose()
    by_id = gs.DeviceCSR.from_edges(e[:, 0], e[:, 1], N, CPU, directed=directed, duplicates="all", order="id")
    assert torch.equal(att.rowptr, by_id.rowptr) and torch.equal(att.col, by_id.col) and att.max_deg == by_id.max_deg


def test_symmetrized_directed_is_the_undirected_id_build():
    gs = pkg()
    e = _edges()[0]
    sym = gs.DeviceCSR.from_edges(e[:, 0], e[:, 1], N, CPU, directed=True).symmetrized()
    und = gs.DeviceCSR.from_edges(e[:, 0], e[:, 1], N, CPU, order="id")
    assert torch.equal(sym.rowptr, und.rowptr) and torch.equal(sym.col, und.col) and sym.max_deg == und.max_deg
    assert sym.col.dtype == torch.int32 and sym.n_rows == N + 1


def _problem_arrays():
    e = _edges()[0].copy()
    e[-2] = (N - 1, 0)                                  # the last node has a row, in both graphs (scipy infers the shape)
    rng = np.random.RandomState(11)
    folds = np.array(["train"] * N)
    folds[rng.rand(N) < 0.4] = "val"
    folds[[0, N - 1]] = "train"
    feats = rng.normal(size=(N, 6)).astype(np.float32)
    targets = rng.randint(0, 3, size=(N, 1))
    return e, folds, feats, targets


def test_problem_from_edges_is_the_converter_s_problem():
    gs = pkg()
    cv = gb.importlib_convert()
    e, folds, feats, targets = _problem_arrays()
    ref = cv.build_problem(cv.graph_from_edgelist(e, n_nodes=N), feats, targets, folds, "classification", 3, sparse=True)
    want = gs.NodeProblem.from_arrays("classification", 3, ref["adj"], ref["train_adj"], ref["feats"], ref["folds"],
                                      ref["targets"], cuda=False)
    got = gs.problem_from_edges("classification", 3, e, feats, folds, targets, cuda=False)
    for k in ("adj", "train_adj"):
        a, b = getattr(got, k).tocsr(), getattr(want, k).tocsr()
        assert a.shape == b.shape and np.array_equal(a.indptr, b.indptr)
        assert np.array_equal(a.indices, b.indices) and np.array_equal(a.data, b.data)
    assert got.n_nodes == want.n_nodes and torch.equal(got.feats, want.feats)
    assert np.array_equal(got.folds, want.folds) and np.array_equal(got.targets, want.targets)
    assert all(np.array_equal(got.nodes[m], want.nodes[m]) for m in ("train", "val", "test"))
    ids = torch.from_numpy(got.nodes["train"][:16].astype(np.int64))
    frontier = []
    for p in (got, want):
        sampler = gs.sampler_lookup["sparse_uniform_neighbor_sampler"](adj=p.train_adj, rng="compat")
        np.random.seed(5)
        frontier.append(sampler(ids, n_samples=7))
    assert torch.equal(frontier[0], frontier[1]) and int((frontier[0] != 0).sum()) > 0


def test_convert_edges_writes_the_converter_s_file(tmp_path):
    cv = gb.importlib_convert()
    e, folds, feats, targets = _problem_arrays()
    for name, arr in (("E", e), ("T", targets), ("F", folds), ("X", feats)):
        np.save(str(tmp_path / (name + ".npy")), arr)
    out = str(tmp_path / "got.npz")
    cv.main(["edges", "--edges", str(tmp_path / "E.npy"), "--targets", str(tmp_path / "T.npy"), "--folds",
             str(tmp_path / "F.npy"), "--feats", str(tmp_path / "X.npy"), "--task", "classification", "--outpath", out])
    ref = cv.build_problem(cv.graph_from_edgelist(e, n_nodes=N), feats, targets, folds, "classification",
                           len(np.unique(targets)), sparse=True)
    cv.save_problem(ref, str(tmp_path / "want.npz"))
    with np.load(out) as g, np.load(str(tmp_path / "want.npz")) as w:
        assert sorted(g.files) == sorted(w.files)
        for k in w.files:
            assert g[k].dtype == w[k].dtype and np.array_equal(g[k], w[k]), k
    with pytest.raises(SystemExit):
        cv.main(["edges", "--edges", str(tmp_path / "E.npy")])
    with pytest.raises(SystemExit):
        cv.main(["cora"])


def test_convert_edges_carries_weights_and_times(tmp_path):
    gs = pkg()
    cv = gb.importlib_convert()
    e, folds, feats, targets = _problem_arrays()
    _, w, t, _ = _edges()
    node_time = np.arange(N, dtype=np.int64)
    pw = gs.NodeProblem(cv.convert_edges(e, targets, folds, str(tmp_path / "w.npz"), feats, weight=w, device=CPU),
                        cuda=False)
    ref = gs.graph_from_edges(e, N, weight=w, sel=folds == "train", device=CPU)
    assert isinstance(pw.train_adj, gs.WeightedAdj) and np.array_equal(pw.train_adj.weight, ref.weight)
    assert np.array_equal(pw.train_adj.adj.data, ref.adj.data)
    pt = gs.NodeProblem(cv.convert_edges(e, targets, folds, str(tmp_path / "t.npz"), feats, time=t,
                                         node_time=node_time, device=CPU), cuda=False)
    ref = gs.graph_from_edges(e, N, time=t, device=CPU)
    assert isinstance(pt.adj, gs.TemporalAdj) and np.array_equal(pt.adj.time, ref.time)
    assert np.array_equal(pt.adj.adj.data, ref.adj.data) and np.array_equal(pt.node_time[1:], node_time)


def test_to_scipy_is_what_from_scipy_reads():
    gs = pkg()
    e = _edges()[0]
    csr = gs.DeviceCSR.from_edges(e[:, 0], e[:, 1], N, CPU)
    m = csr.to_scipy()
    assert m.shape == (N + 1, csr.max_deg) and m.data.dtype == np.int64
    back = gs.DeviceCSR.from_scipy(m, CPU)
    assert torch.equal(back.rowptr, csr.rowptr) and torch.equal(back.col, csr.col) and back.max_deg == csr.max_deg


def test_refusals_and_errors():
    gs = pkg()
    e, w, t, sel = _edges()
    with pytest.raises(ValueError, match="together"):
        _host(e, N, weight=w, time=t)
    with pytest.raises(ValueError, match="order"):
        _host(e, N, order="reverse")
    with pytest.raises(ValueError, match="duplicates"):
        _host(e, N, duplicates="max")
    with pytest.raises(ValueError, match="needs edge weights"):
        _host(e, N, duplicates="sum")
    with pytest.raises(ValueError, match="needs edge times"):
        _host(e, N, order="time")
    for kw in (dict(order="id"), dict(order="insertion"), dict(duplicates="first")):
        with pytest.raises(ValueError, match="time order"):
            _host(e, N, time=t, **kw)
    with pytest.raises(ValueError, match="2\\^31"):                       # from the shapes, before anything is allocated
        gs.ops.edges_check(2 ** 30, 10, False, False, False, None, None)
    assert gs.ops.edges_check(2 ** 30, 10, False, False, True, None, None) == ("insertion", "first")
    with pytest.raises(ValueError, match="62 bits"):
        gs.ops.edges_check(10, 2 ** 31, False, False, False, None, None)
    with pytest.raises(ValueError, match="sel"):
        _host(e, N, sel=sel[:-1])
    with pytest.raises(ValueError, match="weight"):
        _host(e, N, weight=w[:-1])
    with pytest.raises(ValueError, match="time"):
        _host(e, N, time=t[:-1])
    for bad in (-1, N):
        b = e.copy()
        b[7, 1] = bad
        with pytest.raises(IndexError):
            _host(b, N)
    with pytest.raises(ValueError, match="finite"):
        gs.DeviceCSR.from_edges(e[:, 0], e[:, 1], N, CPU, weight=-w)
    tt = t.copy()
    tt[3] = np.iinfo(np.int64).max
    with pytest.raises(ValueError):
        gs.DeviceCSR.from_edges(e[:, 0], e[:, 1], N, CPU, time=tt)
    with pytest.raises(ValueError, match="integers"):
        gs.DeviceCSR.from_edges(e[:, 0], e[:, 1], N, CPU, time=t.astype(np.float32))
    weighted = gs.DeviceCSR.from_edges(e[:, 0], e[:, 1], N, CPU, weight=w)
    temporal = gs.DeviceCSR.from_edges(e[:, 0], e[:, 1], N, CPU, time=t)
    assert weighted.edge_cdf is not None and temporal.etime is not None
    for csr, word in ((weighted, "CDF"), (temporal, "time order")):
        with pytest.raises(ValueError, match=word):
            csr.transpose()
        with pytest.raises(ValueError, match=word):
            csr.symmetrized()
    bad = gs.DeviceCSR(torch.tensor([0, 1, 2]), torch.tensor([1, 2], dtype=torch.int32), 2, 1)
    with pytest.raises(IndexError):
        bad.transpose()


def test_the_c_entries_refuse_bad_arguments_without_a_gpu():
    L = pkg()._native.lib()
    EINVAL, p = -1, 256
    assert L.gsage_edges_expand(p, p, 4, 10, None, 0, 4, 8, None, None) == EINVAL and b"aligned" in L.gsage_last_error()
    assert L.gsage_edges_expand(p, p, 4, 16, None, 0, 4, p, None, None) == EINVAL and b"n_nodes" in L.gsage_last_error()
    assert L.gsage_edges_expand(p, p, 2 ** 30, 10, None, 0, 4, p, None, None) == EINVAL and b"2^31" in L.gsage_last_error()
    assert L.gsage_edges_expand(None, None, 0, 10, None, 0, 4, None, None, None) == 0
    assert L.gsage_edges_expand_csr(p, p, 16, 4, 0, 4, p, p, None, None) == EINVAL and b"n_rows" in L.gsage_last_error()
    assert L.gsage_edges_expand_csr(p, p, 10, 4, 0, 4, p, None, None, None) == EINVAL and b"rowof" in L.gsage_last_error()
    assert L.gsage_edges_mark(p, p, 4, 4, 0, p, p, None, 0, None, None) == EINVAL and b"exactly one" in L.gsage_last_error()
    assert L.gsage_edges_mark(p, p, 4, 4, 0, p, None, p, 0, None, None) == EINVAL and b"wsum" in L.gsage_last_error()
    assert L.gsage_edges_row_keys(None, None, 4, 4, p, None) == EINVAL
    assert L.gsage_edges_time_keys(p, 4, 2, 0, p, None) == EINVAL and b"eshift" in L.gsage_last_error()
    assert L.gsage_edges_finish(p, p, None, None, 4, 0, 4, None, None, 4, 0, p, None, 0, 0, p, None, None, 4, None) == EINVAL
    assert L.gsage_edges_finish(None, None, None, None, 0, 0, 4, None, None, 4, 0, None, None, 0, 0, None, None, None, 0,
                                None) == 0
    assert L.gsage_edges_rowptr(p, None, 4, 0, 4, None, 0, None) == EINVAL and b"rowptr" in L.gsage_last_error()
