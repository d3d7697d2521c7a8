"""K-means without a GPU: the host path of ops.kmeans_pass / ops.kmeans_update / gs.kmeans meets tests/kmeans_ref.py on the
GPU tests' own inputs, the tie rule, the empty-cluster rule, k_live and the spherical mode hold, bad arguments are refused
with a sentence (and with GSAGE_EINVAL through the C ABI), gs.cluster_metrics scores hand-made tables, k-means++ finds
every blob of a well-separated toy, and train.py --cluster prints its line."""
import importlib
import json

import numpy as np
import pytest
import torch

import kmeans_ref as kr
from cli_problems import sparse_problem
from conftest import pkg

MODES = ("bf16", "fp32")


@pytest.fixture(autouse=True)
def _dtype():
    gs = pkg()
    yield
    gs.ops.set_compute_dtype("bf16")


def _host_pass(case, mode, **kw):
    gs = pkg()
    gs.ops.set_compute_dtype(mode)
    n, D, K, splits = case
    c = kr.make_case(n, D, K)
    table = torch.from_numpy(c["buf"])[:, :D]                   # a view of the NaN-padded buffer
    Cn = torch.from_numpy(c["Cn"].copy())
    bias = torch.from_numpy(kr.bias_of(c["Cn"], mode))
    return c, Cn, bias, gs.ops.kmeans_pass(table, torch.from_numpy(c["ids"]), Cn, bias, splits=splits, **kw)


# ---- 1. the reference's own condition, and the host path ---------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", kr.CASES)
def test_reference_leaves_few_rows_ambiguous_and_the_bound_bites(case, mode):
    """At most 1 % of a case's rows are ambiguous; the reference is within its own bound (excess 0); a result with one
    row moved to another cluster, or with one row dropped, is outside it."""
    n, D, K, splits = case
    ref = kr.case_reference(n, D, K, mode)
    print("%r %s: %d ambiguous of %d" % (case, mode, int(ref["ambiguous"].sum()), n))
    assert ref["ambiguous"].mean() <= kr.MAX_AMBIGUOUS
    fl = kr.from_labels(ref, ref["a"])
    r = kr.check_pass((fl["sums"], fl["counts"], fl["inertia"], 0, ref["a"], fl["dist"]), ref, splits)
    assert max(r.values()) == 0.0
    c = kr.make_case(n, D, K)
    if c["duplicate"] is not None:
        assert fl["counts"][c["duplicate"]] == 0                 # the copy of centroid 0 stays empty
    if n > 1 and K > 1:
        other = ref["a"].copy()
        other[n // 2] = (other[n // 2] + 1) % K                  # sums, counts and inertia of another labelling
        fo = kr.from_labels(ref, other)
        with pytest.raises(AssertionError):
            kr.check_pass((fo["sums"], fo["counts"], fo["inertia"], 0, ref["a"]), ref, splits)
        with pytest.raises(AssertionError):
            kr.check_pass((fl["sums"] - ref["X"][0], fl["counts"], fl["inertia"], 0, ref["a"]), ref, splits)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", [(1, 1, 1, 0), (33, 7, 2, 0), (257, 72, 31, 7), (300, 264, 65, 0)])
def test_host_pass_meets_the_reference(case, mode):
    n, D, K, splits = case
    c, Cn, bias, res = _host_pass(case, mode, want_dist=True)
    sums, counts, inertia, changed, labels, dist = res
    assert sums.dtype == torch.float32 and tuple(sums.shape) == (K, D) and counts.dtype == torch.int64
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (n,) and dist.dtype == torch.float32
    assert tuple(res.partial.shape) == (1, K * D + K + 2)
    ref = kr.case_reference(n, D, K, mode)
    kr.check_pass([v.numpy() for v in res], ref, splits, what="host %s %r" % (mode, case))
    assert np.array_equal(labels.numpy(), ref["a"])              # float64 against float64: every row
    lab, = pkg().ops.kmeans_pass(torch.from_numpy(c["buf"])[:, :D], torch.from_numpy(c["ids"]), Cn, bias, accumulate=False)
    assert torch.equal(lab, labels)


def test_labels_in_counts_the_changes_and_k_live_limits_the_clusters():
    n, D, K = 257, 72, 31
    c, Cn, bias, res = _host_pass((n, D, K, 0), "fp32")
    gs = pkg()
    table, ids = torch.from_numpy(c["buf"])[:, :D], torch.from_numpy(c["ids"])
    same = gs.ops.kmeans_pass(table, ids, Cn, bias, labels_in=res[4])
    assert int(same[3]) == 0
    flipped = res[4].clone()
    flipped[[3, 50, 256]] = K - 1                                # the empty duplicate: never a row's label
    assert int(gs.ops.kmeans_pass(table, ids, Cn, bias, labels_in=flipped)[3]) == 3
    live = gs.ops.kmeans_pass(table, ids, Cn, bias, k_live=3)
    assert int(live[4].max()) <= 2 and int(live[1][3:].sum()) == 0 and int(live[1].sum()) == n
    ref = kr.case_reference(n, D, K, "fp32", k_live=3)
    kr.check_pass([v.numpy() for v in live], ref, 0, what="k_live = 3")
    with pytest.raises(ValueError, match=r"k_live must be in \[1, K = 31\]"):
        gs.ops.kmeans_pass(table, ids, Cn, bias, k_live=32)


# ---- 2. the rules ------------------------------------------------------------------------------------------------------
def test_equal_scores_go_to_the_smallest_cluster_and_an_empty_cluster_keeps_its_centroid():
    gs = pkg()
    gs.ops.set_compute_dtype("fp32")
    X = torch.tensor([[1.0, 0.0], [0.9, 0.1], [0.0, 1.0], [0.1, 0.9], [-1.0, 0.0]])
    Cn = torch.tensor([[0.0, 1.0], [1.0, 0.0], [1.0, 0.0], [0.0, 1.0], [7.0, 7.0]])       # 2 copies 1, 3 copies 0
    bias = torch.zeros(5)
    assert gs.ops.kmeans_update(Cn, bias) is None                                          # the bias only
    assert torch.equal(bias, torch.tensor([-0.5, -0.5, -0.5, -0.5, -49.0]))
    res = gs.ops.kmeans_pass(X, torch.arange(5), Cn, bias)
    assert res[4].tolist() == [1, 1, 0, 0, 0]                    # (row 4 is as far from 0 as from 1: the smaller)
    assert res[1].tolist() == [3, 2, 0, 0, 0]
    before = Cn.clone()
    inertia, changed, empty = gs.ops.kmeans_update(Cn, bias, res.partial)
    assert int(empty) == 3 and int(changed) == 0 and float(inertia) == float(res[2])
    assert torch.equal(Cn[2:], before[2:])                       # bit for bit
    assert torch.allclose(Cn[0], torch.tensor([-0.9, 1.9]) / 3) and torch.allclose(Cn[1], torch.tensor([0.95, 0.05]))
    assert torch.equal(bias[2:], torch.tensor([-0.5, -0.5, -49.0]))
    assert torch.allclose(bias[:2], -0.5 * (Cn[:2] ** 2).sum(dim=1))


@pytest.mark.parametrize("mode", MODES)
def test_update_meets_the_reference_and_spherical_gives_unit_centroids(mode):
    gs = pkg()
    n, D, K = 257, 72, 31
    c, Cn, bias, res = _host_pass((n, D, K, 0), mode)
    for spherical in (False, True):
        C2, b2 = Cn.clone(), bias.clone()
        hist = (torch.zeros(4), torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int32),
                torch.tensor([2], dtype=torch.int64))
        assert gs.ops.kmeans_update(C2, b2, res.partial, spherical=spherical, history=hist) is None
        want_c, want_b, want_e = kr.update_reference(res[0].double().numpy(), res[1].numpy(), c["Cn"], mode, spherical)
        assert np.abs(C2.double().numpy() - want_c).max() <= 2.0 ** -23 * np.abs(want_c).max()
        assert np.abs(b2.double().numpy() - want_b).max() <= 2.0 ** -20
        assert int(hist[3]) == 3 and int(hist[2][2]) == want_e == 1 and float(hist[0][2]) == float(res[2])
        assert hist[0].tolist()[:2] == [0.0, 0.0] and int(hist[2][3]) == 0            # only slot 2 was written
        assert torch.equal(C2[K - 1], Cn[K - 1])
        if spherical:
            live = res[1] > 0
            assert float((C2[live].double().norm(dim=1) - 1.0).abs().max()) <= 4 * 2.0 ** -24
            assert torch.equal(b2, torch.zeros(K))


# ---- 3. the fit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_plus_plus_puts_a_centre_in_every_blob_and_the_fit_recovers_them(seed, mode):
    gs = pkg()
    gs.ops.set_compute_dtype(mode)
    X, planted = kr.blobs(seed)
    Xt = torch.from_numpy(X)
    cen, bias = gs.infer._kmeans_init(Xt, torch.arange(600), 5, "++", seed, False)
    nearest = np.argmin(((cen.numpy()[:, None, :] - 2.0 * np.eye(5, 32)[None]) ** 2).sum(axis=2), axis=1)
    assert sorted(nearest.tolist()) == [0, 1, 2, 3, 4]
    km = gs.kmeans(Xt, 5, init="++", seed=seed)
    m = gs.cluster_metrics(km.labels, torch.from_numpy(planted))
    assert m == {"n": 600, "clusters": 5, "nmi": 1.0, "purity": 1.0}
    assert km.n_iter == 10 and int(km.changed_history[0]) == 600 and int(km.changed_history[-1]) == 0
    h = km.inertia_history.double()
    # (|x| <= 2.01 here: the slack of unit rows times 2.01^2, rounded up to 5)
    assert bool((h[1:] <= h[:-1] + 2 * 5.0 * kr.inertia_slack(600, 32)).all())
    assert torch.equal(km.predict(Xt), km.labels) and torch.equal(km.predict(Xt, torch.arange(5)), km.labels[:5])
    again = gs.kmeans(Xt, 5, init="++", seed=seed)
    assert torch.equal(again.centroids, km.centroids) and torch.equal(again.labels, km.labels)
    assert torch.equal(again.inertia_history, km.inertia_history)


def test_fit_equals_its_composition_and_stopping_early_changes_nothing():
    gs = pkg()
    gs.ops.set_compute_dtype("fp32")
    c = kr.make_case(257, 72, 31)
    X, ids = torch.from_numpy(c["table"].copy()), torch.from_numpy(c["ids"])
    init = torch.from_numpy(c["Cn"])
    km = gs.kmeans(X, 31, nodes=ids, iters=40, init=init)
    assert km.n_iter < 40 and km.n_iter % 10 == 0
    C, b = init.clone(), torch.zeros(31)
    gs.ops.kmeans_update(C, b)
    labels, hist = None, []
    for _ in range(40):
        res = gs.ops.kmeans_pass(X, ids, C, b, labels_in=labels)
        labels = res[4]
        hist.append(gs.ops.kmeans_update(C, b, res.partial))
    assert torch.equal(km.centroids, C) and torch.equal(km.labels, labels) and float(km.inertia) == float(hist[-1][0])
    assert km.inertia_history.tolist() == [float(h[0]) for h in hist[:km.n_iter]]
    assert km.changed_history.tolist()[1:] == [int(h[1]) for h in hist[1:km.n_iter]]
    assert all(int(h[1]) == 0 and float(h[0]) == float(km.inertia) for h in hist[km.n_iter:])
    assert int(km.empty_history[-1]) >= 1                        # the duplicate


def test_random_init_n_init_and_spherical():
    gs = pkg()
    gs.ops.set_compute_dtype("fp32")
    X, planted = kr.blobs(0)
    Xt = torch.from_numpy(X)
    fits = [gs.kmeans(Xt, 5, init="random", seed=s) for s in (3, 4, 5)]
    best = gs.kmeans(Xt, 5, init="random", seed=3, n_init=3)
    want = min(fits, key=lambda f: (float(f.inertia), f.seed))
    assert best.seed == want.seed and torch.equal(best.centroids, want.centroids)
    rows = {tuple(r) for r in X.tolist()}
    cen0, _ = gs.infer._kmeans_init(Xt, torch.arange(600), 5, "random", 3, False)
    assert len({tuple(r) for r in cen0.tolist()}) == 5 and all(tuple(r) in rows for r in cen0.tolist())
    sp = gs.kmeans(torch.nn.functional.normalize(Xt, dim=1), 5, init="++", seed=0, spherical=True)
    assert float((sp.centroids.double().norm(dim=1) - 1.0).abs().max()) <= 4 * 2.0 ** -24
    assert torch.equal(sp.bias, torch.zeros(5))
    assert gs.cluster_metrics(sp.labels, torch.from_numpy(planted))["nmi"] == 1.0


# ---- 4. the metric -----------------------------------------------------------------------------------------------------
def test_cluster_metrics_on_hand_made_tables():
    gs = pkg()
    y = torch.tensor([0, 0, 0, 1, 1, 2, 2, 2, 2])
    relabelled = torch.tensor([2, 2, 2, 0, 0, 1, 1, 1, 1], dtype=torch.int32)
    assert gs.cluster_metrics(relabelled, y) == {"n": 9, "clusters": 3, "nmi": 1.0, "purity": 1.0}
    # two independent partitions: every (cluster, class) cell holds the product of its margins
    u = torch.arange(6).repeat_interleave(4) % 2
    v = torch.arange(24) % 4
    m = gs.cluster_metrics(u, v)
    assert m["clusters"] == 2 and abs(m["nmi"]) <= 1e-12 and m["purity"] == 0.25
    # a hand-computed table [[3, 1], [0, 4]]: I = sum p log(p / (pu pv)), H(U) = H(V) = log 2
    lab = torch.tensor([0, 0, 0, 0, 1, 1, 1, 1])
    tgt = torch.tensor([0, 0, 0, 1, 1, 1, 1, 1])
    T = np.array([[3.0, 1.0], [0.0, 4.0]]) / 8
    pu, pv = T.sum(1), T.sum(0)
    mi = sum(T[i, j] * np.log(T[i, j] / (pu[i] * pv[j])) for i in range(2) for j in range(2) if T[i, j] > 0)
    hu, hv = -(pu * np.log(pu)).sum(), -(pv * np.log(pv)).sum()
    m = gs.cluster_metrics(lab, tgt)
    assert abs(m["nmi"] - mi / ((hu + hv) / 2)) <= 1e-12 and m["purity"] == 7 / 8
    assert gs.cluster_metrics(torch.tensor([0, 3, 3]), torch.tensor([1, 0, 0]), n_classes=5)["clusters"] == 2
    with pytest.raises(ValueError, match="no regression or multilabel targets"):
        gs.cluster_metrics(lab, tgt.float())
    with pytest.raises(ValueError, match="no multilabel targets"):
        gs.cluster_metrics(lab, torch.zeros(8, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"class id out of range \[0, 1\)"):
        gs.cluster_metrics(lab, tgt, n_classes=1)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_einval_without_gpu():
    L = pkg()._native.lib()
    ok = dict(table=16, dtype=1, ldx=8, N=10, ids=16, n=5, Cn=16, bias=16, K=4, D=8, k_live=4, labels_in=None, splits=0,
              partial=16, labels_out=16, dist_out=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.gsage_kmeans_pass(a["table"], a["dtype"], a["ldx"], a["N"], a["ids"], a["n"], a["Cn"], a["bias"], a["K"],
                                   a["D"], a["k_live"], a["labels_in"], a["splits"], a["partial"], a["labels_out"],
                                   a["dist_out"], None)
    for kw, word in ((dict(K=129), b"K must"), (dict(K=0), b"K must"), (dict(D=1025), b"D must"), (dict(D=0), b"D must"),
                     (dict(n=0), b"n must"), (dict(n=2 ** 31), b"n must"), (dict(ldx=7), b"ldx"), (dict(dtype=7), b"dtype"),
                     (dict(k_live=0), b"k_live"), (dict(k_live=5), b"k_live"), (dict(splits=1025), b"splits"),
                     (dict(splits=-1), b"splits"), (dict(Cn=None), b"null"), (dict(N=0), b"N must"),
                     (dict(partial=None, labels_out=None), b"null"), (dict(n=2 ** 24, splits=1), b"splits")):
        assert call(**kw) == -1 and word in L.gsage_last_error(), (kw, L.gsage_last_error())
    uok = dict(partial=16, S=3, K=4, D=8, dtype=1, spherical=0, Cn=16, bias=16, ih=16, ch=16, eh=16, index=16, cap=5)

    def upd(**kw):
        a = dict(uok, **kw)
        return L.gsage_kmeans_update(a["partial"], a["S"], a["K"], a["D"], a["dtype"], a["spherical"], a["Cn"], a["bias"],
                                     a["ih"], a["ch"], a["eh"], a["index"], a["cap"], None)
    for kw, word in ((dict(K=129), b"K must"), (dict(D=0), b"D must"), (dict(S=1025), b"S must"), (dict(S=-1), b"S must"),
                     (dict(dtype=7), b"dtype"), (dict(spherical=2), b"spherical"), (dict(bias=None), b"null"),
                     (dict(index=None), b"null"), (dict(partial=None), b"null"), (dict(cap=0), b"capacity")):
        assert upd(**kw) == -1 and word in L.gsage_last_error(), (kw, L.gsage_last_error())
    W = 41 * 72 + 41 + 2
    assert L.gsage_kmeans_pass_scratch(1000, 41, 72, 0) == 32 * W
    assert L.gsage_kmeans_pass_scratch(1000, 41, 72, 7) == 7 * W
    assert L.gsage_kmeans_pass_scratch(10 ** 6, 41, 72, 0) == 256 * W                   # never more than 256 rows
    assert L.gsage_kmeans_pass_scratch(2 ** 24 - 32, 41, 72, 1) == W
    for bad in ((0, 4, 8, 0), (5, 129, 8, 0), (5, 4, 1025, 0), (5, 4, 8, 1025), (2 ** 31, 4, 8, 0), (2 ** 24, 4, 8, 1)):
        assert L.gsage_kmeans_pass_scratch(*bad) == -1


def test_python_refusals_name_their_reason():
    gs = pkg()
    X = torch.zeros(10, 8)
    X[:, 0] = torch.arange(10)
    with pytest.raises(ValueError, match=r"number of clusters must be in \[1, 128\]"):
        gs.kmeans(torch.zeros(200, 8), 129)
    with pytest.raises(ValueError, match=r"D must be in \[1, 1024\]"):
        gs.kmeans(torch.zeros(10, 1025), 2)
    with pytest.raises(ValueError, match="k = 4 clusters asked of 3 distinct rows"):
        gs.kmeans(X, 4, nodes=torch.tensor([1, 2, 2, 5, 5, 1]))
    bad = X.clone()
    bad[3, 2] = float("inf")
    with pytest.raises(ValueError, match="non-finite values"):
        gs.kmeans(bad, 2)
    assert gs.kmeans(bad, 2, nodes=torch.tensor([0, 1, 2, 4])).n_iter >= 1               # only the rows to cluster count
    with pytest.raises(IndexError, match="node id out of range of the 10 embedding rows"):
        gs.kmeans(X, 2, nodes=torch.tensor([0, 10]))
    with pytest.raises(IndexError, match="node id out of range"):
        gs.kmeans(X, 2, nodes=torch.tensor([-1, 3]))
    with pytest.raises(ValueError, match="iters must be at least 1"):
        gs.kmeans(X, 2, iters=0)
    with pytest.raises(ValueError, match="n_init must be at least 1"):
        gs.kmeans(X, 2, n_init=0)
    with pytest.raises(ValueError, match="node ids must be integers"):
        gs.kmeans(X, 2, nodes=torch.tensor([0.0, 1.0]))
    with pytest.raises(ValueError, match='init must be "\\+\\+", "random" or a \\[k, D\\] tensor'):
        gs.kmeans(X, 2, init="farthest")
    with pytest.raises(ValueError, match=r"init as a tensor must be float \[2, 8\]"):
        gs.kmeans(X, 2, init=torch.zeros(3, 8))
    with pytest.raises(ValueError, match="centroids must be fp32"):
        gs.ops.kmeans_pass(X, torch.arange(10), torch.zeros(2, 8, dtype=torch.float64), torch.zeros(2))
    with pytest.raises(ValueError, match="the table has 8 columns"):
        gs.ops.kmeans_pass(X, torch.arange(10), torch.zeros(2, 9), torch.zeros(2))
    with pytest.raises(ValueError, match=r"labels_in must be int32 \[10\]"):
        gs.ops.kmeans_pass(X, torch.arange(10), torch.zeros(2, 8), torch.zeros(2), labels_in=torch.zeros(10))
    with pytest.raises(ValueError, match=r"partial must be fp32 \[S, 20\]"):
        gs.ops.kmeans_update(torch.zeros(2, 8), torch.zeros(2), torch.zeros(1, 19))


# ---- 6. command line ---------------------------------------------------------------------------------------------------
ARGV = ["--problem-path", "<memory>", "--sampler-class", "sparse_uniform_neighbor_sampler", "--aggregator-class", "mean",
        "--epochs", "1", "--batch-size", "128", "--n-train-samples", "5,3", "--n-val-samples", "5,3", "--output-dims",
        "16,16", "--no-cuda", "--show-test"]


def _cluster_lines(out):
    return [json.loads(l)["cluster"] for l in out.splitlines() if l.startswith('{"cluster"')]


@pytest.mark.parametrize("task", ["classification", "regression_mae"])
def test_cli_cluster_prints_its_lines_and_saves_the_clusters(task, tmp_path, capsys):
    train = importlib.import_module("pytorch-graphsage_amd.train")
    path = str(tmp_path / "clusters.npz")
    train.main(ARGV + ["--cluster", "4", "--cluster-iters", "20", "--cluster-seed", "1", "--save-clusters", path],
               problem=sparse_problem(task, cuda=False))
    lines = _cluster_lines(capsys.readouterr().out)
    assert [l["fold"] for l in lines] == ["val", "test"]
    for l in lines:
        want = {"fold", "k", "iters", "inertia"} | ({"nmi", "purity"} if task == "classification" else set())
        assert set(l) == want and l["k"] == 4 and 1 <= l["iters"] <= 20 and np.isfinite(l["inertia"]) and l["inertia"] >= 0
        if task == "classification":
            assert 0.0 <= l["nmi"] <= 1.0 and 0.0 < l["purity"] <= 1.0
    z = np.load(path)
    assert z["nodes"].shape == (900,) and z["labels"].shape == (900,) and z["centroids"].shape == (4, 32)
    assert sorted(z["nodes"].tolist()) == list(range(1, 901)) and set(z["labels"].tolist()) <= {0, 1, 2, 3}


def test_cli_cluster_refuses_bad_flags(capsys):
    train = importlib.import_module("pytorch-graphsage_amd.train")
    with pytest.raises(SystemExit, match="--save-clusters goes with --cluster K"):
        train.main(ARGV + ["--save-clusters", "x.npz"], problem=sparse_problem("classification", cuda=False))
    with pytest.raises(SystemExit, match="--cluster-iters >= 1"):
        train.main(ARGV + ["--cluster", "3", "--cluster-iters", "0"], problem=sparse_problem("classification", cuda=False))
    with pytest.raises(SystemExit, match=r"--cluster: kmeans: the number of clusters must be in \[1, 128\]"):
        train.main(ARGV + ["--cluster", "129"], problem=sparse_problem("classification", cuda=False))
    capsys.readouterr()
