"""Graph propagation without a GPU (propagate.py, ops.propagate_step in host mode): against the float64 restatement of
the definition, every refusal, the C ABI's argument validation, the train.py flags, and the planted-partition toy on
which Correct and Smooth and label propagation must beat the noisy base predictions."""
import ctypes
import importlib
import sys

import numpy as np
import pytest
import torch

import propagate_ref as R
from conftest import pkg
from full_neighbour_ref import make_model, sparse_graph
from util import close

TOL = 2e-5                          # the project's fp32 bound (host mode computes in fp32 torch)


def _csr(indptr, col, n):
    gs = pkg()
    return gs.DeviceCSR(torch.from_numpy(np.asarray(indptr, dtype=np.int64)),
                        torch.from_numpy(np.asarray(col, dtype=np.int32)), n, 1)


@pytest.fixture(scope="module")
def graph():
    rng = np.random.RandomState(3)
    n = 400
    _, indptr, data = sparse_graph(n, rng, max_deg=12, long_row=(17, 700))
    return {"n": n + 1, "indptr": indptr, "col": data.astype(np.int32), "rng": rng}


# ---- 1. host mode against float64 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["sym", "row", "col"])
@pytest.mark.parametrize("clamp", [None, (0.0, 1.0)])
@pytest.mark.parametrize("iters", [0, 1, 4, 5])
def test_host_propagate_matches_float64(graph, norm, clamp, iters):
    gs = pkg()
    n, C = graph["n"], 7
    rng = np.random.RandomState(iters)
    x = rng.normal(size=(n, C)).astype(np.float32)
    base = rng.normal(size=(n, C)).astype(np.float32)
    adj = _csr(graph["indptr"], graph["col"], n)
    got = gs.propagate(adj, torch.from_numpy(x), iters, 0.8, base=torch.from_numpy(base), norm=norm, clamp=clamp)
    ref = R.propagate(graph["indptr"], graph["col"], x, iters, 0.8, base=base, norm=norm, clamp=clamp)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, C)
    close(got.numpy(), ref, "propagate", TOL, TOL)
    if iters == 0:
        assert torch.equal(got, torch.from_numpy(x))


def test_host_propagate_default_base_and_fixed_rows(graph):
    gs = pkg()
    n, C = graph["n"], 5
    rng = np.random.RandomState(9)
    x = rng.rand(n, C).astype(np.float32)
    ids = np.arange(1, n, 3)
    vals = rng.rand(ids.size, C).astype(np.float32)
    adj = _csr(graph["indptr"], graph["col"], n)
    got = gs.propagate(adj, torch.from_numpy(x), 6, 0.7, clamp=(0, 1), fixed=(torch.from_numpy(ids), torch.from_numpy(vals)))
    ref = R.propagate(graph["indptr"], graph["col"], x, 6, 0.7, clamp=(0.0, 1.0), fixed=(ids, vals))
    close(got.numpy(), ref, "fixed rows", TOL, TOL)
    # an empty row keeps (1 - alpha) * base: row 0 is the empty dummy
    close(got[0].numpy(), 0.3 * x[0].astype(np.float64), "empty row", TOL, TOL)


def test_host_step_drops_an_out_of_range_id_and_raises_the_flag(graph):
    gs = pkg()
    n, C = graph["n"], 6
    col = graph["col"].copy()
    e = int(graph["indptr"][40])                       # first edge of row 40 (degree >= 1)
    col[e] = n
    adj = _csr(graph["indptr"], col, n)
    y = torch.from_numpy(np.random.RandomState(1).normal(size=(n, 8)).astype(np.float32))
    out = torch.zeros(n, C)
    gs.ops.propagate_step(adj, None, y, None, None, None, 1.0, 0.0, -float("inf"), float("inf"), C, out=out)
    assert int(adj.err_flag.item()) == 1
    dst, src, bad = R.edges(graph["indptr"], col, n)
    assert bad == 1
    ref, _ = R.step(dst, src, n, y.numpy().astype(np.float64)[:, :C], None, np.ones(n), np.ones(n), 1.0, 0.0, -np.inf, np.inf)
    close(out.numpy(), ref, "dropped edge", TOL, TOL)
    with pytest.raises(IndexError):
        gs.propagate(adj, y[:, :C].contiguous(), 2, 0.5)


@pytest.mark.parametrize("task", ["classification", "multilabel_classification"])
def test_host_label_propagation_matches_float64(graph, task):
    gs = pkg()
    n, C = graph["n"], 4
    rng = np.random.RandomState(5)
    nodes = np.sort(rng.choice(np.arange(1, n), 120, replace=False))
    tg = rng.randint(0, C, size=nodes.size) if task == "classification" else (rng.rand(nodes.size, C) < 0.4).astype(np.float32)
    adj = _csr(graph["indptr"], graph["col"], n)
    got = gs.label_propagation(adj, torch.from_numpy(tg), torch.from_numpy(nodes), n_classes=C, task=task, iters=20)
    ref = R.label_propagation(graph["indptr"], graph["col"], n, tg, nodes, C, task=task, iters=20)
    close(got.numpy(), ref, "label propagation", TOL, TOL)


@pytest.mark.parametrize("autoscale", [True, False])
@pytest.mark.parametrize("task", ["classification", "multilabel_classification"])
def test_host_correct_and_smooth_matches_float64(graph, task, autoscale):
    gs = pkg()
    n, C = graph["n"], 5
    rng = np.random.RandomState(6)
    ptr, col = R.symmetrise(graph["indptr"], graph["col"], n)
    nodes = np.sort(rng.choice(np.arange(1, n), 150, replace=False))
    tg = rng.randint(0, C, size=nodes.size) if task == "classification" else (rng.rand(nodes.size, C) < 0.4).astype(np.float32)
    logits = rng.normal(size=(n, C)).astype(np.float32)
    adj = _csr(ptr, col, n)
    got = gs.correct_and_smooth(adj, torch.from_numpy(logits), torch.from_numpy(tg), torch.from_numpy(nodes), task,
                                iters=(12, 9), alpha=(0.8, 0.7), autoscale=autoscale, scale=0.9)
    ref = R.correct_and_smooth(ptr, col, logits, tg, nodes, task, iters=(12, 9), alpha=(0.8, 0.7), autoscale=autoscale,
                               scale=0.9)
    if autoscale:                                      # no row sits at the cut-off, where fp32 could fall on the other side
        s = ref["s_raw"][np.isfinite(ref["s_raw"])]
        assert not ((s > 0.99 * R.AUTOSCALE_MAX) & (s < 1.01 * R.AUTOSCALE_MAX)).any()
    close(got.numpy(), ref["G"], "correct and smooth", TOL, TOL)


# ---- 2. refusals -------------------------------------------------------------------------------------------------------
def test_refusals(graph):
    gs = pkg()
    n = graph["n"]
    adj = _csr(graph["indptr"], graph["col"], n)
    x = torch.zeros(n, 3)
    nodes, tg = torch.tensor([1, 2]), torch.tensor([0, 1])
    with pytest.raises(ValueError, match="classification or multilabel_classification"):
        gs.label_propagation(adj, torch.zeros(2, 1), nodes, task="regression_mae")
    with pytest.raises(ValueError, match="classification or multilabel_classification"):
        gs.correct_and_smooth(adj, x, tg, nodes, "regression_mae")
    dense = gs.DenseAdj(torch.zeros(n, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="dense adjacency"):
        gs.propagate(dense, x, 1, 0.5)
    weighted = _csr(graph["indptr"], graph["col"], n).with_weights(np.ones(graph["col"].size, dtype=np.float32))
    with pytest.raises(ValueError, match="weighted adjacency"):
        gs.propagate(weighted, x, 1, 0.5)
    with pytest.raises(ValueError, match="weighted adjacency"):
        gs.correct_and_smooth(weighted, x, tg, nodes, "classification")
    block = gs.infer.closure(adj, torch.tensor([5, 9]), 1).blocks[1]
    with pytest.raises(ValueError, match="Block of a closure"):
        gs.propagate(block, x, 1, 0.5)
    with pytest.raises(ValueError, match=r"\[1, 1024\]"):
        gs.propagate(adj, torch.zeros(n, 1025), 1, 0.5)
    with pytest.raises(ValueError, match="norm must be one of"):
        gs.propagate(adj, x, 1, 0.5, norm="both")
    with pytest.raises(IndexError):
        gs.label_propagation(adj, tg, torch.tensor([1, n]), n_classes=3)


def test_correct_smooth_eval_refuses_what_full_neighbour_inference_refuses():
    gs = pkg()
    rng = np.random.RandomState(0)
    n, D, C = 60, 8, 3
    adj, _, _ = sparse_graph(n, rng, max_deg=5)
    feats = rng.normal(size=(n + 1, D)).astype(np.float32)
    folds = np.array(["train"] * 40 + ["val"] * 10 + ["test"] * (n + 1 - 50))
    prob = gs.NodeProblem.from_arrays("classification", C, adj, adj, feats, folds,
                                      rng.randint(0, C, size=(n + 1, 1)), cuda=False)
    model = make_model("lstm", "identity", adj, D, C=C)
    with pytest.raises(ValueError, match="LSTMAggregator"):
        gs.correct_smooth_eval(model, prob)
    prob.task = "regression_mae"
    with pytest.raises(ValueError, match="classification or multilabel_classification"):
        gs.correct_smooth_eval(make_model("mean", "identity", adj, D, C=C), prob)


def test_correct_smooth_eval_host_scores_every_fold():
    gs = pkg()
    rng = np.random.RandomState(1)
    n, D, C = 200, 8, 3
    adj, _, _ = sparse_graph(n, rng, max_deg=6)
    feats = rng.normal(size=(n + 1, D)).astype(np.float32)
    folds = np.array(["train"] * 120 + ["val"] * 40 + ["test"] * (n + 1 - 160))
    prob = gs.NodeProblem.from_arrays("classification", C, adj, adj, torch.from_numpy(feats), folds,
                                      feats[:, :C].argmax(1).reshape(-1, 1), cuda=False)
    model = make_model("mean", "identity", adj, D, C=C)
    res = gs.correct_smooth_eval(model, prob, iters=(5, 5), label_prop=True)
    assert res["task"] == "classification"
    for fold in ("val", "test"):
        assert set(res[fold]) == {"base", "corrected", "smoothed", "label_prop"}
        for v in res[fold].values():
            assert 0.0 <= v["micro"] <= 1.0 and 0.0 <= v["macro"] <= 1.0


# ---- 3. the C ABI validates its arguments before it touches a GPU -------------------------------------------------------
def _abi_call(L, **kw):
    p = ctypes.c_void_p(64)                            # a plausible, 16-byte aligned address: nothing dereferences it
    a = dict(y=p, ldy=44, base=p, ldb=44, a=p, b=p, alpha=0.8, beta=0.2, lo=0.0, hi=1.0, C=41, rowptr=p, col=p, n_rows=100,
             order=p, n_short=100, slices=None, n_slices=0, long_rows=None, n_long=0, slice_len=256, partials=None, ldp=52,
             out=ctypes.c_void_p(128), ldo=44, yout=ctypes.c_void_p(256), ldyo=44, err=None, stream=None)
    a.update(kw)
    return L.gsage_propagate(a["y"], a["ldy"], a["base"], a["ldb"], a["a"], a["b"], a["alpha"], a["beta"], a["lo"], a["hi"],
                             a["C"], a["rowptr"], a["col"], a["n_rows"], a["order"], a["n_short"], a["slices"],
                             a["n_slices"], a["long_rows"], a["n_long"], a["slice_len"], a["partials"], a["ldp"], a["out"],
                             a["ldo"], a["yout"], a["ldyo"], a["err"], a["stream"])


@pytest.mark.parametrize("kw,word", [
    (dict(C=0), b"[1, 1024]"), (dict(C=1025, ldy=1028, ldb=1028, ldo=1028, ldyo=1028), b"[1, 1024]"),
    (dict(C=5, ldy=6), b"ldy"), (dict(out=None, yout=None), b"both null"), (dict(base=None, beta=0.2), b"base is null"),
    (dict(ldo=40), b"ldo"), (dict(ldyo=43), b"ldyo"), (dict(ldb=8), b"ldb"), (dict(y=ctypes.c_void_p(68)), b"aligned"),
    (dict(out=ctypes.c_void_p(64)), b"alias"), (dict(n_slices=2, n_long=1, n_short=90, slices=ctypes.c_void_p(64),
                                                     long_rows=ctypes.c_void_p(64), partials=ctypes.c_void_p(64), ldp=48),
                                                b"partials"),
    (dict(lo=1.0, hi=0.0), b"lo <= hi"), (dict(n_rows=0), b"n_rows")])
def test_abi_rejects_bad_arguments_without_a_gpu(kw, word):
    L = pkg()._native.lib()
    assert _abi_call(L, **kw) == -1
    assert word in L.gsage_last_error(), L.gsage_last_error()


def test_abi_scales_rejects_bad_arguments_without_a_gpu():
    L = pkg()._native.lib()
    p = ctypes.c_void_p(64)
    assert L.gsage_propagate_scales(p, 10, 3, p, p, None) == -1 and b"norm" in L.gsage_last_error()
    assert L.gsage_propagate_scales(p, 0, 0, p, p, None) == -1 and b"n_rows" in L.gsage_last_error()
    assert L.gsage_propagate_scales(p, 10, 0, None, p, None) == -1 and b"null" in L.gsage_last_error()


def test_host_scales_are_the_definition(graph):
    gs = pkg()
    n = graph["n"]
    for norm in ("sym", "row", "col"):
        a, b = gs.ops.propagate_scales(torch.from_numpy(graph["indptr"]), n, norm)
        ra, rb = R.scales(graph["indptr"], n, norm)
        close(a.numpy(), ra, norm + " a", 1e-6, 1e-7)
        close(b.numpy(), rb, norm + " b", 1e-6, 1e-7)


# ---- 4. command line ------------------------------------------------------------------------------------------------------
def test_cli_flags_parse_and_unsupervised_is_refused():
    train = importlib.import_module("pytorch-graphsage_amd.train")
    args = train.parse_args(["--problem-path", "x", "--correct-smooth", "--cs-iters", "30,20", "--cs-alpha", "0.9,0.6",
                             "--cs-no-autoscale", "--label-prop"])
    assert args.correct_smooth and args.cs_no_autoscale and args.label_prop
    assert train.cs_settings(args) == ((30, 20), (0.9, 0.6))
    args = train.parse_args(["--problem-path", "x"])
    assert not args.correct_smooth and not args.label_prop and train.cs_settings(args) == ((50, 50), (0.8, 0.8))
    with pytest.raises(SystemExit, match="--correct-smooth: --unsupervised trains no classifier"):
        train.main(["--problem-path", "x", "--correct-smooth", "--unsupervised"])
    with pytest.raises(SystemExit, match="--label-prop goes with --correct-smooth"):
        train.main(["--problem-path", "x", "--label-prop"])
    with pytest.raises(SystemExit, match="--cs-iters must be two counts"):
        train.main(["--problem-path", "x", "--correct-smooth", "--cs-iters", "50"])


def test_cli_names_correct_smooth_when_the_model_is_refused(capsys):
    from cli_problems import sparse_problem
    train = importlib.import_module("pytorch-graphsage_amd.train")
    with pytest.raises(SystemExit, match=r"--probe / --correct-smooth: .*LSTMAggregator"):
        train.main(["--problem-path", "<memory>", "--no-cuda", "--sampler-class", "sparse_uniform_neighbor_sampler",
                    "--aggregator-class", "lstm", "--n-train-samples", "5,3", "--n-val-samples", "5,3", "--output-dims",
                    "16,16", "--correct-smooth"], problem=sparse_problem("classification", cuda=False))
    capsys.readouterr()


def test_workspace_owns_the_buffers_of_a_call(graph):
    gs = pkg()
    mod = sys.modules[gs.propagate.__module__]
    n = graph["n"]
    adj = _csr(graph["indptr"], graph["col"], n)
    x = torch.rand(n, 5)
    ws = mod.Workspace()
    got = gs.propagate(adj, x, 4, 0.8, clamp=(0, 1), workspace=ws)
    assert ws.result.data_ptr() == got.data_ptr() and adj in ws.held
    tensors = [t for t in ws.held if torch.is_tensor(t)]
    assert len({t.data_ptr() for t in tensors}) >= 6          # a, b, x_0 (= base), y_0, the result, the ping-pong pair
    assert torch.equal(got, gs.propagate(adj, x, 4, 0.8, clamp=(0, 1)))


# ---- 5. the toy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_toy_correct_and_smooth_beats_the_base_predictions(seed):
    """1 200 nodes, 5 planted classes, 30 % labelled, every 7th node isolated, noisy base logits.  In float64 the test
    accuracies of seeds 0-3 are base 0.31-0.33, corrected 0.80-0.81, smoothed 0.84-0.85, label propagation 0.79-0.82."""
    gs = pkg()
    t = R.toy(seed)
    adj = _csr(t["indptr"], t["col"], t["n_rows"])
    nodes, tg = torch.from_numpy(t["train"]), torch.from_numpy(t["labels"][t["train"]])
    logits = torch.from_numpy(t["logits"])
    mod = sys.modules[gs.propagate.__module__]
    Z, E, Zr, G = mod._correct_and_smooth(adj, logits, tg, nodes, "classification", (50, 50), (0.8, 0.8), "sym", True, 1.0)
    lp = gs.label_propagation(adj, tg, nodes, n_classes=R.TOY_C)
    assert torch.equal(G, gs.correct_and_smooth(adj, logits, tg, nodes, "classification"))
    base, corrected, smoothed, labelprop = R.toy_accuracies(t, {"Zr": Zr.numpy(), "G": G.numpy()}, lp.numpy())
    print("toy seed %d: base %.3f corrected %.3f smoothed %.3f label propagation %.3f"
          % (seed, base, corrected, smoothed, labelprop))
    assert smoothed > corrected > base and labelprop > base
    ref = R.correct_and_smooth(t["indptr"], t["col"], t["logits"], t["labels"][t["train"]], t["train"], "classification")
    close(G.numpy(), ref["G"], "toy G", TOL, TOL)
    # the isolated nodes' residuals stay exactly 0: nothing reaches them
    iso = np.diff(t["indptr"]) == 0
    unl = np.ones(t["n_rows"], dtype=bool)
    unl[t["train"]] = False
    assert not E[torch.from_numpy(iso & unl)].any()
    assert torch.equal(Zr[torch.from_numpy(iso & unl)], Z[torch.from_numpy(iso & unl)])
