"""Graph propagation on the MI355X (csrc/gsage_propagate.hip behind ops.propagate_step / propagate.py): one step
against the float64 restatement across the team sizes and store paths, the out-of-range rule, 50 iterations, bitwise
determinism, label propagation and Correct and Smooth against float64, GPU == host mode on the toy, two launches per
step whatever the graph, and the train.py flags."""
import importlib
import json
import sys

import numpy as np
import pytest
import torch

import propagate_ref as R
from cli_problems import sparse_problem
from conftest import pkg
from full_neighbour_ref import sparse_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5                          # the project's fp32 bound (test_gpu_full_neighbour.py), absolute plus relative
LONG = (17, 20500)                  # one row far above infer.SLICE_LEN
EMPTY, ONLY_EMPTY = 10, 5           # row 10 has no edges; row 5's only neighbour is row 10
ALPHA, BETA = 0.8, 0.2
SENTINEL = -777.0


def near(got, ref, what):
    """|got - ref| <= TOL + TOL * |ref|, element by element"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref) - TOL * np.abs(ref)
    assert float(err.max()) <= TOL, (what, "largest excess error %g at %r" % (float(err.max()), np.unravel_index(err.argmax(), err.shape)))


def _csr(indptr, col, n):
    gs = pkg()
    return gs.DeviceCSR(torch.from_numpy(np.asarray(indptr, dtype=np.int64)).to(DEV),
                        torch.from_numpy(np.asarray(col, dtype=np.int32)).to(DEV), n, 1)


@pytest.fixture(scope="module")
def graph():
    """1 501 rows: row 0 the empty dummy, every 7th row empty, rows of degree 1, one row of 20 500 edges."""
    rng = np.random.RandomState(21)
    n = 1500
    _, indptr, data = sparse_graph(n, rng, max_deg=40, long_row=LONG)
    col = data.astype(np.int32)
    deg = np.diff(indptr)
    assert deg[EMPTY] == 0 and deg[ONLY_EMPTY] == 1 and deg[0] == 0 and (deg == 0).sum() > 150
    col[indptr[ONLY_EMPTY]] = EMPTY
    assert (deg[col] == 0).sum() > 100                 # edges that point at empty rows
    sptr, scol = R.symmetrise(indptr, col, n + 1)
    return {"n": n + 1, "indptr": indptr, "col": col, "sym": (sptr, scol)}


_REF = {}


def _one_step_case(gs, graph, C, norm):
    """Inputs of a one-step case and its float64 accumulation (shared by the clamp / output variants)."""
    key = (C, norm)
    if key not in _REF:
        n = graph["n"]
        rng = np.random.RandomState(C)
        Cp = (C + 3) // 4 * 4
        adj = _csr(graph["indptr"], graph["col"], n)
        a, b = gs.ops.propagate_scales(adj.rowptr, n, norm)
        x = torch.from_numpy(rng.normal(size=(n, Cp)).astype(np.float32)).to(DEV)
        y = torch.zeros(n, Cp + 4, dtype=torch.float32, device=DEV)           # a row stride above round_up(C, 4)
        y[:, :Cp] = b.view(-1, 1) * x
        base = torch.from_numpy(rng.normal(size=(n, Cp)).astype(np.float32)).to(DEV)
        dst, src, bad = R.edges(graph["indptr"], graph["col"], n)
        assert bad == 0
        acc = R.row_sums(dst, src, n, y[:, :C].double().cpu().numpy())
        _REF[key] = (adj, a, b, y, base, acc)
    return _REF[key]


# ---- 1. one step against float64 ---------------------------------------------------------------------------------------
# C: one chunk, a padded chunk, teams of 8 (C <= 32), 16 (41), 32 (121, 128) and 64 (130: 33 chunks), and 260: 65 chunks,
# where a team of 64 lanes wraps once
@pytest.mark.parametrize("norm", ["sym", "row", "col"])
@pytest.mark.parametrize("C", [1, 3, 41, 121, 128, 130, 260])
def test_one_step_matches_float64(graph, C, norm):
    gs = pkg()
    n = graph["n"]
    adj, a, b, y, base, acc = _one_step_case(gs, graph, C, norm)
    plan = gs.infer.plan(adj)
    assert plan["n_long"] == 1 and plan["n_slices"] == 81
    a64, b64, base64 = a.double().cpu().numpy(), b.double().cpu().numpy(), base[:, :C].double().cpu().numpy()
    for lo, hi in ((-float("inf"), float("inf")), (-0.5, 0.75)):
        ref = np.minimum(np.maximum(BETA * base64 + ALPHA * (a64[:, None] * acc), lo), hi)
        for mode in ("out", "yout", "both"):
            ld = (C + 3) // 4 * 4 + 8                                         # strided outputs: ldo > C
            out = torch.full((n, ld), SENTINEL, dtype=torch.float32, device=DEV) if mode != "yout" else None
            yout = torch.full((n, ld), SENTINEL, dtype=torch.float32, device=DEV) if mode != "out" else None
            gs.ops.propagate_step(adj, plan, y, base, a, b, ALPHA, BETA, lo, hi, C, out=out, yout=yout)
            what = "C=%d %s clamp=(%g, %g) %s" % (C, norm, lo, hi, mode)
            if out is not None:
                got = out.cpu()
                assert bool((got[:, C:] == SENTINEL).all()), what + ": a column >= C was stored"
                near(got[:, :C].numpy(), ref, what)
                near(got[LONG[0], :C].numpy(), ref[LONG[0]], what + " long row")
                near(got[ONLY_EMPTY, :C].numpy(), ref[ONLY_EMPTY], what + " row whose only neighbour is empty")
                want = torch.clamp(BETA * base[EMPTY, :C], lo, hi)
                assert torch.equal(out[EMPTY, :C], want), what + ": an empty row is beta * base exactly"
                assert torch.equal(out[0, :C], torch.clamp(BETA * base[0, :C], lo, hi))
            if yout is not None:
                got = yout.cpu()
                assert bool((got[:, C:] == SENTINEL).all()), what + ": a column >= C of yout was stored"
                near(got[:, :C].numpy(), b64[:, None] * ref, what + " yout")
                if out is not None:
                    assert torch.equal(yout[:, :C], b.view(-1, 1) * out[:, :C])
    assert int(adj.err_flag.item()) == 0


def test_one_step_without_scales_and_without_base(graph):
    """a = b = NULL read as 1 (yout = out bit for bit), base = NULL with beta = 0."""
    gs = pkg()
    n, C = graph["n"], 41
    adj, _, _, y, _, _ = _one_step_case(gs, graph, C, "row")                  # (norm row: y = x)
    dst, src, _ = R.edges(graph["indptr"], graph["col"], n)
    acc = R.row_sums(dst, src, n, y[:, :C].double().cpu().numpy())
    out, yout = (torch.zeros(n, 44, dtype=torch.float32, device=DEV) for _ in range(2))
    gs.ops.propagate_step(adj, gs.infer.plan(adj), y, None, None, None, 0.5, 0.0, -float("inf"), float("inf"), C,
                          out=out, yout=yout)
    near(out[:, :C].cpu().numpy(), 0.5 * acc, "no scales, no base")
    assert torch.equal(out, yout)


def test_scales_match_the_definition(graph):
    gs = pkg()
    n = graph["n"]
    rowptr = torch.from_numpy(graph["indptr"]).to(DEV)
    for norm in ("sym", "row", "col"):
        a, b = gs.ops.propagate_scales(rowptr, n, norm)
        ra, rb = R.scales(graph["indptr"], n, norm)
        assert np.allclose(a.cpu().numpy(), ra, rtol=1e-6, atol=0) and np.allclose(b.cpu().numpy(), rb, rtol=1e-6, atol=0)
        assert float(a[EMPTY]) == (1.0 if norm == "col" else 0.0) and float(b[EMPTY]) == (1.0 if norm == "row" else 0.0)


# ---- 2. an id outside the graph ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [100, LONG[0]])
def test_out_of_range_id_is_dropped_and_flagged(graph, row):
    gs = pkg()
    n, C = graph["n"], 41
    adj, a, b, y, base, acc = _one_step_case(gs, graph, C, "sym")
    plan = gs.infer.plan(adj)
    inf = float("inf")
    clean = torch.zeros(n, 44, dtype=torch.float32, device=DEV)
    gs.ops.propagate_step(adj, plan, y, base, a, b, ALPHA, BETA, -inf, inf, C, out=clean)
    col = graph["col"].copy()
    e = int(graph["indptr"][row]) + 1
    assert graph["indptr"][row + 1] > e
    col[e] = n                                                                # one edge patched to n_rows
    bad = _csr(graph["indptr"], col, n)
    got = torch.zeros(n, 44, dtype=torch.float32, device=DEV)
    gs.ops.propagate_step(bad, gs.infer.plan(bad), y, base, a, b, ALPHA, BETA, -inf, inf, C, out=got)
    assert int(bad.err_flag.item()) == 1 and int(adj.err_flag.item()) == 0
    dropped = acc[row] - y[int(graph["col"][e]), :C].double().cpu().numpy()
    ref = BETA * base[row, :C].double().cpu().numpy() + ALPHA * float(a[row]) * dropped
    near(got[row, :C].cpu().numpy(), ref, "the row with the edge dropped")
    others = torch.ones(n, dtype=torch.bool, device=DEV)
    others[row] = False
    assert torch.equal(got[others], clean[others])


# ---- 3. fifty iterations -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def iterated(graph):
    """x_0, and the float64 iterates 1, 2, 3, 49 and 50 on the symmetrised graph (alpha 0.8, clamp (0, 1))."""
    n, C = graph["n"], 41
    x = np.random.RandomState(4).rand(n, C).astype(np.float32)
    sptr, scol = graph["sym"]
    dst, src, _ = R.edges(sptr, scol, n)
    a, b = R.scales(sptr, n, "sym")
    xs, cur, base = {}, x.astype(np.float64), x.astype(np.float64)
    y = b[:, None] * cur
    for t in range(1, 51):
        cur, y = R.step(dst, src, n, y, base, a, b, 0.8, 1.0 - 0.8, 0.0, 1.0)
        if t <= 3 or t >= 49:
            xs[t] = cur
    return x, xs


@pytest.mark.parametrize("iters", [1, 2, 3, 49, 50])
def test_fifty_iterations_match_float64(graph, iterated, iters):
    """Odd and even counts end in different ping-pong buffers.  Iterates 49 and 50 differ by about 0.8^49 = 2e-5, so the
    parity is also checked at 1, 2 and 3, where neighbouring iterates are far apart."""
    gs = pkg()
    x, xs = iterated
    adj = _csr(*graph["sym"], graph["n"])
    got = gs.propagate(adj, torch.from_numpy(x).to(DEV), iters, 0.8, clamp=(0.0, 1.0))
    assert got.dtype == torch.float32 and tuple(got.shape) == x.shape
    near(got.cpu().numpy(), xs[iters], "%d iterations" % iters)
    assert np.abs(xs[2] - xs[1]).max() > 1e-2 and np.abs(xs[3] - xs[2]).max() > 1e-2


def test_zero_iterations_return_the_input(graph, iterated):
    gs = pkg()
    x = torch.from_numpy(iterated[0]).to(DEV)
    assert torch.equal(gs.propagate(_csr(*graph["sym"], graph["n"]), x, 0, 0.8, clamp=(0.0, 1.0)), x)


# ---- 4. determinism ----------------------------------------------------------------------------------------------------
def test_bitwise_deterministic_and_independent_of_the_grid(graph, iterated):
    gs = pkg()
    n, x = graph["n"], torch.from_numpy(iterated[0]).to(DEV)
    indptr, col = graph["indptr"], graph["col"]                               # (the long row: n_long == 1)
    adj = _csr(indptr, col, n)
    r1 = gs.propagate(adj, x, 7, 0.8, clamp=(0.0, 1.0))
    r2 = gs.propagate(adj, x, 7, 0.8, clamp=(0.0, 1.0))
    assert gs.infer.plan(adj)["n_long"] == 1 and torch.equal(r1, r2)
    # 700 more empty rows: another grid, the same rows
    big = _csr(np.concatenate([indptr, np.full(700, indptr[-1])]), col, n + 700)
    xb = torch.cat([x, torch.rand(700, x.shape[1], device=DEV)])
    r3 = gs.propagate(big, xb, 7, 0.8, clamp=(0.0, 1.0))
    assert torch.equal(r3[:n], r1)
    # another slice length: another summation order of the long row, the same numbers to round-off
    r4 = gs.propagate(_csr(indptr, col, n), x, 7, 0.8, clamp=(0.0, 1.0), slice_len=64)
    near(r4.cpu().numpy(), r1.cpu().numpy(), "slice_len 64 against 256")
    ref = R.propagate(indptr, col, iterated[0], 7, 0.8, clamp=(0.0, 1.0))
    near(r1.cpu().numpy(), ref, "7 iterations with the long row")


# ---- 5. label propagation, Correct and Smooth ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def labelled(graph):
    """The symmetrised graph plus an island of six unlabelled rows in a ring; 30 % of the other rows labelled."""
    n = graph["n"]
    sptr, scol = graph["sym"]
    ring = np.arange(n, n + 6)
    icol = np.stack([np.roll(ring, 1), np.roll(ring, -1)], 1).reshape(-1)
    ptr = np.concatenate([sptr, sptr[-1] + 2 * np.arange(1, 7)])
    col = np.concatenate([scol, icol]).astype(np.int32)
    rng = np.random.RandomState(8)
    nodes = np.sort(rng.choice(np.arange(1, n), int(0.3 * n), replace=False))
    # rows no labelled node reaches: the island, and the rows without edges that carry no label
    unreached = np.concatenate([ring, np.setdiff1d(np.flatnonzero(np.diff(ptr)[:n] == 0), nodes)])
    return {"n": n + 6, "ptr": ptr, "col": col, "nodes": nodes, "unreached": unreached, "rng": rng}


def _targets(task, m, C, rng):
    return rng.randint(0, C, size=m) if task == "classification" else (rng.rand(m, C) < 0.3).astype(np.float32)


@pytest.mark.parametrize("task,C", [("classification", 41), ("multilabel_classification", 121)])
def test_label_propagation_matches_float64(labelled, task, C):
    gs = pkg()
    g = labelled
    tg = _targets(task, g["nodes"].size, C, np.random.RandomState(C))
    got = gs.label_propagation(_csr(g["ptr"], g["col"], g["n"]), torch.from_numpy(tg).to(DEV),
                               torch.from_numpy(g["nodes"]).to(DEV), n_classes=C, task=task)
    ref = R.label_propagation(g["ptr"], g["col"], g["n"], tg, g["nodes"], C, task=task)
    near(got.cpu().numpy(), ref, "label propagation")
    assert not got[torch.from_numpy(g["unreached"]).to(DEV)].any()


@pytest.mark.parametrize("autoscale", [True, False])
@pytest.mark.parametrize("task,C", [("classification", 41), ("multilabel_classification", 121)])
def test_correct_and_smooth_matches_float64(labelled, task, C, autoscale):
    gs = pkg()
    g = labelled
    rng = np.random.RandomState(C + autoscale)
    tg = _targets(task, g["nodes"].size, C, rng)
    logits = rng.normal(size=(g["n"], C)).astype(np.float32)
    ref = R.correct_and_smooth(g["ptr"], g["col"], logits, tg, g["nodes"], task, autoscale=autoscale, scale=0.9)
    if autoscale:                      # no row within 1 % of the cut-off, where fp32 could fall on the other side
        s = ref["s_raw"][np.isfinite(ref["s_raw"])]
        assert not ((s > 0.99 * R.AUTOSCALE_MAX) & (s < 1.01 * R.AUTOSCALE_MAX)).any()
    adj = _csr(g["ptr"], g["col"], g["n"])
    mod = sys.modules[gs.propagate.__module__]
    Z, E, Zr, G = mod._correct_and_smooth(adj, torch.from_numpy(logits).to(DEV), torch.from_numpy(tg).to(DEV),
                                          torch.from_numpy(g["nodes"]).to(DEV), task, (50, 50), (0.8, 0.8), "sym",
                                          autoscale, 0.9)
    near(E.cpu().numpy(), ref["E"], "E")
    near(Zr.cpu().numpy(), ref["Zr"], "Zr")
    near(G.cpu().numpy(), ref["G"], "G")
    un = torch.from_numpy(g["unreached"]).to(DEV)
    assert not E[un].any(), "rows no labelled node reaches keep E == 0 exactly"
    assert torch.equal(Zr[un], Z[un])
    pub = gs.correct_and_smooth(adj, torch.from_numpy(logits).to(DEV), torch.from_numpy(tg).to(DEV),
                                torch.from_numpy(g["nodes"]).to(DEV), task, autoscale=autoscale, scale=0.9)
    assert torch.equal(pub, G)


# ---- 6. GPU == host mode on the toy ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_gpu_equals_host_mode_on_the_toy(seed):
    gs = pkg()
    t = R.toy(seed)
    mod = sys.modules[gs.propagate.__module__]
    res = {}
    for dev in ("cpu", DEV):
        adj = gs.DeviceCSR(torch.from_numpy(t["indptr"]).to(dev), torch.from_numpy(t["col"]).to(dev), t["n_rows"], 1)
        nodes, tg = torch.from_numpy(t["train"]).to(dev), torch.from_numpy(t["labels"][t["train"]]).to(dev)
        _, _, Zr, G = mod._correct_and_smooth(adj, torch.from_numpy(t["logits"]).to(dev), tg, nodes, "classification",
                                              (50, 50), (0.8, 0.8), "sym", True, 1.0)
        lp = gs.label_propagation(adj, tg, nodes, n_classes=R.TOY_C)
        res[dev] = {"Zr": Zr.cpu().numpy(), "G": G.cpu().numpy(), "lp": lp.cpu().numpy()}
    for k in ("Zr", "G", "lp"):
        near(res[DEV][k], res["cpu"][k], "toy %s, gpu against host mode" % k)
    ref = R.correct_and_smooth(t["indptr"], t["col"], t["logits"], t["labels"][t["train"]], t["train"], "classification")
    rlp = R.label_propagation(t["indptr"], t["col"], t["n_rows"], t["labels"][t["train"]], t["train"], R.TOY_C)
    want = R.toy_accuracies(t, ref, rlp)
    got = R.toy_accuracies(t, res[DEV], res[DEV]["lp"])
    print("toy seed %d: base %.3f corrected %.3f smoothed %.3f label propagation %.3f" % ((seed,) + got))
    assert got == want
    assert got[2] > got[1] > got[0] and got[3] > got[0]


# ---- 7. two launches per step, whatever the graph ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1500, 300])
def test_ten_iterations_are_twenty_launches(n):
    gs = pkg()
    rng = np.random.RandomState(n)
    _, indptr, data = sparse_graph(n, rng, max_deg=40, long_row=LONG if n == 1500 else None)
    adj = _csr(indptr, data, n + 1)
    x = torch.rand(n + 1, 41, device=DEV)
    direct = gs.propagate(adj, x, 10, 0.8, clamp=(0.0, 1.0))                  # (builds the plan and the scales)
    torch.cuda.synchronize()
    c0 = gs._native.launch_count()
    again = gs.propagate(adj, x, 10, 0.8, clamp=(0.0, 1.0))
    torch.cuda.synchronize()
    assert gs._native.launch_count() - c0 == 20 and torch.equal(again, direct)
    # recorded: the list stores raw pointers, so the workspace owns every buffer the launches touch
    mod = sys.modules[gs.propagate.__module__]
    ws = mod.Workspace()
    with gs._native.CommandList.record() as cl:
        rec = gs.propagate(adj, x, 10, 0.8, clamp=(0.0, 1.0), workspace=ws)
    assert len(cl) == 20 and rec.data_ptr() == ws.result.data_ptr()
    # whatever the allocator hands out now must not be a buffer of the list: fill a dozen blocks of the same size
    junk = [torch.full((n + 1, 44), SENTINEL, device=DEV) for _ in range(12)]
    held = {t.data_ptr() for t in ws.held if torch.is_tensor(t)}
    assert len(held) >= 6 and not held & {t.data_ptr() for t in junk}
    stream = gs.ops._stream()
    for _ in range(2):                                                        # a replay gives the same bits, every time
        rec.fill_(SENTINEL)
        cl.replay(stream)
        torch.cuda.synchronize()
        assert torch.equal(rec, direct)
    del junk


# ---- 8. command line ------------------------------------------------------------------------------------------------------
ARGV = ["--problem-path", "<memory>", "--sampler-class", "sparse_uniform_neighbor_sampler", "--aggregator-class", "mean",
        "--epochs", "1", "--batch-size", "128", "--n-train-samples", "5,3", "--n-val-samples", "5,3", "--output-dims",
        "16,16", "--full-neighbour-eval", "--correct-smooth", "--label-prop", "--show-test"]


@pytest.mark.parametrize("task", ["classification", "multilabel_classification"])
def test_cli_prints_its_lines(task, capsys):
    train = importlib.import_module("pytorch-graphsage_amd.train")
    train.main(ARGV, problem=sparse_problem(task))
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    cs = [l["correct_smooth"] for l in lines if "correct_smooth" in l]
    lp = [l["label_prop"] for l in lines if "label_prop" in l]
    assert [l["fold"] for l in cs] == ["val", "test"] and [l["fold"] for l in lp] == ["val", "test"]
    for l in cs:
        assert set(l) == {"fold", "task", "base", "corrected", "smoothed"} and l["task"] == task
        for k in ("base", "corrected", "smoothed"):
            assert set(l[k]) == {"micro", "macro"} and 0.0 <= l[k]["micro"] <= 1.0 and 0.0 <= l[k]["macro"] <= 1.0
    for l in lp:
        assert set(l) == {"fold", "task", "micro", "macro"} and 0.0 <= l["micro"] <= 1.0
    # "base" is what --full-neighbour-eval prints for the same fold
    val = [l for l in lines if "val_metric" in l][-1]["val_metric"]
    test = [l for l in lines if "test_f1" in l][-1]["test_f1"]
    assert cs[0]["base"] == val and cs[1]["base"] == test


def test_cli_refuses_a_regression_problem(capsys):
    train = importlib.import_module("pytorch-graphsage_amd.train")
    with pytest.raises(SystemExit, match="--correct-smooth: labels are propagated as class scores"):
        train.main(ARGV, problem=sparse_problem("regression_mae"))
    capsys.readouterr()
