"""The linear probe without a GPU: tests/probe_ref.py is the reference's losses (float64 torch autograd), its bound bites on
the GPU tests' own inputs, the host path of ops.probe_pass / gs.linear_probe meets it, and bad arguments are refused."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import probe_ref as pr
from conftest import pkg

MODES = ("bf16", "fp32")


@pytest.fixture(autouse=True)
def _dtype():
    gs = pkg()
    yield
    gs.ops.set_compute_dtype("bf16")


def _bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).double().numpy()


# ---- 1. the definition is the reference's loss ----------------------------------------------------------------------
@pytest.mark.parametrize("task", pr.TASKS)
@pytest.mark.parametrize("case", [(33, 20, 5, 1), (257, 264, 65, 3)])
def test_reference_equals_float64_autograd(case, task):
    """loss, dW and db of probe_ref equal float64 autograd of F.cross_entropy / F.multilabel_soft_margin_loss -- the
    reference's ProblemLosses -- to 1e-12 relative."""
    n, D, C, _ = case
    c = pr.make_case(n, D, C, task)
    ref = pr.case_reference(n, D, C, task, "fp32")
    X = torch.from_numpy(ref["X"])
    W = torch.from_numpy(c["W"].astype(np.float64)).requires_grad_(True)
    b = torch.from_numpy(c["b"].astype(np.float64)).requires_grad_(True)
    z = X @ W.t() + b
    if task == "classification":
        loss = F.cross_entropy(z, torch.from_numpy(c["y"]))
    else:
        loss = F.multilabel_soft_margin_loss(z, torch.from_numpy(c["y"].astype(np.float64)))
    loss.backward()
    rel = lambda a, want: float(np.abs(a - want).max() / np.abs(want).max())
    assert abs(ref["loss"] - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    assert rel(ref["dW"], W.grad.numpy()) <= 1e-12
    assert rel(ref["db"], b.grad.numpy()) <= 1e-12


# ---- 2. the bound bites ------------------------------------------------------------------------------------------------
def _mutants(c, ref, mode):
    """(name, (loss, dW, db)) of results that are wrong in one way each."""
    n, C = c["n"], c["C"]
    X, G = ref["X"], ref["G"]
    out = []
    if n > 1:
        keep = np.arange(n) != n // 2
        out.append(("one row dropped", (ref["rows"][keep].sum() / n, G[keep].T @ X[keep] / n, G[keep].sum(axis=0) / n)))
        s = n / (n - 1.0)
        out.append(("1 / (n - 1) for 1 / n", (ref["loss"] * s, ref["dW"] * s, ref["db"] * s)))
    out.append(("db omitted", (ref["loss"], ref["dW"], np.zeros_like(ref["db"]))))
    y = np.array(c["y"], copy=True)
    a, bcl = 0, c["missing"]                                    # class 0 occurs, class `missing` never does
    if c["task"] == "classification":
        y[c["y"] == a] = bcl
    else:
        y[:, [a, bcl]] = y[:, [bcl, a]]
    sw = pr.reference(c["table"], c["ids"], y, c["W"], c["b"], c["task"], mode)
    out.append(("two classes' targets exchanged", (sw["loss"], sw["dW"], sw["db"])))
    Gr = _bf16(G)
    out.append(("G rounded to one bf16", (ref["loss"], Gr.T @ X / n, ref["db"])))
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("task", pr.TASKS)
@pytest.mark.parametrize("case", pr.CASES)
def test_the_bound_bites_on_the_gpu_tests_inputs(case, task, mode):
    """The reference itself is within the bound (trivially), and a result that drops a row, scales by 1 / (n - 1),
    omits db, exchanges two classes' targets or rounds G to one bf16 is outside it -- on every case of the GPU test."""
    n, D, C, splits = case
    c = pr.make_case(n, D, C, task)
    ref = pr.case_reference(n, D, C, task, mode)
    r = pr.excess((ref["loss"], ref["dW"], ref["db"]), ref, splits)
    assert max(r.values()) == 0.0
    for name, got in _mutants(c, ref, mode):
        r = pr.excess(got, ref, splits)
        print("%-32s loss %.3g  dW %.3g  db %.3g" % (name, r["loss"], r["dW"], r["db"]))
        assert max(r.values()) > 1.0, (name, r)


# ---- 3. the host path ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("task", pr.TASKS)
@pytest.mark.parametrize("case", [(1, 8, 2, 1), (33, 20, 5, 1), (257, 264, 65, 3)])
def test_host_probe_pass_meets_the_reference(case, task, mode):
    gs = pkg()
    gs.ops.set_compute_dtype(mode)
    n, D, C, splits = case
    c = pr.make_case(n, D, C, task)
    ref = pr.case_reference(n, D, C, task, mode)
    table = torch.from_numpy(c["buf"])[:, :D]                   # a view of the NaN-padded buffer
    y = torch.from_numpy(c["ybuf"]) if task == "classification" else torch.from_numpy(c["ybuf"])[:, :C]
    loss, dW, db = gs.ops.probe_pass(table, torch.from_numpy(c["ids"]), y, torch.from_numpy(c["W"]),
                                     torch.from_numpy(c["b"]), task, splits=splits)
    assert loss.dtype == dW.dtype == db.dtype == torch.float32 and tuple(dW.shape) == (C, D) and tuple(db.shape) == (C,)
    pr.compare((float(loss), dW.numpy(), db.numpy()), ref, splits, what="host %s %s %r" % (task, mode, case))


def _fit_host(seed, multilabel, gs):
    X, y = pr.toy(seed, 8 if multilabel else 5, multilabel)
    task = pr.TASKS[1] if multilabel else pr.TASKS[0]
    probe = gs.linear_probe(torch.from_numpy(X), torch.from_numpy(y[:400]), torch.arange(400), task)
    return probe, torch.from_numpy(X), torch.from_numpy(y)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_host_fit_separates_the_toy_classes(seed):
    gs = pkg()
    probe, X, y = _fit_host(seed, False, gs)
    held = torch.arange(400, 600)
    assert torch.equal(probe.predict(X, held), y[400:])                    # held-out accuracy 1.0
    h = probe.loss_history
    assert tuple(h.shape) == (100,) and h.dtype == torch.float32 and bool((h[1:] <= h[:-1]).all())
    assert tuple(probe.W.shape) == (5, 20) and tuple(probe.b.shape) == (5,)
    again, _, _ = _fit_host(seed, False, gs)
    assert torch.equal(again.W, probe.W) and torch.equal(again.b, probe.b) and torch.equal(again.loss_history, h)


@pytest.mark.parametrize("seed", [0, 1])
def test_host_fit_gets_every_toy_bit_right(seed):
    gs = pkg()
    probe, X, y = _fit_host(seed, True, gs)
    assert torch.equal(probe.predict(X, torch.arange(400, 600)), y[400:] > 0.5)
    assert float(probe.loss_history[-1]) < float(probe.loss_history[0])


def test_host_probe_eval_scores_the_folds():
    gs = pkg()
    X, y = pr.toy(0, 5, False)
    folds = np.array(["train"] * 400 + ["val"] * 100 + ["test"] * 100)

    class P(object):
        task, n_classes, targets = "classification", 5, y.reshape(-1, 1)
        nodes = {m: np.where(folds == m)[0] for m in ("train", "val", "test")}
    res = gs.probe_eval(torch.from_numpy(X), P)
    assert sorted(res) == ["iters", "loss_first", "loss_last", "task", "test", "val"]
    assert res["val"] == {"micro": 1.0, "macro": 1.0} and res["test"] == {"micro": 1.0, "macro": 1.0}
    assert res["loss_last"] < res["loss_first"] and res["iters"] == 100


# ---- 4. refusals -------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_einval_without_gpu():
    L = pkg()._native.lib()
    ok = dict(table=16, dtype=1, ldx=8, N=10, ids=16, n=5, targets=16, task=0, ldy=0, W=16, bias=16, C=4, D=8, splits=0,
              partial=16, loss=16)

    def call(**kw):
        a = dict(ok, **kw)
        return L.gsage_probe_pass(a["table"], a["dtype"], a["ldx"], a["N"], a["ids"], a["n"], a["targets"], a["task"],
                                  a["ldy"], a["W"], a["bias"], a["C"], a["D"], a["splits"], a["partial"], a["loss"], None)
    for kw, word in ((dict(C=129), b"C must"), (dict(C=0), b"C must"), (dict(D=1025), b"D must"), (dict(n=0), b"n must"),
                     (dict(n=2 ** 31), b"n must"), (dict(ldx=7), b"ldx"), (dict(task=2), b"task"), (dict(dtype=7), b"dtype"),
                     (dict(task=1, ldy=3), b"ldy"), (dict(splits=1025), b"splits"), (dict(splits=-1), b"splits"),
                     (dict(W=None), b"null"), (dict(loss=None), b"null"), (dict(N=0), b"N must")):
        assert call(**kw) == -1 and word in L.gsage_last_error(), (kw, L.gsage_last_error())
    assert L.gsage_probe_pass_scratch(1000, 41, 72, 0) == 32 * (41 * 72 + 41 + 1)
    assert L.gsage_probe_pass_scratch(1000, 41, 72, 7) == 7 * (41 * 72 + 41 + 1)
    assert L.gsage_probe_pass_scratch(10 ** 6, 41, 72, 0) == 256 * (41 * 72 + 41 + 1)      # never more than 256 rows
    for bad in ((0, 4, 8, 0), (5, 129, 8, 0), (5, 4, 1025, 0), (5, 4, 8, 1025), (2 ** 31, 4, 8, 0)):
        assert L.gsage_probe_pass_scratch(*bad) == -1


def test_python_refusals_name_their_reason():
    gs = pkg()
    X = torch.zeros(10, 8)
    ids = torch.arange(6)
    yc = torch.tensor([0, 1, 2, 0, 1, 2])
    ym = torch.zeros(6, 3)
    with pytest.raises(ValueError, match="a linear probe is a classifier"):
        gs.linear_probe(X, torch.zeros(6), ids, "regression_mae")
    with pytest.raises(ValueError, match=r"number of classes must be in \[1, 128\]"):
        gs.linear_probe(X, yc, ids, "classification", n_classes=129)
    with pytest.raises(ValueError, match=r"D must be in \[1, 1024\]"):
        gs.linear_probe(torch.zeros(10, 1025), yc, ids, "classification")
    with pytest.raises(ValueError, match="integer class ids"):
        gs.linear_probe(X, yc.float(), ids, "classification", n_classes=3)
    with pytest.raises(ValueError, match=r"must have shape \[6\]"):
        gs.linear_probe(X, yc[:5], ids, "classification", n_classes=3)
    with pytest.raises(ValueError, match="must be floating point"):
        gs.linear_probe(X, ym.long(), ids, "multilabel_classification")
    with pytest.raises(ValueError, match=r"must have shape \[6, 3\]"):
        gs.linear_probe(X, ym[:, :2], ids, "multilabel_classification", n_classes=3)
    with pytest.raises(ValueError, match=r"must lie in \[0, 1\]"):
        gs.linear_probe(X, ym + 2.0, ids, "multilabel_classification")
    with pytest.raises(IndexError, match="node id out of range"):
        gs.linear_probe(X, yc, ids + 5, "classification")
    with pytest.raises(ValueError, match="node ids must be integers"):
        gs.linear_probe(X, yc, ids.float(), "classification")
    with pytest.raises(ValueError, match=r"class id out of range \[0, 2\)"):
        gs.linear_probe(X, yc, ids, "classification", n_classes=2)
    with pytest.raises(ValueError, match="W must be fp32"):
        gs.ops.probe_pass(X, ids, yc, torch.zeros(3, 8, dtype=torch.float64), torch.zeros(3), "classification")
    with pytest.raises(ValueError, match="the table has 8 columns"):
        gs.ops.probe_pass(X, ids, yc, torch.zeros(3, 9), torch.zeros(3), "classification")
