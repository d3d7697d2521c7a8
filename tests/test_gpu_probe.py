"""The linear probe on the MI355X (csrc/gsage_probe.hip behind ops.probe_pass / gs.linear_probe / train.py --probe)
against tests/probe_ref.py: the pass within the derived bound for both modes and tasks at the shapes where the kernel
takes another path, bit-identical from call to call, the fit equal to its composition, the toy problems the float64
reference separates, and the command line.  No time is asserted."""
import json

import numpy as np
import pytest
import torch
from scipy import sparse

import probe_ref as pr
from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("bf16", "fp32")


@pytest.fixture(autouse=True)
def _dtype():
    gs = pkg()
    yield
    gs.ops.set_compute_dtype("bf16")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _operands(c, mode):
    """The case on the device: the table as a view of the NaN-padded buffer in the mode's dtype (ldx = D + 3), the
    multilabel targets as a view of theirs (ldy = C + 2)."""
    gs = pkg()
    D, C = c["D"], c["C"]
    table = _dev(c["buf"]).to(gs.ops.torch_dtype(mode))[:, :D]
    assert table.stride(0) == D + 3 and bool(torch.isnan(_dev(c["buf"])[:, D:]).all())
    y = _dev(c["ybuf"]) if c["task"] == "classification" else _dev(c["ybuf"])[:, :C]
    return table, _dev(c["ids"]), y, _dev(c["W"]), _dev(c["b"])


def _pass(case, task, mode, splits=None):
    gs = pkg()
    gs.ops.set_compute_dtype(mode)
    n, D, C, sp = case
    c = pr.make_case(n, D, C, task)
    table, ids, y, W, b = _operands(c, mode)
    loss, dW, db = gs.ops.probe_pass(table, ids, y, W, b, task, splits=sp if splits is None else splits)
    return loss, dW, db


# ---- 1. the pass against float64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("task", pr.TASKS)
@pytest.mark.parametrize("case", pr.CASES)
def test_pass_within_the_bound(case, task, mode):
    gs = pkg()
    n, D, C, splits = case
    before = gs._native.launch_count()
    loss, dW, db = _pass(case, task, mode)
    assert gs._native.launch_count() - before == 3                      # pass, loss, finalise -- nothing else
    assert tuple(dW.shape) == (C, D) and tuple(db.shape) == (C,) and loss.dim() == 0
    ref = pr.case_reference(n, D, C, task, mode)
    pr.compare((float(loss), dW.cpu().numpy(), db.cpu().numpy()), ref, splits, what="%s %s %r" % (task, mode, case))
    miss = pr.make_case(n, D, C, task)["missing"]
    assert float(db[miss]) > 0.0                                        # a class that never occurs is only pushed down


# ---- 2. determinism --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("task", pr.TASKS)
def test_two_calls_are_bit_identical_and_splits_agree(task, mode):
    case = (1000, 72, 41, 7)
    a, b = _pass(case, task, mode), _pass(case, task, mode)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    n, D, C, _ = case
    ref = pr.case_reference(n, D, C, task, mode)
    for splits in (0, 1, 64):
        o = _pass(case, task, mode, splits=splits)
        # both lie within their own bound of the reference, so they agree within twice the (larger) bound
        for got, sp in ((a, 7), (o, splits)):
            pr.compare((float(got[0]), got[1].cpu().numpy(), got[2].cpu().numpy()), ref, sp, what="splits %d" % sp)
        far = pr.excess((float(o[0]), o[1].cpu().numpy(), o[2].cpu().numpy()),
                        dict(ref, loss=float(a[0]), dW=a[1].double().cpu().numpy(), db=a[2].double().cpu().numpy()),
                        max(splits, 7) if splits else 1, scale=2.0)
        assert max(far.values()) <= 1.0, (splits, far)


# ---- 3. the fit equals its composition ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("task", pr.TASKS)
def test_fit_equals_three_rounds_of_pass_and_adam(task, mode):
    gs = pkg()
    gs.ops.set_compute_dtype(mode)
    n, D, C = 257, 264, 65
    c = pr.make_case(n, D, C, task)
    table, ids, y, _, _ = _operands(c, mode)
    emb = table.contiguous()
    probe = gs.linear_probe(emb, y, ids, task, n_classes=C, iters=3, lr=0.1, weight_decay=1e-3)
    W = torch.nn.Parameter(torch.zeros(C, D, device=DEV))
    b = torch.nn.Parameter(torch.zeros(C, device=DEV))
    opt = gs.optim.FlatAdam([W, b], lr=0.1, weight_decay=1e-3)
    losses = []
    for _ in range(3):
        loss, dW, db = gs.ops.probe_pass(emb, ids, y, W.data, b.data, task)
        W.grad.copy_(dW)
        b.grad.copy_(db)
        opt.step()
        losses.append(loss)
    assert torch.equal(probe.W, W.data) and torch.equal(probe.b, b.data)
    assert torch.equal(probe.loss_history, torch.stack(losses))
    assert float(W.data.abs().max()) > 0.0 and float(losses[2]) < float(losses[0])
    again = gs.linear_probe(emb, y, ids, task, n_classes=C, iters=3, lr=0.1, weight_decay=1e-3)
    assert torch.equal(again.W, probe.W) and torch.equal(again.b, probe.b)
    assert torch.equal(again.loss_history, probe.loss_history)


# ---- 4. end to end on data the reference separates ---------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fit_separates_the_toy_classes(seed):
    gs = pkg()
    X, y = pr.toy(seed, 5, False)
    for dev in (DEV, "cpu"):
        Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
        probe = gs.linear_probe(Xd, yd[:400], torch.arange(400), "classification", n_classes=5)
        assert torch.equal(probe.predict(Xd, torch.arange(400, 600)), yd[400:]), dev       # held-out accuracy 1.0
        h = probe.loss_history.cpu()
        assert tuple(h.shape) == (100,) and bool((h[1:] <= h[:-1]).all()), dev


@pytest.mark.parametrize("seed", [0, 1])
def test_fit_gets_every_toy_bit_right(seed):
    gs = pkg()
    X, y = pr.toy(seed, 8, True)
    for dev in (DEV, "cpu"):
        Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
        probe = gs.linear_probe(Xd, yd[:400], torch.arange(400), "multilabel_classification")
        assert torch.equal(probe.predict(Xd, torch.arange(400, 600)), yd[400:] > 0.5), dev


def test_probe_eval_scores_the_folds_on_the_device():
    gs = pkg()
    X, y = pr.toy(0, 5, False)
    folds = np.array(["train"] * 400 + ["val"] * 100 + ["test"] * 100)

    class P(object):
        task, n_classes, targets = "classification", 5, y.reshape(-1, 1)
        nodes = {m: np.where(folds == m)[0] for m in ("train", "val", "test")}
    res = gs.probe_eval(torch.from_numpy(X).to(DEV), P)
    assert res["val"] == {"micro": 1.0, "macro": 1.0} and res["test"] == {"micro": 1.0, "macro": 1.0}
    assert res["loss_last"] < res["loss_first"]


# ---- 5. command line -----------------------------------------------------------------------------------------------
def _cli_problem(task):
    """A 900-node sparse problem (own copy of test_gpu_round4's multilabel builder): features normal, targets one bit
    per class from the features' signs (multilabel, C = 4), their arg-max over five columns (classification), or a
    column (regression)."""
    gs = pkg()
    rng = np.random.RandomState(0)
    n, D = 900, 12
    degs = rng.randint(1, 12, size=n + 1)
    degs[0] = 0
    rows = np.repeat(np.arange(n + 1), degs)
    cols = np.concatenate([np.arange(d) for d in degs])
    adj = sparse.csr_matrix((rng.randint(1, n + 1, size=rows.shape[0]), (rows, cols)))
    feats = rng.normal(size=(n + 1, D)).astype(np.float32)
    feats[0] = 0
    folds = np.array(["train"] * 601 + ["val"] * 150 + ["test"] * 150)
    folds[0] = "dummy"
    if task == "multilabel_classification":
        C, targets = 4, (feats[:, :4] > 0).astype(np.float32)
    elif task == "classification":
        C, targets = 5, np.argmax(feats[:, :5], axis=1).astype(np.int64).reshape(-1, 1)
    else:
        C, targets = 1, feats[:, :1].copy()
    return gs.NodeProblem.from_arrays(task, C, adj, adj, feats, folds, targets, cuda=True)


ARGV = ["--problem-path", "<memory>", "--sampler-class", "sparse_uniform_neighbor_sampler", "--aggregator-class", "mean",
        "--epochs", "1", "--batch-size", "128", "--n-train-samples", "5,3", "--n-val-samples", "5,3", "--output-dims",
        "16,16", "--probe", "--show-test"]
PROBE_KEYS = {"fold", "task", "micro", "macro", "loss_first", "loss_last"}


def _probe_lines(out):
    return [json.loads(l)["probe"] for l in out.splitlines() if l.startswith('{"probe"')]


@pytest.mark.parametrize("unsupervised", [True, False])
@pytest.mark.parametrize("task", pr.TASKS)
def test_cli_probe_prints_its_lines(task, unsupervised, capsys):
    import importlib
    train = importlib.import_module("pytorch-graphsage_amd.train")
    train.main(ARGV + (["--unsupervised"] if unsupervised else []), problem=_cli_problem(task))
    lines = _probe_lines(capsys.readouterr().out)
    assert [l["fold"] for l in lines] == ["val", "test"]
    for l in lines:
        assert set(l) == PROBE_KEYS and l["task"] == task
        assert all(np.isfinite(l[k]) for k in ("micro", "macro", "loss_first", "loss_last"))
        assert 0.0 <= l["micro"] <= 1.0 and 0.0 <= l["macro"] <= 1.0 and l["loss_last"] < l["loss_first"]


def test_cli_probe_refuses_a_regression_problem(capsys):
    import importlib
    train = importlib.import_module("pytorch-graphsage_amd.train")
    with pytest.raises(SystemExit, match="--probe: a linear probe is a classifier"):
        train.main(ARGV, problem=_cli_problem("regression_mae"))
    capsys.readouterr()
