"""The wide head without a GPU: tests/wide_head_ref.py is the reference's head (float64 autograd of F.normalize -> fc ->
F.cross_entropy / F.multilabel_soft_margin_loss on the live rows), the host path of ops.wide_head meets it, head_why_not
answers as before without `wide` and covers the two new cases with it, and gsage_head_wide refuses bad arguments before
any launch."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wide_head_ref as wr
from conftest import pkg
from util import close

gs = pkg()
nat = gs._native
EINVAL = -1          # GSAGE_EINVAL (include/gsage.h)


# ---- 1. the definition is the reference's head ---------------------------------------------------------------------------
@pytest.mark.parametrize("task", wr.TASKS)
@pytest.mark.parametrize("case", [(33, 121, 256, None), (16, 65, 32, 1), (33, 7, 40, 20), (2, 2, 8, None)])
def test_reference_equals_float64_autograd_on_the_live_rows(case, task):
    B, C, D, nv = case
    c = wr.make_case(B, C, D, task)
    ref = wr.reference(c["E"], c["W"], c["b"], c["y"], task, nv)
    bv = B if nv is None else nv
    E, W, b = (torch.from_numpy(c[k].astype(np.float64)).requires_grad_(True) for k in ("E", "W", "b"))
    preds = F.normalize(E, dim=1) @ W.t() + b
    if task == "classification":
        loss = F.cross_entropy(preds[:bv], torch.from_numpy(c["y"][:bv]))
    else:
        loss = F.multilabel_soft_margin_loss(preds[:bv], torch.from_numpy(c["y"][:bv].astype(np.float64)))
    loss.backward()
    rel = lambda a, want: float(np.abs(a - want).max() / np.abs(want).max())
    assert abs(ref["loss"] - float(loss.detach())) <= 1e-10 * abs(float(loss.detach()))
    assert rel(ref["preds"], preds.detach().numpy()) <= 1e-10
    assert rel(ref["dE"], E.grad.numpy()) <= 1e-10
    assert rel(ref["dW"], W.grad.numpy()) <= 1e-10
    assert rel(ref["db"], b.grad.numpy()) <= 1e-10
    if bv < B:
        assert not ref["dE"][bv:].any()


# ---- 2. ops.wide_head in host mode ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task", wr.TASKS)
@pytest.mark.parametrize("case", [(33, 121, 256, None), (16, 65, 32, 1), (33, 121, 256, 20)])
def test_ops_wide_head_on_cpu_tensors(case, task):
    B, C, D, nv = case
    c, ref = wr.case_reference(B, C, D, task, nv)
    t = lambda k: torch.from_numpy(c[k])
    preds, loss, dE, dW, db = gs.ops.wide_head(t("E"), t("W"), t("b"), t("y"), task, n_valid=nv)
    close(preds.numpy(), ref["preds"], "preds", 1e-5, 1e-6)
    assert abs(float(loss) - ref["loss"]) < 1e-5 * max(1.0, abs(ref["loss"]))
    close(dE.numpy(), ref["dE"], "dE", 1e-5, 1e-7)
    close(dW.numpy(), ref["dW"], "dW", 1e-5, 1e-7)
    close(db.numpy(), ref["db"], "db", 1e-5, 1e-7)
    fwd = gs.ops.wide_head(t("E"), t("W"), t("b"), None, task)
    assert torch.equal(fwd[0], preds) and fwd[1:] == (None, None, None, None)
    assert gs.ops.wide_head(t("E"), t("W"), t("b"), t("y"), task, dE_dtype=torch.bfloat16)[2].dtype == torch.bfloat16


def test_ops_wide_head_names_the_argument_it_refuses():
    c = wr.make_case(4, 3, 8, "classification")
    E, W, b, y = (torch.from_numpy(c[k]) for k in ("E", "W", "b", "y"))
    bad = [
        ("E must", dict(E=E.double())), ("W must", dict(W=W.double())), ("b must", dict(b=b[:2])),
        ("E has", dict(E=E[:, :7])), ("rows \\(classes\\)", dict(W=torch.zeros(129, 8), b=torch.zeros(129))),
        ("columns", dict(E=torch.zeros(4, 1025), W=torch.zeros(3, 1025))), ("targets must be int64", dict(targets=y.float())),
        ("n_valid", dict(n_valid=5)), ("n_valid", dict(n_valid=0)), ("dE_dtype", dict(dE_dtype=torch.float16)),
        ("task must be", dict(task="regression_mae")),
    ]
    for pattern, change in bad:
        kw = dict(E=E, W=W, b=b, targets=y, task="classification")
        kw.update(change)
        with pytest.raises(ValueError, match=pattern):
            gs.ops.wide_head(**kw)
    with pytest.raises(ValueError, match="multilabel targets must be fp32"):
        gs.ops.wide_head(E, W, b, torch.zeros(4, 2), "multilabel_classification")


# ---- 3. head_why_not -----------------------------------------------------------------------------------------------------------
def _model(n_classes, fc_in=None):
    from scipy import sparse
    adj = sparse.csr_matrix((np.array([1, 2, 1]), np.array([0, 1, 0]), np.array([0, 0, 2, 3])), shape=(3, 2))
    specs = [{"n_train_samples": 2, "n_val_samples": 2, "output_dim": 8, "activation": F.relu},
             {"n_train_samples": 2, "n_val_samples": 2, "output_dim": 8, "activation": lambda x: x}]
    m = gs.GSSupervised(sampler_class=gs.sampler_lookup["sparse_uniform_neighbor_sampler"], adj=adj, train_adj=adj,
                        prep_class=gs.prep_lookup["identity"], aggregator_class=gs.aggregator_lookup["mean"],
                        input_dim=4, n_nodes=3, n_classes=n_classes, layer_specs=specs)
    if fc_in is not None:
        m.fc = torch.nn.Linear(fc_in, n_classes)
    return m


def test_head_why_not_without_wide_answers_as_before():
    """the six calls of test_host_mode.py, with and without an explicit wide=False; no draw from torch's generator"""
    E, L = gs.engine.FusedMeanTrainStep, gs.ProblemLosses
    i64, f32 = torch.zeros(1, dtype=torch.int64), torch.zeros(1)
    state = torch.get_rng_state()
    for kw in ({}, {"wide": False}):
        assert E.head_why_not(_model(5), L.classification, i64, 512, True, **kw) is None
        assert E.head_why_not(_model(1), L.regression_mae, f32, 512, True, **kw) is None
        assert E.head_why_not(_model(4), L.multilabel_classification, f32, 512, False, **kw) is None
        for why in (E.head_why_not(_model(4), L.multilabel_classification, f32, 512, True, **kw),
                    E.head_why_not(_model(100), L.classification, i64, 512, True, **kw),
                    E.head_why_not(_model(1), L.regression_mae, f32, 4096, True, **kw)):
            assert "no fused kernel" in why and "only a fused head can ignore the padding" in why
    m = _model(121)
    state2 = torch.get_rng_state()
    E.head_why_not(m, L.multilabel_classification, f32, 512, True, wide=True)
    E.head_why_not(m, L.multilabel_classification, f32, 512, True)
    assert torch.equal(torch.get_rng_state(), state2), "head_why_not consumed torch's generator (the run's own)"
    torch.set_rng_state(state)


@pytest.mark.parametrize("engine", ["FusedMeanTrainStep", "FusedPoolTrainStep", "FusedAttnTrainStep"])
def test_head_why_not_with_wide_covers_padded_multilabel_and_wide_classification(engine):
    E, L = getattr(gs.engine, engine), gs.ProblemLosses
    i64, f32 = torch.zeros(1, dtype=torch.int64), torch.zeros(1)
    assert E.head_why_not(_model(4), L.multilabel_classification, f32, 512, True, wide=True) is None
    assert E.head_why_not(_model(121), L.multilabel_classification, f32, 512, True, wide=True) is None
    assert E.head_why_not(_model(100), L.classification, i64, 512, True, wide=True) is None
    # classification with <= 64 classes and the L1 head are what they were
    assert E.head_why_not(_model(5), L.classification, i64, 512, True, wide=True) is None
    assert E.head_why_not(_model(1), L.regression_mae, f32, 512, True, wide=True) is None
    assert "no fused kernel" in E.head_why_not(_model(1), L.regression_mae, f32, 4096, True, wide=True)
    # beyond the limits: a sentence that names the limit
    why = E.head_why_not(_model(129), L.multilabel_classification, f32, 512, True, wide=True)
    assert "128" in why and "129" in why
    why = E.head_why_not(_model(129), L.classification, i64, 512, True, wide=True)
    assert "128" in why and "129" in why
    why = E.head_why_not(_model(121, fc_in=1025), L.multilabel_classification, f32, 512, True, wide=True)
    assert "1024" in why and "1025" in why
    why = E.head_why_not(_model(121), L.multilabel_classification, f32, 512, False, world=2, wide=True)
    assert "data-parallel" in why


# ---- 4. gsage_head_wide refuses bad arguments before any launch (no GPU needed) -----------------------------------------------
def _call(C=121, D=256, B=16, task=1, ldy=None, scratch=True, targets=True, dE=True, lde=None, ldd=None):
    """gsage_head_wide on host buffers that are never dereferenced: every refusal precedes the launch"""
    L = nat.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    ldy = max(C, 1) if ldy is None else ldy
    return L.gsage_head_wide(p, D if lde is None else lde, p, p, p if targets else None, task, ldy, B, C, D, p,
                             p if dE else None, nat.F32, D if ldd is None else ldd, None, None, None,
                             p if scratch else None, None, 0, None)


@pytest.mark.parametrize("kw,word", [
    (dict(C=0), "n_classes"), (dict(C=129), "n_classes"), (dict(D=1025), "width"), (dict(D=0), "width"),
    (dict(ldy=120), "ldy"), (dict(task=2), "task"), (dict(task=-1), "task"), (dict(scratch=False), "scratch"),
    (dict(lde=255), "lde"), (dict(ldd=255), "ldd"), (dict(dE=False), "go together"), (dict(B=0), "B must"),
])
def test_kernel_entry_returns_einval_with_a_sentence(kw, word):
    assert _call(**kw) == EINVAL
    assert word in nat.lib().gsage_last_error().decode()


def test_scratch_size_is_one_partial_row_per_sixteen_rows():
    L = nat.lib()
    assert L.gsage_head_wide_scratch(512, 121, 256) == 32 * (121 * 256 + 121 + 1)
    assert L.gsage_head_wide_scratch(33, 3, 8) == 3 * (3 * 8 + 3 + 1)
    for bad in ((0, 3, 8), (4, 0, 8), (4, 129, 8), (4, 3, 1025), (4, 3, 0)):
        assert L.gsage_head_wide_scratch(*bad) == -1


def test_a_refused_call_consumes_the_pending_live_row_count():
    """gsage_head_n_valid_next is taken before any return path: after a refused gsage_head_wide the thread's slot is
    empty (gsage_head_n_valid_pending peeks at it without taking), so no later head launch inherits the count."""
    L = nat.lib()
    word = (ctypes.c_int32 * 1)(7)
    assert L.gsage_head_n_valid_pending() == 0
    for kw in (dict(C=129), dict(task=5), dict(scratch=False)):
        assert L.gsage_head_n_valid_next(ctypes.addressof(word)) == 0
        assert L.gsage_head_n_valid_pending() == 1
        assert L.gsage_head_n_valid_pending() == 1               # (the peek itself does not consume)
        assert _call(**kw) == EINVAL                         # refused: the pending word goes with it
        assert L.gsage_head_n_valid_pending() == 0
