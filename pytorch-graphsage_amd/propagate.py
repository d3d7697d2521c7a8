"""
propagate.py -- propagation over the graph AFTER the encoder has run: label propagation and "Correct and Smooth"
(Huang et al., 2020, "Combining Label Propagation and Simple Models Out-performs Graph Neural Networks").

Everything here iterates one step over a sparse adjacency (a store.DeviceCSR):

    x_{t+1} = clamp((1 - alpha) * base + alpha * S x_t),        S = diag(a) A diag(b)

with A the stored rows of the adjacency (an empty row sums to 0 -- it is NOT sent to the dummy -- and duplicates
count) and a, b the scales of `norm`: "sym" a = b = deg^-1/2 (D^-1/2 A D^-1/2 on an adjacency that stores both
directions of every edge; on any other adjacency the same formula over the stored rows, nothing is symmetrised here:
store.DeviceCSR.symmetrized() builds the adjacency that stores both directions), "row"
a = 1 / deg, b = 1 (D^-1 A), "col" a = 1, b = 1 / deg (A D^-1); 0 where deg == 0.

On the GPU one step is ops.propagate_step (csrc/gsage_propagate.hip): the kernel walks the plan infer.plan builds for
the full-neighbourhood segment reduce, sums the rows of the PRE-SCALED iterate y = b (.) x, applies a, the residual
and the clamp in its epilogue and writes the next step's y itself.  The loop issues the library's two launches per
step and nothing else: no host synchronisation, no torch op.  CPU tensors take the same definition in torch (host mode).

Refused with one sentence each: regression problems, a dense adjacency, a weighted adjacency (edge weights are out of
scope here; importance neighbourhoods included), a Block of a closure, more than 1024 columns, and -- in
correct_smooth_eval -- a model infer.check_supported refuses.
"""
import numpy as np
import torch

from . import _native as nat
from . import infer, ops
from .store import DenseAdj, DeviceCSR, WeightedAdj, _round_up

TASKS = ("classification", "multilabel_classification")
AUTOSCALE_MAX = 1000.0


# --------------------------------------------------------------------------------------------
# checks
# --------------------------------------------------------------------------------------------
def check_adj(adj, who="propagate"):
    """Raise ValueError naming why `adj` cannot be propagated over; else return None."""
    if isinstance(adj, infer.Block):
        raise ValueError("%s: a Block of a closure holds the rows of a query set, not the graph to propagate over" % who)
    if isinstance(adj, DenseAdj) or (torch.is_tensor(adj) and adj.dim() == 2):
        raise ValueError("%s: a dense adjacency holds neighbour samples, not the edges to propagate over" % who)
    if isinstance(adj, WeightedAdj) or getattr(adj, "edge_cdf", None) is not None:
        raise ValueError("%s: a weighted adjacency is not supported (edge weights are out of scope; propagation is "
                         "over the unweighted stored edges)" % who)
    if not isinstance(adj, DeviceCSR):
        raise ValueError("%s: adj must be a store.DeviceCSR, not %s" % (who, type(adj).__name__))


def check_task(task, who="propagate"):
    if task not in TASKS:
        raise ValueError("%s: labels are propagated as class scores -- the task must be classification or "
                         "multilabel_classification, not %r" % (who, task))


def _check_width(C, who):
    if not 1 <= C <= ops.PROP_C_MAX:
        raise ValueError("%s: the number of columns must lie in [1, %d], not %d" % (who, ops.PROP_C_MAX, C))


def _ids(nodes, dev, n, who):
    ids = torch.as_tensor(nodes)
    if ids.is_floating_point() or ids.dtype == torch.bool:
        raise ValueError("%s: node ids must be integers, not %s" % (who, ids.dtype))
    ids = ids.to(dev).long().contiguous().view(-1)
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= n):
        raise IndexError("%s: node id out of range of the %d rows" % (who, n))
    return ids


def _scales(adj, norm):
    """(a, b) of `norm` for `adj`, cached on the adjacency object the way the plan is."""
    cache = getattr(adj, "_propagate_scales", None)
    if cache is None:
        cache = adj._propagate_scales = {}
    if norm not in cache:
        cache[norm] = ops.propagate_scales(adj.rowptr, adj.n_rows, norm)
    return cache[norm]


def _padded(x, n, C, dev):
    """x's first n rows as a fresh fp32 [n, round_up(C, 4)] buffer, zero in the padding columns."""
    out = torch.zeros(n, _round_up(C, 4), dtype=torch.float32, device=dev)
    out[:, :C] = x[:n]
    return out


# --------------------------------------------------------------------------------------------
# the iteration
# --------------------------------------------------------------------------------------------
class Workspace(object):
    """Every buffer the launches of one propagate() call read or write -- x_0's pre-scaled copy, base, the ping-pong
    pair, the result, the long rows' partial sums --, the scales, the plan and the adjacency.  A command list stores raw
    device pointers and keeps nothing alive, so a caller that RECORDS the call passes a Workspace and holds it for as long
    as the list is replayed; `result` is the view propagate() returned, which every replay fills again."""

    def __init__(self):
        self.held, self.result = [], None

    def hold(self, *things):
        self.held.extend(t for t in things if t is not None)


def propagate(adj, x, iters, alpha, base=None, norm="sym", clamp=None, fixed=None, slice_len=infer.SLICE_LEN,
              workspace=None):
    """x_iters of  x_{t+1} = clamp((1 - alpha) * base + alpha * S x_t),  x_0 = x  -> fp32 [n_rows, C].

    adj: a store.DeviceCSR on x's device; x: a float [n_rows, C] tensor, C <= 1024; base: like x (default: x itself);
    norm: "sym", "row" or "col" (the module's docstring); clamp: None or (lo, hi); fixed = (ids, values): those rows
    of `base` AND of x_0 are overwritten with `values` [len(ids), C] before iterating -- how labelled rows are held.
    iters = 0 returns x_0.  slice_len: the plan's (infer.plan).

    CUDA: per step the two launches of ops.propagate_step on two ping-pong buffers; set-up -- the scales (cached on the
    adjacency), the pre-scaled y_0, padding to a 4-float row -- and the final slice are torch ops.  Deterministic: no
    atomics.  A stored id outside the graph is an IndexError after the loop (adj.check()).

    The work buffers are locals: once the call returns only the result's buffer is alive.  To RECORD the launches in a
    command list (_native.CommandList) pass workspace=Workspace() and keep it as long as the list -- it then owns every
    buffer the launches touch, and since x_0's pre-scaled copy is kept apart from the ping-pong pair, every replay
    refills the returned view with the same bits.  Without a workspace a recorded call must not be replayed.

    With base = x this is also the feature smoother of SGC / APPNP-style models (alpha * S x + (1 - alpha) * x_0
    iterated over up to 1024 feature columns); nothing more is built for that here."""
    check_adj(adj)
    ops.propagate_norm(norm)
    if not torch.is_tensor(x) or x.dim() != 2 or not x.is_floating_point():
        raise ValueError("propagate: x must be a [n_rows, C] float tensor")
    iters = int(iters)
    if iters < 0:
        raise ValueError("propagate: iters must be >= 0, not %d" % iters)
    dev, n, C = x.device, int(adj.n_rows), int(x.shape[1])
    _check_width(C, "propagate")
    if adj.device != dev:
        raise ValueError("propagate: the adjacency is on %s, x on %s" % (adj.device, dev))
    if int(x.shape[0]) < n:
        raise ValueError("propagate: %d rows of x for an adjacency of %d rows" % (int(x.shape[0]), n))
    if base is not None and (not torch.is_tensor(base) or base.dim() != 2 or int(base.shape[1]) != C
                             or int(base.shape[0]) < n):
        raise ValueError("propagate: base must have x's shape")
    lo, hi = (-float("inf"), float("inf")) if clamp is None else (float(clamp[0]), float(clamp[1]))
    if not lo <= hi:
        raise ValueError("propagate: clamp needs lo <= hi")
    alpha = float(alpha)
    with torch.no_grad():
        X0 = _padded(x, n, C, dev)
        B0 = X0 if base is None and fixed is None else _padded(x if base is None else base, n, C, dev)
        if fixed is not None:
            ids = _ids(fixed[0], dev, n, "propagate")
            vals = torch.as_tensor(fixed[1]).to(dev).float()
            if vals.dim() != 2 or tuple(vals.shape) != (int(ids.shape[0]), C):
                raise ValueError("propagate: fixed values must have shape [%d, %d]" % (int(ids.shape[0]), C))
            X0[ids] = B0[ids] = torch.nn.functional.pad(vals, (0, X0.shape[1] - C))
        if iters == 0:
            return X0[:, :C]
        a, b = _scales(adj, norm)
        plan = infer.plan(adj, slice_len)
        y = y0 = b.view(-1, 1) * X0
        ping = [torch.zeros_like(X0) for _ in range(min(2, iters - 1))]
        res = torch.zeros_like(X0)
        partials = None
        if plan["n_slices"] and dev.type == "cuda":
            ldp = int(nat.lib().gsage_segment_reduce_ldp(C))
            partials = torch.empty(plan["n_slices"], ldp, dtype=torch.float32, device=dev)
        for t in range(iters):                    # the library's two launches per step, nothing else
            last = t == iters - 1
            nxt = None if last else ping[t & 1]
            ops.propagate_step(adj, plan, y, B0, a, b, alpha, 1.0 - alpha, lo, hi, C, out=res if last else None,
                               yout=nxt, partials=partials)
            y = nxt
        adj.check()
        if workspace is not None:
            workspace.hold(adj, plan, a, b, X0, B0, y0, res, partials, *ping)
            workspace.result = res[:, :C]
        return res[:, :C]                         # (a view of the last step's output buffer)


# --------------------------------------------------------------------------------------------
# label propagation, Correct and Smooth
# --------------------------------------------------------------------------------------------
def _label_rows(targets, ids, n_classes, task, dev, who):
    """Y fp32 [len(ids), C]: one-hot rows of class ids, or the 0/1 rows themselves -> (Y, C)."""
    check_task(task, who)
    t = torch.as_tensor(targets).to(dev)
    m = int(ids.shape[0])
    if task == "classification":
        if t.is_floating_point() or t.dtype == torch.bool or t.numel() != m:
            raise ValueError("%s: classification targets must be %d integer class ids, not %s %s"
                             % (who, m, t.dtype, tuple(t.shape)))
        t = t.long().view(-1)
        C = int(n_classes) if n_classes is not None else (int(t.max()) + 1 if m else 1)
        _check_width(C, who)
        if m and (int(t.min()) < 0 or int(t.max()) >= C):
            raise ValueError("%s: class id out of range [0, %d)" % (who, C))
        Y = torch.zeros(m, C, dtype=torch.float32, device=dev)
        Y[torch.arange(m, device=dev), t] = 1.0
        return Y, C
    if t.dim() != 2 or int(t.shape[0]) != m:
        raise ValueError("%s: multilabel targets must have shape [%d, C], not %s" % (who, m, tuple(t.shape)))
    C = int(n_classes) if n_classes is not None else int(t.shape[1])
    _check_width(C, who)
    if int(t.shape[1]) < C:
        raise ValueError("%s: multilabel targets have %d columns, n_classes = %d" % (who, int(t.shape[1]), C))
    return t[:, :C].float().contiguous(), C


def label_propagation(adj, targets, nodes, n_classes=None, task="classification", iters=50, alpha=0.8, norm="sym"):
    """Scores fp32 [n_rows, C] of plain label propagation: base = the one-hot rows of `targets` (classification) or
    the 0/1 rows themselves (multilabel_classification) on `nodes`, 0 elsewhere; x_0 = base;
    propagate(..., clamp=(0, 1)).  targets: one per node of `nodes`, in its order.  iters = 50 and alpha = 0.8 are the
    common published defaults; nobody has tuned them on a graph of this project."""
    check_adj(adj, "label_propagation")
    check_task(task, "label_propagation")
    dev, n = adj.device, int(adj.n_rows)
    ids = _ids(nodes, dev, n, "label_propagation")
    Y, C = _label_rows(targets, ids, n_classes, task, dev, "label_propagation")
    base = torch.zeros(n, C, dtype=torch.float32, device=dev)
    base[ids] = Y
    return propagate(adj, base, iters, alpha, norm=norm, clamp=(0.0, 1.0))


def _correct_and_smooth(adj, logits, targets, nodes, task, iters, alpha, norm, autoscale, scale):
    who = "correct_and_smooth"
    check_adj(adj, who)
    check_task(task, who)
    if not torch.is_tensor(logits) or logits.dim() != 2 or not logits.is_floating_point():
        raise ValueError("%s: logits must be a [n_rows, C] float tensor" % who)
    dev, n, C = logits.device, int(adj.n_rows), int(logits.shape[1])
    _check_width(C, who)
    if int(logits.shape[0]) < n:
        raise ValueError("%s: %d rows of logits for an adjacency of %d rows" % (who, int(logits.shape[0]), n))
    try:
        (it_c, it_s), (al_c, al_s) = (int(v) for v in iters), (float(v) for v in alpha)
    except (TypeError, ValueError):
        raise ValueError("%s: iters and alpha are pairs (correct, smooth)" % who)
    ids = _ids(nodes, dev, n, who)
    Y, _ = _label_rows(targets, ids, C, task, dev, who)
    with torch.no_grad():
        z = logits[:n].float()
        Z = torch.softmax(z, dim=1) if task == "classification" else torch.sigmoid(z)
        E0 = torch.zeros_like(Z)
        E0[ids] = Y - Z[ids]
        if autoscale:
            E = propagate(adj, E0, it_c, al_c, norm=norm, clamp=(-1.0, 1.0))
            sigma = E0[ids].abs().sum(dim=1).mean() if ids.numel() else torch.zeros((), device=dev)
            s = sigma / E.abs().sum(dim=1)
            s = torch.where(torch.isfinite(s) & (s <= AUTOSCALE_MAX), s, torch.ones_like(s))
            Zr = Z + s.view(-1, 1) * E
        else:
            E = propagate(adj, E0, it_c, al_c, norm=norm, clamp=(-1.0, 1.0), fixed=(ids, E0[ids]))
            Zr = Z + float(scale) * E
        G0 = Zr.clone()
        G0[ids] = Y
        G = propagate(adj, G0, it_s, al_s, norm=norm, clamp=(0.0, 1.0))
    return Z, E, Zr, G


def correct_and_smooth(adj, logits, targets, nodes, task, iters=(50, 50), alpha=(0.8, 0.8), norm="sym", autoscale=True,
                       scale=1.0):
    """Correct and Smooth over `adj` -> smoothed scores G fp32 [n_rows, C].

    logits: [n_rows, C] for EVERY row of the adjacency (what infer.full_neighbour returns without `nodes`); targets:
    the labels of `nodes` (class ids, or 0/1 rows for multilabel_classification), in its order.  Z = softmax(logits)
    (classification) or sigmoid(logits) (multilabel); Y = the one-hot or 0/1 targets.
      correct:  E0 = Y - Z on `nodes`, 0 elsewhere;  E = propagate(E0, iters[0], alpha[0], clamp=(-1, 1))
        autoscale=True:   sigma = mean over nodes of ||E0[v]||_1,  s_v = sigma / ||E[v]||_1 (1 where that is not finite
                          or exceeds 1000),  Zr = Z + s (.) E
        autoscale=False:  the labelled rows of E are held at E0 (propagate's fixed=),  Zr = Z + scale * E
      smooth:   G0 = Zr with the rows of `nodes` replaced by Y;  G = propagate(G0, iters[1], alpha[1], clamp=(0, 1))
    The defaults (50 + 50 iterations, alpha 0.8, autoscale) are the common published ones; nobody has tuned them on a
    graph of this project."""
    return _correct_and_smooth(adj, logits, targets, nodes, task, iters, alpha, norm, autoscale, scale)[3]


def correct_smooth_eval(model, problem, iters=(50, 50), alpha=(0.8, 0.8), norm="sym", autoscale=True, scale=1.0,
                        label_prop=False, folds=("val", "test")):
    """Correct and Smooth on a trained GSSupervised: logits of every row by infer.full_neighbour over the evaluation
    adjacency, labels from problem.nodes['train'], the folds scored with the problem's F1 metric (on the device for
    CUDA tensors) before and after ->
    {"task", fold: {"base", "corrected", "smoothed"[, "label_prop"]} each {"micro", "macro"} (None for an empty fold)}.
    "base" scores the logits themselves: what train.py --full-neighbour-eval prints for the fold.  label_prop=True also
    scores plain label_propagation (iters[1], alpha[1]) from the same labels.  Validation labels are never used."""
    from .problem import batch_metric
    task = problem.task
    check_task(task, "correct_smooth_eval")
    infer.check_supported(model)
    dev = problem.feats.device
    adj = model.val_sampler.csr(dev)
    check_adj(adj, "correct_smooth_eval")

    def fold(name):
        nodes = np.asarray(problem.nodes[name]).reshape(-1)
        y = torch.as_tensor(np.asarray(problem.targets[nodes]))
        y = y.long().view(-1) if task == "classification" else y.float()
        return torch.as_tensor(nodes).long().to(dev), y.to(dev)

    logits, emb = infer.full_neighbour(model, problem.feats, adj=adj, embeddings=True)

    def fold_logits(nodes):
        # "base" must be the score train.py --full-neighbour-eval prints: full_neighbour(nodes=fold) applies `fc` to the
        # fold's SELECTED embedding rows, and a projection of another row count may sum in another order, so the fold is
        # scored from the same call shape -- on the embeddings already computed, not from a second inference pass
        with torch.no_grad():
            if dev.type == "cuda":
                return ops.linear(emb[nodes], model.fc.weight, model.fc.bias, compute_dtype="fp32")
            return model.fc(emb[nodes])

    nodes, y = fold("train")
    C = int(logits.shape[1])
    Z, _, Zr, G = _correct_and_smooth(adj, logits, y, nodes, task, iters, alpha, norm, autoscale, scale)
    lp = label_propagation(adj, y, nodes, n_classes=C, task=task, iters=int(iters[1]), alpha=float(alpha[1]),
                           norm=norm) if label_prop else None
    # the F1 metric reads logits: arg-max for classification, > 0 for multilabel -- a score is positive above 1/2
    shift = 0.5 if task == "multilabel_classification" else 0.0
    out = {"task": task}
    for name in folds:
        nodes, y = fold(name)
        if not nodes.numel():
            out[name] = None
            continue
        res = {"base": batch_metric(task, y, fold_logits(nodes)),
               "corrected": batch_metric(task, y, (Zr[nodes] - shift).contiguous()),
               "smoothed": batch_metric(task, y, (G[nodes] - shift).contiguous())}
        if lp is not None:
            res["label_prop"] = batch_metric(task, y, (lp[nodes] - shift).contiguous())
        out[name] = res
    return out
