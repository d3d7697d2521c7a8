#!/usr/bin/env python
"""
gen_golden_wide_head.py -- golden vectors for the fused engines with the WIDE head (TEST INFRASTRUCTURE, runs
ONLY in the build container; same harness and shims as gen_golden.py, layout of gen_golden_engine.py).

engine_kat.npz pins the engines on cross-entropy with at most 7 classes.  This script drives the REFERENCE's
GSSupervised.train_step (models.py:97-104) for two steps on the problems gsage_head_wide is for:

  w0  mean      2 layers  fan-out 5/3    output_dim 128/128  multilabel, 121 labels (PPI's count), L2 decay, weights
                                                             scaled by 0.02 so that clip_grad_norm acts
  w1  max_pool  2 layers  fan-out 5/3    output_dim 64/64    cross-entropy over 100 classes, L2 decay
  w2  mean      3 layers  fan-out 4/3/2  output_dim 16/16/8  multilabel, 70 labels; fc input 16 (narrower than a k-slab)

and records inputs (graph, features, initial weights, seed ids, targets -- multilabel targets are random bits as fp32
[B, C] --, the `sel` of every hop of both steps) and outputs (predictions, loss and pre-clip gradient norm of both
steps, clipped gradients of step 0, weights after the two Adam updates).

    python -B tests/golden/gen_golden_wide_head.py      # writes tests/golden/wide_head_kat.npz and its volumes
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch
from torch.nn import functional as F

import gen_golden as gg          # imports the reference with the harness shims

models, nn_modules, problem = gg.models, gg.nn_modules, gg.problem
_np = gg._to_numpy

BIG_BYTES = 100 << 10          # arrays at least this large go to a volume
VOLUME_BYTES = 900 << 10       # raw bytes per volume (fp32 noise does not compress)

CASES = [
    # (aggregator, fanouts, out_dims, D, n_nodes, B, task, n_classes, lr_schedule, weight_decay, weight scale)
    ("mean", (5, 3), (128, 128), 24, 200, 13, "multilabel_classification", 121, "constant", 5e-4, 0.02),
    ("max_pool", (5, 3), (64, 64), 16, 160, 10, "classification", 100, "constant", 5e-4, 1.0),
    ("mean", (4, 3, 2), (16, 16, 8), 12, 150, 9, "multilabel_classification", 70, "linear", 0.0, 1.0),
]


def main():
    out = {}
    for case, (aggn, fan, odims, D, n, B, task, C, sched, wd, fscale) in enumerate(CASES):
        grng = np.random.RandomState(900 + case)
        degs = grng.randint(0, 14, size=n + 1)
        degs[0], degs[2], degs[n] = 0, 0, 3
        adj = gg.make_ref_csr(n, degs, grng)
        tdegs = np.minimum(degs, grng.randint(0, 11, size=n + 1))
        tdegs[n] = 2
        tdegs[5] = max(tdegs[5], 1)
        train_adj = gg.make_ref_csr(n, tdegs, grng)
        n_rows = adj.shape[0]
        feats_np = grng.normal(size=(n_rows, D)).astype(np.float32)
        feats_np[0] = 0
        feats = torch.FloatTensor(feats_np)

        torch.manual_seed(60 + case)
        np.random.seed(60 + case)
        L = len(fan)
        specs = [{"n_train_samples": fan[l], "n_val_samples": fan[l], "output_dim": odims[l],
                  "activation": F.relu if l < L - 1 else (lambda x: x)} for l in range(L)]
        model = models.GSSupervised(**{
            "sampler_class": nn_modules.sampler_lookup["sparse_uniform_neighbor_sampler"],
            "adj": adj, "train_adj": train_adj,
            "prep_class": nn_modules.prep_lookup["identity"],
            "aggregator_class": nn_modules.aggregator_lookup[aggn],
            "input_dim": D, "n_nodes": n_rows, "n_classes": C, "layer_specs": specs,
            "lr_init": 0.01, "lr_schedule": sched, "weight_decay": wd,
        })
        with torch.no_grad():
            for prm in model.agg_layers.parameters():
                prm.mul_(fscale)
        p = "w%d_" % case
        out[p + "cfg"] = np.array([aggn, "identity", task, sched])
        out[p + "fanouts"] = np.array(fan)
        out[p + "out_dims"] = np.array(odims)
        out[p + "weight_decay"] = np.array(wd)
        out[p + "n_classes"] = np.array(C)
        out[p + "feats"] = feats_np
        out.update(gg.csr_arrays(adj, p + "adj_"))
        out.update(gg.csr_arrays(train_adj, p + "tadj_"))
        out.update(gg.sd_arrays(model, p + "w0_"))

        ids = torch.LongTensor(grng.randint(1, n_rows, size=B))
        ids[0] = 2                                   # a seed without neighbours: samples the dummy node
        if task == "classification":
            targets = torch.LongTensor(grng.randint(0, C, size=(B, 1)))
        else:
            targets = torch.FloatTensor(grng.randint(0, 2, size=(B, C)).astype(np.float32))
        loss_fn = getattr(problem.ProblemLosses, task)
        out[p + "ids"] = _np(ids)
        out[p + "targets"] = _np(targets)

        np.random.seed(8765 + case)
        for step in range(2):
            model.set_progress(0.25 * step)
            out[p + "lr%d" % step] = np.array(model.lr)
            w_before = {k: v.clone() for k, v in model.state_dict().items()}
            with gg.ChoiceRecorder() as rec:
                preds = model.train_step(ids=ids, feats=feats, targets=targets, loss_fn=loss_fn)
            sels = [c[1] for c in rec.calls]
            assert len(sels) == L
            for h, sv in enumerate(sels):
                out[p + "s%d_sel%d" % (step, h)] = sv.astype(np.int32)
            out[p + "s%d_preds" % step] = _np(preds).copy()
            if step == 0:
                for k, v in model.named_parameters():
                    out[p + "s0_cg_%s" % k] = _np(v.grad).copy()                 # clipped grads
            w_after = {k: v.clone() for k, v in model.state_dict().items()}
            # loss and pre-clip gradient norm: replay the same draws on the pre-step weights
            model.load_state_dict(w_before)
            model.optimizer.zero_grad()
            with gg.ChoiceReplayer(sels):
                pr2 = model(ids, feats, train=True)
            loss = loss_fn(pr2, targets.squeeze())
            loss.backward()
            tn = torch.sqrt(sum((q.grad.detach() ** 2).sum() for q in model.parameters() if q.grad is not None))
            assert np.allclose(_np(pr2), _np(preds), atol=1e-6)
            out[p + "s%d_loss" % step] = np.array(float(loss))
            out[p + "s%d_gradnorm" % step] = np.array(float(tn))
            model.load_state_dict(w_after)
        out.update(gg.sd_arrays(model, p + "w2_"))
        print("w%d %s %s C %d fan %s dims %s: loss %.4f -> %.4f, |g| %.3f" % (
            case, aggn, task, C, fan, odims, float(out[p + "s0_loss"]), float(out[p + "s1_loss"]),
            float(out[p + "s0_gradnorm"])))
    out["n_cases"] = np.array(len(CASES))
    # No committed file may exceed 1 MiB, and three fp32 copies of the weights (initial, clipped gradient, after two
    # steps) of w0 and w1 alone are 3 MB of incompressible floats: wide_head_kat.npz holds every small array, the large
    # ones are dealt in recording order to the volumes wide_head_kat.<k>.npz, each under VOLUME_BYTES.  A reader merges
    # whatever volumes it finds next to the main file.
    for old in os.listdir(HERE):
        if old.startswith("wide_head_kat.") and old.endswith(".npz"):
            os.remove(os.path.join(HERE, old))
    small = {k: v for k, v in out.items() if np.asarray(v).nbytes < BIG_BYTES}
    volumes, room = [], 0
    for k, v in out.items():
        if k in small:
            continue
        if not volumes or room < v.nbytes:
            volumes.append({})
            room = VOLUME_BYTES
        volumes[-1][k] = v
        room -= v.nbytes
    small["n_volumes"] = np.array(len(volumes))
    paths = [os.path.join(HERE, "wide_head_kat.npz")] + [os.path.join(HERE, "wide_head_kat.%d.npz" % (i + 1))
                                                         for i in range(len(volumes))]
    for path, arrays in zip(paths, [small] + volumes):
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < (1 << 20), path
    print("wide_head_kat: %d cases, %s MB" % (len(CASES), " + ".join("%.2f" % (os.path.getsize(q) / 1e6) for q in paths)))


if __name__ == "__main__":
    main()
