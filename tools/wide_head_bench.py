#!/usr/bin/env python
"""wide_head_bench.py -- what the fused wide head (csrc/gsage_head_wide.hip, engine wide_head=True) buys a multilabel
train step, at a PPI-like shape: 56 944 nodes, 50 features, 2-layer mean aggregator 128/128, fan-out 25/10, C = 121
labels (random bits), B = 512 seeds, bf16 storage, a synthetic graph of mean degree ~28, Philox sampler.

One JSON line per measurement, appended to --out (default profiles/wide_head_bench.jsonl), all in one process:
  engine_wide_head    ms / step of FusedMeanTrainStep(wide_head=True): the whole step one native command list
  engine_torch_head   ms / step of the same engine with the stock-torch head (what an unpadded multilabel problem gets
                      today: a hipGraph around autograd over normalize / fc / loss)
  module_path         ms / step of GSSupervised.train_step (what a padded multilabel problem gets today)
  head_wide_launch    us of the gsage_head_wide launch alone, from the recorded step's timing marks
The three paths alternate: every round times `--steps` back-to-back steps of each between two device events; the first
`--warmup` rounds are dropped and the median, minimum and maximum of the other `--reps` rounds are reported, so a drift
of the machine shows in the spread.  Needs a GPU: there is no CPU fallback.

    python tools/wide_head_bench.py [--steps 20] [--reps 7] [--warmup 2] [--out PATH]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gs = importlib.import_module("pytorch-graphsage_amd")


def timed(fn, steps):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=56944)
    ap.add_argument("--feats", type=int, default=50)
    ap.add_argument("--classes", type=int, default=121)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "wide_head_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wide_head_bench: needs the GPU (nothing is measured without one)")
    dev = torch.device("cuda")
    gs.ops.set_compute_dtype("bf16")
    gs.ops.warmup(dev)

    from scipy import sparse
    rng = np.random.RandomState(0)
    n, B, C = args.nodes, args.batch, args.classes
    deg = rng.randint(1, 56, size=n)
    deg[0] = 0
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    data = rng.randint(1, n, size=int(indptr[-1])).astype(np.int32)
    adj = sparse.csr_matrix((data, gs.store.row_positions(indptr), indptr), shape=(n, int(deg.max())))
    store = gs.FeatureStore.from_array(rng.standard_normal((n, args.feats)).astype(np.float32), dev, dtype="bf16")
    specs = [{"n_train_samples": 25, "n_val_samples": 25, "output_dim": 128, "activation": F.relu},
             {"n_train_samples": 10, "n_val_samples": 10, "output_dim": 128, "activation": lambda x: x}]
    common = dict(sampler_class=lambda adj: gs.nn_modules.SparseUniformNeighborSampler(adj, rng="philox"), adj=adj,
                  train_adj=adj, prep_class=gs.prep_lookup["identity"], aggregator_class=gs.aggregator_lookup["mean"],
                  input_dim=args.feats, n_nodes=n, n_classes=C, layer_specs=specs)
    models = []
    for _ in range(3):                                   # three twins: an engine re-points its model's Parameters
        torch.manual_seed(0)
        models.append(gs.GSSupervised(**common).to(dev))
    seeds = torch.from_numpy(rng.randint(1, n, size=B)).to(dev)
    targets = torch.from_numpy(rng.randint(0, 2, size=(B, C)).astype(np.float32)).to(dev)
    loss_fn = gs.ProblemLosses.multilabel_classification
    cls = gs.engine.fused_engine_for(models[0], store)
    assert cls is not None, gs.engine.why_no_fused_engine(models[0], store)
    wide = cls(models[0], store, loss_fn, seeds, targets, wide_head=True)
    stock = cls(models[1], store, loss_fn, seeds, targets)
    assert wide.fused_wide and not stock.fused_wide and not stock.fused_head
    paths = [("engine_wide_head", lambda: wide(seeds, targets)),
             ("engine_torch_head", lambda: stock(seeds, targets)),
             ("module_path", lambda: models[2].train_step(seeds, store, targets, loss_fn))]
    t = {name: [] for name, _ in paths}
    for it in range(args.warmup + args.reps):
        for name, fn in paths:
            ms = timed(fn, args.steps)
            if it >= args.warmup:
                t[name].append(ms)

    info = gs._native.device_info()
    base = {"arch": info["arch"] if info else None, "nodes": n, "feats": args.feats, "fan": [25, 10], "dims": [128, 128],
            "B": B, "C": C, "task": "multilabel_classification", "precision": "bf16", "steps": args.steps,
            "reps": args.reps, "warmup": args.warmup, "stamp": time.strftime("%Y-%m-%d")}
    rows = [dict(base, what="engine_wide_head", capture=wide.capture_mode, ms_per_step=stats(t["engine_wide_head"])),
            dict(base, what="engine_torch_head", capture=stock.capture_mode, ms_per_step=stats(t["engine_torch_head"])),
            dict(base, what="module_path", ms_per_step=stats(t["module_path"]))]
    rows[0]["wide_over_torch_head"] = rows[0]["ms_per_step"]["median"] / rows[1]["ms_per_step"]["median"]
    rows[0]["wide_over_module_path"] = rows[0]["ms_per_step"]["median"] / rows[2]["ms_per_step"]["median"]
    wide.instrument(True)
    marks = []
    for _ in range(args.warmup + args.reps):
        wide(seeds, targets)
        torch.cuda.synchronize()
        marks.append(wide.last_launch_ms().get("head_wide"))
    wide.instrument(False)
    marks = [1e3 * m for m in marks[args.warmup:] if m is not None]
    if marks:
        rows.append(dict(base, what="head_wide_launch", D=int(models[0].fc.weight.shape[1]), us=stats(marks),
                         note="one kernel timed at dispatch inside the recorded step"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
