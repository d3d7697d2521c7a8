#!/usr/bin/env python
"""weighted_bench.py -- what weighted graphs cost on the GPU, at the Reddit shape (232 965 nodes, degrees uniform in
1..841: ~98 M edges, 602 features, fan-out 25/10, dims 128/128, B = 512, bf16 compute) on store.DeviceCSR.synthetic with
weights drawn on the device (exp of a normal: three decades of spread, 5 % zeros).

One JSON line per measurement, appended to --out (default profiles/weighted_bench.jsonl), all in one process:
  edge_cdf_build        ms of gsage_edge_cdf_build (both launches) and the table's bytes
  hop/M12800_n10, hop/M512_n25
                        us / launch of gsage_sample_csr_weighted next to gsage_sample_csr_philox on the same ids
  segment_reduce        ms / call (both launches) of gsage_segment_reduce_weighted next to SEG_MEAN, same bf16 table, D = 128
  train_step            ms / step of GSSupervised.train_step on the module path with the weighted sampler next to the
                        uniform (Philox) one, same model, same seeds
Times are device events around `--steps` back-to-back calls after `--warmup` calls; the two sides of every comparison
alternate `--rounds` times and every round is reported, so that a drift of the machine shows in the spread.  Needs a GPU:
there is no CPU fallback."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch
from scipy import sparse
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gs = importlib.import_module("pytorch-graphsage_amd")


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def pair(fa, fb, steps, warmup, rounds):
    """(times of fa, times of fb), alternating"""
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(fa, steps, warmup))
        tb.append(timed(fb, steps, warmup))
    return ta, tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--deg-hi", type=int, default=841)
    ap.add_argument("--feats", type=int, default=602)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "weighted_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "weighted_bench needs a GPU"
    dev = torch.device("cuda")
    gs.ops.set_compute_dtype("bf16")
    gs.ops.warmup(dev)
    n, B = args.nodes, args.batch

    csr = gs.DeviceCSR.synthetic(n, 1, args.deg_hi, dev, seed=1)
    gen = torch.Generator(device=dev).manual_seed(3)
    w = torch.exp(torch.randn(csr.nnz, device=dev, generator=gen) * 2.3)
    w[torch.rand(csr.nnz, device=dev, generator=gen) < 0.05] = 0.0
    info = gs._native.device_info()
    base = {"arch": info["arch"] if info else None, "nodes": n, "edges": csr.nnz, "max_degree": args.deg_hi,
            "steps": args.steps, "warmup": args.warmup, "stamp": time.strftime("%Y-%m-%d")}
    rows = []

    # ---- the table
    t = [timed(lambda: gs.ops.edge_cdf(csr.rowptr, w, n), 5, 2) for _ in range(args.rounds)]
    csr.with_weights(w)
    rows.append(dict(base, what="edge_cdf_build", launches=2, ms_per_call=float(np.median(t)), rounds_ms=t,
                     table_bytes=csr.nnz * 8, weight_bytes=csr.nnz * 4,
                     note="includes zero-filling the output tensor (ops.edge_cdf)"))

    # ---- one hop
    rng = np.random.RandomState(0)
    for M, fan in ((12800, 10), (512, 25)):
        ids = torch.from_numpy(rng.randint(1, n, size=M)).to(dev)
        out = torch.empty(M * fan, dtype=torch.int64, device=dev)
        ph = {"seed": 1, "call_base": 0}
        tw, tu = pair(lambda: gs.ops.sample_csr_weighted(csr, ids, fan, ph, out=out),
                      lambda: gs.ops.sample_csr(csr, ids, fan, philox=ph, out=out), 200, 20, args.rounds)
        rows.append(dict(base, what="hop/M%d_n%d" % (M, fan), M=M, n=fan,
                         weighted_us=1e3 * float(np.median(tw)), uniform_us=1e3 * float(np.median(tu)),
                         weighted_rounds_us=[1e3 * v for v in tw], uniform_rounds_us=[1e3 * v for v in tu]))

    # ---- the full-neighbourhood mean
    D = 128
    table = gs.FeatureStore.synthetic(n, D, dev, dtype="bf16", seed=2).data
    out = torch.empty(n, D, dtype=torch.float32, device=dev)
    nat = gs._native
    gs.infer.plan(csr)
    tw, tu = pair(lambda: gs.infer.segment_reduce(csr, table[:, :D], nat.SEG_WEIGHTED_MEAN, out),
                  lambda: gs.infer.segment_reduce(csr, table[:, :D], nat.SEG_MEAN, out), 5, 2, args.rounds)
    rows.append(dict(base, what="segment_reduce", D=D, table="bf16", launches=2,
                     weighted_ms=float(np.median(tw)), mean_ms=float(np.median(tu)), weighted_rounds_ms=tw,
                     mean_rounds_ms=tu, bytes_rows=csr.nnz * D * 2, bytes_cdf=csr.nnz * 8, bytes_col=csr.nnz * 4))
    del table, out

    # ---- a module-path train step
    ph_adj = sparse.csr_matrix((np.array([1, 1]), np.array([0, 0]), np.array([0, 0, 1, 2])), shape=(3, 1))
    store = gs.FeatureStore.synthetic(n, args.feats, dev, dtype="bf16", seed=2)
    specs = [{"n_train_samples": f, "n_val_samples": f, "output_dim": 128,
              "activation": (lambda x: x) if i == 1 else F.relu} for i, f in enumerate((25, 10))]
    models = {}
    for name, sampler, adj in (("uniform", lambda adj: gs.nn_modules.SparseUniformNeighborSampler(adj, rng="philox"), ph_adj),
                               ("weighted", gs.find_sampler("sparse_weighted_neighbor_sampler"),
                                gs.WeightedAdj(ph_adj, np.ones(2, dtype=np.float32)))):
        torch.manual_seed(0)
        m = gs.GSSupervised(sampler_class=sampler, adj=adj, train_adj=adj, prep_class=gs.prep_lookup["identity"],
                            aggregator_class=gs.aggregator_lookup["mean"], input_dim=args.feats, n_nodes=n, n_classes=41,
                            layer_specs=specs).to(dev)
        m.train_sampler.use_device_csr(csr)
        m.val_sampler.use_device_csr(csr)
        models[name] = m
    seeds = torch.from_numpy(rng.randint(1, n, size=B)).to(dev)
    targets = torch.from_numpy(rng.randint(0, 41, size=(B, 1))).to(dev)
    loss = gs.ProblemLosses.classification
    tw, tu = pair(lambda: models["weighted"].train_step(seeds, store, targets, loss),
                  lambda: models["uniform"].train_step(seeds, store, targets, loss), args.steps, args.warmup, args.rounds)
    rows.append(dict(base, what="train_step", B=B, fan=[25, 10], dims=[128, 128], feats=args.feats, precision="bf16",
                     weighted_ms=float(np.median(tw)), uniform_ms=float(np.median(tu)), weighted_rounds_ms=tw,
                     uniform_rounds_ms=tu))
    csr.check()
    with open(args.out, "a") as f:
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
