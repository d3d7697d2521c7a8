#!/usr/bin/env python
"""Layer-wise full-neighbourhood inference (infer.full_neighbour) on the MI355X: one JSON line per configuration.

  layers_ms[l]        wall time of layer l (projections + segment reduce), CUDA events
  reduce_ms[l]        the segment-reduce call of layer l (its two launches)
  edges_per_s         edges of the adjacency (degree-0 rows count one) / reduce time, per layer
  reduce_bytes        bytes the reduce REQUESTS: one table row chunk per edge + the int32 id + the output rows
  effective_frac_of_8TBs  reduce_bytes / reduce time / 8 TB/s -- "effective": the L2 / Infinity Cache may serve part
                      of it (the projected table of the Reddit shape is ~60 MB)
  sampled_eval_ms     the sampled forward-only evaluation (the fused engine's evaluate_fold) over every node, same
                      model, fan-out 25/10 -- the path full_neighbour replaces

Configurations: the Reddit-scale synthetic of BASELINE.md (232 965 rows + dummy, 602-d bf16 features, mean degree
~421, a few rows of degree 21 657) and a sparser papers-like shape (8 M rows, degree 14..44, 128-d), each with the
mean and the max-pool aggregator, 2 layers at 128/128, bf16.

    python tools/full_neighbour_bench.py [--configs reddit,papers] [--aggs mean,max_pool] [--reps 3] [--no-sampled]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def reddit_csr(gs, dev, n_rows=232966, hot=(21657, 20000, 15000, 12000), seed=0):
    """mean degree ~421 (uniform 1..841), row 0 the dummy, a few hot rows up to the BASELINE maximum 21 657"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    deg = torch.randint(1, 842, (n_rows,), dtype=torch.int64, device=dev, generator=gen)
    deg[0] = 0
    for i, d in enumerate(hot):
        deg[1 + 977 * i] = d
    rowptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
    torch.cumsum(deg, 0, out=rowptr[1:])
    col = torch.randint(1, n_rows, (int(rowptr[-1]),), dtype=torch.int32, device=dev, generator=gen)
    return gs.DeviceCSR(rowptr, col, n_rows, int(deg.max()))


def build(gs, name, agg, dev):
    if name == "reddit":
        csr = reddit_csr(gs, dev)
        store = gs.FeatureStore.synthetic(csr.n_rows, 602, dev, dtype="bf16", seed=2)
    else:
        csr = gs.DeviceCSR.synthetic(8_000_001, 14, 44, dev, max_deg=4096, seed=1, empty_every=1000)
        store = gs.FeatureStore.synthetic(csr.n_rows, 128, dev, dtype="bf16", seed=2)
    from scipy import sparse
    ph = sparse.csr_matrix((np.array([1, 1]), np.array([0, 0]), np.array([0, 0, 1, 2])), shape=(3, 1))
    gs.nn_modules.SparseUniformNeighborSampler.rng_default = "philox"
    specs = [{"n_train_samples": f, "n_val_samples": f, "output_dim": 128,
              "activation": (lambda x: x) if i == 1 else F.relu} for i, f in enumerate((25, 10))]
    torch.manual_seed(0)
    model = gs.GSSupervised(sampler_class=gs.sampler_lookup["sparse_uniform_neighbor_sampler"], adj=ph, train_adj=ph,
                            prep_class=gs.prep_lookup["identity"], aggregator_class=gs.aggregator_lookup[agg],
                            input_dim=store.dim, n_nodes=csr.n_rows, n_classes=41, layer_specs=specs).to(dev)
    model.val_sampler.use_device_csr(csr)
    model.train_sampler.use_device_csr(csr)
    return csr, store, model


def timed_call(gs, model, store, csr, reps):
    """(total ms, per-layer ms, per-layer reduce ms) of the best of `reps` calls"""
    infer = gs.infer
    marks = {"layer": [], "reduce": []}
    orig_layer, orig_reduce = infer._layer_device, infer.segment_reduce

    def ev():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def layer(*a, **k):
        e0 = ev()
        r = orig_layer(*a, **k)
        marks["layer"].append((e0, ev()))
        return r

    def reduce(*a, **k):
        e0 = ev()
        r = orig_reduce(*a, **k)
        marks["reduce"].append((e0, ev()))
        return r

    infer._layer_device, infer.segment_reduce = layer, reduce
    best = None
    try:
        for _ in range(reps):
            marks["layer"].clear()
            marks["reduce"].clear()
            torch.cuda.synchronize()
            t0 = ev()
            gs.full_neighbour(model, store, adj=csr)
            t1 = ev()
            torch.cuda.synchronize()
            rec = (t0.elapsed_time(t1), [a.elapsed_time(b) for a, b in marks["layer"]],
                   [a.elapsed_time(b) for a, b in marks["reduce"]])
            if best is None or rec[0] < best[0]:
                best = rec
    finally:
        infer._layer_device, infer.segment_reduce = orig_layer, orig_reduce
    return best


def sampled_eval_ms(gs, model, store, csr, B=512):
    nodes = np.arange(1, csr.n_rows)
    chunks = np.array_split(np.arange(nodes.shape[0]), nodes.shape[0] // B + 1)
    Bm = max(int(c.shape[0]) for c in chunks)
    ids = torch.from_numpy(np.stack([np.concatenate([nodes[c], np.repeat(nodes[c[:1]], Bm - c.shape[0])])
                                     for c in chunks])).cuda()
    live = [int(c.shape[0]) for c in chunks]
    cls = gs.engine.fused_engine_for(model, store)
    tg = torch.zeros(Bm, 1, dtype=torch.int64, device=ids.device)
    eng = cls(model, store, gs.ProblemLosses.classification, ids[0], tg, eval_only=True)
    eng.evaluate_fold(ids[:2], live[:2])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.evaluate_fold(ids, live)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, cls.__name__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="reddit,papers")
    ap.add_argument("--aggs", default="mean,max_pool")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-sampled", action="store_true")
    args = ap.parse_args()
    gs = importlib.import_module("pytorch-graphsage_amd")
    dev = torch.device("cuda", 0)
    gs.ops.set_compute_dtype("bf16")
    for name in args.configs.split(","):
        for agg in args.aggs.split(","):
            csr, store, model = build(gs, name, agg, dev)
            gs.full_neighbour(model, store, adj=csr)                 # plan + warm-up
            torch.cuda.synchronize()
            total, layers, reduces = timed_call(gs, model, store, csr, args.reps)
            deg = csr.rowptr[1:] - csr.rowptr[:-1]
            edges = int(deg.clamp(min=1).sum())
            # reduced table: the projected 128-wide bf16 table (mean), the 512-wide relu(MLP) output (max-pool)
            width, out_b = (128, 4) if agg == "mean" else (512, 4)
            rbytes = edges * (width * 2 + 4) + csr.n_rows * width * out_b + csr.n_rows * 8
            rec = {"config": name, "aggregator": agg, "n_rows": csr.n_rows, "edges": edges, "feat_dim": store.dim,
                   "dims": [128, 128], "dtype": "bf16", "total_ms": total, "layers_ms": layers, "reduce_ms": reduces,
                   "reduced_width": width, "reduce_bytes": rbytes,
                   "edges_per_s": [edges / (r * 1e-3) for r in reduces],
                   "effective_frac_of_8TBs": [rbytes / (r * 1e-3) / HBM_PEAK for r in reduces],
                   "plan": {k: gs.infer.plan(csr)[k] for k in ("n_short", "n_slices", "n_long", "slice_len")}}
            if not args.no_sampled:
                try:
                    ms, eng = sampled_eval_ms(gs, model, store, csr)
                    rec.update({"sampled_eval_ms": ms, "sampled_engine": eng, "sampled_fanout": [25, 10],
                                "sampled_nodes": csr.n_rows - 1})
                except Exception as e:                  # (recorded, not hidden: the line says why it is missing)
                    rec["sampled_eval_error"] = "%s: %s" % (type(e).__name__, e)
            csr.check()
            print(json.dumps(rec))
            sys.stdout.flush()
            del csr, store, model
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
