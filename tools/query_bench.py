#!/usr/bin/env python
"""Full-neighbourhood inference for a query set (infer.query: k-hop closure blocks) next to the whole-graph path
(infer.full_neighbour) on the MI355X, in one process: one JSON line per query-set size, appended to
profiles/query_bench.jsonl.

  graph               the papers-like synthetic of tools/full_neighbour_bench.py (8 M rows, degree 14..44, 128-d bf16
                      features), mean aggregator, 2 layers at 128/128
  whole_ms            full_neighbour(nodes=queries): every layer for every row, then the queries' rows
  query_ms            query(): closure build + row gather + the layers over the blocks + head
  closure_ms          closure() alone (its launches and its one readback per level)
  layers_ms           query_ms' remainder, timed on its own: gather, projections, block reduces, head, given the closure
  sizes               |S_0| .. |S_L|: rows per level of the closure; block_edges: edges per block
Every figure is the median of --reps calls after --warmup calls, a host clock around work that ends in a device
synchronise; min and max are recorded next to it.  The two paths alternate inside the same loop.

    python tools/query_bench.py [--queries 1000,100000] [--reps 7] [--warmup 2] [--rows 8000001] [--out PATH]
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", default="1000,100000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=8_000_001)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("query_bench: needs the GPU (nothing is measured without one)")
    gs = importlib.import_module("pytorch-graphsage_amd")
    fnb = importlib.import_module("full_neighbour_bench")
    infer = gs.infer
    dev = torch.device("cuda", 0)
    gs.ops.set_compute_dtype("bf16")
    csr, store, model = fnb.build(gs, "papers", "mean", dev)
    if args.rows != csr.n_rows:
        csr = gs.DeviceCSR.synthetic(args.rows, 14, 44, dev, max_deg=4096, seed=1, empty_every=1000)
        store = gs.FeatureStore.synthetic(csr.n_rows, 128, dev, dtype="bf16", seed=2)
    depth = len(list(model.agg_layers.children()))
    gs.full_neighbour(model, store, adj=csr)                          # the whole-graph plan
    for nq in (int(v) for v in args.queries.split(",")):
        q = torch.from_numpy(np.random.RandomState(nq).randint(1, csr.n_rows, size=nq)).to(dev)
        rec = {"n_rows": csr.n_rows, "nnz": csr.nnz, "feat_dim": store.dim, "dims": [128, 128], "dtype": "bf16",
               "aggregator": "mean", "queries": nq, "reps": args.reps, "warmup": args.warmup}
        t = {"whole_ms": [], "query_ms": [], "closure_ms": [], "layers_ms": []}
        for it in range(args.warmup + args.reps):
            whole_ms, whole = timed(lambda: gs.full_neighbour(model, store, nodes=q, adj=csr))
            query_ms, got = timed(lambda: infer.query(model, store, q, adj=csr))
            # (the closure is built twice per iteration, inside query() and on its own: each figure is a whole call)
            closure_ms, cl = timed(lambda: infer.closure(csr, q, depth))
            layers_ms, again = timed(lambda: infer.query(model, store, q, adj=csr, closure=cl))
            if it >= args.warmup:
                for k, v in (("whole_ms", whole_ms), ("query_ms", query_ms), ("closure_ms", closure_ms),
                             ("layers_ms", layers_ms)):
                    t[k].append(v)
        rec.update({k: stats(v) for k, v in t.items()})
        rec["sizes"] = cl.sizes()
        rec["block_edges"] = [int(b.col.shape[0]) for b in cl.blocks[1:]]
        rec["max_abs_diff_vs_whole"] = float((got - whole).abs().max())
        rec["bitwise_repeatable"] = bool(torch.equal(got, again))
        rec["speedup_median"] = rec["whole_ms"]["median"] / rec["query_ms"]["median"]
        csr.check()
        line = json.dumps(rec)
        print(line)
        sys.stdout.flush()
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
