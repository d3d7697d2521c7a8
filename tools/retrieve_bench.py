#!/usr/bin/env python
"""Top-k retrieval over an embedding table (ops.topk_ip: csrc/gsage_retrieve.hip) next to the torch formulation a user
writes today, on the MI355X, in one process: one JSON line per query count, appended to profiles/retrieve_bench.jsonl.

  table               random unit rows at the Reddit shape: N = 232 965, D = 256; k = 10, exclude = "self"
  kernel_ms           ops.topk_ip(table, table[q], k, query_ids=q, exclude="self") -- the query-row gather, scan, merge
  torch_ms            table[q] @ table.T, the self column set to -inf, .topk(k), in chunks of queries whose score block
                      stays under 1 GiB; same compute dtype (the table is cast once, outside both timings)
  table_bytes_per_s   (Q <= 512) bytes of the table over kernel_ms, and its share of the 8 TB/s HBM peak: every query
                      tile has to read the whole table once, so this is the bound of a small Q
  flop_per_s          (Q = N) 2 Q N D over kernel_ms, and its share of the 2.5 PFLOP/s dense bf16 peak
  splits              the split count the library chose
  ids_equal           share of the [Q, k] ids on which both paths agree (the torch path rounds its bf16 scores to bf16
                      and has no tie order, so less than 1 is expected in the bf16 mode)
Every figure is the median of --reps calls after --warmup calls, a host clock around work that ends in a device
synchronise; min and max are recorded next to it.  The two paths alternate inside the same loop.

    python tools/retrieve_bench.py [--queries 1,512,32768,232965] [--dtype bf16] [--reps 7] [--warmup 2] [--out PATH]
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

HBM_PEAK = 8.0e12
BF16_PEAK = 2.5e15


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def torch_topk(table, q, k):
    """What a user writes today: chunked so the score block stays under 1 GiB."""
    N = int(table.shape[0])
    chunk = max(1, (1 << 30) // (N * table.element_size()))
    ids, scores = [], []
    for o in range(0, int(q.shape[0]), chunk):
        qq = q[o:o + chunk]
        s = table[qq] @ table.t()
        s[torch.arange(int(qq.shape[0]), device=s.device), qq] = float("-inf")
        v, i = s.topk(k, dim=1)
        ids.append(i)
        scores.append(v)
    return torch.cat(ids), torch.cat(scores)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", default="1,512,32768,232965")
    ap.add_argument("--rows", type=int, default=232965)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieve_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("retrieve_bench: needs the GPU (nothing is measured without one)")
    gs = importlib.import_module("pytorch-graphsage_amd")
    dev = torch.device("cuda", 0)
    gs.ops.set_compute_dtype(args.dtype)
    N, D, k = args.rows, args.dim, args.k
    gen = torch.Generator(device=dev).manual_seed(0)
    emb = torch.nn.functional.normalize(torch.randn(N, D, device=dev, generator=gen), dim=1)
    table = emb.to(gs.ops.torch_dtype()).contiguous()
    del emb
    for nq in (int(v) for v in args.queries.split(",")):
        q = torch.arange(N, device=dev) if nq == N else \
            torch.from_numpy(np.random.RandomState(nq).randint(0, N, size=nq)).to(dev)
        _, splits = gs.ops.topk_ip_workspace(nq, N, k, 0)
        rec = {"n_rows": N, "dim": D, "k": k, "exclude": "self", "dtype": args.dtype, "queries": nq, "splits": splits,
               "reps": args.reps, "warmup": args.warmup}
        t = {"kernel_ms": [], "torch_ms": []}
        for it in range(args.warmup + args.reps):
            kernel_ms, got = timed(lambda: gs.ops.topk_ip(table, table[q], k, query_ids=q, exclude="self"))
            torch_ms, ref = timed(lambda: torch_topk(table, q, k))
            if it >= args.warmup:
                t["kernel_ms"].append(kernel_ms)
                t["torch_ms"].append(torch_ms)
        rec.update({key: stats(v) for key, v in t.items()})
        sec = rec["kernel_ms"]["median"] * 1e-3
        if nq <= 512:
            rec["table_bytes_per_s"] = N * D * table.element_size() / sec
            rec["share_of_hbm_peak"] = rec["table_bytes_per_s"] / HBM_PEAK
        if nq == N:
            rec["flop_per_s"] = 2.0 * nq * N * D / sec
            rec["share_of_bf16_peak"] = rec["flop_per_s"] / BF16_PEAK
        rec["ids_equal"] = float((got[0] == ref[0]).float().mean())
        rec["kernel_over_torch"] = rec["kernel_ms"]["median"] / rec["torch_ms"]["median"]
        line = json.dumps(rec)
        print(line)
        sys.stdout.flush()
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
