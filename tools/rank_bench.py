#!/usr/bin/env python
"""Exact link ranking over an embedding table (ops.rank_ip: csrc/gsage_rank.hip) next to the torch formulation a user
writes today, on the MI355X, in one process: one JSON line per (exclude, pair count), appended to
profiles/rank_bench.jsonl.

  table               random unit rows at the Reddit shape: N = 232 965, D = 256
  pairs               Q random (src, dst) pairs; exclude = "self", and "neighbours" over a random strictly ascending CSR
                      of mean degree 50
  kernel_ms           ops.rank_ip(table, table[src], dst, query_ids=src, csr, exclude) -- the query-row gather, scan,
                      (filter,) finish
  torch_ms            (table[src] @ table.T > score[:, None]).sum(1) + 1 with score = the pair's own dot product, in
                      chunks of pairs whose score block stays under 1 GiB; same compute dtype.  It excludes nothing, has
                      no tie rule and rounds its bf16 scores to bf16 -- it is the UNFILTERED rank, timed for both modes
  flop_per_s          2 Q N D over kernel_ms, and its share of the 2.5 PFLOP/s dense bf16 peak
  table_bytes_per_s   (Q <= 512) bytes of the table over kernel_ms, and its share of the 8 TB/s HBM peak
  ranks_equal         share of the pairs on which both paths give the same rank (exclude = "self" only; less than 1 is
                      expected: ties, bf16-rounded scores and the self row on the torch side)
Every figure is the median of --reps calls after --warmup calls, a host clock around work that ends in a device
synchronise; min and max are recorded next to it.  The two paths alternate inside the same loop.

    python tools/rank_bench.py [--pairs 512,32768,262144] [--dtype bf16] [--reps 7] [--warmup 2] [--out PATH]
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


def torch_rank(table, src, dst):
    """What a user writes today: chunked so the score block stays under 1 GiB."""
    N = int(table.shape[0])
    chunk = max(1, (1 << 30) // (N * table.element_size()))
    out = []
    for o in range(0, int(src.shape[0]), chunk):
        q = table[src[o:o + chunk]]
        score = (q * table[dst[o:o + chunk]]).sum(1)
        out.append(((q @ table.t()) > score[:, None]).sum(1) + 1)
    return torch.cat(out)


def random_csr(gs, N, mean_deg, dev):
    """rows of degree uniform in [0, 2 * mean_deg], distinct sorted columns (duplicates of the draw dropped)"""
    gen = torch.Generator(device=dev).manual_seed(1)
    deg = torch.randint(0, 2 * mean_deg + 1, (N,), device=dev, generator=gen)
    rowptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    torch.cumsum(deg, 0, out=rowptr[1:])
    col = torch.randint(0, N, (int(rowptr[-1]),), dtype=torch.int32, device=dev, generator=gen)
    return gs.infer.filter_csr(gs.DeviceCSR(rowptr, col, N, 2 * mean_deg))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="512,32768,262144")
    ap.add_argument("--rows", type=int, default=232965)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--degree", type=int, default=50)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rank_bench: needs the GPU (nothing is measured without one)")
    gs = importlib.import_module("pytorch-graphsage_amd")
    dev = torch.device("cuda", 0)
    gs.ops.set_compute_dtype(args.dtype)
    N, D = args.rows, args.dim
    gen = torch.Generator(device=dev).manual_seed(0)
    emb = torch.nn.functional.normalize(torch.randn(N, D, device=dev, generator=gen), dim=1)
    table = emb.to(gs.ops.torch_dtype()).contiguous()
    del emb
    csr = random_csr(gs, N, args.degree, dev)
    for exclude in ("self", "neighbours"):
        for nq in (int(v) for v in args.pairs.split(",")):
            rng = np.random.RandomState(nq)
            src = torch.from_numpy(rng.randint(0, N, size=nq)).to(dev)
            dst = torch.from_numpy(rng.randint(0, N, size=nq)).to(dev)
            _, splits = gs.ops.rank_ip_workspace(nq, N, 0)
            rec = {"n_rows": N, "dim": D, "exclude": exclude, "dtype": args.dtype, "pairs": nq, "splits": splits,
                   "csr_mean_degree": float(csr.nnz) / N, "reps": args.reps, "warmup": args.warmup}
            t = {"kernel_ms": [], "torch_ms": []}
            for it in range(args.warmup + args.reps):
                kernel_ms, got = timed(lambda: gs.ops.rank_ip(table, table[src], dst, query_ids=src, csr=csr,
                                                              exclude=exclude))
                torch_ms, ref = timed(lambda: torch_rank(table, src, dst))
                if it >= args.warmup:
                    t["kernel_ms"].append(kernel_ms)
                    t["torch_ms"].append(torch_ms)
            rec.update({key: stats(v) for key, v in t.items()})
            sec = rec["kernel_ms"]["median"] * 1e-3
            rec["flop_per_s"] = 2.0 * nq * N * D / sec
            rec["share_of_bf16_peak"] = rec["flop_per_s"] / BF16_PEAK
            if nq <= 512:
                rec["table_bytes_per_s"] = N * D * table.element_size() / sec
                rec["share_of_hbm_peak"] = rec["table_bytes_per_s"] / HBM_PEAK
            if exclude == "self":
                rec["ranks_equal"] = float((got[0] == ref).float().mean())
            rec["kernel_over_torch"] = rec["kernel_ms"]["median"] / rec["torch_ms"]["median"]
            line = json.dumps(rec)
            print(line)
            sys.stdout.flush()
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
