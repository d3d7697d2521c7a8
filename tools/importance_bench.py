#!/usr/bin/env python
"""importance_bench.py -- what importance neighbourhoods cost on the GPU, at the Reddit shape (232 965 nodes, degrees
uniform in 1..841: ~98 M edges) on store.DeviceCSR.synthetic, uniform steps and weighted steps (weights drawn on the
device: exp of a normal, 5 % zeros), for (n_walks, walk_len, top) = (50, 2, 16) and (200, 5, 32).

One JSON line per (parameters, mode), appended to --out (default profiles/importance_bench.jsonl), all in one process:
  kernel_ms     gsage_importance_walks over every row, one launch
  compact_ms    the row offsets (torch.cumsum) and gsage_importance_compact
  cdf_ms        gsage_edge_cdf_build on the counts (both launches, with the output's zero-fill: ops.edge_cdf)
  build_ms      DeviceCSR.importance as a caller sees it (the three above, the id vector, the validation of the weights,
                check()'s readback)
  torch_ms      the same neighbourhoods in stock torch ops, uniform steps only: steps by rand * degree + gather, counts
                by sort / unique_consecutive, top-T by topk on packed (count, id) keys over a padded [rows, landings]
                matrix, in chunks whose buffers stay under 1 GiB.  Its draws are torch's, so its rows are not the
                kernel's rows; what it costs is what is compared.
Each figure is the median of --reps timed calls (device events) after --warmup calls; every call's time is reported.
Needs a GPU: there is no CPU fallback."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gs = importlib.import_module("pytorch-graphsage_amd")


def timed(fn, reps, warmup):
    """-> ms of every one of `reps` calls"""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def torch_importance(csr, R, L, T, gen):
    """(col int32 [n, T], w fp32 [n, T], deg int32 [n]) by stock torch ops, uniform steps"""
    n, dev, nnz = csr.n_rows, csr.device, csr.nnz
    per = max(1, (1 << 30) // (R * L * 8 * 6))                          # six int64 [rows, R * L] buffers at a time
    cols, ws, degs = [], [], []
    for o in range(0, n, per):
        m = min(per, n - o)
        v = torch.arange(o, o + m, device=dev).repeat_interleave(R)
        u, alive = v.clone(), torch.ones(m * R, dtype=torch.bool, device=dev)
        land = torch.full((m * R, L), -1, dtype=torch.int64, device=dev)
        for s in range(L):
            beg = csr.rowptr[u]
            deg = csr.rowptr[u + 1] - beg
            alive &= deg > 0
            off = (torch.rand(m * R, device=dev, generator=gen, dtype=torch.float64) * deg).long()
            nu = csr.col[(beg + torch.minimum(off, (deg - 1).clamp_(min=0))).clamp_(max=nnz - 1)].long()
            u = torch.where(alive, nu, u)
            land[:, s] = torch.where(alive & (u != v), u, land[:, s])
        src = torch.arange(m, device=dev).repeat_interleave(R * L)
        land = land.view(-1)
        ok = land >= 0
        key, count = torch.unique_consecutive(torch.sort(src[ok] * n + land[ok]).values, return_counts=True)
        ks, kid = key // n, key % n
        first = torch.searchsorted(ks, torch.arange(m, device=dev))
        pos = torch.arange(ks.shape[0], device=dev) - first[ks]
        packed = torch.full((m, R * L), -1, dtype=torch.int64, device=dev)
        packed[ks, pos] = (count << 32) | (0xFFFFFFFF - kid)
        top = torch.topk(packed, min(T, R * L), dim=1).values
        live = top >= 0
        cols.append(torch.where(live, 0xFFFFFFFF - (top & 0xFFFFFFFF), 0).int())
        ws.append(torch.where(live, top >> 32, 0).float())
        degs.append(live.sum(1).int())
    return torch.cat(cols), torch.cat(ws), torch.cat(degs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--deg-hi", type=int, default=841)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "importance_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "importance_bench needs a GPU"
    dev = torch.device("cuda")
    gs.ops.warmup(dev)
    n = args.nodes
    csr = gs.DeviceCSR.synthetic(n, 1, args.deg_hi, dev, seed=1)
    gen = torch.Generator(device=dev).manual_seed(3)
    w = torch.exp(torch.randn(csr.nnz, device=dev, generator=gen) * 2.3)
    w[torch.rand(csr.nnz, device=dev, generator=gen) < 0.05] = 0.0
    weighted = gs.DeviceCSR(csr.rowptr, csr.col, n, csr.max_deg).with_weights(w)
    del w
    info = gs._native.device_info()
    base = {"arch": info["arch"] if info else None, "nodes": n, "edges": csr.nnz, "max_degree": args.deg_hi,
            "reps": args.reps, "warmup": args.warmup, "stamp": time.strftime("%Y-%m-%d")}
    ids = torch.arange(n, dtype=torch.int64, device=dev)
    med = lambda t: float(np.median(t))
    rows = []
    for R, L, T in ((50, 2, 16), (200, 5, 32)):
        for mode, adj in (("uniform", csr), ("weighted", weighted)):
            tk = timed(lambda: gs.ops.importance_walks(adj, ids, R, L, T, 1), args.reps, args.warmup)
            col, cnt, deg = gs.ops.importance_walks(adj, ids, R, L, T, 1)
            tc = timed(lambda: gs.ops.importance_compact(col, cnt, deg), args.reps, args.warmup)
            c2, w2 = gs.ops.importance_compact(col, cnt, deg)
            rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            torch.cumsum(deg, 0, dtype=torch.int64, out=rowptr[1:])
            td = timed(lambda: gs.ops.edge_cdf(rowptr, w2, n), args.reps, args.warmup)
            tb = timed(lambda: adj.importance(R, L, T, seed=1), args.reps, args.warmup)
            row = dict(base, what="importance/R%d_L%d_T%d/%s" % (R, L, T, mode), n_walks=R, walk_len=L, top=T, mode=mode,
                       new_edges=int(c2.shape[0]), kernel_ms=med(tk), compact_ms=med(tc), cdf_ms=med(td),
                       build_ms=med(tb), kernel_calls_ms=tk, compact_calls_ms=tc, cdf_calls_ms=td, build_calls_ms=tb)
            del col, cnt, deg, c2, w2, rowptr
            if mode == "uniform":
                tt = timed(lambda: torch_importance(adj, R, L, T, gen), args.reps, args.warmup)
                row.update(torch_ms=med(tt), torch_calls_ms=tt)
            adj.check()
            rows.append(row)
            line = json.dumps(row)
            print(line)
            sys.stdout.flush()
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
