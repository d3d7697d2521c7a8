#!/usr/bin/env python
"""One Lloyd iteration of k-means (infer.KMeansIteration: csrc/gsage_kmeans.hip, pass + update, a replayed command
list) and a whole 20-iteration fit from fixed centroids (gs.kmeans) next to the torch formulation a user writes today,
on the MI355X, in one process: one JSON line per shape and mode, appended to profiles/kmeans_bench.jsonl.

  shapes              reddit41 / reddit128: every one of N = 232 965 rows, D = 256, K = 41 / 128; random unit rows, the
                      initial centroids K of them; the table is cast to the compute dtype once, outside both timings
  fused_iter_ms       one replay of the recorded iteration (2 launches)
  torch_iter_ms       s = X @ C.T - 0.5 * (C * C).sum(1); a = s.argmax(1); sums = zeros.index_add_(0, a, X.float());
                      counts = bincount(a); C = sums / counts where counts > 0 -- C a fp32 master cast to the compute
                      dtype, as the fused pass sees it
  fused_fit_ms        gs.kmeans(table, K, iters=20, init=C0) as a user calls it: its checks (two readbacks), the
                      recording and two chunks of 10 iterations with their readback
  torch_fit_ms        20 torch iterations and one synchronise
  pass_bytes          N * D * element size: what one pass must read, and pass_bytes_per_s over fused_iter_ms with its
                      share of the 8 TB/s HBM peak (the update also reads the S partial rows: partial_bytes)
Every figure is the median of --reps calls after --warmup calls, a host clock around work that ends in a device
synchronise; min and max are recorded next to it.  The two paths alternate inside the same loop.

    python tools/kmeans_bench.py [--shapes reddit41,reddit128] [--dtypes bf16,fp32] [--reps 7] [--warmup 2] [--out PATH]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
FIT_ITERS = 20
SHAPES = {"reddit41": dict(N=232965, D=256, K=41), "reddit128": dict(N=232965, D=256, K=128)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="reddit41,reddit128")
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_bench: needs the GPU (nothing is measured without one)")
    gs = importlib.import_module("pytorch-graphsage_amd")
    dev = torch.device("cuda", 0)
    for name in args.shapes.split(","):
        sh = SHAPES[name]
        N, D, K = sh["N"], sh["D"], sh["K"]
        gen = torch.Generator(device=dev).manual_seed(0)
        emb = F.normalize(torch.randn(N, D, device=dev, generator=gen), dim=1)
        ids = torch.arange(N, device=dev)
        for dtype in args.dtypes.split(","):
            gs.ops.set_compute_dtype(dtype)
            cdt = gs.ops.torch_dtype()
            table = emb.to(cdt).contiguous()
            C0 = table[torch.randperm(N, device=dev, generator=gen)[:K]].float().contiguous()
            total = args.warmup + args.reps

            cen, bias = C0.clone(), torch.zeros(K, device=dev)
            gs.ops.kmeans_update(cen, bias)
            it = gs.infer.KMeansIteration(table, ids, cen, bias, total, False)
            S = int(it.partial.numel()) // (K * D + K + 2)
            Ct = C0.clone()

            def torch_iteration():
                Cc = Ct.to(cdt)
                s = (table @ Cc.t()).float() - 0.5 * (Cc.float() * Cc.float()).sum(dim=1)
                a = s.argmax(dim=1)
                sums = torch.zeros(K, D, device=dev).index_add_(0, a, table.float())
                counts = torch.bincount(a, minlength=K)
                live = counts > 0
                Ct[live] = sums[live] / counts[live].float()[:, None]
                return a

            def torch_fit():
                Ct.copy_(C0)
                for _ in range(FIT_ITERS):
                    torch_iteration()

            t = {"fused_iter_ms": [], "torch_iter_ms": [], "fused_fit_ms": [], "torch_fit_ms": []}
            fit = None
            for r in range(total):
                a = timed(lambda: it.replay(1))
                b = timed(torch_iteration)

                def fused_fit():
                    nonlocal fit
                    fit = gs.kmeans(table, K, iters=FIT_ITERS, init=C0)
                c = timed(fused_fit)
                d = timed(torch_fit)
                if r >= args.warmup:
                    for key, v in zip(("fused_iter_ms", "torch_iter_ms", "fused_fit_ms", "torch_fit_ms"), (a, b, c, d)):
                        t[key].append(v)
            rec = {"shape": name, "n_rows": N, "dim": D, "clusters": K, "dtype": dtype, "splits": S, "fit_iters": FIT_ITERS,
                   "fit_iters_run": fit.n_iter, "reps": args.reps, "warmup": args.warmup}
            rec.update({key: stats(v) for key, v in t.items()})
            sec = rec["fused_iter_ms"]["median"] * 1e-3
            rec["pass_bytes"] = N * D * table.element_size()
            rec["partial_bytes"] = S * (K * D + K + 2) * 4
            rec["pass_bytes_per_s"] = rec["pass_bytes"] / sec
            rec["share_of_hbm_peak"] = rec["pass_bytes_per_s"] / HBM_PEAK
            rec["fused_over_torch_iter"] = rec["fused_iter_ms"]["median"] / rec["torch_iter_ms"]["median"]
            rec["fused_over_torch_fit"] = rec["fused_fit_ms"]["median"] / rec["torch_fit_ms"]["median"]
            # the two fits took the same steps from the same start: their centroids agree to the modes' round-off
            # unless a row close to two centroids went the other way
            rec["max_abs_centroid_diff"] = float((fit.centroids - Ct).abs().max())
            rec["inertia_last"] = float(fit.inertia)
            line = json.dumps(rec)
            print(line)
            sys.stdout.flush()
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
            del it, fit, table


if __name__ == "__main__":
    main()
