#!/usr/bin/env python
"""One Adam iteration of the linear probe (infer.ProbeIteration: csrc/gsage_probe.hip + gsage_finalize_grads +
gsage_clip_adam_step, a replayed command list) next to the torch formulation a user writes today, on the MI355X, in
one process: one JSON line per shape and mode, appended to profiles/probe_bench.jsonl.

  shapes              reddit: n = 152 410 of N = 232 965 rows, D = 256, C = 41, classification
                      ppi:    n = 44 906 of N = 56 944 rows, D = 256, C = 121, multilabel_classification
                      random unit rows, random targets; the table is cast to the compute dtype once, outside both timings
  fused_ms            one replay of the recorded iteration (4 launches)
  torch_ms            z = X[ids] @ W.T + b; F.cross_entropy / F.multilabel_soft_margin_loss; backward;
                      torch.optim.Adam.step -- W a fp32 master cast to the compute dtype, as the fused pass sees it
  pass_bytes          n * D * element size: what one pass must read, and pass_bytes_per_s over fused_ms with its share
                      of the 8 TB/s HBM peak (the iteration also reads the S partial rows: partial_bytes)
  splits              the partial rows the library chose
Every figure is the median of --reps calls after --warmup calls, a host clock around work that ends in a device
synchronise; min and max are recorded next to it.  The two paths alternate inside the same loop.

    python tools/probe_bench.py [--shapes reddit,ppi] [--dtypes bf16,fp32] [--reps 7] [--warmup 2] [--out PATH]
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
SHAPES = {"reddit": dict(N=232965, n=152410, D=256, C=41, task="classification"),
          "ppi": dict(N=56944, n=44906, D=256, C=121, task="multilabel_classification")}


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
    ap.add_argument("--shapes", default="reddit,ppi")
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_bench: needs the GPU (nothing is measured without one)")
    gs = importlib.import_module("pytorch-graphsage_amd")
    dev = torch.device("cuda", 0)
    for name in args.shapes.split(","):
        sh = SHAPES[name]
        N, n, D, C, task = sh["N"], sh["n"], sh["D"], sh["C"], sh["task"]
        gen = torch.Generator(device=dev).manual_seed(0)
        emb = F.normalize(torch.randn(N, D, device=dev, generator=gen), dim=1)
        ids = torch.randperm(N, device=dev, generator=gen)[:n].contiguous()
        if task == "classification":
            y = torch.randint(0, C, (n,), device=dev, generator=gen)
        else:
            y = (torch.rand(n, C, device=dev, generator=gen) < 0.3).float()
        for dtype in args.dtypes.split(","):
            gs.ops.set_compute_dtype(dtype)
            cdt = gs.ops.torch_dtype()
            table = emb.to(cdt).contiguous()
            ids_c, y_c = gs.ops.probe_check(table, ids, y, C, D, task)
            fit = gs.infer.ProbeIteration(table, ids_c, y_c, task, C, args.warmup + args.reps, 0.1, 0.0)
            W = torch.zeros(C, D, device=dev, requires_grad=True)
            b = torch.zeros(C, device=dev, requires_grad=True)
            opt = torch.optim.Adam([W, b], lr=0.1)
            loss_fn = F.cross_entropy if task == "classification" else F.multilabel_soft_margin_loss

            def torch_iteration():
                opt.zero_grad(set_to_none=True)
                z = (table[ids] @ W.to(cdt).t()).float() + b
                loss_fn(z, y).backward()
                opt.step()

            t = {"fused_ms": [], "torch_ms": []}
            for it in range(args.warmup + args.reps):
                fused_ms = timed(lambda: fit.replay(1))
                torch_ms = timed(torch_iteration)
                if it >= args.warmup:
                    t["fused_ms"].append(fused_ms)
                    t["torch_ms"].append(torch_ms)
            rec = {"shape": name, "task": task, "n_rows": N, "n": n, "dim": D, "classes": C, "dtype": dtype,
                   "splits": fit.splits, "reps": args.reps, "warmup": args.warmup}
            rec.update({key: stats(v) for key, v in t.items()})
            sec = rec["fused_ms"]["median"] * 1e-3
            rec["pass_bytes"] = n * D * table.element_size()
            rec["partial_bytes"] = fit.splits * (C * D + C + 1) * 4
            rec["pass_bytes_per_s"] = rec["pass_bytes"] / sec
            rec["share_of_hbm_peak"] = rec["pass_bytes_per_s"] / HBM_PEAK
            rec["fused_over_torch"] = rec["fused_ms"]["median"] / rec["torch_ms"]["median"]
            # the two paths took the same steps from the same start: their parameters agree to the modes' round-off
            rec["max_abs_w_diff"] = float((fit.flat_p[:C * D].view(C, D) - W.detach()).abs().max())
            rec["loss_last"] = float(fit.loss_history[args.warmup + args.reps - 1])
            line = json.dumps(rec)
            print(line)
            sys.stdout.flush()
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
            del fit, table


if __name__ == "__main__":
    main()
