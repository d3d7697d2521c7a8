#!/usr/bin/env python
"""Graph propagation (ops.propagate_step, gs.correct_and_smooth) on the MI355X against the torch formulation of the
same arithmetic: one JSON line per configuration, printed and appended to profiles/propagate_bench.jsonl.

  step_ms             one propagation step -- gsage_propagate's two launches (sum over the stored neighbours, scale,
                      residual, clamp, the next step's pre-scaled y) --, CUDA events, median of 7 after 2 warm-ups
  step_bytes_per_s    nnz x round_up(C, 4) x 4 bytes (the neighbour rows the step REQUESTS) / step time; "achieved" in the
                      sense of requested: the iterate of the Reddit shape is 41 MB and sits in the Infinity Cache
  cs_ms               a 50 + 50 gs.correct_and_smooth call, set-up included, wall time after a synchronise
  torch_step_ms       the same step as S @ x on a torch.sparse CSR tensor (values a[v] * b[u]) plus the elementwise
  torch_cs_ms         residual and clamp; the same 50 + 50 loop.  Timed in the same process, alternating with ours.

Configurations: the Reddit-scale synthetic of tools/full_neighbour_bench.py (232 965 rows + dummy, mean degree ~421,
9.8e7 edges) with C = 41, and a PPI-like shape (56 944 rows + dummy, degree 1..56, 1.6e6 edges) with C = 121.

    python tools/propagate_bench.py [--configs reddit,ppi] [--reps 7] [--warmup 2] [--no-torch] [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def build(gs, name, dev):
    if name == "reddit":
        return reddit_csr(gs, dev), 41
    return gs.DeviceCSR.synthetic(56945, 1, 56, dev, seed=1, empty_every=97), 121


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def torch_operator(csr, a, b):
    """S = diag(a) A diag(b) as a torch.sparse CSR tensor (duplicates stay separate entries)."""
    deg = csr.rowptr[1:] - csr.rowptr[:-1]
    col = csr.col.long()
    vals = torch.repeat_interleave(a, deg) * b[col]
    return torch.sparse_csr_tensor(csr.rowptr, col, vals, size=(csr.n_rows, csr.n_rows))


def torch_propagate(S, x, iters, alpha, base, lo, hi):
    for _ in range(iters):
        x = torch.clamp((1.0 - alpha) * base + alpha * (S @ x), lo, hi)
    return x


def torch_correct_and_smooth(S, logits, y, nodes):
    """gs.correct_and_smooth's defaults (classification, autoscale) over S @ x"""
    Z = torch.softmax(logits, dim=1)
    Y = torch.zeros(nodes.numel(), Z.shape[1], device=Z.device)
    Y[torch.arange(nodes.numel(), device=Z.device), y] = 1.0
    E0 = torch.zeros_like(Z)
    E0[nodes] = Y - Z[nodes]
    E = torch_propagate(S, E0, 50, 0.8, E0, -1.0, 1.0)
    s = E0[nodes].abs().sum(1).mean() / E.abs().sum(1)
    s = torch.where(torch.isfinite(s) & (s <= 1000.0), s, torch.ones_like(s))
    G0 = Z + s.view(-1, 1) * E
    G0[nodes] = Y
    return torch_propagate(S, G0, 50, 0.8, G0, 0.0, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="reddit,ppi")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "propagate_bench.jsonl"))
    args = ap.parse_args()
    gs = importlib.import_module("pytorch-graphsage_amd")
    dev = torch.device("cuda", 0)
    for name in args.configs.split(","):
        csr, C = build(gs, name, dev)
        n, nnz, Cp = csr.n_rows, csr.nnz, (C + 3) // 4 * 4
        gen = torch.Generator(device=dev).manual_seed(3)
        plan = gs.infer.plan(csr)
        a, b = gs.ops.propagate_scales(csr.rowptr, n, "sym")
        x = torch.rand(n, Cp, device=dev, generator=gen)
        x[:, C:] = 0
        y, nxt = b.view(-1, 1) * x, torch.zeros_like(x)
        logits = torch.randn(n, C, device=dev, generator=gen)
        nodes = torch.arange(1, n, 3, device=dev)
        labels = torch.randint(0, C, (nodes.numel(),), device=dev, generator=gen)

        def ours_step():
            gs.ops.propagate_step(csr, plan, y, x, a, b, 0.8, 0.2, 0.0, 1.0, C, yout=nxt)

        def ours_cs():
            gs.correct_and_smooth(csr, logits, labels, nodes, "classification")

        rec = {"config": name, "n_rows": n, "nnz": nnz, "C": C, "norm": "sym", "reps": args.reps, "warmup": args.warmup,
               "plan": {k: plan[k] for k in ("n_short", "n_slices", "n_long", "slice_len")}}
        S = None
        if not args.no_torch:
            try:
                S = torch_operator(csr, a, b)
                xc, bc = x[:, :C].contiguous(), x[:, :C].contiguous()
                torch_step = lambda: torch_propagate(S, xc, 1, 0.8, bc, 0.0, 1.0)                    # noqa: E731
                torch_cs = lambda: torch_correct_and_smooth(S, logits, labels, nodes)                # noqa: E731
                torch_step()
                torch.cuda.synchronize()
            except Exception as e:                      # (recorded, not hidden: the line says why it is missing)
                rec["torch_error"] = "%s: %s" % (type(e).__name__, e)
                S = None
        t = {"step": [], "cs": [], "torch_step": [], "torch_cs": []}
        for i in range(args.warmup + args.reps):        # alternating: ours, torch, ours, torch, ...
            keep = i >= args.warmup
            for key, fn, timer in (("step", ours_step, event_ms), ("torch_step", torch_step if S is not None else None,
                                                                   event_ms),
                                   ("cs", ours_cs, wall_ms), ("torch_cs", torch_cs if S is not None else None, wall_ms)):
                if fn is not None:
                    ms = timer(fn)
                    if keep:
                        t[key].append(ms)
        csr.check()
        rec["step_ms"], rec["cs_ms"] = median(t["step"]), median(t["cs"])
        rec["step_bytes"] = nnz * Cp * 4
        rec["step_bytes_per_s"] = rec["step_bytes"] / (rec["step_ms"] * 1e-3)
        rec["step_edges_per_s"] = nnz / (rec["step_ms"] * 1e-3)
        if S is not None:
            rec["torch_step_ms"], rec["torch_cs_ms"] = median(t["torch_step"]), median(t["torch_cs"])
            rec["step_speedup_over_torch"] = rec["torch_step_ms"] / rec["step_ms"]
            rec["cs_speedup_over_torch"] = rec["torch_cs_ms"] / rec["cs_ms"]
        line = json.dumps(rec)
        print(line)
        sys.stdout.flush()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        del csr, S, x, y, nxt, logits
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
