#!/usr/bin/env python
"""LSTMAggregator forward + backward on the MI355X: one JSON line per shape, mode and input route.

  ms            per-call times of the repeats (CUDA events around forward + backward, after the warm-up calls)
  median_ms     their median;  spread_ms = max - min: the run-to-run spread of this line's own repeats
  route         "tensor": materialised fp32 neighbour rows that want a gradient (the d neibs GEMM runs);
                "rowref": lazy rows of a FeatureStore in the mode's storage precision (no d neibs)
  path          "hip": this library's kernels (ops.lstm_last);  "stock": torch.nn.LSTM on the same shapes (--stock),
                i.e. what LSTMAggregator.forward ran before: fp32 rows, the whole [M, n, hidden] sequence

Shapes: the Reddit hop 1 (M = 12 800, n = 10, D = 602, hidden 512) and the Reddit seed level (M = 512, n = 25,
D = 256, hidden 512), each uni- and bidirectional; output_dim 128, ReLU.

    python tools/lstm_bench.py [--modes bf16,fp32] [--stock] [--reps 7] [--warmup 3] [--shapes hop1,seed]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"hop1": (12800, 10, 602), "seed": (512, 25, 256)}


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="bf16,fp32")
    ap.add_argument("--shapes", default="hop1,seed")
    ap.add_argument("--stock", action="store_true", help="also time torch.nn.LSTM on the same shapes")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert args.reps >= 5, "medians of at least five repeats"
    gs = importlib.import_module("pytorch-graphsage_amd")
    dev = torch.device("cuda", 0)
    gs.ops.warmup(dev)
    stock_forward = gs.nn_modules.LSTMAggregator.forward

    def stock(self, x, neibs):            # the module's host-mode lines, on CUDA tensors: the path before the kernels
        xt, nt = gs.nn_modules._as_tensor(x).float(), gs.nn_modules._as_tensor(neibs).float()
        seq, _ = self.lstm(nt.view(xt.size(0), -1, nt.size(1)))
        return self._project(xt, seq[:, -1, :].contiguous())

    R = 232966
    for shape in args.shapes.split(","):
        M, n, D = SHAPES[shape]
        rng = np.random.RandomState(0)
        idx = torch.from_numpy(rng.randint(1, R, size=M)).to(dev)
        idn = torch.from_numpy(rng.randint(1, R, size=M * n)).to(dev)
        for bidir in (False, True):
            torch.manual_seed(0)
            agg = gs.aggregator_lookup["lstm"](input_dim=D, output_dim=128, activation=torch.relu, hidden_dim=512,
                                               bidirectional=bidir).to(dev)
            paths = [("hip", m) for m in args.modes.split(",")] + ([("stock", "fp32")] if args.stock else [])
            for path, mode in paths:
                gs.ops.set_compute_dtype(mode)
                store = gs.FeatureStore.synthetic(R, D, dev, dtype=mode, seed=2)
                gs.nn_modules.LSTMAggregator.forward = stock if path == "stock" else stock_forward
                try:
                    for route in ("tensor", "rowref"):
                        if route == "tensor":
                            x = store[idx].materialize()
                            nb = store[idn].materialize().requires_grad_(True)
                        else:
                            x, nb = store[idx], store[idn]

                        def step():
                            agg.zero_grad(set_to_none=True)
                            if route == "tensor":
                                nb.grad = None
                            agg(x, nb).float().sum().backward()
                        before = gs._native.launch_count()
                        ms = timed(step, args.warmup, args.reps)
                        launches = (gs._native.launch_count() - before) // (args.warmup + args.reps)
                        print(json.dumps({"shape": shape, "M": M, "n": n, "D": D, "hidden_dim": 512,
                                          "bidirectional": bidir, "path": path, "mode": mode, "route": route,
                                          "ms": [round(v, 4) for v in ms], "median_ms": float(np.median(ms)),
                                          "spread_ms": max(ms) - min(ms), "gsage_launches_per_call": launches}))
                        sys.stdout.flush()
                finally:
                    gs.nn_modules.LSTMAggregator.forward = stock_forward
                del store
                torch.cuda.empty_cache()
    gs.ops.set_compute_dtype("bf16")


if __name__ == "__main__":
    main()
