#!/usr/bin/env python
"""The FP8 feature table next to the bf16 table of its decoded values on the MI355X: one JSON line per shape and format.

Both formats run in the same process on the same graph, seeds and Philox stream (FusedMeanTrainStep, queue mode), the
FP8 store first quantised from a synthetic bf16 table, the bf16 store decoded from it -- so the two engines compute
the same numbers and differ only in the bytes their gathers read.

  shape         "headline": B = 512, fan-out 25/10, D = 602, 232 965 nodes (BASELINE configs[1]'s shape)
                "papers":   B = 512, fan-out 15/10/5, D = 128, --papers-nodes nodes (configs[4]'s shape; its real
                            111 059 956 nodes make a 28 GB bf16 table)
  ms_per_step   the repeats: each the mean of --steps queued steps between two host syncs, after --warmup steps
  median_ms, range_ms, seed_nodes_per_s (from the median)
  launches_us   mean duration of the launches the engine times in place (engine.TIMED: `gather` = the gather launch,
                `seed_level` = the seed-level launch, which for bf16 also gathers the rows `seed_level_rows` counts)
  gather_rows / gather_bytes / gather_GBps   table rows the gather launch reads per step, their bytes (whole padded
                rows) and the rate over its duration

Every shape runs in a child process of its own under a timeout; a shape that fails or times out ends the run.

    python tools/fp8_bench.py [--shapes headline,papers] [--reps 5] [--steps 40] [--warmup 10] [--out FILE]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"headline": ((25, 10), 602, 232965), "papers": ((15, 10, 5), 128, None)}
B, HIDDEN, N_CLASSES = 512, 128, 41


def child(args):
    import numpy as np
    import torch
    from scipy import sparse
    from torch.nn import functional as F
    gs = importlib.import_module("pytorch-graphsage_amd")
    dev = torch.device("cuda", 0)
    gs.ops.warmup(dev)
    gs.ops.set_compute_dtype("bf16")
    fan, D, n_nodes = SHAPES[args.child]
    n_rows = (n_nodes or args.papers_nodes) + 1
    csr = gs.DeviceCSR.synthetic(n_rows, 14, 44, dev, max_deg=4096, seed=1, empty_every=1000)
    src = gs.FeatureStore.synthetic(n_rows, D, dev, dtype="bf16", seed=2)
    fp8 = src.quantize()
    del src
    torch.cuda.empty_cache()
    stores = {"fp8": fp8, "bf16": fp8.decoded("bf16")}
    total = args.warmup + args.reps * args.steps + 64
    rng = np.random.default_rng(0)
    ids = torch.from_numpy(rng.integers(1, n_rows, size=(total, B))).to(dev)
    tg = torch.from_numpy(rng.integers(0, N_CLASSES, size=(total, B, 1))).to(dev)
    placeholder = sparse.csr_matrix((np.array([1]), (np.array([1]), np.array([0]))), shape=(2, 1))
    rows_per_seed = sum(int(np.prod(fan[:k])) for k in range(len(fan) + 1))
    for fmt in args.formats.split(","):
        store = stores[fmt]
        gs.nn_modules.SparseUniformNeighborSampler.rng_default = "philox"
        specs = [{"n_train_samples": f, "n_val_samples": f, "output_dim": HIDDEN,
                  "activation": (lambda x: x) if i == len(fan) - 1 else F.relu} for i, f in enumerate(fan)]
        torch.manual_seed(0)
        model = gs.GSSupervised(sampler_class=gs.sampler_lookup["sparse_uniform_neighbor_sampler"], adj=placeholder,
                                train_adj=placeholder, prep_class=gs.prep_lookup["identity"],
                                aggregator_class=gs.aggregator_lookup["mean"], input_dim=D, n_nodes=n_rows,
                                n_classes=N_CLASSES, layer_specs=specs, lr_init=0.01).to(dev)
        gs.nn_modules.SparseUniformNeighborSampler.rng_default = "compat"
        model.train_sampler.seed = 123
        model.train_sampler.use_device_csr(csr)
        eng = gs.engine.FusedMeanTrainStep(model, store, gs.ProblemLosses.classification, ids[0], tg[0])
        eng.load_epoch(ids, tg)
        for _ in range(args.warmup):
            eng.step_queue()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            for _ in range(args.steps):
                eng.step_queue()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / args.steps)
        csr.check()
        # the launches the engine can time in place, over 32 further steps
        eng.instrument(True)
        torch.cuda.synchronize()
        acc = {}
        for k in range(36):
            eng.step_queue()
            if k >= 4:
                for name, v in eng.last_launch_ms().items():
                    acc.setdefault(name, []).append(v * 1e3)
        eng.instrument(False)
        torch.cuda.synchronize()
        launches = {k: float(np.mean(v)) for k, v in acc.items()}
        g_rows, t_rows = eng.gather_launch_rows()
        row_bytes = store.ld * store.data.element_size()
        med = float(np.median(ms))
        rec = {"shape": args.child, "format": fmt, "B": B, "fanout": list(fan), "D": D, "n_nodes": n_rows - 1,
               "table_MB": store.nbytes() / 1e6, "row_bytes": row_bytes, "rows_per_seed": rows_per_seed,
               "steps_per_repeat": args.steps, "ms_per_step": [round(v, 5) for v in ms], "median_ms": med,
               "range_ms": [min(ms), max(ms)], "seed_nodes_per_s": B / (med * 1e-3),
               "launches_us": launches, "gather_rows": int(g_rows), "seed_level_rows": int(t_rows),
               "gather_bytes": int(g_rows) * row_bytes}
        if launches.get("gather"):
            rec["gather_GBps"] = rec["gather_bytes"] / (launches["gather"] * 1e-6) / 1e9
        if t_rows and launches.get("seed_level"):
            rec["seed_level_gather_GBps"] = int(t_rows) * row_bytes / (launches["seed_level"] * 1e-6) / 1e9
        print(json.dumps(rec))
        sys.stdout.flush()
        eng.close()
        del eng, model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,papers")
    ap.add_argument("--formats", default="fp8,bf16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--papers-nodes", type=int, default=111_059_956)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per shape (a child process of its own)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8_bench.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert args.reps >= 5, "medians of at least five repeats"
    if args.child:
        return child(args)
    for shape in args.shapes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--formats", args.formats, "--reps",
               str(args.reps), "--steps", str(args.steps), "--warmup", str(args.warmup), "--papers-nodes",
               str(args.papers_nodes)]
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit("fp8_bench: shape %s ran into its %d s limit; nothing further is started" % (shape, args.timeout))
        lines = [l for l in res.stdout.decode().splitlines() if l.startswith("{")]
        with open(args.out, "a") as f:
            for l in lines:
                print(l)
                f.write(l + "\n")
        if res.returncode != 0:
            raise SystemExit("fp8_bench: shape %s ended with status %d; nothing further is started" % (shape, res.returncode))


if __name__ == "__main__":
    main()
