#!/usr/bin/env python
"""unsup_weighted_bench.py -- what weighted walks cost an unsupervised step, at the Reddit shape of
tools/weighted_engine_bench.py (232 965 nodes, degrees uniform in 1..841: ~98 M edges, 602 features, fan-out 25/10, dims
128/128, bf16; weights drawn on the device: exp of a normal, 5 % zeros), B = 512 seeds, walk_len = 5, Q = 20 -- and on the
same graph's importance adjacency (50 walks of 2 steps, top 16: every row at most 16 edges, the one-round-trip path).

One JSON line per measurement and graph, appended to --out (default profiles/unsup_weighted_bench.jsonl), one process:
  builder_launch  us / launch, each launch timed in place by events attached to its dispatch in ONE recorded command
                  list: gsage_unsup_batch_weighted (a wave per walk) and gsage_unsup_batch (a lane per walk, uniform
                  steps: the yardstick) on the same CSR, at walk_len 5 and 16.  Each launch starts from a batch of
                  seeds of its own, another one every replay, so no launch walks rows that the one before it has just
                  brought into the caches.
  step            ms / step of three paths, alternating: (a) GSUnsupervised(weighted_walks=True).train_step on the module
                  path, (b) FusedUnsupWeightedMeanTrainStep, (c) for context FusedUnsupMeanTrainStep (uniform walks and
                  uniform Philox draws) on the same structure.  --warm-rounds rounds are thrown away, then the median
                  and the range of --rounds rounds of --steps steps (device events around the steps).
  in_step         us of the launches (b) and (c) time in place (engine.instrument()): builder, sampler, gather, K5, K5b,
                  head.
Needs a GPU: there is no CPU fallback."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch
from scipy import sparse
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gs = importlib.import_module("pytorch-graphsage_amd")
nat, ops = gs._native, gs.ops


def timed(fn, steps):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "rounds": list(v)}


def builder_launches(csr, cdf_w, cdf_u, batches, Q, reps):
    """us of each builder launch, timed in place inside ONE recorded list replayed `reps` times"""
    B, dev = int(batches.shape[1]), batches.device
    lib, st = nat.lib(), ops._stream()
    slots = {"weighted_len5": (0, 1, True, 5), "uniform_len5": (2, 3, False, 5), "weighted_len16": (4, 5, True, 16),
             "uniform_len16": (6, 7, False, 16)}
    nb = int(batches.shape[0])
    src = [batches[j % nb].clone() for j in range(len(slots))]
    seeds = [torch.zeros(B, dtype=torch.int64, device=dev) for _ in slots]
    ids = torch.zeros(2 * B + Q, dtype=torch.int64, device=dev)
    pw = torch.zeros(B, dtype=torch.float32, device=dev)
    with nat.CommandList.record() as cl:
        for j, (a, b, weighted, wl) in enumerate(slots.values()):
            nat.check(lib.gsage_copy_pair(seeds[j].data_ptr(), src[j].data_ptr(), B * 8, None, None, 0, st), "copy_pair")
            nat.check(lib.gsage_cmdlist_time_next(a, b), "time_next")
            if weighted:
                nat.check(lib.gsage_unsup_batch_weighted(
                    csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.edge_cdf.data_ptr(), csr.n_rows, seeds[j].data_ptr(), B,
                    wl, Q, cdf_w.data_ptr(), cdf_w._gsage_total, 1, None, j, 0, ids.data_ptr(), pw.data_ptr(),
                    csr.err_flag.data_ptr(), st), "unsup_batch_weighted")
            else:
                nat.check(lib.gsage_unsup_batch(
                    csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.n_rows, seeds[j].data_ptr(), B, wl, Q,
                    cdf_u.data_ptr(), cdf_u._gsage_total, 1, None, j, 0, ids.data_ptr(), pw.data_ptr(),
                    csr.err_flag.data_ptr(), st), "unsup_batch")
    got = {k: [] for k in slots}
    for r in range(reps + 5):
        for j in range(len(slots)):
            src[j].copy_(batches[(len(slots) * r + j) % nb])
        cl.replay(st)
        torch.cuda.synchronize()
        if r >= 5:
            for k, (a, b, _, _) in slots.items():
                got[k].append(cl.elapsed_ms(a, b))
    return {k: {"median_us": 1e3 * float(np.median(v)), "min_us": 1e3 * float(min(v)), "max_us": 1e3 * float(max(v))}
            for k, v in got.items()}


def measure(args, base, graph, csr, store, rows):
    dev, n, B, Q = csr.device, csr.n_rows, args.batch, args.negatives
    fans = (25, 10)
    specs = [{"n_train_samples": f, "n_val_samples": f, "output_dim": 128,
              "activation": (lambda x: x) if i == 1 else F.relu} for i, f in enumerate(fans)]
    ph_adj = sparse.csr_matrix((np.array([1, 1]), np.array([0, 0]), np.array([0, 0, 1, 2])), shape=(3, 1))
    w_adj = gs.WeightedAdj(ph_adj, np.ones(2, dtype=np.float32))
    weighted = gs.find_sampler("sparse_weighted_neighbor_sampler")
    uniform = lambda adj: gs.nn_modules.SparseUniformNeighborSampler(adj, rng="philox")      # noqa: E731

    def model(sampler, adj, weighted_walks):
        torch.manual_seed(0)
        m = gs.GSUnsupervised(sampler_class=sampler, adj=adj, train_adj=adj, prep_class=gs.prep_lookup["identity"],
                              aggregator_class=gs.aggregator_lookup["mean"], input_dim=args.feats, n_nodes=n,
                              layer_specs=specs, walk_len=args.walk_len, n_negatives=Q,
                              weighted_walks=weighted_walks).to(dev)
        m.train_sampler.use_device_csr(csr)
        m.val_sampler.use_device_csr(csr)
        return m

    rng = np.random.RandomState(0)
    nb = args.batches
    ids = torch.from_numpy(rng.randint(1, n, size=(nb, B))).to(dev)
    base = dict(base, graph=graph, edges=csr.nnz, max_degree=int(csr.max_deg))

    rows.append(dict(base, what="builder_launch", unit="us/launch", reps=64,
                     note="each launch alone on an idle GPU, a batch of seeds of its own per launch and replay, timed "
                          "by events attached to its dispatch",
                     **builder_launches(csr, ops.neg_cdf(csr, weighted=True), ops.neg_cdf(csr), ids, Q, 64)))

    m_a = model(weighted, w_adj, True)
    e_b = gs.engine.FusedUnsupWeightedMeanTrainStep(model(weighted, w_adj, True), store, ids[0])
    e_c = gs.engine.FusedUnsupMeanTrainStep(model(uniform, ph_adj, False), store, ids[0])
    count = [0]

    def per_call(fn):
        def go():
            k = count[0] % nb
            count[0] += 1
            fn(ids[k])
        return go

    paths = [("a_module_path_weighted_walks", per_call(lambda i: m_a.train_step(i, store))),
             ("b_engine_weighted_walks", per_call(e_b)),
             ("c_engine_uniform", per_call(e_c))]
    times = {name: [] for name, _ in paths}
    for r in range(args.warm_rounds + args.rounds):
        for name, fn in paths:
            t = timed(fn, args.steps)
            if r >= args.warm_rounds:
                times[name].append(t)
    rows.append(dict(base, what="step", unit="ms/step", steps=args.steps, warm_rounds=args.warm_rounds,
                     rounds=args.rounds, batches=nb, **{name: stats(v) for name, v in times.items()}))

    for name, eng in (("b_engine_weighted_walks", e_b), ("c_engine_uniform", e_c)):
        eng.instrument(True)
        marks = {}
        for k in range(40):
            eng(ids[k % nb])
            torch.cuda.synchronize()
            for key, v in eng.last_launch_ms().items():
                marks.setdefault(key, []).append(v)
        rows.append(dict(base, what="in_step", unit="us/launch", steps=40, engine=name,
                         **{k: {"median_us": 1e3 * float(np.median(v[8:])), "min_us": 1e3 * float(min(v[8:])),
                                "max_us": 1e3 * float(max(v[8:]))} for k, v in marks.items()}))
        eng.close()
    csr.check()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--deg-hi", type=int, default=841)
    ap.add_argument("--feats", type=int, default=602)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--negatives", type=int, default=20)
    ap.add_argument("--walk-len", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warm-rounds", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "unsup_weighted_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "unsup_weighted_bench needs a GPU"
    dev = torch.device("cuda")
    ops.set_compute_dtype("bf16")
    ops.warmup(dev)
    n = args.nodes

    csr = gs.DeviceCSR.synthetic(n, 1, args.deg_hi, dev, seed=1)
    gen = torch.Generator(device=dev).manual_seed(3)
    w = torch.exp(torch.randn(csr.nnz, device=dev, generator=gen) * 2.3)
    w[torch.rand(csr.nnz, device=dev, generator=gen) < 0.05] = 0.0
    csr.with_weights(w)
    del w
    store = gs.FeatureStore.synthetic(n, args.feats, dev, dtype="bf16", seed=2)
    info = nat.device_info()
    base = {"arch": info["arch"] if info else None, "nodes": n, "B": args.batch, "Q": args.negatives,
            "walk_len": args.walk_len, "fan": [25, 10], "dims": [128, 128], "feats": args.feats, "precision": "bf16",
            "stamp": time.strftime("%Y-%m-%d")}
    rows = []
    measure(args, base, "reddit_shape_weighted", csr, store, rows)
    t0 = time.time()
    imp = csr.importance(n_walks=50, walk_len=2, top=16, seed=0)
    torch.cuda.synchronize()
    base["importance_build_s"] = time.time() - t0
    measure(args, base, "importance_50_2_16", imp, store, rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
