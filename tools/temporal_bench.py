#!/usr/bin/env python
"""temporal_bench.py -- what the temporal sampler's hop kernel costs next to the uniform one, at the Reddit shape of
tools/distinct_bench.py (232 965 nodes, degrees uniform in 1..841: ~98 M edges) with synthetic int64 edge times
(uniform in [0, 2^40); the rows are put in time order on the device during set-up, which is not timed).

One JSON line per measurement, appended to --out (default profiles/temporal_bench.jsonl), all in one process:
  hop_kernel   us / launch of gsage_sample_csr_temporal at M = 12 800, n = 10 and at M = 512, n = 25, query times at
               the median edge time and at INT64_MAX, both strategies and both inheritance rules, next to
               gsage_sample_csr_philox (the uniform hop kernel) on the same CSR: the five launches of one shape and
               query time alternate inside ONE recorded command list, each timed in place by events attached to its
               dispatch, each on a batch of parents of its own, another one every replay (no launch walks rows the
               launch before it has just brought into the caches); an untimed launch opens the list.  2 warm-up
               replays, the median of 7.
  step         ms / step of GSSupervised.train_step on the module path under the temporal sampler (uniform / seed,
               query times at the median) and under the uniform Philox sampler, alternating; B = 512, fan-out 25/10,
               dims 128/128, 602 bf16 features.  2 warm-up rounds, the median of 7 rounds of --steps steps.
  snapshot     ms of DeviceCSR.snapshot(median time): the count launch, one torch.cumsum, the row copy.
Nothing is asserted.  Needs a GPU: there is no CPU fallback."""
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
INT64_MAX = ops.INT64_MAX
WARM, ROUNDS = 2, 7


def temporal_csr(n, deg_hi, dev):
    """the synthetic CSR with edge times, every row in time order: ONE sort of the key (row << 40) | time"""
    csr = gs.DeviceCSR.synthetic(n, 1, deg_hi, dev, seed=1)
    gen = torch.Generator(device=dev).manual_seed(3)
    deg = csr.rowptr[1:] - csr.rowptr[:-1]
    key = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), deg) << 40
    key += torch.randint(0, 1 << 40, (csr.nnz,), dtype=torch.int64, device=dev, generator=gen)
    key = torch.sort(key).values                     # (the neighbour ids are random: they need not move with the times)
    return csr.with_times(key & ((1 << 40) - 1))


def stats_us(v):
    return {"median_us": 1e3 * float(np.median(v)), "min_us": 1e3 * float(min(v)), "max_us": 1e3 * float(max(v))}


def hop_kernels(csr, M, n, t_query, batches):
    """us of the four temporal variants and of the uniform hop kernel at one shape and one query time"""
    dev = csr.device
    lib, st = nat.lib(), ops._stream()
    variants = [(s, i) for s in ("uniform", "recent") for i in ("seed", "edge")]
    ids = [torch.zeros(M, dtype=torch.int64, device=dev) for _ in range(5)]
    times = torch.full((M,), t_query, dtype=torch.int64, device=dev)
    out, out_t = torch.zeros(M * n, dtype=torch.int64, device=dev), torch.zeros(M * n, dtype=torch.int64, device=dev)
    ph = {"seed": 1}
    tick = torch.zeros(1, dtype=torch.int64, device=dev)
    with nat.CommandList.record() as cl:
        # (an untimed launch in front: the first timed kernel is then not the one that starts the replay)
        nat.check(lib.gsage_counter_add(tick.data_ptr(), 1, None), "counter_add")
        for k, (s, i) in enumerate(variants):
            nat.check(lib.gsage_cmdlist_time_next(2 * k, 2 * k + 1), "time_next")
            ops.sample_csr_temporal(csr, ids[k], times, n, ph, strategy=s, inherit=i, out=out, out_time=out_t)
        nat.check(lib.gsage_cmdlist_time_next(8, 9), "time_next")
        ops.sample_csr(csr, ids[4], n, philox=ph, out=out)
    names = ["temporal_%s_%s" % v for v in variants] + ["uniform_philox"]
    got = {k: [] for k in names}
    nb = int(batches.shape[0])
    for r in range(WARM + ROUNDS):
        for k in range(5):
            ids[k].copy_(batches[(5 * r + k) % nb, :M])
        cl.replay(st)
        torch.cuda.synchronize()
        if r >= WARM:
            for k, name in enumerate(names):
                got[name].append(cl.elapsed_ms(2 * k, 2 * k + 1))
    return {k: stats_us(v) for k, v in got.items()}


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
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "rounds": [float(x) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--deg-hi", type=int, default=841)
    ap.add_argument("--feats", type=int, default=602)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "temporal_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "temporal_bench needs a GPU"
    dev = torch.device("cuda")
    ops.set_compute_dtype("bf16")
    ops.warmup(dev)
    n = args.nodes
    csr = temporal_csr(n, args.deg_hi, dev)
    t_med = int(csr.etime[::97].median())
    info = nat.device_info()
    base = {"arch": info["arch"] if info else None, "nodes": n, "edges": csr.nnz, "max_degree": args.deg_hi,
            "median_edge_time": t_med, "stamp": time.strftime("%Y-%m-%d")}
    rng = np.random.RandomState(0)
    rows = []
    for M, fan in ((12800, 10), (512, 25)):
        batches = torch.from_numpy(rng.randint(1, n, size=(5 * (WARM + ROUNDS), M))).to(dev)
        for label, t in (("median", t_med), ("int64_max", INT64_MAX)):
            rows.append(dict(base, what="hop_kernel", unit="us/launch", M=M, n=fan, query_time=label, warm=WARM,
                             rounds=ROUNDS, **hop_kernels(csr, M, fan, t, batches)))

    # ---- the module-path step under both samplers
    B, fans = 512, (25, 10)
    store = gs.FeatureStore.synthetic(n, args.feats, dev, dtype="bf16", seed=2)
    ph_adj = sparse.csr_matrix((np.array([1, 1]), np.array([0, 0]), np.array([0, 0, 1, 2])), shape=(3, 1))
    specs = [{"n_train_samples": f, "n_val_samples": f, "output_dim": 128,
              "activation": (lambda x: x) if i == 1 else F.relu} for i, f in enumerate(fans)]
    samplers = {"temporal": (gs.find_sampler("sparse_temporal_neighbor_sampler"),
                             gs.TemporalAdj(ph_adj, np.zeros(2, dtype=np.int64))),
                "uniform": (lambda adj: gs.nn_modules.SparseUniformNeighborSampler(adj, rng="philox"), ph_adj)}
    models = {}
    for name, (cls, adj) in samplers.items():
        torch.manual_seed(0)
        m = gs.GSSupervised(sampler_class=cls, adj=adj, train_adj=adj, prep_class=gs.prep_lookup["identity"],
                            aggregator_class=gs.aggregator_lookup["mean"], input_dim=args.feats, n_nodes=n, n_classes=41,
                            layer_specs=specs).to(dev)
        m.train_sampler.use_device_csr(csr)
        m.val_sampler.use_device_csr(csr)
        models[name] = m
    nb = 16
    ids = torch.from_numpy(rng.randint(1, n, size=(nb, B))).to(dev)
    tgs = torch.from_numpy(rng.randint(0, 41, size=(nb, B, 1))).to(dev)
    tq = torch.full((B,), t_med, dtype=torch.int64, device=dev)
    loss = gs.ProblemLosses.classification
    count = [0]

    def step(name):
        def go():
            k = count[0] % nb
            count[0] += 1
            if name == "temporal":
                models[name].train_step(ids[k], store, tgs[k], loss, times=tq)
            else:
                models[name].train_step(ids[k], store, tgs[k], loss)
        return go

    took = {name: [] for name in models}
    for r in range(WARM + ROUNDS):
        for name in models:
            t = timed(step(name), args.steps)
            if r >= WARM:
                took[name].append(t)
    rows.append(dict(base, what="step", unit="ms/step", B=B, fan=list(fans), dims=[128, 128], feats=args.feats,
                     steps=args.steps, warm=WARM, rounds=ROUNDS,
                     **{"module_path_" + name: stats(v) for name, v in took.items()}))

    # ---- the snapshot build
    snaps = []
    for r in range(WARM + ROUNDS):
        t = timed(lambda: csr.snapshot(t_med), 1)
        if r >= WARM:
            snaps.append(t)
    snap = csr.snapshot(t_med)
    rows.append(dict(base, what="snapshot", unit="ms", edges_kept=snap.nnz, warm=WARM, n_rounds=ROUNDS, **stats(snaps)))
    csr.check()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
