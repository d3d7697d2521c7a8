#!/usr/bin/env python
"""temporal_walk_bench.py -- what temporal walks cost next to the plain unsupervised path, on the synthetic Reddit-shape
temporal CSR of tools/temporal_bench.py (232 965 nodes, degrees uniform in 1..841, int64 edge times uniform in
[0, 2^40)); B = 512 seeds, Q = 20 negatives.

One JSON line per measurement, appended to --out (default profiles/temporal_walk_bench.jsonl), all in one process, the
paths of a measurement alternating; 2 warm-up rounds, the median and range of 7:
  builder   us / launch of gsage_unsup_batch_temporal under both rules next to gsage_unsup_batch on the same CSR, at
            walk_len 5 and 16, query times at the median edge time and at INT64_MAX: the three launches sit in ONE
            recorded command list, each timed in place by events attached to its dispatch, each on seeds of its own,
            other ones every replay (cold rows); an untimed launch opens the list.
  step      ms / step of GSUnsupervised.train_step on the module path with temporal_walks=True over the temporal sampler
            (uniform / seed, query times at the median) and with the plain walks over the uniform Philox sampler; fan-out
            25/10, dims 128/128, 602 bf16 features, walk_len 5.  The median of 7 rounds of --steps steps.
  engine    ms / step of FusedUnsupTemporalMeanTrainStep and of FusedUnsupMeanTrainStep on the same structure.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from temporal_bench import ROUNDS, WARM, stats, stats_us, temporal_csr, timed      # noqa: E402

gs = importlib.import_module("pytorch-graphsage_amd")
nat, ops = gs._native, gs.ops
INT64_MAX = ops.INT64_MAX
B, Q = 512, 20


def builders(csr, cdf, walk_len, t_query, batches):
    """us of the temporal builder under both rules and of the plain builder at one walk_len and one query time"""
    dev = csr.device
    lib, st = nat.lib(), ops._stream()
    names = ["temporal_seed", "temporal_edge", "plain"]
    seeds = [torch.zeros(B, dtype=torch.int64, device=dev) for _ in names]
    times = torch.full((B,), t_query, dtype=torch.int64, device=dev)
    ids, out_t = torch.zeros(2 * B + Q, dtype=torch.int64, device=dev), torch.zeros(2 * B + Q, dtype=torch.int64, device=dev)
    pw = torch.zeros(B, device=dev)
    tick = torch.zeros(1, dtype=torch.int64, device=dev)
    with nat.CommandList.record() as cl:
        # (an untimed launch in front: the first timed kernel is then not the one that starts the replay)
        nat.check(lib.gsage_counter_add(tick.data_ptr(), 1, None), "counter_add")
        for k, rule in enumerate((0, 1)):
            nat.check(lib.gsage_cmdlist_time_next(2 * k, 2 * k + 1), "time_next")
            nat.check(lib.gsage_unsup_batch_temporal(
                csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.etime.data_ptr(), csr.n_rows, seeds[k].data_ptr(),
                times.data_ptr(), B, walk_len, Q, cdf.data_ptr(), cdf._gsage_total, 1, tick.data_ptr(), 0, 0, rule, None,
                ids.data_ptr(), out_t.data_ptr(), pw.data_ptr(), csr.err_flag.data_ptr(), None), "unsup_batch_temporal")
        nat.check(lib.gsage_cmdlist_time_next(4, 5), "time_next")
        nat.check(lib.gsage_unsup_batch(csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.n_rows, seeds[2].data_ptr(), B,
                                        walk_len, Q, cdf.data_ptr(), cdf._gsage_total, 1, tick.data_ptr(), 0, 0,
                                        ids.data_ptr(), pw.data_ptr(), csr.err_flag.data_ptr(), None), "unsup_batch")
    got = {k: [] for k in names}
    nb = int(batches.shape[0])
    for r in range(WARM + ROUNDS):
        for k in range(3):
            seeds[k].copy_(batches[(3 * r + k) % nb])
        cl.replay(st)
        torch.cuda.synchronize()
        if r >= WARM:
            for k, name in enumerate(names):
                got[name].append(cl.elapsed_ms(2 * k, 2 * k + 1))
    return {k: stats_us(v) for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--deg-hi", type=int, default=841)
    ap.add_argument("--feats", type=int, default=602)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "temporal_walk_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "temporal_walk_bench needs a GPU"
    dev = torch.device("cuda")
    ops.set_compute_dtype("bf16")
    ops.warmup(dev)
    n = args.nodes
    csr = temporal_csr(n, args.deg_hi, dev)
    cdf = ops.neg_cdf(csr)
    t_med = int(csr.etime[::97].median())
    info = nat.device_info()
    base = {"arch": info["arch"] if info else None, "nodes": n, "edges": csr.nnz, "max_degree": args.deg_hi,
            "median_edge_time": t_med, "B": B, "Q": Q, "warm": WARM, "rounds": ROUNDS, "stamp": time.strftime("%Y-%m-%d")}
    rng = np.random.RandomState(0)
    rows = []
    batches = torch.from_numpy(rng.randint(1, n, size=(3 * (WARM + ROUNDS), B))).to(dev)
    for walk_len in (5, 16):
        for label, t in (("median", t_med), ("int64_max", INT64_MAX)):
            rows.append(dict(base, what="builder", unit="us/launch", walk_len=walk_len, query_time=label,
                             **builders(csr, cdf, walk_len, t, batches)))

    # ---- the module-path step and the engine step, temporal walks next to the plain ones
    fans = (25, 10)
    store = gs.FeatureStore.synthetic(n, args.feats, dev, dtype="bf16", seed=2)
    ph_adj = sparse.csr_matrix((np.array([1, 1]), np.array([0, 0]), np.array([0, 0, 1, 2])), shape=(3, 1))
    specs = [{"n_train_samples": f, "n_val_samples": f, "output_dim": 128,
              "activation": (lambda x: x) if i == 1 else F.relu} for i, f in enumerate(fans)]
    samplers = {"temporal": (gs.find_sampler("sparse_temporal_neighbor_sampler"),
                             gs.TemporalAdj(ph_adj, np.zeros(2, dtype=np.int64))),
                "plain": (lambda adj: gs.nn_modules.SparseUniformNeighborSampler(adj, rng="philox"), ph_adj)}

    def make(name):
        cls, adj = samplers[name]
        torch.manual_seed(0)
        m = gs.GSUnsupervised(sampler_class=cls, adj=adj, train_adj=adj, prep_class=gs.prep_lookup["identity"],
                              aggregator_class=gs.aggregator_lookup["mean"], input_dim=args.feats, n_nodes=n,
                              layer_specs=specs, walk_len=5, n_negatives=Q, temporal_walks=name == "temporal").to(dev)
        m.train_sampler.use_device_csr(csr)
        m.val_sampler.use_device_csr(csr)
        return m
    nb = 16
    ids = torch.from_numpy(rng.randint(1, n, size=(nb, B))).to(dev)
    tq = torch.full((B,), t_med, dtype=torch.int64, device=dev)
    count = [0]

    def run(fns, what, **extra):
        took = {name: [] for name in fns}
        for r in range(WARM + ROUNDS):
            for name, fn in fns.items():
                t = timed(fn, args.steps)
                if r >= WARM:
                    took[name].append(t)
        rows.append(dict(base, what=what, unit="ms/step", fan=list(fans), dims=[128, 128], feats=args.feats, walk_len=5,
                         steps=args.steps, **dict(extra, **{name: stats(v) for name, v in took.items()})))

    def batch():
        count[0] += 1
        return ids[count[0] % nb]
    models = {name: make(name) for name in samplers}
    run({"module_path_temporal": lambda: models["temporal"].train_step(batch(), store, times=tq),
         "module_path_plain": lambda: models["plain"].train_step(batch(), store)}, "step")
    del models
    m_t, m_p = make("temporal"), make("plain")
    e_t = gs.engine.FusedUnsupTemporalMeanTrainStep(m_t, store, ids[0], example_times=tq)
    e_p = gs.engine.FusedUnsupMeanTrainStep(m_p, store, ids[0])
    run({"engine_temporal": lambda: e_t(batch(), tq), "engine_plain": lambda: e_p(batch())}, "engine",
        engines=[type(e_t).__name__, type(e_p).__name__])
    csr.check()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
