#!/usr/bin/env python
"""distinct_bench.py -- what the distinct-draw sampler costs and what it removes, at the Reddit shape of
tools/weighted_engine_bench.py (232 965 nodes, degrees uniform in 1..841: ~98 M edges, 602 features, fan-out 25/10, dims
128/128, B = 512, bf16, 41 classes).

One JSON line per measurement, appended to --out (default profiles/distinct_bench.jsonl), all in one process:
  step            ms / step of the paths over the same structure, alternating: (a) GSSupervised.train_step on the module
                  path under the distinct sampler, (b) FusedDistinctMeanTrainStep per call, (c) the same engine in queue
                  mode, (d) FusedMeanTrainStep (uniform Philox draws) per call and (e) in queue mode.  --warm-rounds
                  rounds are thrown away, then the median and the range of --rounds rounds of --steps steps (device
                  events around the steps, closed by a synchronisation).
  sampler_launch  us / launch on frontiers of that shape, each launch timed in place by events attached to its dispatch
                  in a recorded command list: gsage_sample_hops_distinct, the two gsage_sample_csr_distinct launches it
                  replaces, gsage_sample_hops (uniform) on the same CSR.  Each of the three starts from a batch of seeds
                  of its own, another one every replay: no launch walks rows that the launch before it, or the replay
                  before, has just brought into the caches.
  in_step         us of the queue step's launches of (c), timed in place (engine.instrument()): the sampler launch next
                  to the gather, seed-level, K5 and K5b launches.
  sampling_error  reported, nothing asserted: the mean absolute difference between sampled-evaluation logits and
                  gs.full_neighbour logits on the same nodes, for the uniform and for the distinct sampler, same
                  weights, fp32, on a smaller synthetic graph (--err-nodes nodes, degrees uniform in 1..--err-deg-hi,
                  fan-out 25/10) whose rows are partly shorter and partly longer than the fan-outs -- the variance the
                  sampler is meant to remove.
Needs a GPU: there is no CPU fallback."""
import argparse
import ctypes
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


def stats(v, scale=1.0):
    v = [scale * x for x in v]
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "rounds": v}


def sampler_launches(csr, batches, fans, reps):
    """us of each sampler launch, timed in place inside ONE recorded list replayed `reps` times; the all-hops launch,
    the per-hop pair and the uniform one each start from a batch of seeds of their own (copied into hop 0 by a launch
    of the list), and every replay moves all three on to other batches"""
    B, dev = int(batches.shape[1]), batches.device
    sizes = [B, B * fans[0], B * fans[0] * fans[1]]
    ids = torch.zeros(sum(sizes), dtype=torch.int64, device=dev)
    ids[:B] = batches[0]
    hop1, hop2 = ids[B:B + sizes[1]], ids[B + sizes[1]:]
    d = nat.HopsDesc()
    d.rowptr, d.col, d.n_rows = csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.n_rows
    d.ids, d.B, d.n_hops = ids.data_ptr(), B, 2
    for k in range(5):
        d.fan[k] = fans[k] if k < 2 else 1
    d.max_deg, d.seed, d.err_flag = csr.max_deg, 1, csr.err_flag.data_ptr()
    lib, st = nat.lib(), ops._stream()
    ph = {"seed": 1}
    slots = {"hops_distinct": (0, 1), "per_hop_distinct_1": (2, 3), "per_hop_distinct_2": (4, 5), "hops_uniform": (6, 7)}
    nb = int(batches.shape[0])
    src = [batches[j % nb].clone() for j in range(3)]

    def seeds_of(j):
        nat.check(lib.gsage_copy_pair(ids.data_ptr(), src[j].data_ptr(), B * 8, None, None, 0, st), "copy_pair")

    with nat.CommandList.record() as cl:
        seeds_of(0)
        nat.check(lib.gsage_cmdlist_time_next(0, 1), "time_next")
        nat.check(lib.gsage_sample_hops_distinct(ctypes.addressof(d), st), "hops_distinct")
        seeds_of(1)
        nat.check(lib.gsage_cmdlist_time_next(2, 3), "time_next")
        ops.sample_csr_distinct(csr, ids[:B], fans[0], dict(ph, call_base=0), out=hop1)
        nat.check(lib.gsage_cmdlist_time_next(4, 5), "time_next")
        ops.sample_csr_distinct(csr, hop1, fans[1], dict(ph, call_base=1), out=hop2)
        seeds_of(2)
        nat.check(lib.gsage_cmdlist_time_next(6, 7), "time_next")
        nat.check(lib.gsage_sample_hops(ctypes.addressof(d), st), "sample_hops")
    got = {k: [] for k in slots}
    for r in range(reps + 5):
        for j in range(3):
            src[j].copy_(batches[(3 * r + j) % nb])
        cl.replay(st)
        torch.cuda.synchronize()
        if r >= 5:
            for k, (a, b) in slots.items():
                got[k].append(cl.elapsed_ms(a, b))
    out = {k: {"median_us": 1e3 * float(np.median(v)), "min_us": 1e3 * float(min(v)), "max_us": 1e3 * float(max(v))}
           for k, v in got.items()}
    out["per_hop_distinct_sum"] = {"median_us": out["per_hop_distinct_1"]["median_us"] + out["per_hop_distinct_2"]["median_us"]}
    return out


def sampling_error(args, dev, fans):
    """mean |sampled-evaluation logits - full-neighbourhood logits| under either sampler, same weights, fp32"""
    ops.set_compute_dtype("fp32")
    try:
        n = args.err_nodes
        csr = gs.DeviceCSR.synthetic(n, 1, args.err_deg_hi, dev, seed=5)
        store = gs.FeatureStore.synthetic(n, 64, dev, dtype="fp32", seed=6)
        ph_adj = sparse.csr_matrix((np.array([1, 1]), np.array([0, 0]), np.array([0, 0, 1, 2])), shape=(3, 1))
        specs = [{"n_train_samples": f, "n_val_samples": f, "output_dim": 128,
                  "activation": (lambda x: x) if i == 1 else F.relu} for i, f in enumerate(fans)]
        models = {}
        for name, cls in (("uniform", lambda adj: gs.nn_modules.SparseUniformNeighborSampler(adj, rng="philox")),
                          ("distinct", gs.find_sampler("sparse_distinct_neighbor_sampler"))):
            torch.manual_seed(0)
            m = gs.GSSupervised(sampler_class=cls, adj=ph_adj, train_adj=ph_adj, prep_class=gs.prep_lookup["identity"],
                                aggregator_class=gs.aggregator_lookup["mean"], input_dim=64, n_nodes=n, n_classes=41,
                                layer_specs=specs).to(dev)
            m.train_sampler.use_device_csr(csr)
            m.val_sampler.use_device_csr(csr)
            models[name] = m
        models["distinct"].load_state_dict(models["uniform"].state_dict())
        ids = torch.from_numpy(np.random.RandomState(1).randint(1, n, size=512)).to(dev)
        full = gs.full_neighbour(models["uniform"], store, nodes=ids).float()
        out = {}
        for name, m in models.items():
            with torch.no_grad():
                got = m(ids, store, train=False).float()
            out["mean_abs_diff_" + name] = float((got - full).abs().mean())
        out["mean_abs_logit"] = float(full.abs().mean())
        deg = (csr.rowptr[1:] - csr.rowptr[:-1])[ids]
        out["share_of_nodes_with_degree_at_most_25"] = float((deg <= fans[0]).float().mean())
        csr.check()
        return dict(out, nodes=n, max_degree=args.err_deg_hi, eval_nodes=512, feats=64, precision="fp32")
    finally:
        ops.set_compute_dtype("bf16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--deg-hi", type=int, default=841)
    ap.add_argument("--feats", type=int, default=602)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warm-rounds", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--queue-batches", type=int, default=16)
    ap.add_argument("--err-nodes", type=int, default=20000)
    ap.add_argument("--err-deg-hi", type=int, default=50)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "distinct_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "distinct_bench needs a GPU"
    dev = torch.device("cuda")
    ops.set_compute_dtype("bf16")
    ops.warmup(dev)
    n, B, fans = args.nodes, args.batch, (25, 10)

    csr = gs.DeviceCSR.synthetic(n, 1, args.deg_hi, dev, seed=1)
    info = nat.device_info()
    base = {"arch": info["arch"] if info else None, "nodes": n, "edges": csr.nnz, "max_degree": args.deg_hi, "B": B,
            "fan": list(fans), "dims": [128, 128], "feats": args.feats, "classes": 41, "precision": "bf16",
            "hops_spw": int(os.environ.get("GSAGE_HOPS_SPW", "1")), "stamp": time.strftime("%Y-%m-%d")}

    ph_adj = sparse.csr_matrix((np.array([1, 1]), np.array([0, 0]), np.array([0, 0, 1, 2])), shape=(3, 1))
    store = gs.FeatureStore.synthetic(n, args.feats, dev, dtype="bf16", seed=2)
    specs = [{"n_train_samples": f, "n_val_samples": f, "output_dim": 128,
              "activation": (lambda x: x) if i == 1 else F.relu} for i, f in enumerate(fans)]
    distinct = gs.find_sampler("sparse_distinct_neighbor_sampler")
    uniform = lambda adj: gs.nn_modules.SparseUniformNeighborSampler(adj, rng="philox")      # noqa: E731

    def model(sampler):
        torch.manual_seed(0)
        m = gs.GSSupervised(sampler_class=sampler, adj=ph_adj, train_adj=ph_adj, prep_class=gs.prep_lookup["identity"],
                            aggregator_class=gs.aggregator_lookup["mean"], input_dim=args.feats, n_nodes=n, n_classes=41,
                            layer_specs=specs).to(dev)
        m.train_sampler.use_device_csr(csr)
        m.val_sampler.use_device_csr(csr)
        return m

    rng = np.random.RandomState(0)
    nb = args.queue_batches
    ids = torch.from_numpy(rng.randint(1, n, size=(nb, B))).to(dev)
    tgs = torch.from_numpy(rng.randint(0, 41, size=(nb, B, 1))).to(dev)
    loss = gs.ProblemLosses.classification
    DE, ME = gs.engine.FusedDistinctMeanTrainStep, gs.engine.FusedMeanTrainStep

    m_a = model(distinct)
    e_b = DE(model(distinct), store, loss, ids[0], tgs[0])
    e_c = DE(model(distinct), store, loss, ids[0], tgs[0]).load_epoch(ids, tgs)
    e_d = ME(model(uniform), store, loss, ids[0], tgs[0])
    e_e = ME(model(uniform), store, loss, ids[0], tgs[0]).load_epoch(ids, tgs)
    count = [0]

    def per_call(fn):
        def go():
            k = count[0] % nb
            count[0] += 1
            fn(ids[k], tgs[k])
        return go

    paths = [("a_module_path_distinct", per_call(lambda i, t: m_a.train_step(i, store, t, loss))),
             ("b_distinct_engine_per_call", per_call(e_b)),
             ("c_distinct_engine_queue", e_c.step_queue),
             ("d_uniform_engine_per_call", per_call(e_d)),
             ("e_uniform_engine_queue", e_e.step_queue)]
    times = {name: [] for name, _ in paths}
    for r in range(args.warm_rounds + args.rounds):
        for name, fn in paths:
            t = timed(fn, args.steps)
            if r >= args.warm_rounds:
                times[name].append(t)
    rows = [dict(base, what="step", unit="ms/step", steps=args.steps, warm_rounds=args.warm_rounds, rounds=args.rounds,
                 queue_batches=nb, tail_rows=int(e_c._tail_rows), ring=int(e_c.P),
                 **{name: stats(v) for name, v in times.items()})]

    rows.append(dict(base, what="sampler_launch", unit="us/launch", reps=64,
                     note="each launch alone on an idle GPU, a batch of seeds of its own per launch and replay, timed "
                          "by events attached to its dispatch",
                     **sampler_launches(csr, ids, fans, 64)))

    e_c.instrument(True)
    marks = {}
    for _ in range(40):
        e_c.step_queue()
        torch.cuda.synchronize()
        for k, v in e_c.last_launch_ms().items():
            marks.setdefault(k, []).append(v)
    rows.append(dict(base, what="in_step", unit="us/launch", steps=40, engine="c_distinct_engine_queue",
                     **{k: {"median_us": 1e3 * float(np.median(v[8:])), "min_us": 1e3 * float(min(v[8:])),
                            "max_us": 1e3 * float(max(v[8:]))} for k, v in marks.items()}))
    csr.check()
    rows.append(dict({"arch": base["arch"], "stamp": base["stamp"], "fan": list(fans), "dims": [128, 128], "classes": 41},
                     what="sampling_error", unit="logit", note="reported, not asserted",
                     **sampling_error(args, dev, fans)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
