#!/usr/bin/env python
"""weighted_engine_bench.py -- what the fused engine over weighted adjacencies buys, at the Reddit shape of
tools/weighted_bench.py (232 965 nodes, degrees uniform in 1..841: ~98 M edges, 602 features, fan-out 25/10, dims
128/128, B = 512, bf16, 41 classes; weights drawn on the device: exp of a normal, 5 % zeros).

One JSON line per measurement, appended to --out (default profiles/weighted_engine_bench.jsonl), all in one process:
  step            ms / step of the paths over the same structure, alternating: (a) GSSupervised.train_step on the weighted
                  module path, (b) FusedWeightedMeanTrainStep per call, (c) the same engine in queue mode -- once per
                  search form of the sampler (GSAGE_WEIGHTED_SEARCH=kary / binary while its lists are recorded) --,
                  (d) for context FusedMeanTrainStep (uniform Philox draws) in queue mode.  --warm-rounds rounds are
                  thrown away, then the median and the range of --rounds rounds of --steps steps (device events around
                  the steps, closed by a synchronisation).
  sampler_launch  us / launch on frontiers of that shape, each launch timed in place by events attached to its dispatch
                  in a recorded command list: gsage_sample_hops_weighted with the 8-ary and with the binary search, the
                  two gsage_sample_csr_weighted launches it replaces, gsage_sample_hops (uniform) on the same structure.
                  Each of the four starts from a batch of seeds of its own, another one every replay (16 batches touch
                  ~700 MB of the cdf table): no launch walks rows that the launch before it, or the replay before,
                  has just brought into the caches.
  in_step         us of the queue step's launches of (c), per search form, timed in place (engine.instrument()): the
                  sampler launch next to the gather, seed-level, K5 and K5b launches.
Needs a GPU: there is no CPU fallback."""
import argparse
import contextlib
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


@contextlib.contextmanager
def search(form):
    """GSAGE_WEIGHTED_SEARCH=form while launches are issued or recorded (read per call; a list keeps its form)"""
    saved = os.environ.get("GSAGE_WEIGHTED_SEARCH")
    os.environ["GSAGE_WEIGHTED_SEARCH"] = form
    try:
        yield
    finally:
        if saved is None:
            del os.environ["GSAGE_WEIGHTED_SEARCH"]
        else:
            os.environ["GSAGE_WEIGHTED_SEARCH"] = saved


def sampler_launches(csr, batches, fans, reps):
    """us of each sampler launch, timed in place inside ONE recorded list replayed `reps` times; the 8-ary launch,
    the binary one, the per-hop pair and the uniform one each start from a batch of seeds of their own (copied into
    hop 0 by a launch of the list), and every replay moves all four on to other batches"""
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
    slots = {"hops_weighted_8ary": (0, 1), "hops_weighted_binary": (2, 3), "per_hop_weighted_1": (4, 5),
             "per_hop_weighted_2": (6, 7), "hops_uniform": (8, 9)}
    nb = int(batches.shape[0])
    src = [batches[j % nb].clone() for j in range(4)]

    def seeds_of(j):
        nat.check(lib.gsage_copy_pair(ids.data_ptr(), src[j].data_ptr(), B * 8, None, None, 0, st), "copy_pair")

    with nat.CommandList.record() as cl:
        for j, (form, (a, b)) in enumerate((("kary", slots["hops_weighted_8ary"]),
                                            ("binary", slots["hops_weighted_binary"]))):
            seeds_of(j)
            with search(form):
                nat.check(lib.gsage_cmdlist_time_next(a, b), "time_next")
                nat.check(lib.gsage_sample_hops_weighted(ctypes.addressof(d), csr.edge_cdf.data_ptr(), st), "hops_weighted")
        seeds_of(2)
        nat.check(lib.gsage_cmdlist_time_next(4, 5), "time_next")
        ops.sample_csr_weighted(csr, ids[:B], fans[0], dict(ph, call_base=0), out=hop1)
        nat.check(lib.gsage_cmdlist_time_next(6, 7), "time_next")
        ops.sample_csr_weighted(csr, hop1, fans[1], dict(ph, call_base=1), out=hop2)
        seeds_of(3)
        nat.check(lib.gsage_cmdlist_time_next(8, 9), "time_next")
        nat.check(lib.gsage_sample_hops(ctypes.addressof(d), st), "sample_hops")
    got = {k: [] for k in slots}
    for r in range(reps + 5):
        for j in range(4):
            src[j].copy_(batches[(4 * r + j) % nb])
        cl.replay(st)
        torch.cuda.synchronize()
        if r >= 5:
            for k, (a, b) in slots.items():
                got[k].append(cl.elapsed_ms(a, b))
    out = {k: {"median_us": 1e3 * float(np.median(v)), "min_us": 1e3 * float(min(v)), "max_us": 1e3 * float(max(v))}
           for k, v in got.items()}
    out["per_hop_weighted_sum"] = {"median_us": out["per_hop_weighted_1"]["median_us"] + out["per_hop_weighted_2"]["median_us"]}
    return out


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
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "weighted_engine_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "weighted_engine_bench needs a GPU"
    dev = torch.device("cuda")
    ops.set_compute_dtype("bf16")
    ops.warmup(dev)
    n, B, fans = args.nodes, args.batch, (25, 10)

    csr = gs.DeviceCSR.synthetic(n, 1, args.deg_hi, dev, seed=1)
    gen = torch.Generator(device=dev).manual_seed(3)
    w = torch.exp(torch.randn(csr.nnz, device=dev, generator=gen) * 2.3)
    w[torch.rand(csr.nnz, device=dev, generator=gen) < 0.05] = 0.0
    csr.with_weights(w)
    del w
    info = nat.device_info()
    base = {"arch": info["arch"] if info else None, "nodes": n, "edges": csr.nnz, "max_degree": args.deg_hi, "B": B,
            "fan": list(fans), "dims": [128, 128], "feats": args.feats, "classes": 41, "precision": "bf16",
            "hops_spw": int(os.environ.get("GSAGE_HOPS_SPW", "1")), "stamp": time.strftime("%Y-%m-%d")}

    ph_adj = sparse.csr_matrix((np.array([1, 1]), np.array([0, 0]), np.array([0, 0, 1, 2])), shape=(3, 1))
    store = gs.FeatureStore.synthetic(n, args.feats, dev, dtype="bf16", seed=2)
    specs = [{"n_train_samples": f, "n_val_samples": f, "output_dim": 128,
              "activation": (lambda x: x) if i == 1 else F.relu} for i, f in enumerate(fans)]
    weighted = gs.find_sampler("sparse_weighted_neighbor_sampler")
    uniform = lambda adj: gs.nn_modules.SparseUniformNeighborSampler(adj, rng="philox")      # noqa: E731

    def model(sampler, adj):
        torch.manual_seed(0)
        m = gs.GSSupervised(sampler_class=sampler, adj=adj, train_adj=adj, prep_class=gs.prep_lookup["identity"],
                            aggregator_class=gs.aggregator_lookup["mean"], input_dim=args.feats, n_nodes=n, n_classes=41,
                            layer_specs=specs).to(dev)
        m.train_sampler.use_device_csr(csr)
        m.val_sampler.use_device_csr(csr)
        return m

    w_adj = gs.WeightedAdj(ph_adj, np.ones(2, dtype=np.float32))
    rng = np.random.RandomState(0)
    nb = args.queue_batches
    ids = torch.from_numpy(rng.randint(1, n, size=(nb, B))).to(dev)
    tgs = torch.from_numpy(rng.randint(0, 41, size=(nb, B, 1))).to(dev)
    loss = gs.ProblemLosses.classification
    WE, ME = gs.engine.FusedWeightedMeanTrainStep, gs.engine.FusedMeanTrainStep

    m_a = model(weighted, w_adj)
    e_b = WE(model(weighted, w_adj), store, loss, ids[0], tgs[0])
    e_c = {}
    for form in ("kary", "binary"):
        with search(form):
            e_c[form] = WE(model(weighted, w_adj), store, loss, ids[0], tgs[0]).load_epoch(ids, tgs)
    e_d = ME(model(uniform, ph_adj), store, loss, ids[0], tgs[0]).load_epoch(ids, tgs)
    count = [0]

    def per_call(fn):
        def go():
            k = count[0] % nb
            count[0] += 1
            fn(ids[k], tgs[k])
        return go

    paths = [("a_module_path_weighted", per_call(lambda i, t: m_a.train_step(i, store, t, loss))),
             ("b_engine_per_call", per_call(e_b)),
             ("c_engine_queue_8ary", e_c["kary"].step_queue),
             ("c_engine_queue_binary", e_c["binary"].step_queue),
             ("d_uniform_engine_queue", e_d.step_queue)]
    times = {name: [] for name, _ in paths}
    for r in range(args.warm_rounds + args.rounds):
        for name, fn in paths:
            t = timed(fn, args.steps)
            if r >= args.warm_rounds:
                times[name].append(t)
    rows = [dict(base, what="step", unit="ms/step", steps=args.steps, warm_rounds=args.warm_rounds, rounds=args.rounds,
                 queue_batches=nb, tail_rows=int(e_c["kary"]._tail_rows), ring=int(e_c["kary"].P),
                 **{name: stats(v) for name, v in times.items()})]

    rows.append(dict(base, what="sampler_launch", unit="us/launch", reps=64,
                     note="each launch alone on an idle GPU, a batch of seeds of its own per launch and replay, timed "
                          "by events attached to its dispatch",
                     **sampler_launches(csr, ids, fans, 64)))

    for form in ("kary", "binary"):
        eng = e_c[form]
        with search(form):
            eng.instrument(True)
        marks = {}
        for _ in range(40):
            eng.step_queue()
            torch.cuda.synchronize()
            for k, v in eng.last_launch_ms().items():
                marks.setdefault(k, []).append(v)
        rows.append(dict(base, what="in_step", unit="us/launch", steps=40, engine="c_engine_queue", search=form,
                         **{k: {"median_us": 1e3 * float(np.median(v[8:])), "min_us": 1e3 * float(min(v[8:])),
                                "max_us": 1e3 * float(max(v[8:]))} for k, v in marks.items()}))
    csr.check()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
