#!/usr/bin/env python
"""biased_walk_bench.py -- what node2vec's second-order steps and restarts cost (include/gsage.h, "Biased walks"), at the
Reddit shape of tools/unsup_weighted_bench.py (232 965 nodes, degrees uniform in 1..841: ~98 M edges; weights drawn on
the device: exp of a normal, 5 % zeros).  Nothing here is a threshold: the yardstick of every line is the plain entry
measured in the same process.

One JSON line per measurement, appended to --out (default profiles/biased_walk_bench.jsonl), one process:
  builder_launch  us / launch at B = 512, Q = 20, walk_len 5 and 16, each launch timed in place by events attached to
                  its dispatch in a recorded command list (one list per walk_len, a batch of seeds of its own per launch
                  and replay): the plain entry, the biased entry at neutral parameters, at (p, q) = (4, 0.25) and at
                  (0.25, 4); uniform and weighted proposals.
  importance      ms / call over every node at 50/2/16 and 200/5/32, the paths alternating, 2 warm-up calls, median and
                  range of 7: plain, biased-neutral, (4, 0.25), restart 0.15; uniform and weighted steps.
  step            ms / step of FusedUnsupMeanTrainStep with walk_p = 4, walk_q = 0.25 beside the plain engine, alternating
                  (fan-out 25/10, dims 128/128, 602 bf16 features).
  rounds          the tool's own replay, in Python integers, of the walks of one batch (checked against the device's
                  positives): mean rounds per second-order step and the share of those steps with a round whose
                  acceptance word only the previous node's row could decide.  No kernel is instrumented.
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
PAIRS = {"plain": None, "neutral": (1.0, 1.0), "p4_q0.25": (4.0, 0.25), "p0.25_q4": (0.25, 4.0)}


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def builder_launches(csr, cdf_w, cdf_u, batches, Q, wl, reps):
    """us of each builder launch at walk_len wl, timed in place inside ONE recorded list replayed `reps` times"""
    B, dev = int(batches.shape[1]), batches.device
    lib, st = nat.lib(), ops._stream()
    slots = [(mode, name, pq) for mode in ("uniform", "weighted") for name, pq in PAIRS.items()]     # 8 slots: 16 marks
    nb = int(batches.shape[0])
    src = [batches[j % nb].clone() for j in range(len(slots))]
    seeds = [torch.zeros(B, dtype=torch.int64, device=dev) for _ in slots]
    ids = torch.zeros(2 * B + Q, dtype=torch.int64, device=dev)
    pw = torch.zeros(B, dtype=torch.float32, device=dev)
    with nat.CommandList.record() as cl:
        for j, (mode, name, pq) in enumerate(slots):
            weighted = mode == "weighted"
            cdf = cdf_w if weighted else cdf_u
            ecdf = csr.edge_cdf.data_ptr() if weighted else None
            nat.check(lib.gsage_copy_pair(seeds[j].data_ptr(), src[j].data_ptr(), B * 8, None, None, 0, st), "copy_pair")
            nat.check(lib.gsage_cmdlist_time_next(2 * j, 2 * j + 1), "time_next")
            head = (csr.rowptr.data_ptr(), csr.col.data_ptr())
            tail = (csr.n_rows, seeds[j].data_ptr(), B, wl, Q, cdf.data_ptr(), cdf._gsage_total, 1, None, j, 0)
            out = (ids.data_ptr(), pw.data_ptr(), csr.err_flag.data_ptr(), st)
            if pq is not None:
                nat.check(lib.gsage_unsup_batch_biased(*(head + (ecdf,) + tail + pq + out)), "unsup_batch_biased")
            elif weighted:
                nat.check(lib.gsage_unsup_batch_weighted(*(head + (ecdf,) + tail + out)), "unsup_batch_weighted")
            else:
                nat.check(lib.gsage_unsup_batch(*(head + tail + out)), "unsup_batch")
    got = {"%s/%s" % (mode, name): [] for mode, name, _ in slots}
    for r in range(reps + 5):
        for j in range(len(slots)):
            src[j].copy_(batches[(len(slots) * r + j) % nb])
        cl.replay(st)
        torch.cuda.synchronize()
        if r >= 5:
            for j, (mode, name, _) in enumerate(slots):
                got["%s/%s" % (mode, name)].append(1e3 * cl.elapsed_ms(2 * j, 2 * j + 1))
    return {k: {"median_us": float(np.median(v)), "min_us": float(min(v)), "max_us": float(max(v))} for k, v in got.items()}


def alternating(paths, reps, warmup):
    """ms of every call of every path: the paths take turns, `warmup` turns are thrown away"""
    times = {name: [] for name, _ in paths}
    for r in range(warmup + reps):
        for name, fn in paths:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if r >= warmup:
                times[name].append(a.elapsed_time(b))
    return times


def replay_rounds(csr, cdf, seeds, wl, Q, p, q, seed, call):
    """The uniform biased builder's walks of one batch in Python integers, rows fetched from the device as needed.
    -> (positives int64 [B], second-order steps, rounds, steps with a round only the previous node's row decides)"""
    th_ret, th_near, th_far, _ = ops.walk_thresholds(p, q)
    lo, hi = min(th_near, th_far), max(th_near, th_far)
    rp = csr.rowptr
    rows = {}

    def row(v):
        if v not in rows:
            rows[v] = csr.col[int(rp[v]):int(rp[v + 1])].cpu().numpy()
        return rows[v]
    klo, khi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    pos, steps, rounds, scanned = [], 0, 0, 0
    for g, s in enumerate(seeds.tolist()):
        c = (g & 0xFFFFFFFF, g >> 32, call & 0xFFFFFFFF, call >> 32)
        t = 1 + ((ops._philox4(c, (klo, khi ^ ops.UNSUP_TAG_LEN))[0] * wl) >> 32)
        v, prev = s, -1
        for j in range(t):
            nbrs = row(v)
            if len(nbrs) == 0:
                break
            legacy = ops._philox4(c, (klo, khi ^ (ops.UNSUP_TAG_STEP | (j >> 2))))[j & 3]
            if prev < 0:
                prev, v = v, int(nbrs[(legacy * len(nbrs)) >> 32])
                continue
            steps += 1
            needs_row = False
            for k in range(ops.WALK_ROUNDS):
                nb = ops._philox4(c, (klo, khi ^ (ops.WALK_BIAS_TAG | (j << 8) | k)))
                x = int(nbrs[((legacy if k == 0 else nb[0]) * len(nbrs)) >> 32])
                rounds += 1
                if x == prev:
                    th = th_ret
                else:
                    needs_row = needs_row or lo <= nb[2] < hi
                    th = th_near if bool((row(prev) == x).any()) else th_far
                if nb[2] < th:
                    break
            scanned += int(needs_row)
            prev, v = v, x
        pos.append(v)
    return np.asarray(pos, dtype=np.int64), steps, rounds, scanned


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--deg-hi", type=int, default=841)
    ap.add_argument("--feats", type=int, default=602)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--negatives", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "biased_walk_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "biased_walk_bench needs a GPU"
    dev = torch.device("cuda")
    ops.set_compute_dtype("bf16")
    ops.warmup(dev)
    n, B, Q = args.nodes, args.batch, args.negatives
    csr = gs.DeviceCSR.synthetic(n, 1, args.deg_hi, dev, seed=1)
    gen = torch.Generator(device=dev).manual_seed(3)
    w = torch.exp(torch.randn(csr.nnz, device=dev, generator=gen) * 2.3)
    w[torch.rand(csr.nnz, device=dev, generator=gen) < 0.05] = 0.0
    weighted = gs.DeviceCSR(csr.rowptr, csr.col, n, csr.max_deg).with_weights(w)
    del w
    info = nat.device_info()
    base = {"arch": info["arch"] if info else None, "nodes": n, "edges": csr.nnz, "max_degree": args.deg_hi,
            "stamp": time.strftime("%Y-%m-%d")}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def emit(row):
        line = json.dumps(row)
        print(line)
        sys.stdout.flush()
        with open(args.out, "a") as f:
            f.write(line + "\n")

    rng = np.random.RandomState(0)
    batches = torch.from_numpy(rng.randint(1, n, size=(args.batches, B))).to(dev)
    cdf_u, cdf_w = ops.neg_cdf(csr), ops.neg_cdf(weighted, weighted=True)
    for wl in (5, 16):
        emit(dict(base, what="builder_launch", unit="us/launch", B=B, Q=Q, walk_len=wl, reps=64,
                  note="each launch alone on an idle GPU, a batch of seeds of its own per launch and replay",
                  **builder_launches(weighted, cdf_w, cdf_u, batches, Q, wl, 64)))

    ids = torch.arange(n, dtype=torch.int64, device=dev)
    variants = [("plain", {}), ("neutral", {"_biased": True}), ("p4_q0.25", {"p": 4.0, "q": 0.25}),
                ("restart0.15", {"restart": 0.15})]
    for R, L, T in ((50, 2, 16), (200, 5, 32)):
        for mode, adj in (("uniform", csr), ("weighted", weighted)):
            paths = [(name, (lambda kw=kw: ops.importance_walks(adj, ids, R, L, T, 1, **kw))) for name, kw in variants]
            times = alternating(paths, args.reps, args.warmup)
            adj.check()
            emit(dict(base, what="importance", unit="ms/call", n_walks=R, walk_len=L, top=T, mode=mode, reps=args.reps,
                      warmup=args.warmup, **{name: stats(v) for name, v in times.items()}))

    # the tool's own replay of one batch: rounds per second-order step, steps that needed the previous node's row
    for name, (p, q) in (("p4_q0.25", (4.0, 0.25)), ("p0.25_q4", (0.25, 4.0))):
        for wl in (5, 16):
            seeds = batches[0][:256]
            got, _ = ops.unsup_batch(csr, seeds, wl, Q, cdf_u, {"seed": 1, "call_base": 0}, p=p, q=q)
            pos, steps, rounds, scanned = replay_rounds(csr, cdf_u, seeds.cpu(), wl, Q, p, q, 1, 0)
            assert np.array_equal(got[256:512].cpu().numpy(), pos), "the replay and the kernel disagree"
            emit(dict(base, what="rounds", pq=name, walk_len=wl, walks=256, second_order_steps=steps,
                      mean_rounds_per_step=rounds / max(steps, 1), share_of_steps_with_a_scan=scanned / max(steps, 1)))

    # the unsupervised engine: biased positives beside the plain engine of the same run
    fans = (25, 10)
    specs = [{"n_train_samples": f, "n_val_samples": f, "output_dim": 128,
              "activation": (lambda x: x) if i == 1 else F.relu} for i, f in enumerate(fans)]
    ph_adj = sparse.csr_matrix((np.array([1, 1]), np.array([0, 0]), np.array([0, 0, 1, 2])), shape=(3, 1))
    store = gs.FeatureStore.synthetic(n, args.feats, dev, dtype="bf16", seed=2)

    def engine(walk_p, walk_q):
        torch.manual_seed(0)
        m = gs.GSUnsupervised(sampler_class=lambda adj: gs.nn_modules.SparseUniformNeighborSampler(adj, rng="philox"),
                              adj=ph_adj, train_adj=ph_adj, prep_class=gs.prep_lookup["identity"],
                              aggregator_class=gs.aggregator_lookup["mean"], input_dim=args.feats, n_nodes=n,
                              layer_specs=specs, walk_len=5, n_negatives=Q, walk_p=walk_p, walk_q=walk_q).to(dev)
        m.train_sampler.use_device_csr(csr)
        m.val_sampler.use_device_csr(csr)
        return gs.engine.FusedUnsupMeanTrainStep(m, store, batches[0])
    engines = [("plain", engine(1.0, 1.0)), ("p4_q0.25", engine(4.0, 0.25))]
    count = [0]

    def run(eng):
        def go():
            for _ in range(args.steps):
                eng(batches[count[0] % args.batches])
                count[0] += 1
        return go
    times = alternating([(name, run(e)) for name, e in engines], args.reps, args.warmup)
    emit(dict(base, what="step", unit="ms/step", engine="FusedUnsupMeanTrainStep", B=B, Q=Q, walk_len=5, fan=list(fans),
              dims=[128, 128], feats=args.feats, steps=args.steps, reps=args.reps, warmup=args.warmup,
              **{name: stats([t / args.steps for t in v]) for name, v in times.items()}))
    for _, e in engines:
        e.close()
    csr.check()


if __name__ == "__main__":
    main()
