#!/usr/bin/env python
"""graph_build_bench.py -- what building a graph on the device costs (include/gsage.h, "Graph construction") at a
synthetic Reddit-shape edge list: --edges (default 5.5e7) undirected input edges over 232 965 nodes, ids uniform, 2 %
of the list repeated as it is and 2 % repeated reversed, a few self-loops -- 1.1e8 records.

One JSON line per measurement, appended to --out (default profiles/graph_build_bench.jsonl), all in one process:
  from_edges_insertion / from_edges_id   DeviceCSR.from_edges under order="insertion" (the reference's order: two
                 sorts) and order="id" (one sort)
  from_edges_train   the `sel` build of the training graph (66 % of the nodes selected), order="insertion"
  transpose / symmetrized   of the "id" build
each next to a stock-torch formulation of the same definition (torch.sort(stable=True) / unique_consecutive on the
packed keys) in the same process, alternating, 2 warm-up calls, the median and range of 7; a host clock around the
call and a device synchronise.  `equal` says whether the two results were the same arrays (compared once, untimed).
  context        at 1e6 edges: the host-mode builder (numpy) and convert.graph_from_edgelist + make_sparse_adjacency
                 (the Python loop this replaces), one call each
Nothing is asserted.  Needs a GPU: there is no CPU fallback."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gs = importlib.import_module("pytorch-graphsage_amd")
nat, ops = gs._native, gs.ops
WARM, ROUNDS = 2, 7


def edge_list(n, E, dev, seed=0):
    gen = torch.Generator(device=dev).manual_seed(seed)
    e = torch.randint(0, n, (E, 2), dtype=torch.int64, device=dev, generator=gen)
    k = E // 50
    e[E - 2 * k:E - k] = e[:k]                                # repeated
    e[E - k:] = e[k:2 * k].flip(1)                            # repeated, reversed
    e[::100003, 1] = e[::100003, 0]                           # self-loops
    return e[:, 0].contiguous(), e[:, 1].contiguous()


# ---- the same definition in stock torch ------------------------------------------------------------------------
def _rowptr(rows, n_rows):
    rowptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=rows.device)
    torch.cumsum(torch.bincount(rows, minlength=n_rows), 0, out=rowptr[1:])
    return rowptr


def torch_from_edges(src, dst, n, order, sel=None):
    b = max(int(n).bit_length(), 1)
    sent = (1 << (2 * b)) - 1
    live = torch.ones_like(src, dtype=torch.bool) if sel is None else sel[src] & sel[dst]
    fwd = torch.where(live, (src << b) | dst, sent)
    rev = torch.where(live & (src != dst), (dst << b) | src, sent)
    keys = torch.stack([fwd, rev], 1).view(-1)
    ks, ps = torch.sort(keys, stable=True)
    if order == "id":
        uk = torch.unique_consecutive(ks)
        uk = uk[uk < sent]
    else:
        first = torch.ones_like(ks, dtype=torch.bool)
        first[1:] = ks[1:] != ks[:-1]
        first &= ks < sent
        kept = torch.sort(ps[first]).values                   # the kept records, in record order
        uk = keys[kept]
        uk = uk[torch.sort(uk >> b, stable=True).indices]
    return _rowptr((uk >> b) + 1, n + 1), ((uk & ((1 << b) - 1)) + 1).to(torch.int32)


def torch_transpose(csr):
    deg = csr.rowptr[1:] - csr.rowptr[:-1]
    rows = torch.repeat_interleave(torch.arange(csr.n_rows, dtype=torch.int64, device=csr.device), deg)
    c = csr.col.to(torch.int64)
    return _rowptr(c, csr.n_rows), rows[torch.sort(c, stable=True).indices].to(torch.int32)


def torch_symmetrized(csr):
    b = max(int(csr.n_rows).bit_length(), 1)
    deg = csr.rowptr[1:] - csr.rowptr[:-1]
    rows = torch.repeat_interleave(torch.arange(csr.n_rows, dtype=torch.int64, device=csr.device), deg)
    c = csr.col.to(torch.int64)
    uk = torch.unique_consecutive(torch.sort(torch.cat([(rows << b) | c, (c << b) | rows])).values)
    return _rowptr(uk >> b, csr.n_rows), (uk & ((1 << b) - 1)).to(torch.int32)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}


def pair(ours, theirs):
    """ours() -> DeviceCSR, theirs() -> (rowptr, col): alternating, 2 warm-up calls, 7 timed"""
    took = {"hip": [], "torch": []}
    for r in range(WARM + ROUNDS):
        for name, fn in (("hip", ours), ("torch", theirs)):
            ms, out = clock(fn)
            if r >= WARM:
                took[name].append(ms)
            del out
    a, (rp, col) = ours(), theirs()
    equal = bool(torch.equal(a.rowptr, rp) and torch.equal(a.col, col))
    return {"hip": stats(took["hip"]), "torch": stats(took["torch"]), "equal": equal, "nnz": a.nnz, "max_deg": a.max_deg}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--edges", type=int, default=55000000)
    ap.add_argument("--context-edges", type=int, default=1000000)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "graph_build_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "graph_build_bench needs a GPU"
    dev = torch.device("cuda")
    ops.warmup(dev)
    n, E = args.nodes, args.edges
    src, dst = edge_list(n, E, dev)
    sel = torch.rand(n, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) < 0.66
    info = nat.device_info()
    base = {"arch": info["arch"] if info else None, "nodes": n, "input_edges": E, "records": 2 * E, "warm": WARM,
            "rounds": ROUNDS, "unit": "ms/call", "stamp": time.strftime("%Y-%m-%d")}
    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)
    b = max(int(n).bit_length(), 1)
    passes = lambda bits: (bits + 7) // 8                     # gsage_sort_rows: three launches per 8-bit pass
    for order in ("insertion", "id"):
        before = nat.launch_count()
        gs.DeviceCSR.from_edges(src, dst, n, dev, order=order)
        calls = nat.launch_count() - before                   # (the counter ticks once per C entry, a sort included)
        sorts = [2 * b, b] if order == "insertion" else [2 * b]
        emit(dict(base, what="from_edges_" + order, library_calls=calls, key_bits=sorts,
                  kernel_launches=calls - len(sorts) + 3 * sum(passes(s) for s in sorts),
                  **pair(lambda: gs.DeviceCSR.from_edges(src, dst, n, dev, order=order),
                         lambda: torch_from_edges(src, dst, n, order))))
    emit(dict(base, what="from_edges_train", selected=int(sel.sum()),
              **pair(lambda: gs.DeviceCSR.from_edges(src, dst, n, dev, sel=sel),
                     lambda: torch_from_edges(src, dst, n, "insertion", sel))))
    csr = gs.DeviceCSR.from_edges(src, dst, n, dev, order="id")
    emit(dict(base, what="transpose", stored_edges=csr.nnz, **pair(csr.transpose, lambda: torch_transpose(csr))))
    emit(dict(base, what="symmetrized", stored_edges=csr.nnz, **pair(csr.symmetrized, lambda: torch_symmetrized(csr))))
    del csr

    # ---- context: the host-mode builder and the Python loop this replaces, at 1e6 edges
    cv = importlib.import_module("pytorch-graphsage_amd.convert")
    Ec = min(args.context_edges, E)
    s_h, d_h = src[:Ec].cpu(), dst[:Ec].cpu()
    t0 = time.perf_counter()
    host = gs.DeviceCSR.from_edges(s_h, d_h, n, torch.device("cpu"))
    t_host = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    ref = cv.make_sparse_adjacency(cv.graph_from_edgelist(torch.stack([s_h, d_h], 1).numpy(), n_nodes=n))
    t_loop = 1e3 * (time.perf_counter() - t0)
    ms, got = clock(lambda: gs.DeviceCSR.from_edges(src[:Ec], dst[:Ec], n, dev))
    ms, got = clock(lambda: gs.DeviceCSR.from_edges(src[:Ec], dst[:Ec], n, dev))
    emit(dict(base, what="context", input_edges=Ec, records=2 * Ec, host_mode_ms=t_host, python_loop_ms=t_loop,
              hip_ms=ms, calls=1, equal=bool(torch.equal(got.col.cpu(), host.col) and
                                             np.array_equal(ref.data, host.col.numpy().astype(np.int64)))))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
