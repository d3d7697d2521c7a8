"""What the temporal-sampler tests share, written from the definition of include/gsage.h ("Temporal neighbours") in
Python integers on oracle.cpu.philox4x32_10 -- no code of the product: the count, the sampler and the snapshot in their
SERIAL form, the one test graph whose rows sit on either side of every search-round boundary with its query times, and
the small problem of the model tests."""
from functools import partial

import numpy as np
import torch
from scipy import sparse
from torch.nn import functional as F

from conftest import pkg
from oracle import cpu as ocpu

TAG = 0x54000000
M64 = (1 << 64) - 1
INT64_MAX = (1 << 63) - 1
BIG = 1 << 62
STRATEGIES, RULES = ("uniform", "recent"), ("seed", "edge")


# ---- the definition ----------------------------------------------------------------------------------------------
def word(seed, call, g):
    """w(g): word g & 3 of Philox block g >> 2 under the sampler's own key"""
    g &= M64
    call &= M64
    blk = g >> 2
    w = ocpu.philox4x32_10((blk & 0xFFFFFFFF, blk >> 32, call & 0xFFFFFFFF, call >> 32),
                           (seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ TAG))
    return int(w[g & 3])


def count(etime, beg, end, t):
    """the number of edges e in [beg, end) with etime[e] < t: one look at every edge, in Python integers"""
    return sum(1 for e in range(beg, end) if int(etime[e]) < t)


def sample(rowptr, col, etime, n_rows, ids, times, n, seed, call, g0, strategy, inherit, counts=None):
    """-> (out int64 [M * n], out_time int64 [M * n], err): gsage_sample_csr_temporal.  counts: a dict
    (row, t) -> cnt that is filled and reused (the serial count of a long row is slow)"""
    assert strategy in STRATEGIES and inherit in RULES
    M = len(ids)
    out, out_time, err = np.zeros(M * n, dtype=np.int64), np.zeros(M * n, dtype=np.int64), 0
    for i in range(M):
        v, t = int(ids[i]), int(times[i])
        out_time[i * n:(i + 1) * n] = t
        if v < 0 or v >= n_rows:
            err = 1
            continue
        beg, end = int(rowptr[v]), int(rowptr[v + 1])
        if counts is not None and (v, t) in counts:
            cnt = counts[(v, t)]
        else:
            cnt = count(etime, beg, end, t)
            if counts is not None:
                counts[(v, t)] = cnt
        if cnt == 0:
            continue
        for j in range(n):
            if strategy == "uniform":
                off = (word(seed, call, g0 + i * n + j) * cnt) >> 32
            else:
                off = cnt - 1 - (j % cnt)
            assert 0 <= off < cnt
            out[i * n + j] = col[beg + off]
            if inherit == "edge":
                out_time[i * n + j] = etime[beg + off]
    return out, out_time, err


def sample_hops(rowptr, col, etime, n_rows, seeds, times, fans, seed, call0, strategy, inherit, counts=None):
    """-> ([(ids, times) of hop 0, hop 1, ...], err): hop k under call index call0 + k - 1, g0 = 0"""
    hops, err = [(np.asarray(seeds, dtype=np.int64), np.asarray(times, dtype=np.int64))], 0
    for k, n in enumerate(fans, 1):
        o, ot, e = sample(rowptr, col, etime, n_rows, hops[-1][0], hops[-1][1], n, seed, call0 + k - 1, 0, strategy,
                          inherit, counts)
        hops.append((o, ot))
        err |= e
    return hops, err


def snapshot(rowptr, col, etime, t):
    """-> (rowptr, col, etime) of the edges with etime < t, in their order: the edge list, filtered one by one"""
    keep = [e for e in range(len(col)) if int(etime[e]) < t]
    rp = [0]
    for v in range(len(rowptr) - 1):
        rp.append(rp[-1] + sum(1 for e in range(int(rowptr[v]), int(rowptr[v + 1])) if int(etime[e]) < t))
    return (np.asarray(rp, dtype=np.int64), np.asarray(col)[keep].astype(np.int32),
            np.asarray(etime)[keep].astype(np.int64))


# ---- the test graph ----------------------------------------------------------------------------------------------
# degrees on either side of every search-round boundary (16, 256, 4096) and of a wave's 64 lanes; the first four rows
# are what one wave of the hop kernel holds together when the parents are taken in row order: 3, 300, 4097 and 0 edges
DEGREES = [3, 300, 4097, 0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257]
PAIRED = (17, 64, 300, 4097)          # rows that end (and begin) in a pair of times that differ only above bit 32


class Graph(object):
    def __init__(self, rowptr, col, etime):
        self.rowptr, self.col, self.etime = rowptr, col, etime
        self.n = len(rowptr) - 1
        self.deg = np.diff(rowptr)

    def csr(self, device="cpu"):
        gs = pkg()
        csr = gs.DeviceCSR(torch.from_numpy(self.rowptr).to(device), torch.from_numpy(self.col).to(device), self.n,
                           max(int(self.deg.max()), 1))
        return csr.with_times(torch.from_numpy(self.etime).to(device))


_GRAPH = []


def graph():
    """14 rows (DEGREES).  Position k of a row happens at time 3 * (k // 5) - 40: tie runs of five edges, one of which
    straddles every multiple of 80 and, of the multiples of 16, 16, 32, 48 and 64 (positions 15..19, 30..34, 45..49,
    60..64); the first runs are negative.  A PAIRED row begins with the times -2^62 - 2^32, -2^62 and ends with
    2^62, 2^62 + 2^32: their low 32 bits are equal."""
    if _GRAPH:
        return _GRAPH[0]
    rng = np.random.RandomState(54)
    deg = np.asarray(DEGREES, dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    n = len(DEGREES)
    col = rng.randint(1, n, size=int(rowptr[-1])).astype(np.int32)        # (never 0: a 0 in a frontier is the dummy)
    etime = np.zeros(int(rowptr[-1]), dtype=np.int64)
    for v, d in enumerate(DEGREES):
        t = 3 * (np.arange(d, dtype=np.int64) // 5) - 40
        if d in PAIRED:
            t[:2] = [-BIG - (1 << 32), -BIG]
            t[-2:] = [BIG, BIG + (1 << 32)]
        assert (np.diff(t) >= 0).all()
        etime[rowptr[v]:rowptr[v + 1]] = t
    _GRAPH.append(Graph(rowptr, col, etime))
    return _GRAPH[0]


KINDS = ("below every edge", "the first edge's time", "inside a tie run", "between two edges", "above every edge",
         "INT64_MAX")


def query_times(g, v):
    """the six query times of row v, in the order of KINDS"""
    beg, d = int(g.rowptr[v]), int(g.deg[v])
    if d == 0:
        return [-5, 0, 7, 8, 9, INT64_MAX]
    t = [int(x) for x in g.etime[beg:beg + d]]
    mid = t[d // 2]                                       # a value of the middle: its whole run is excluded
    if d in PAIRED:
        between = BIG + 1                                 # between the last two, whose low 32 bits are both 0
    else:
        between = t[d // 3] + 1                           # the values step by 3: + 1 lies between two runs
    return [t[0] - 1, t[0], mid, between, t[-1] + 1, INT64_MAX]


def parents(M=None):
    """(ids, times): kind after kind, inside a kind the rows in order -- adjacent parents are different rows, the
    first four (one wave of the hop kernel) of 3, 300, 4097 and 0 edges.  M: that many of them, cycled"""
    g = graph()
    ids, times = [], []
    for k in range(len(KINDS)):
        for v in range(g.n):
            ids.append(v)
            times.append(query_times(g, v)[k])
    if M is not None:
        ids = [ids[i % len(ids)] for i in range(M)]
        times = [times[i % len(times)] for i in range(M)]
    return np.asarray(ids, dtype=np.int64), np.asarray(times, dtype=np.int64)


# ---- the problem of the model tests ------------------------------------------------------------------------------
T_SNAP = 1000


def problem(n=60, D=16, C=3, seed=7, counts=(1, 2, 3, 6)):
    """dict(adj, time, indptr, data, etime, feats, targets, C, n, tadj): n nodes + row 0 in the reference's sparse
    convention; every row (row 0 too) has a number of edges before T_SNAP drawn from `counts` and 0..4 edges at or
    after it, one of them AT T_SNAP: the strict comparison decides.  The times arrive shuffled inside a row --
    TemporalAdj puts them in order; indptr / data / etime are the rows in time order (ties in stored order)."""
    gs = pkg()
    rng = np.random.RandomState(seed)
    early = rng.choice(np.asarray(counts), size=n + 1)
    late = rng.randint(0, 5, size=n + 1)
    deg = early + late
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    data = rng.randint(1, n + 1, size=int(indptr[-1])).astype(np.int64)
    time = np.zeros(int(indptr[-1]), dtype=np.int64)
    for v in range(n + 1):
        t = np.concatenate([rng.randint(-50, T_SNAP, size=early[v]), rng.randint(T_SNAP, T_SNAP + 50, size=late[v])])
        if late[v]:
            t[early[v]] = T_SNAP
        time[indptr[v]:indptr[v + 1]] = rng.permutation(t)
    cols = np.arange(indptr[-1]) - np.repeat(indptr[:-1], deg)
    adj = sparse.csr_matrix((data, cols, indptr), shape=(n + 1, int(deg.max())))
    order = np.concatenate([indptr[v] + np.argsort(time[indptr[v]:indptr[v + 1]], kind="stable") for v in range(n + 1)])
    feats = rng.normal(size=(n + 1, D)).astype(np.float32)
    targets = feats[:, :C].argmax(1).reshape(-1, 1)
    return dict(adj=adj, time=time, indptr=indptr, data=data[order], etime=time[order], feats=feats, targets=targets,
                C=C, n=n, early=early, tadj=gs.TemporalAdj(adj, time))


def model(p, dims, fans, sampler="sparse_temporal_neighbor_sampler", strategy="recent", inherit="seed", seed=3, adj=None):
    gs = pkg()
    torch.manual_seed(seed)
    specs = [{"n_train_samples": f, "n_val_samples": f, "output_dim": h,
              "activation": (lambda x: x) if i == len(dims) - 1 else F.relu} for i, (f, h) in enumerate(zip(fans, dims))]
    cls = gs.find_sampler(sampler)
    if sampler == "sparse_temporal_neighbor_sampler":
        cls = partial(cls, strategy=strategy, inherit=inherit)
    adj = p["tadj"] if adj is None else adj
    return gs.GSSupervised(sampler_class=cls, adj=adj, train_adj=adj, prep_class=gs.prep_lookup["identity"],
                           aggregator_class=gs.aggregator_lookup["mean"], input_dim=p["feats"].shape[1],
                           n_nodes=p["n"] + 1, n_classes=p["C"], layer_specs=specs)
