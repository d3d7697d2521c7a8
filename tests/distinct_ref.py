"""What the distinct-sampler tests share, written from the definition of include/gsage.h ("Distinct neighbours") in
Python integers on oracle.cpu.philox4x32_10 -- no code of the product: the sampler in its SERIAL form (the partial
Fisher-Yates shuffle over a virtual array), the test graph whose rows sit on every edge of the definition for the n in
use, and the small problems of the model tests."""
import numpy as np
import torch
from scipy import sparse
from torch.nn import functional as F

from conftest import pkg
from oracle import cpu as ocpu

TAG = 0x44000000
M64 = (1 << 64) - 1


# ---- the sampler -------------------------------------------------------------------------------------------------
def word(seed, call, g):
    """w(g): word g & 3 of Philox block g >> 2 under the sampler's own key"""
    g &= M64
    call &= M64
    blk = g >> 2
    w = ocpu.philox4x32_10((blk & 0xFFFFFFFF, blk >> 32, call & 0xFFFFFFFF, call >> 32),
                           (seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ TAG))
    return int(w[g & 3])


def offsets(deg, n, words):
    """the n offsets into a row of degree deg > 0 from the parent's words w_0 .. w_{n-1}: serial form"""
    if deg <= n:
        r = (words[0] * deg) >> 32
        return [(j + r) % deg for j in range(n)]
    a, out = {}, []                                       # the virtual array: a[x] = x unless written
    for j in range(n):
        t = j + ((words[j] * (deg - j)) >> 32)
        assert j <= t < deg
        aj = a.get(j, j)                                  # a[j] read before the write
        out.append(a.get(t, t))
        a[t] = aj
    return out


def sample(rowptr, col, n_rows, ids, n, seed, call, g0):
    """-> (out int64 [M * n], err): gsage_sample_csr_distinct"""
    out, err = np.zeros(len(ids) * n, dtype=np.int64), 0
    for i, v in enumerate(ids):
        v = int(v)
        if v < 0 or v >= n_rows:
            err = 1
            continue
        beg, deg = int(rowptr[v]), int(rowptr[v + 1]) - int(rowptr[v])
        if deg <= 0:
            continue
        ws = [word(seed, call, g0 + i * n + j) for j in range(n)]
        for j, o in enumerate(offsets(deg, n, ws)):
            out[i * n + j] = col[beg + o]
    return out, err


def sample_hops(rowptr, col, n_rows, seeds, fans, seed, call0, rank=0):
    """-> ([hop 0, hop 1, ...], err): hop k under call index call0 + k - 1 and g0 = rank * |hop k|"""
    hops, err = [np.asarray(seeds, dtype=np.int64)], 0
    for k, n in enumerate(fans, 1):
        out, e = sample(rowptr, col, n_rows, hops[-1], n, seed, call0 + k - 1, rank * len(hops[-1]) * n)
        hops.append(out)
        err |= e
    return hops, err


# ---- the test graph ----------------------------------------------------------------------------------------------
N_ROWS = 41
ROWS = {"ordinary": 0, "degree 0": 1, "degree 1": 2, "degree 2": 3, "n - 1": 4, "n": 5, "n + 1": 6, "2n": 7, 300: 8,
        "repeated column": 9, 1000: 10, "last": N_ROWS - 1}


class Graph(object):
    def __init__(self, rowptr, col):
        self.rowptr, self.col = rowptr, col
        self.n = len(rowptr) - 1
        self.deg = np.diff(rowptr)

    def csr(self, device="cpu"):
        gs = pkg()
        return gs.DeviceCSR(torch.from_numpy(self.rowptr).to(device), torch.from_numpy(self.col).to(device), self.n,
                            max(int(self.deg.max()), 1))


_GRAPHS = {}


def graph(n):
    """41 rows on every edge of the definition at n samples per parent (ROWS), the others of degree 1..24"""
    if n in _GRAPHS:
        return _GRAPHS[n]
    rng = np.random.RandomState(1000 + n)
    deg = rng.randint(1, 25, size=N_ROWS)
    deg[:11] = [7, 0, 1, 2, max(n - 1, 0), n, n + 1, 2 * n, 300, n + 2, 1000]
    deg[N_ROWS - 1] = n + 3
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.randint(0, N_ROWS, size=int(rowptr[-1])).astype(np.int32)
    b = int(rowptr[ROWS["repeated column"]])
    col[b + 1] = col[b]                                   # one column stored twice: "distinct" is distinct EDGES
    g = Graph(rowptr, col)
    _GRAPHS[n] = g
    return g


def arranged(n):
    """the rows of ROWS that exist at this n, in a fixed order"""
    return [ROWS[k] for k in ("ordinary", "degree 0", "degree 1", "degree 2", "n - 1", "n", "n + 1", "2n", 300,
                              "repeated column", 1000, "last")]


def parents(M, n, rng):
    """M parent ids: the arranged rows first (the longest chases, rows n + 1 and 1000, in front when M is small)"""
    first = [ROWS["n + 1"], ROWS[1000], ROWS["n"]] + arranged(n)
    ids = rng.randint(0, N_ROWS, size=M)
    ids[:min(M, len(first))] = first[:M]
    return ids.astype(np.int64)


# ---- the problems of the model tests -----------------------------------------------------------------------------
def problem(n=500, D=16, C=3, seed=7, degrees=None):
    """dict(adj, indptr, data, feats, folds, targets, C): n nodes + the dummy row 0 in the reference's sparse
    convention; degrees: the set every row's degree is drawn from (default 0..11 with rows of degree 0)"""
    rng = np.random.RandomState(seed)
    if degrees is None:
        deg = rng.randint(1, 12, size=n + 1)
        deg[0] = 0
        deg[9::23] = 0
    else:
        deg = rng.choice(np.asarray(degrees), size=n + 1)         # (row 0 too: no row reads the dummy by default)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    data = rng.randint(1, n + 1, size=int(indptr[-1]))
    cols = np.arange(indptr[-1]) - np.repeat(indptr[:-1], deg)
    adj = sparse.csr_matrix((data, cols, indptr), shape=(n + 1, int(deg.max())))
    feats = rng.normal(size=(n + 1, D)).astype(np.float32)
    feats[0] = 0
    k = int(0.65 * n)
    folds = np.array(["train"] * k + ["val"] * (n // 5) + ["test"] * (n + 1 - k - n // 5))
    folds[0] = "dummy"
    targets = feats[:, :C].argmax(1).reshape(-1, 1)
    return dict(adj=adj, indptr=indptr, data=data, feats=feats, folds=folds, targets=targets, C=C, n=n)


def model(p, dims, fans, agg="mean", prep="identity", sampler="sparse_distinct_neighbor_sampler", seed=3, adj=None,
          train_adj=None, **kw):
    gs = pkg()
    torch.manual_seed(seed)
    specs = [{"n_train_samples": f, "n_val_samples": f, "output_dim": h,
              "activation": (lambda x: x) if i == len(dims) - 1 else F.relu} for i, (f, h) in enumerate(zip(fans, dims))]
    return gs.GSSupervised(sampler_class=gs.find_sampler(sampler), adj=p["adj"] if adj is None else adj,
                           train_adj=p["adj"] if train_adj is None else train_adj, prep_class=gs.prep_lookup[prep],
                           aggregator_class=gs.aggregator_lookup[agg],
                           input_dim=p["feats"].shape[1] if prep == "identity" else None, n_nodes=p["n"] + 1,
                           n_classes=p["C"], layer_specs=specs, **kw)
