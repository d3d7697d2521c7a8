"""infer.plan, the host-side schedule of gsage_segment_reduce, as properties on CPU tensors: the partition into short
and long rows, the order of the short ones, the slices of the long ones and their first-slice indices, the cache."""
import numpy as np
import pytest
import torch

import segment_reduce_ref as sr
from conftest import pkg

SLICE_LENS = [8, 16, 256]


def _graphs():
    """the kernel tests' two graphs and a few random ones (the last: no empty row, every degree above 16)"""
    out = [("L8", sr.graph(8)), ("L256", sr.graph(256))]
    for seed, (lo, hi, n) in enumerate([(0, 40, 300), (0, 9, 64), (17, 600, 40)]):
        rng = np.random.RandomState(seed)
        out.append(("random%d" % seed, sr.from_degrees(rng.randint(lo, hi + 1, size=n), rng, 8)))
    return out


GRAPHS = _graphs()


@pytest.mark.parametrize("slice_len", SLICE_LENS)
@pytest.mark.parametrize("name,g", GRAPHS, ids=[n for n, _ in GRAPHS])
def test_plan_properties(name, g, slice_len):
    gs = pkg()
    p = gs.infer.plan(g.csr(), slice_len=slice_len)
    deg, rowptr = g.deg, g.rowptr
    order, longs, slices = p["order"].numpy(), p["long_rows"].numpy(), p["slices"].numpy()
    assert p["slice_len"] == slice_len
    assert p["order"].dtype == torch.int32 and p["long_rows"].dtype == torch.int64 and p["slices"].dtype == torch.int64
    assert order.shape == (p["n_short"],) and longs.shape == (p["n_long"], 2) and slices.shape == (p["n_slices"], 2)
    assert all(t.is_contiguous() for t in (p["order"], p["long_rows"], p["slices"]))
    # every row in exactly one of the two lists; degree == slice_len is short
    assert sorted(order.tolist() + longs[:, 0].tolist()) == list(range(g.n))
    assert (deg[order] <= slice_len).all() and (deg[longs[:, 0]] > slice_len).all()
    # short rows: degree-descending, ties in ascending row index (a stable sort)
    assert order.tolist() == sorted(order.tolist(), key=lambda v: (-deg[v], v))
    # long rows in ascending row index, each with ceil(deg / slice_len) consecutive slices from its first-slice index
    assert longs[:, 0].tolist() == sorted(longs[:, 0].tolist())
    nxt = 0
    for row, first in longs.tolist():
        ns = -(-int(deg[row]) // slice_len)
        assert first == nxt, (row, first, nxt)
        mine = slices[first:first + ns]
        assert (mine[:, 0] == row).all()
        assert mine[:, 1].tolist() == [int(rowptr[row]) + k * slice_len for k in range(ns)]
        covered = np.concatenate([np.arange(b, min(b + slice_len, rowptr[row + 1])) for b in mine[:, 1]])
        assert covered.tolist() == list(range(int(rowptr[row]), int(rowptr[row + 1])))
        nxt += ns
    assert p["n_slices"] == nxt


def test_degree_exactly_slice_len_is_short_and_one_more_is_long():
    gs = pkg()
    for L in (8, 256):
        g = sr.graph(L)
        p = gs.infer.plan(g.csr(), slice_len=L)
        short, longs = set(p["order"].tolist()), dict(p["long_rows"].tolist())
        assert g.at[L] in short and g.at[L - 1] in short
        for d in (L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 3 * L + 5):
            assert g.at[d] in longs and g.deg[g.at[d]] == d
        # first non-dummy row, the middle, the last row: long, and the first of them owns slice 0
        assert longs[1] == 0 and g.n // 2 in longs and g.n - 1 in longs
        assert {int(g.deg[v]) for v in short} >= {0, 1, 7, 8}


def test_first_slice_indices_differ_with_several_long_rows():
    """what one long row cannot show: the exclusive running sum of the slice counts"""
    gs = pkg()
    deg = np.array([0, 9, 3, 25, 8, 16, 17, 0, 40])
    g = sr.from_degrees(deg, np.random.RandomState(0), 8)
    p = gs.infer.plan(g.csr(), slice_len=8)
    assert p["long_rows"].tolist() == [[1, 0], [3, 2], [5, 6], [6, 8], [8, 11]]
    assert p["n_slices"] == 16 and p["n_short"] == 4
    assert p["order"].tolist() == [4, 2, 0, 7]
    assert p["slices"][2:6].tolist() == [[3, 12], [3, 20], [3, 28], [3, 36]]


def test_plan_cache():
    gs = pkg()
    adj = sr.graph(8).csr()
    a = gs.infer.plan(adj, slice_len=8)
    assert gs.infer.plan(adj, slice_len=8) is a
    b = gs.infer.plan(adj)
    assert b is not a and b["slice_len"] == gs.infer.SLICE_LEN == 256 and a["slice_len"] == 8
    assert gs.infer.plan(adj) is b
    assert b["n_long"] == 0 and a["n_long"] >= 70


def test_dense_adjacency_plans_as_k_edges_per_row():
    gs = pkg()
    rng = np.random.RandomState(2)
    n, K = 50, 12
    adj = gs.DenseAdj(torch.from_numpy(rng.randint(0, n, size=(n, K)).astype(np.int64)))
    rowptr, col, rows = gs.infer._csr(adj)
    assert rows == n and rowptr.tolist() == [K * v for v in range(n + 1)]
    assert col.dtype == torch.int32 and torch.equal(col.long(), adj.adj.reshape(-1))
    p = gs.infer.plan(adj)                              # K <= 256: every row short, in row order (all ties)
    assert p["n_short"] == n and p["n_long"] == 0 and p["n_slices"] == 0 and p["order"].tolist() == list(range(n))
    p = gs.infer.plan(adj, slice_len=8)                 # K = 12: every row long, two slices each
    assert p["n_short"] == 0 and p["n_long"] == n and p["n_slices"] == 2 * n
    assert p["long_rows"].tolist() == [[v, 2 * v] for v in range(n)]
    assert p["slices"].tolist() == [[v, K * v + 8 * k] for v in range(n) for k in range(2)]
