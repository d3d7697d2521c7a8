"""A plain restatement, with explicit loops over rows and neighbours, of the k-hop closure of a query set and its
blocks (infer.closure, csrc/gsage_block.hip):

    S_L     = the queries with duplicates removed, in order of first appearance
    S_{l-1} = S_l unchanged as a prefix, then the nodes of N(S_l) and the dummy 0 not yet present, in ascending id
    block l = the stored rows of S_l, whole, in stored order, duplicates kept, every id replaced by its position in
              S_{l-1} (its local index); a weighted adjacency's cdf segments verbatim; the dummy's local index

An id outside [0, n) -- a query or a stored neighbour -- is dropped from the sets (`bad` says that one was seen); in a
block's col it is the dummy's local index."""
import numpy as np


class RefBlock(object):
    def __init__(self, rowptr, col, orig, cdf, n_dst, n_src, dummy):
        self.rowptr, self.col, self.orig, self.cdf = rowptr, col, orig, cdf
        self.n_dst, self.n_src, self.dummy = n_dst, n_src, dummy


class RefClosure(object):
    """sets[l]: int64 ids of S_l (l = 0 .. L); blocks[l]: RefBlock (l = 1 .. L; blocks[0] is None); index[i]: the local
    index of query i in S_L (-1: outside the graph); bad: an id outside [0, n) was met."""

    def __init__(self, sets, blocks, index, bad):
        self.sets, self.blocks, self.index, self.bad = sets, blocks, index, bad


def closure_ref(rowptr, col, n, queries, depth, cdf=None):
    rowptr, col = np.asarray(rowptr), np.asarray(col)
    where, S, bad = {}, [], False
    for q in (int(x) for x in np.asarray(queries).reshape(-1)):
        if not 0 <= q < n:
            bad = True
        elif q not in where:
            where[q] = len(S)
            S.append(q)
    index = np.array([where.get(int(q), -1) for q in np.asarray(queries).reshape(-1)], dtype=np.int64)
    sets, blocks = {depth: np.array(S, dtype=np.int64)}, [None] * (depth + 1)
    for l in range(depth, 0, -1):
        dst = list(S)
        new = set() if 0 in where else {0}
        for v in dst:                                        # every member's row, not just the newest members'
            for u in (int(x) for x in col[rowptr[v]:rowptr[v + 1]]):
                if not 0 <= u < n:
                    bad = True
                elif u not in where:
                    new.add(u)
        for u in sorted(new):
            where[u] = len(S)
            S.append(u)
        brow, bcol, orig, bcdf = [0], [], [], []
        for v in dst:
            for e in range(int(rowptr[v]), int(rowptr[v + 1])):
                u = int(col[e])
                orig.append(u)
                bcol.append(where[u] if 0 <= u < n else where[0])
                if cdf is not None:
                    bcdf.append(int(cdf[e]))
            brow.append(len(bcol))
        blocks[l] = RefBlock(np.array(brow, dtype=np.int64), np.array(bcol, dtype=np.int32),
                             np.array(orig, dtype=np.int64), None if cdf is None else np.array(bcdf, dtype=np.int64),
                             len(dst), len(S), where[0])
        sets[l - 1] = np.array(S, dtype=np.int64)
    return RefClosure([sets[l] for l in range(depth + 1)], blocks, index, bad)


def assert_equal(got, ref, what, n=None, cdf=False):
    """infer.Closure `got` (CPU or CUDA tensors) is `ref`, integer for integer."""
    assert got.depth == len(ref.sets) - 1, what
    for l, want in enumerate(ref.sets):
        have = got.sets[l].cpu().numpy()
        assert have.dtype == np.int64 and np.array_equal(have, want), (what, "S_%d" % l, have[:20], want[:20])
    assert np.array_equal(got.index.cpu().numpy(), ref.index), (what, "index")
    assert got.blocks[0] is None
    for l in range(1, got.depth + 1):
        b, r = got.blocks[l], ref.blocks[l]
        assert (b.n_dst, b.n_src, b.dummy, b.n_rows) == (r.n_dst, r.n_src, r.dummy, r.n_dst), (what, "block %d sizes" % l)
        assert np.array_equal(b.rowptr.cpu().numpy(), r.rowptr), (what, "block %d rowptr" % l)
        col = b.col.cpu().numpy()
        assert col.dtype == np.int32 and np.array_equal(col, r.col), (what, "block %d col" % l)
        # every edge names the node the stored row names (an id outside the graph: the dummy)
        src = ref.sets[l - 1][col]
        ok = (r.orig >= 0) & (r.orig < (n if n is not None else np.iinfo(np.int64).max))
        assert np.array_equal(src[ok], r.orig[ok]) and (src[~ok] == 0).all(), (what, "block %d edges" % l)
        if cdf:
            assert np.array_equal(b.edge_cdf.cpu().numpy(), r.cdf), (what, "block %d cdf" % l)
        else:
            assert b.edge_cdf is None
