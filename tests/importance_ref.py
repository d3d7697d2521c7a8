"""What the importance-neighbourhood tests share, written from the definition of include/gsage.h ("Importance
neighbourhoods") in Python integers on oracle.cpu.philox4x32_10 -- no code of the product: the walks, the visit counts
and the top-T under the total order (count descending, id ascending), the per-edge table through
tests/weighted_ref.build_cdf, and the two test graphs."""
import numpy as np

import weighted_ref as wr
from oracle import cpu as ocpu

TAG = 0x49000000
M32 = 0xFFFFFFFF
SEED = 0x0F1E2D3C4B5A6978

# (n_walks, walk_len, top) of the GPU tests and the number of sources each runs with: every 64-lane boundary of the
# walks, every size class of the sorts (64, 256, 512 / 1024 and 4096 slots), the limit n_walks * walk_len = 4096
CASES = [((1, 1, 1), 72), ((10, 2, 3), 72), ((63, 3, 16), 72), ((64, 1, 64), 72), ((65, 5, 8), 3), ((200, 5, 32), 3),
         ((256, 16, 64), 3), ((4096, 1, 64), 1)]


def ranked(rowptr, col, cdf, n_rows, v, R, L, seed):
    """-> ([(node, count)] of source v in the total order, err)"""
    v = int(v)
    if v < 0 or v >= n_rows:
        return [], 1
    counts, err = {}, 0
    key = (seed & M32, ((seed >> 32) & M32) ^ TAG)
    for r in range(R):
        u = v
        for s in range(L):
            if s % 2 == 0:
                w = ocpu.philox4x32_10((v & M32, r, s >> 1, 0), key)
            k = 2 * (s & 1)
            r64 = (w[k] << 32) | w[k + 1]
            b, e = int(rowptr[u]), int(rowptr[u + 1])
            if cdf is None:
                if e - b <= 0:
                    break
                nu = int(col[b + ((r64 * (e - b)) >> 64)])
            else:
                T = int(cdf[e - 1]) if e > b else 0
                if T == 0:
                    break
                x = (r64 * T) >> 64
                nu = int(col[next(j for j in range(b, e) if int(cdf[j]) > x)])
            if nu < 0 or nu >= n_rows:
                err = 1
                break
            u = nu
            if u != v:
                counts[u] = counts.get(u, 0) + 1
    return sorted(counts.items(), key=lambda kv: (-kv[1], kv[0])), err


_ROWS = {}


def rows(g, weighted, ids, R, L, T, seed=SEED):
    """gsage_importance_walks over graph g (a Graph of weighted_ref or of graph_b()) -> (col int32 [M, T], w fp32
    [M, T], deg int32 [M], err, ranked lists).  A source's ranked list is computed once per (graph, mode, R, L, seed)."""
    M = len(ids)
    col, w, deg, err, lists = np.zeros((M, T), np.int32), np.zeros((M, T), np.float32), np.zeros(M, np.int32), 0, []
    for i, v in enumerate(ids):
        key = (id(g), bool(weighted), int(v), R, L, seed)
        if key not in _ROWS:                              # (the entry keeps g alive: its id stays its own)
            _ROWS[key] = ranked(g.rowptr, g.col, g.cdf if weighted else None, g.n, v, R, L, seed) + (g,)
        lst, e, _ = _ROWS[key]
        err |= e
        lists.append(lst)
        k = min(T, len(lst))
        deg[i] = k
        for j in range(k):
            col[i, j], w[i, j] = lst[j][0], lst[j][1]
    return col, w, deg, err, lists


def cases_met(lists, T):
    """which of the cases the tests are for a set of ranked lists holds under `top` = T"""
    met = set()
    for lst in lists:
        d = len(lst)
        if d > T:
            met.add("distinct > T")
            if lst[T - 1][1] == lst[T][1]:
                met.add("tie straddling T")
        elif d == 0:
            met.add("distinct = 0")
        elif d < T:
            met.add("0 < distinct < T")
        if any(lst[j][1] == lst[j + 1][1] for j in range(min(d, T) - 1)):
            met.add("tie inside T")
    return met


ALL_CASES = {"distinct > T", "tie straddling T", "distinct = 0", "0 < distinct < T", "tie inside T"}


# ---- the arranged graph ------------------------------------------------------------------------------------------
B_ROWS = {"degree 0": 0, "cycle": (1, 6), "hub": 10, "leaves": (11, 19), "self loop": 20, "chain": (21, 24),
          "bad edge": 25, "leads to the bad edge": 26}


class GraphB(object):
    def __init__(self, rowptr, col):
        self.rowptr, self.col, self.cdf, self.weight = rowptr, col, None, None
        self.n = len(rowptr) - 1
        self.deg = np.diff(rowptr)


_B = {}


def graph_b(bad=True):
    """40 rows, unweighted: a directed cycle 1 -> 2 -> .. -> 6 -> 1 (equal counts: the id decides); a star, hub 10 ->
    leaves 11..19 -> hub (landings on the source vanish); row 20 whose only edge is a self-loop (an empty result); the
    chain 21 -> 22 -> 23 -> 24, 24 of degree 0 (walks that stop early); row 25 with an edge to n_rows = 40 (the error
    flag; bad=False: to 27 instead) and row 26 leading there; rows 27..39 of random degree 1..5."""
    if bad in _B:
        return _B[bad]
    rng = np.random.RandomState(77)
    n = 40
    rows_ = {v: [] for v in range(n)}
    for v in range(1, 7):
        rows_[v] = [v + 1 if v < 6 else 1]
    rows_[10] = list(range(11, 20))
    for v in range(11, 20):
        rows_[v] = [10]
    rows_[20] = [20]
    rows_[21], rows_[22], rows_[23] = [22], [23], [24]
    rows_[25] = [26, n if bad else 27]
    rows_[26] = [25]
    for v in range(27, n):
        rows_[v] = [int(x) for x in rng.randint(1, 25, size=rng.randint(1, 6))]
    deg = np.array([len(rows_[v]) for v in range(n)], dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = np.array([u for v in range(n) for u in rows_[v]], dtype=np.int32)
    _B[bad] = GraphB(rowptr, col)
    return _B[bad]


def sources(g, M):
    """M source ids of graph g: the rows the arranged cases sit in first, then every row, then repeats"""
    if g.n == 40:
        first = [10, 5, 20, 21, 11, 1, 0, 24, 25, 26]
    else:
        first = [wr.ROWS[1000], wr.ROWS["degree 1"], wr.ROWS["degree 0"], wr.ROWS["all zero"], wr.ROWS[257],
                 wr.ROWS["one drawable of 20"], wr.ROWS["all denormal"]]
    rest = [v for v in range(g.n) if v not in first]
    seq = first + rest
    return np.array([seq[i % len(seq)] for i in range(M)], dtype=np.int64)
