"""The restatement the weighted-walk tests compare against (test infrastructure): gsage_unsup_batch_weighted written from
the comment of include/gsage.h in Python integers -- the table and the test graph are weighted_ref's, Philox, the walk
lengths and the negatives are unsup_ref's; no code of the product.  The step's draw is written out from the header's
formula AND checked against weighted_ref.draw_x (the same 128-bit product under another counter layout and tag).

  build_batch   -> (ids, pair_w, err); asserts that no step lands through an edge of quantum 0
  rounds        how many round trips the wave's search takes for a row of a given degree, at the least and at the most
  deep_graph    rows of degree 4096, 4097 and 262 145 (past 64^3) whose first edges are heavy, so that draws fall into
                the first sixty-fourth of a range (the longest searches) as well as anywhere else
  seeds_on_rows seeds that start a walk on every arranged row of a graph
"""
import numpy as np

import unsup_ref
import weighted_ref as wr

TAG_WSTEP = 0x5A000000


def build_batch(rowptr, col, ecdf, n_rows, seeds, walk_len, Q, cdf, seed, call, g0=0, trace=None):
    """-> (ids int64 [2B + Q], pair_w float32 [B], err flag);  trace: a list that receives (degree of the row, position
    of the drawn edge in it) for every step taken"""
    rowptr, col, seeds = np.asarray(rowptr), np.asarray(col), np.asarray(seeds)
    ecdf = np.asarray(ecdf, dtype=np.uint64)
    B = len(seeds)
    ids = np.zeros(2 * B + Q, dtype=np.int64)
    pair_w = np.zeros(B, dtype=np.float32)
    err = 0
    for i in range(B):
        s, g = int(seeds[i]), g0 + i
        if not 0 <= s < n_rows:
            err = 1
            continue                                     # ids[i] = ids[B + i] = 0, pair_w[i] = 0
        t = 1 + ((unsup_ref._P(g, call, seed, unsup_ref.TAG_LEN)[0] * walk_len) >> 32)
        v = s
        for j in range(t):
            beg, end = int(rowptr[v]), int(rowptr[v + 1])
            T = int(ecdf[end - 1]) if end > beg else 0
            if T == 0:
                break
            tag = TAG_WSTEP | (j >> 1)
            w = unsup_ref._P(g, call, seed, tag)
            k = 2 * (j & 1)
            x = (((w[k] << 32) | w[k + 1]) * T) >> 64
            # weighted_ref's 128-bit draw reads block g' >> 1 under ITS tag: the same words for g' = 2 g + (j & 1) and
            # a seed whose high word carries the difference of the two tags
            assert x == wr.draw_x(seed ^ ((tag ^ wr.TAG) << 32), call, 2 * g + (j & 1), T)
            e = beg + int(np.flatnonzero(ecdf[beg:end] > np.uint64(x))[0])            # a linear scan, on purpose
            assert int(ecdf[e]) - (int(ecdf[e - 1]) if e > beg else 0) > 0, ("a step through an edge of quantum 0", v, e)
            if trace is not None:
                trace.append((end - beg, e - beg))
            v = int(col[e])
            if not 0 <= v < n_rows:
                err, v = 1, 0
                break
        ids[i], ids[B + i], pair_w[i] = s, v, 0.0 if v == s else 1.0
    # the negatives: exactly the unweighted builder's (the walks of that call are thrown away)
    plain, _, _ = unsup_ref.build_batch(rowptr, col, n_rows, np.zeros(1, dtype=np.int64), 1, Q, cdf, seed, call)
    ids[2 * B:] = plain[2:]
    return ids, pair_w, err


def neg_table(rowptr, ecdf):
    """float64 [n]: the running sum of degree^0.75 with weight 0 for a row whose T_v is 0"""
    rowptr = np.asarray(rowptr)
    deg = np.diff(rowptr).astype(np.float64)
    for v in range(len(deg)):
        if deg[v] > 0 and int(ecdf[rowptr[v + 1] - 1]) == 0:
            deg[v] = 0.0
    return np.cumsum(deg ** 0.75)


def rounds(deg):
    """(fewest, most) round trips of a search that narrows a range of more than 64 entries to one sixty-fourth per
    round of 64 evenly spaced probes and reads a range of at most 64 entries in one: the sub-range of the first probe
    keeps its left end (one entry more than the others), so the most is reached by draws that stay in front."""
    def go(n, first):
        r = 1
        while n > 64:
            span = n - 1
            n = (span >> 6) + 1 if first else (span * 2 >> 6) - (span >> 6)
            r += 1
        return r
    return go(deg, False), go(deg, True)


DEEP_ROWS = {4096: 0, 4097: 1, 262145: 2, "short": (3, 4, 5, 6, 7)}
_DEEP = []


def deep_graph():
    """8 rows: degrees 4096, 4097, 262 145, then 3, 64, 65, 130 and 1.  A tenth of the weights are zero, the first two
    edges of every deep row carry a quarter of the row's weight each, every column points into the 8 rows."""
    if _DEEP:
        return _DEEP[0]
    rng = np.random.RandomState(64)
    degs = [4096, 4097, 262145, 3, 64, 65, 130, 1]
    rows = []
    for d in degs:
        w = np.exp(rng.normal(size=d) * 1.5).astype(np.float32)
        w[rng.rand(d) < 0.1] = 0.0
        if d > 1000:
            w[0] = w[1] = np.float32(0.5 * float(w[2:].sum(dtype=np.float64)))
        elif d == 1:
            w[0] = 1.0
        else:
            w[rng.randint(d)] = 3.0
        rows.append(w)
    rowptr = np.concatenate([[0], np.cumsum(degs)]).astype(np.int64)
    weight = np.concatenate(rows).astype(np.float32)
    col = rng.randint(0, len(degs), size=int(rowptr[-1])).astype(np.int32)
    g = wr.Graph(rowptr, col, weight)
    assert [rounds(d)[1] for d in (64, 65, 4096, 4097, 262145)] == [1, 2, 2, 3, 4]
    assert [rounds(d)[0] for d in (65, 4096, 4097, 262145)] == [2, 2, 2, 3]
    _DEEP.append(g)
    return g


def seeds_on_rows(g, B, rng, rows=None):
    """B seeds: the arranged rows first (as many as fit), the rest uniform"""
    rows = list(wr.ROWS.values()) if rows is None else list(rows)
    s = rng.randint(0, g.n, size=B).astype(np.int64)
    k = min(B, len(rows))
    s[:k] = rows[:k]
    return s
