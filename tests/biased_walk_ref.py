"""The restatement the biased-walk tests compare against (test infrastructure): gsage_unsup_batch_biased and
gsage_importance_walks_biased written from the comment of include/gsage.h ("Biased walks") in Python integers on
oracle.cpu.philox4x32_10 -- no code of the product.  Membership is a Python loop over the stored columns of the previous
node's row; walk lengths and negatives are unsup_ref's, the per-edge table weighted_ref's.

  thresholds    (theta_return, theta_near, theta_far, theta_restart) from the header's double formula
  build_batch   -> (ids, pair_w, err); trace receives one (rounds used, accepted, scanned) per second-order step
  ranked / rows the importance walks -> ranked lists / padded rows; trace counts steps and restarts
  gadget_graph  the membership-scan graph: previous-node rows of degree 1 .. 1000 with the candidate first, last,
                absent or repeated;  star_graph: a hub and its pendant leaves;  six_rows: every class, a repeated column
"""
import math

import numpy as np

import unsup_ref
import weighted_ref as wr
from oracle import cpu as ocpu

TAG_BIAS, TAG_WSTEP, TAG_IMPORTANCE = 0x42000000, 0x5A000000, 0x49000000
M32 = 0xFFFFFFFF
ROUNDS = 32
SEED = 0x1234567887654321
PAIRS = [(4.0, 0.25), (0.25, 4.0), (2.0, 0.5), (0.125, 8.0), (8.0, 0.125)]


def thresholds(p, q, restart=0.0):
    a = (1.0 / p, 1.0, 1.0 / q)
    a_max = max(a)
    th = [1 << 32 if x == a_max else int(math.floor((x / a_max) * 4294967296.0)) for x in a]
    return th[0], th[1], th[2], int(math.floor(restart * 4294967296.0))


def _stored(rowptr, col, t, x):
    for e in range(int(rowptr[t]), int(rowptr[t + 1])):                     # a linear scan, on purpose
        if int(col[e]) == x:
            return True
    return False


def _theta(th, rowptr, col, t, x):
    """-> (theta of x's class after the previous node t, whether only the row of t could tell for this word range)"""
    if x == t:
        return th[0], False
    return (th[1] if _stored(rowptr, col, t, x) else th[2]), th[1] != th[2]


def _first_order(rowptr, col, ecdf, v, words, wide):
    """the first-order step from v: words = (w0, w1) of the proposal; wide: importance's 64-bit uniform rule.
    -> the stored id, or None for a dead end"""
    beg, end = int(rowptr[v]), int(rowptr[v + 1])
    deg = end - beg
    if deg <= 0:
        return None
    r64 = (words[0] << 32) | words[1]
    if ecdf is not None:
        T = int(ecdf[end - 1])
        if T == 0:
            return None
        x = (r64 * T) >> 64
        return int(col[next(e for e in range(beg, end) if int(ecdf[e]) > x)])
    if wide:
        return int(col[beg + ((r64 * deg) >> 64)])
    return int(col[beg + ((words[0] * deg) >> 32 if deg <= 2 ** 32 - 1 else words[0])])


# ---- the builder -------------------------------------------------------------------------------------------------------
def build_batch(rowptr, col, ecdf, n_rows, seeds, walk_len, Q, cdf, seed, call, p, q, g0=0, trace=None):
    """ecdf: the per-edge table (uint64 [nnz]) or None for uniform proposals.
    -> (ids int64 [2B + Q], pair_w float32 [B], err flag)"""
    rowptr, col, seeds = np.asarray(rowptr), np.asarray(col), np.asarray(seeds)
    th = thresholds(p, q)
    B = len(seeds)
    ids = np.zeros(2 * B + Q, dtype=np.int64)
    pair_w = np.zeros(B, dtype=np.float32)
    err = 0
    for i in range(B):
        s, g = int(seeds[i]), g0 + i
        if not 0 <= s < n_rows:
            err = 1
            continue
        t_i = 1 + ((unsup_ref._P(g, call, seed, unsup_ref.TAG_LEN)[0] * walk_len) >> 32)
        v, prev = s, None
        for j in range(t_i):
            x = None
            for k in range(ROUNDS):
                Bk = unsup_ref._P(g, call, seed, TAG_BIAS | (j << 8) | k)
                if k > 0:
                    words = (Bk[0], Bk[1])
                elif ecdf is not None:
                    w = unsup_ref._P(g, call, seed, TAG_WSTEP | (j >> 1))
                    words = (w[2 * (j & 1)], w[2 * (j & 1) + 1])
                else:
                    words = (unsup_ref._P(g, call, seed, unsup_ref.TAG_STEP | (j >> 2))[j & 3], 0)
                x = _first_order(rowptr, col, ecdf, v, words, False)
                if x is None or not 0 <= x < n_rows or prev is None:
                    break
                theta, band = _theta(th, rowptr, col, prev, x)
                ok = Bk[2] < theta
                if ok or k == ROUNDS - 1:
                    if trace is not None:
                        trace.append((k + 1, ok, band and min(th[1], th[2]) <= Bk[2] < max(th[1], th[2])))
                    break
            if x is None:                                  # a dead end: the walk ends at v
                break
            if not 0 <= x < n_rows:
                err, v = 1, 0
                break
            prev, v = v, x
        ids[i], ids[B + i], pair_w[i] = s, v, 0.0 if v == s else 1.0
    plain, _, _ = unsup_ref.build_batch(rowptr, col, n_rows, np.zeros(1, dtype=np.int64), 1, Q, cdf, seed, call)
    ids[2 * B:] = plain[2:]
    return ids, pair_w, err


# ---- importance ----------------------------------------------------------------------------------------------------------
def ranked(rowptr, col, cdf, n_rows, v, R, L, seed, p, q, restart, trace=None):
    """-> ([(node, count)] of source v in the total order, err);  trace: a dict whose "steps" (steps s >= 1 of walks
    still going) and "restarts" are counted up"""
    v = int(v)
    if v < 0 or v >= n_rows:
        return [], 1
    th = thresholds(p, q, restart)
    counts, err = {}, 0
    key = (seed & M32, ((seed >> 32) & M32) ^ TAG_IMPORTANCE)
    for r in range(R):
        u, prev = v, None
        for s in range(L):
            N0 = ocpu.philox4x32_10((v & M32, r, s, 1), key)
            if s >= 1:
                if trace is not None:
                    trace["steps"] = trace.get("steps", 0) + 1
                if N0[3] < th[3]:
                    if trace is not None:
                        trace["restarts"] = trace.get("restarts", 0) + 1
                    u, prev = v, None
                    continue
            x = None
            for k in range(ROUNDS):
                Nk = N0 if k == 0 else ocpu.philox4x32_10((v & M32, r, s, 1 + k), key)
                if k == 0:
                    w = ocpu.philox4x32_10((v & M32, r, s >> 1, 0), key)
                    words = (w[2 * (s & 1)], w[2 * (s & 1) + 1])
                else:
                    words = (Nk[0], Nk[1])
                x = _first_order(rowptr, col, cdf, u, words, True)
                if x is None or not 0 <= x < n_rows or prev is None:
                    break
                if Nk[2] < _theta(th, rowptr, col, prev, x)[0]:
                    break
            if x is None:
                break
            if not 0 <= x < n_rows:
                err = 1
                break
            prev, u = u, x
            if u != v:
                counts[u] = counts.get(u, 0) + 1
    return sorted(counts.items(), key=lambda kv: (-kv[1], kv[0])), err


_ROWS = {}


def rows(g, weighted, ids, R, L, T, p, q, restart, seed=SEED):
    """gsage_importance_walks_biased over graph g -> (col int32 [M, T], w fp32 [M, T], deg int32 [M], err).  A
    source's ranked list is computed once per (graph, mode, R, L, p, q, restart, seed)."""
    M = len(ids)
    col, w, deg, err = np.zeros((M, T), np.int32), np.zeros((M, T), np.float32), np.zeros(M, np.int32), 0
    for i, v in enumerate(ids):
        key = (id(g), bool(weighted), int(v), R, L, p, q, restart, seed)
        if key not in _ROWS:                              # (the entry keeps g alive: its id stays its own)
            _ROWS[key] = ranked(g.rowptr, g.col, g.cdf if weighted else None, g.n, v, R, L, seed, p, q, restart) + (g,)
        lst, e, _ = _ROWS[key]
        err |= e
        k = min(T, len(lst))
        deg[i] = k
        for j in range(k):
            col[i, j], w[i, j] = lst[j][0], lst[j][1]
    return col, w, deg, err


# ---- graphs ----------------------------------------------------------------------------------------------------------------
def _graph(rows_, weights=None):
    deg = np.array([len(r) for r in rows_], dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = np.array([u for r in rows_ for u in r], dtype=np.int32)
    if weights is None:
        weight = np.ones(len(col), dtype=np.float32)
    else:
        weight = np.array([x for r in weights for x in r], dtype=np.float32)
    return wr.Graph(rowptr, col, weight)


GADGET_DEGREES = (1, 63, 64, 65, 128, 129, 255, 256, 257, 1000)     # (a trip of the scan: 4 loads of 64 columns)
PLACEMENTS = ("first", "last", "absent", "repeated")
_CACHE = {}


def gadget_graph():
    """One gadget of four nodes (t, v, x, y) per (degree of row t, placement of x in it): row t holds v everywhere but
    where x sits (in the weighted reading those entries weigh 0: stored, never drawn), row v = [x, y], x and y are dead
    ends.  A walk from t steps to v and then chooses between x -- near exactly when row t stores it -- and y, far.
    -> (Graph, [(t, degree, placement)])"""
    if "gadget" in _CACHE:
        return _CACHE["gadget"]
    rows_, weights, cases = [], [], []
    rng = np.random.RandomState(3)
    for d in GADGET_DEGREES:
        for place in PLACEMENTS:
            if d == 1 and place != "absent":
                continue
            t = len(rows_)
            v, x, y = t + 1, t + 2, t + 3
            row = [v] * d
            at = {"first": [0], "last": [d - 1], "absent": [], "repeated": [0, d // 2, d - 1]}[place]
            for k in at:
                row[k] = x
            rows_ += [row, [x, y], [], []]
            weights += [[0.0 if u == x else float(rng.uniform(0.5, 2.0)) for u in row], [1.0, 1.0], [], []]
            cases.append((t, d, place))
    _CACHE["gadget"] = (_graph(rows_, weights), cases)
    return _CACHE["gadget"]


def star_graph(leaves=5):
    """node 0 the hub, nodes 1..leaves pendant: their only neighbour is the hub"""
    if ("star", leaves) not in _CACHE:
        _CACHE[("star", leaves)] = _graph([list(range(1, leaves + 1))] + [[0]] * leaves)
    return _CACHE[("star", leaves)]


SIX = dict(t=0, v=1, a=2, b=3, c=4, d=5)


def six_rows():
    """row(t) = [v, a, b], row(v) = [t, a, b, c, d, d]; a, b, c, d are dead ends"""
    return [[1, 2, 3], [0, 2, 3, 4, 5, 5], [], [], [], []]


def six_probabilities(p, q):
    """the exact node2vec distribution of the step from v after t: {node: a_class * multiplicity / sum}"""
    a = {0: 1.0 / p, 2: 1.0, 3: 1.0, 4: 1.0 / q, 5: 2.0 / q}
    total = sum(a.values())
    return {u: x / total for u, x in a.items()}
