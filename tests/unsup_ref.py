"""Restatements the unsupervised-GraphSAGE tests compare against (test infrastructure):

  build_batch   the batch builder of include/gsage.h ("Unsupervised GraphSAGE"), written from that comment's formula in
                numpy / Python integers on top of oracle.cpu.philox4x32_10 -- no code shared with the product
  head          the skip-gram head's definition in torch float64 autograd
  walk_graph    the 60-node CSR of the builder tests;  model_problem  the 200-node problem of the model tests
"""
import numpy as np
import torch

from oracle import cpu as ocpu

TAG_LEN, TAG_STEP, TAG_NEG = 0x4C000000, 0x53000000, 0x4E000000
M32 = 0xFFFFFFFF


def _P(c, call, seed, tag):
    return ocpu.philox4x32_10([c & M32, (c >> 32) & M32, call & M32, (call >> 32) & M32],
                              [seed & M32, ((seed >> 32) & M32) ^ tag])


def build_batch(rowptr, col, n_rows, seeds, walk_len, Q, cdf, seed, call, g0=0):
    """-> (ids int64 [2B + Q], pair_w float32 [B], err flag)"""
    rowptr, col, seeds = np.asarray(rowptr), np.asarray(col), np.asarray(seeds)
    cdf = np.asarray(cdf, dtype=np.float64)
    B = len(seeds)
    ids = np.zeros(2 * B + Q, dtype=np.int64)
    pair_w = np.zeros(B, dtype=np.float32)
    err = 0
    for i in range(B):
        s, g = int(seeds[i]), g0 + i
        if not 0 <= s < n_rows:
            err = 1
            continue                                     # ids[i] = ids[B + i] = 0, pair_w[i] = 0
        t = 1 + ((_P(g, call, seed, TAG_LEN)[0] * walk_len) >> 32)
        v = s
        for j in range(t):
            beg = int(rowptr[v])
            deg = int(rowptr[v + 1]) - beg
            if deg <= 0:
                break
            word = _P(g, call, seed, TAG_STEP | (j >> 2))[j & 3]
            off = (word * deg) >> 32 if deg <= 2 ** 32 - 1 else word
            v = int(col[beg + off])
            if not 0 <= v < n_rows:
                err, v = 1, 0
                break
        ids[i], ids[B + i], pair_w[i] = s, v, 0.0 if v == s else 1.0
    total = cdf[n_rows - 1]
    for q in range(Q):
        r = _P(q, call, seed, TAG_NEG)
        u = np.float64((r[0] << 21) | (r[1] >> 11)) * np.float64(2.0 ** -53)
        x = u * total
        first = next((i for i in range(n_rows) if cdf[i] > x), n_rows - 1)          # a linear scan, on purpose
        ids[2 * B + q] = min(first, n_rows - 1)
    return ids, pair_w, err


def degree_cdf(rowptr):
    deg = np.diff(np.asarray(rowptr)).astype(np.float64)
    return np.cumsum(deg ** 0.75)


def head(E, B, Q, pair_w, neg_weight):
    """float64 autograd of the head's definition -> (loss, aff [B, 1 + Q], dE), all float64 tensors"""
    E = E.detach().double().clone().requires_grad_(True)
    w = pair_w.detach().double()
    z = E / E.norm(dim=1, keepdim=True).clamp(min=1e-12)
    a = (z[:B] * z[B:2 * B]).sum(1)
    n = z[:B] @ z[2 * B:2 * B + Q].t()
    # softplus(x) = log(1 + e^x), written smooth: the kinks of max(x, 0) and |x| would hand autograd the derivative 1
    # instead of sigmoid(0) = 1/2 at an affinity of exactly 0 (an all-zero row); |x| <= 1 here, nothing overflows
    softplus = lambda x: torch.log1p(torch.exp(x))                                # noqa: E731
    loss = ((w * softplus(-a)).sum() + neg_weight * softplus(n).sum()) / B
    loss.backward()
    return loss.detach(), torch.cat([a.unsqueeze(1), n], 1).detach(), E.grad.detach()


def walk_graph():
    """60 nodes: 0 and 7 have no edges, 5 has only a self-loop, 10 -> 11 -> ... -> 15 -> 10 is a chain of degree 1,
    20 has 300 edges, every other node 1..6.  -> (rowptr int64 [61], col int32 [nnz])"""
    rng = np.random.RandomState(11)
    n = 60
    rows = []
    for v in range(n):
        if v in (0, 7):
            rows.append([])
        elif v == 5:
            rows.append([5])
        elif 10 <= v <= 15:
            rows.append([v + 1 if v < 15 else 10])
        elif v == 20:
            rows.append(list(rng.randint(1, n, size=300)))
        else:
            rows.append(list(rng.randint(1, n, size=rng.randint(1, 7))))
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]).astype(np.int32)
    return rowptr, col


def model_problem():
    """The model tests' problem: 200 rows (row 0 the dummy) in the reference's sparse convention, 16-d features, folds,
    and one fixed explicit batch (B = 64, Q = 20) built by build_batch above.
    -> dict(adj, feats, folds, targets, batch_ids, pair_w)"""
    from scipy import sparse
    rng = np.random.RandomState(5)
    n, D = 200, 16
    deg = rng.randint(1, 9, size=n)
    deg[0] = 0
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    data = rng.randint(1, n, size=int(indptr[-1]))
    cols = np.arange(indptr[-1]) - np.repeat(indptr[:-1], deg)
    adj = sparse.csr_matrix((data, cols, indptr), shape=(n, int(deg.max())))
    feats = rng.normal(size=(n, D)).astype(np.float32)
    feats[0] = 0
    folds = np.array(["train"] * 140 + ["val"] * 40 + ["test"] * 20)
    targets = rng.randint(0, 3, size=(n, 1))
    seeds = rng.permutation(np.arange(1, n))[:64]
    ids, pair_w, err = build_batch(indptr, data, n, seeds, 5, 20, degree_cdf(indptr), seed=0, call=0)
    assert err == 0
    return {"adj": adj, "feats": feats, "folds": folds, "targets": targets, "batch_ids": ids, "pair_w": pair_w}
