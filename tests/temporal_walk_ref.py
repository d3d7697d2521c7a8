"""The temporal batch builder (include/gsage.h, "Temporal walks") restated from that comment in Python integers: Philox
through unsup_ref._P (oracle.cpu.philox4x32_10), the count through temporal_ref.count (one look at every edge), the
negatives through unsup_ref.build_batch -- no code of the product.  Test infrastructure."""
import numpy as np

import temporal_ref as tr
import unsup_ref as ur

TAG_TSTEP = 0x56000000
RULES = tr.RULES


def build_batch(rowptr, col, etime, n_rows, seeds, times, walk_len, Q, cdf, seed, call, g0=0, inherit="seed", n_valid=None,
                counts=None):
    """-> (ids int64 [2B + Q], pair_w float32 [B], out_times int64 [2B + Q], err flag, traces): traces[i] is the list of
    (node, tau, cnt, off) of walk i, one entry per step it looked at (the last one has cnt == 0 and off None when the
    walk ended early).  counts: a dict (row, t) -> cnt, filled and reused (the serial count of a long row is slow)."""
    assert inherit in RULES
    B = len(seeds)
    ids = np.zeros(2 * B + Q, dtype=np.int64)
    out_times = np.zeros(2 * B + Q, dtype=np.int64)
    pair_w = np.zeros(B, dtype=np.float32)
    err, traces = 0, []
    for i in range(B):
        s, tau, g = int(seeds[i]), int(times[i]), g0 + i
        out_times[i] = out_times[B + i] = tau
        trace = []
        traces.append(trace)
        if not 0 <= s < n_rows:
            err = 1
            continue                                     # ids[i] = ids[B + i] = 0, pair_w[i] = 0
        t = 1 + ((ur._P(g, call, seed, ur.TAG_LEN)[0] * walk_len) >> 32)
        v = s
        for j in range(t):
            beg, end = int(rowptr[v]), int(rowptr[v + 1])
            if counts is not None and (v, tau) in counts:
                cnt = counts[(v, tau)]
            else:
                cnt = tr.count(etime, beg, end, tau) if end - beg < 2 ** 32 else 0
                if counts is not None:
                    counts[(v, tau)] = cnt
            if end - beg >= 2 ** 32:
                err = 1
            if cnt == 0:
                trace.append((v, tau, 0, None))
                break
            word = ur._P(g, call, seed, TAG_TSTEP | (j >> 2))[j & 3]
            off = (word * cnt) >> 32
            trace.append((v, tau, cnt, off))
            v = int(col[beg + off])
            if inherit == "edge":
                tau = int(etime[beg + off])
            if not 0 <= v < n_rows:
                err, v = 1, 0
                break
        ids[i], ids[B + i], pair_w[i] = s, v, 0.0 if v == s else 1.0
    # the negatives: the plain builder's (any in-range seed serves; g0 does not enter)
    neg, _, _ = ur.build_batch(rowptr, col, n_rows, [0], 1, Q, cdf, seed, call)
    ids[2 * B:] = neg[2:]
    b = B if n_valid is None else min(max(int(n_valid), 1), B)
    for q in range(Q):
        out_times[2 * B + q] = int(times[q % b])
    return ids, pair_w, out_times, err, traces


# ---- the grid both test files walk (host mode and the kernel against the same restatement, computed once) -------------
SEED = 0x1234567887654321
CALL_BASE, CALL_CTR, G0 = 3, 2, 5                       # all non-zero; the call index is their sum of the first two
MS, WALK_LENS, QS = (1, 15, 16, 17, 84, 257), (1, 5, 16), (1, 20, 64)
_COUNTS, _REF = {}, {}


def n_valid_of(M, walk_len, Q, rule):
    """the live count a grid case runs with beside NULL: one of 1, 2, B - 1, B, B + 5, a different one from case to case"""
    k = MS.index(M) + WALK_LENS.index(walk_len) + QS.index(Q) + RULES.index(rule)
    return (1, 2, M - 1, M, M + 5)[k % 5]


def degree_cdf():
    return ur.degree_cdf(tr.graph().rowptr)


def reference(M, walk_len, Q, rule, n_valid=None):
    """build_batch on temporal_ref.graph() with the seeds and times temporal_ref.parents(M) and the table degree_cdf()
    (the builder's INPUT: both test files hand the product this very table), computed once per case"""
    key = (M, walk_len, Q, rule, n_valid)
    if key not in _REF:
        g = tr.graph()
        seeds, times = tr.parents(M)
        _REF[key] = build_batch(g.rowptr, g.col, g.etime, g.n, seeds, times, walk_len, Q, degree_cdf(), SEED,
                                CALL_BASE + CALL_CTR, G0, rule, n_valid, _COUNTS)
    return _REF[key]


def table(device="cpu"):
    """degree_cdf() as the tensor ops.unsup_batch_temporal takes (its total attached, as ops.neg_cdf attaches it)"""
    import torch
    cdf = torch.from_numpy(degree_cdf()).to(device)
    cdf._gsage_total = float(degree_cdf()[-1])
    return cdf


# ---- the model of the model tests --------------------------------------------------------------------------------------
def model(p, dims=(16, 8), fans=(3, 2), strategy="uniform", inherit="seed", seed=3, walk_len=3, n_negatives=5,
          sampler="sparse_temporal_neighbor_sampler", adj=None, **kw):
    """GSUnsupervised on temporal_ref.problem() (mean aggregators, identity prep); kw: temporal_walks, weighted_walks, .."""
    from functools import partial

    import torch
    from torch.nn import functional as F

    from conftest import pkg
    gs = pkg()
    torch.manual_seed(seed)
    specs = [{"n_train_samples": f, "n_val_samples": f, "output_dim": h,
              "activation": (lambda x: x) if i == len(dims) - 1 else F.relu} for i, (f, h) in enumerate(zip(fans, dims))]
    cls = gs.find_sampler(sampler)
    if sampler == "sparse_temporal_neighbor_sampler":
        cls = partial(cls, strategy=strategy, inherit=inherit)
    adj = p["tadj"] if adj is None else adj
    return gs.GSUnsupervised(sampler_class=cls, adj=adj, train_adj=adj, prep_class=gs.prep_lookup["identity"],
                             aggregator_class=gs.aggregator_lookup["mean"], input_dim=p["feats"].shape[1],
                             n_nodes=p["n"] + 1, layer_specs=specs, walk_len=walk_len, n_negatives=n_negatives, **kw)
