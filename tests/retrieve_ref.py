"""The definition of top-k retrieval by inner product (include/gsage.h, "Retrieval over embeddings") in numpy float64,
and the tolerance rules a floating-point result is held to.

    s(q, j) = sum_d Qm[q, d] * E[j, d] over the ALLOWED rows j; the k best under the total order (score descending,
    row id ascending), best first; fewer than k allowed rows: id -1, score -inf; a NaN score is never selected.

Operands are first rounded the way the mode under test sees them: RNE to bf16 for "bf16", untouched fp32 for "fp32".
"""
import numpy as np
import torch


def round_operand(x, mode):
    x = np.ascontiguousarray(x, dtype=np.float32)
    if mode == "bf16":
        return torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    assert mode == "fp32"
    return x


def scores64(E, Qm, mode):
    return round_operand(Qm, mode).astype(np.float64) @ round_operand(E, mode).astype(np.float64).T


def allowed_mask(Q, N, exclude="none", query_ids=None, rowptr=None, col=None):
    ok = np.ones((Q, N), dtype=bool)
    if exclude == "none":
        return ok
    assert exclude in ("self", "neighbours") and query_ids is not None and len(query_ids) == Q
    for q, v in enumerate(np.asarray(query_ids, dtype=np.int64)):
        if 0 <= v < N:
            ok[q, v] = False
            if exclude == "neighbours":
                nb = np.asarray(col[rowptr[v]:rowptr[v + 1]], dtype=np.int64)
                ok[q, nb[(nb >= 0) & (nb < N)]] = False
    return ok


def topk_ref(E, Qm, k, mode, exclude="none", query_ids=None, rowptr=None, col=None):
    """-> (ids int64 [Q, k], scores float64 [Q, k], S float64 [Q, N], allowed bool [Q, N])"""
    S = scores64(E, Qm, mode)
    Q, N = S.shape
    ok = allowed_mask(Q, N, exclude, query_ids, rowptr, col) & ~np.isnan(S)
    ids = np.full((Q, k), -1, dtype=np.int64)
    sc = np.full((Q, k), -np.inf, dtype=np.float64)
    for q in range(Q):
        cand = np.flatnonzero(ok[q])                                   # ascending ids
        best = cand[np.argsort(-S[q, cand], kind="stable")][:k]        # stable: ties keep ascending ids
        ids[q, :best.size] = best
        sc[q, :best.size] = S[q, best]
    return ids, sc, S, ok


def check_tolerance(got_ids, got_scores, E, Qm, k, mode, exclude="none", query_ids=None, rowptr=None, col=None,
                    min_unambiguous=0.6):
    """The rules of a floating-point result (every query, none skipped).  eps(q, j) = 4 * D * 2^-24 * |q| * |e_j|:
    any order of fp32 accumulation of D terms errs by at most D * 2^-24 * sum|a_d b_d| <= D * 2^-24 * |a| |b|; the
    factor 4 covers the rounded products of the fp32 mode and an accumulator that truncates instead of rounding.
    -> the fraction of queries whose reference gap between rank k and rank k + 1 exceeds 4 eps (their id SETS must
    equal the reference's), asserted to be at least min_unambiguous."""
    got_ids = np.asarray(got_ids, dtype=np.int64)
    got_scores = np.asarray(got_scores, dtype=np.float64)
    ref_ids, _, S, ok = topk_ref(E, Qm, k, mode, exclude, query_ids, rowptr, col)
    Er, Qr = round_operand(E, mode).astype(np.float64), round_operand(Qm, mode).astype(np.float64)
    Q, N = S.shape
    D = Er.shape[1]
    en, qn = np.linalg.norm(Er, axis=1), np.linalg.norm(Qr, axis=1)
    assert got_ids.shape == (Q, k) and got_scores.shape == (Q, k)
    clear = 0
    for q in range(Q):
        eps = 4.0 * D * 2.0 ** -24 * qn[q] * en                       # per row j
        n_ok = int(ok[q].sum())
        n_ret = min(k, n_ok)
        ids, sc = got_ids[q], got_scores[q]
        assert (ids[n_ret:] == -1).all() and np.isneginf(sc[n_ret:]).all(), (q, "tail")
        ids, sc = ids[:n_ret], sc[:n_ret]
        assert ((ids >= 0) & (ids < N)).all() and np.unique(ids).size == n_ret, (q, "ids distinct and in range")
        assert ok[q, ids].all(), (q, "an excluded row was returned")
        assert (np.abs(sc - S[q, ids]) <= eps[ids]).all(), (q, float(np.abs(sc - S[q, ids]).max()), float(eps.max()))
        d = np.diff(sc)
        assert (d <= 0).all(), (q, "scores increase")
        assert (np.diff(ids)[d == 0] > 0).all(), (q, "equal scores must carry ascending ids")
        if n_ret < n_ok:
            t = int(np.argmin(S[q, ids]))
            out = ok[q].copy()
            out[ids] = False
            j = np.flatnonzero(out)
            # a row left out lost to EVERY returned row in the kernel's arithmetic: s*_j - eps_j <= s*_t + eps_t
            worst = S[q, j] - (S[q, ids[t]] + eps[j] + eps[ids[t]])
            assert (worst <= 0).all(), (q, "a better row was left out by", float(worst.max()))
            order = np.flatnonzero(ok[q])
            order = order[np.argsort(-S[q, order], kind="stable")]
            a, b = order[k - 1], order[k]
            if S[q, a] - S[q, b] > 4.0 * max(eps[a], eps[b]):
                clear += 1
                assert set(ids.tolist()) == set(ref_ids[q].tolist()), (q, "id set differs from the reference")
        else:
            clear += 1
            assert set(ids.tolist()) == set(ref_ids[q, :n_ret].tolist()), (q, "id set differs from the reference")
    frac = clear / float(Q)
    assert frac >= min_unambiguous, "only %.0f %% of the queries have a clear gap at rank k" % (100 * frac)
    return frac


# ---- shared data ------------------------------------------------------------------------------------------------------
def integer_case(N, Q, D, seed=0):
    """Entries in {-1, 0, 1}: every product and partial sum is exact in bf16 and in fp32, in any order; the scores are
    small integers and many rows tie."""
    rng = np.random.RandomState(seed)
    return rng.randint(-1, 2, size=(N, D)).astype(np.float32), rng.randint(-1, 2, size=(Q, D)).astype(np.float32)


def unit_rows(N, D, seed):
    x = np.random.RandomState(seed).normal(size=(N, D))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def hub_csr(N=50):
    """One hub row (2) of degree 40 with unsorted columns and one duplicate, one row of degree 0 (5), one self-loop
    (9), degree 3 elsewhere.  -> (rowptr int64 [N + 1], col int32)"""
    rng = np.random.RandomState(3)
    rows = []
    for v in range(N):
        if v == 2:
            c = rng.permutation(N)[:39]
            c = np.concatenate([c, c[:1]])                                  # a duplicate column; stays unsorted
        elif v == 5:
            c = np.zeros(0, dtype=np.int64)
        elif v == 9:
            c = np.array([30, 9, 4])
        else:
            c = rng.randint(0, N, size=3)
        rows.append(np.asarray(c, dtype=np.int32))
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return rowptr, np.concatenate(rows).astype(np.int32)
