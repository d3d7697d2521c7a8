"""The definition of exact link ranking by inner product (include/gsage.h, "Exact link ranking over embeddings") in numpy
float64, and the interval a floating-point result is held to.

    rank(q) = 1 + |{ j allowed for q, j != t : (s(q, j), j) beats (s(q, t), t) }|,  t = target_ids[q]; "beats": score
    descending, row id ascending; a NaN score beats nothing; a target out of range or with a NaN score: rank 0.
    Excluded for q: ({query_ids[q]} u the CSR row's columns) minus {t}.

Operands are rounded the way the mode under test sees them (retrieve_ref.round_operand).
"""
import numpy as np

import retrieve_ref as rr


def allowed_mask(Q, N, target_ids, exclude="none", query_ids=None, rowptr=None, col=None):
    """Rows that may count against the target: retrieve_ref's exclusion, and never the target itself."""
    ok = rr.allowed_mask(Q, N, exclude, query_ids, rowptr, col)
    for q, t in enumerate(np.asarray(target_ids, dtype=np.int64)):
        if 0 <= t < N:
            ok[q, t] = False
    return ok


def rank_ref(E, Qm, target_ids, mode, exclude="none", query_ids=None, rowptr=None, col=None):
    """-> (rank int64 [Q], score float64 [Q] (-inf: target out of range), S float64 [Q, N], allowed bool [Q, N])"""
    S = rr.scores64(E, Qm, mode)
    Q, N = S.shape
    tg = np.asarray(target_ids, dtype=np.int64)
    ok = allowed_mask(Q, N, tg, exclude, query_ids, rowptr, col)
    rank = np.zeros(Q, dtype=np.int64)
    score = np.full(Q, -np.inf)
    ids = np.arange(N)
    for q in range(Q):
        t = tg[q]
        if not 0 <= t < N:
            continue
        score[q] = S[q, t]
        if np.isnan(S[q, t]):
            continue
        with np.errstate(invalid="ignore"):
            beats = (S[q] > S[q, t]) | ((S[q] == S[q, t]) & (ids < t))
        rank[q] = 1 + int((beats & ok[q]).sum())
    return rank, score, S, ok


def rank_interval(E, Qm, target_ids, mode, exclude="none", query_ids=None, rowptr=None, col=None):
    """The interval [lo, hi] every rank must lie in on floating-point data, with eps(q, j) = 4 * D * 2^-24 * |q| * |e_j|
    exactly as retrieve_ref.check_tolerance derives it (any order of fp32 accumulation of D terms, times 4 for the
    rounded products and a truncating accumulator):
        lo = 1 + #{allowed j != t : S_j - eps_j > S_t + eps_t}      rows that beat the target whatever the rounding
        hi = 1 + #{allowed j != t : S_j + eps_j >= S_t - eps_t}     rows that may
    -> (lo, hi, ref) int64 [Q]; ref = the float64 rank."""
    ref, _, S, ok = rank_ref(E, Qm, target_ids, mode, exclude, query_ids, rowptr, col)
    Er, Qr = rr.round_operand(E, mode).astype(np.float64), rr.round_operand(Qm, mode).astype(np.float64)
    D = Er.shape[1]
    en, qn = np.linalg.norm(Er, axis=1), np.linalg.norm(Qr, axis=1)
    tg = np.asarray(target_ids, dtype=np.int64)
    Q = S.shape[0]
    lo, hi = np.zeros(Q, dtype=np.int64), np.zeros(Q, dtype=np.int64)
    for q in range(Q):
        t = tg[q]
        eps = 4.0 * D * 2.0 ** -24 * qn[q] * en
        lo[q] = 1 + int((ok[q] & (S[q] - eps > S[q, t] + eps[t])).sum())
        hi[q] = 1 + int((ok[q] & (S[q] + eps >= S[q, t] - eps[t])).sum())
    assert (lo <= ref).all() and (ref <= hi).all()
    return lo, hi, ref


def ascending_csr(rowptr, col):
    """The same edges with every row's columns strictly ascending (sorted, duplicates dropped)."""
    rows = [np.unique(col[rowptr[v]:rowptr[v + 1]]) for v in range(len(rowptr) - 1)]
    new_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return new_ptr, np.concatenate(rows).astype(np.int32)
