"""Exact link ranking on the MI355X (csrc/gsage_rank.hip behind ops.rank_ip / gs.link_rank) against tests/rank_ref.py:
exact on integer data with ties, tails, bit-identical for every split count, bit-identical scores with gsage_topk_ip, the
filter subtraction, unranked targets, the derived rank interval on random unit rows, and the public path.  No time is
asserted.

The rank-interval figures of test_random_unit_rows_within_the_rank_interval go to GSAGE_PARITY_LOG
(profiles/rank_parity.jsonl); the test prints each figure before it asserts."""
import numpy as np
import pytest
import torch

import rank_ref as kr
import retrieve_ref as rr
from conftest import pkg
from full_neighbour_ref import make_model, sparse_graph
from util import note_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _dtype():
    gs = pkg()
    yield
    gs.ops.set_compute_dtype("bf16")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


_REF = {}


def _integer(D):
    """The integer case of width D, its float64 scores, and per query the row ids best first (exact in both modes)."""
    if D not in _REF:
        E, Qm = rr.integer_case(1001, 33, D, seed=D)
        S = rr.scores64(E, Qm, "fp32")
        _REF[D] = (E, Qm, S)
    return _REF[D]


def _tied_targets(S, rng, most_at_least):
    """Per query: one seeded draw, and one target out of the score value most rows share: the middle one of the rows
    that tie there.  (Scores of D entries in {-1, 0, 1} spread like sqrt(D): at D <= 48 a hundred and more of the 1001
    rows share the commonest value, at D = 256 a few dozen do.)"""
    Q, N = S.shape
    drawn = rng.randint(0, N, size=Q)
    tied = np.zeros(Q, dtype=np.int64)
    most = 0
    for q in range(Q):
        vals, counts = np.unique(S[q], return_counts=True)
        rows = np.flatnonzero(S[q] == vals[np.argmax(counts)])
        most = max(most, rows.size)
        tied[q] = rows[rows.size // 2]
    assert most >= most_at_least
    return drawn, tied


# ---- 1. exact, with ties everywhere ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("D", [40, 48, 256])
def test_exact_on_integer_data_with_ties(D, mode):
    gs = pkg()
    gs.ops.set_compute_dtype(mode)
    E, Qm, S = _integer(D)
    Ed, Qd = _dev(E), _dev(Qm)
    for tg in _tied_targets(S, np.random.RandomState(D), 100 if D <= 48 else 30):
        want_rank, want_sc, _, _ = kr.rank_ref(E, Qm, tg, mode)
        before = gs._native.launch_count()
        rank, sc = gs.ops.rank_ip(Ed, Qd, _dev(tg))
        assert gs._native.launch_count() - before == 2                  # scan + finish, nothing else
        assert rank.dtype == torch.int64 and sc.dtype == torch.float32
        assert torch.equal(rank.cpu(), torch.from_numpy(want_rank))
        assert torch.equal(sc.cpu(), torch.from_numpy(want_sc.astype(np.float32)))
    qid = np.random.RandomState(D + 1).randint(0, 1001, size=33)
    want_rank, want_sc, _, _ = kr.rank_ref(E, Qm, tg, mode, "self", qid)
    before = gs._native.launch_count()
    rank, sc = gs.ops.rank_ip(Ed, Qd, _dev(tg), query_ids=_dev(qid), exclude="self")
    assert gs._native.launch_count() - before == 2                      # "self" is folded into the scan
    assert torch.equal(rank.cpu(), torch.from_numpy(want_rank))
    assert torch.equal(sc.cpu(), torch.from_numpy(want_sc.astype(np.float32)))


# ---- 2. tails ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_tails_and_rows_that_are_not_whole_16_byte_chunks(mode):
    """N and Q around the 32-row tile; D = 45 (no multiple of a chunk in either mode) out of wider buffers whose pad
    columns hold garbage, so that rows start unaligned: nothing past a row's D columns may be read."""
    gs = pkg()
    gs.ops.set_compute_dtype(mode)
    dt = gs.ops.torch_dtype()
    Eall, Qall = rr.integer_case(65, 33, 45, seed=8)
    rng = np.random.RandomState(9)
    for N in (1, 31, 32, 33, 65):
        for Q in (1, 32, 33):
            E, Qm = Eall[:N], Qall[:Q]
            tg, qid = rng.randint(0, N, size=Q), rng.randint(0, N, size=Q)
            want_rank, want_sc, _, _ = kr.rank_ref(E, Qm, tg, mode, "self", qid)
            for ld in (45, 47, 48):
                Eb = torch.full((N, ld), 7.0, dtype=dt, device=DEV)
                Qb = torch.full((Q, ld), -5.0, dtype=dt, device=DEV)
                Eb[:, :45] = _dev(E).to(dt)
                Qb[:, :45] = _dev(Qm).to(dt)
                rank, sc = gs.ops.rank_ip(Eb[:, :45], Qb[:, :45], _dev(tg), query_ids=_dev(qid), exclude="self")
                assert torch.equal(rank.cpu(), torch.from_numpy(want_rank)), (N, Q, ld)
                assert torch.equal(sc.cpu(), torch.from_numpy(want_sc.astype(np.float32))), (N, Q, ld)


# ---- 3. grid independence ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("case", ["integer", "float"])
def test_result_is_bit_identical_for_every_split_count(case, mode):
    gs = pkg()
    gs.ops.set_compute_dtype(mode)
    rng = np.random.RandomState(1)
    if case == "integer":
        E, Qm, _ = _integer(48)
    else:
        E = rng.normal(size=(5003, 256)).astype(np.float32)
        Qm = rng.normal(size=(70, 256)).astype(np.float32)
    N, Q = E.shape[0], Qm.shape[0]
    rowptr, col = kr.ascending_csr(*rr.hub_csr(50))
    rowptr = np.concatenate([rowptr, np.full(N - 50, rowptr[-1])]).astype(np.int64)
    csr = gs.DeviceCSR(_dev(rowptr), _dev(col), N, 40)
    Ed, Qd, tg, qid = _dev(E), _dev(Qm), _dev(rng.randint(0, N, size=Q)), _dev(rng.randint(0, 50, size=Q))
    first = None
    for splits in (1, 3, 7, 0):
        for _ in range(2):
            got = gs.ops.rank_ip(Ed, Qd, tg, query_ids=qid, csr=csr, exclude="neighbours", splits=splits)
            if first is None:
                first = got
            assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1]), splits
        nbytes, used = gs.ops.rank_ip_workspace(Q, N, splits)
        assert nbytes == 4 * Q * (used + 1)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        out = (torch.zeros(Q, dtype=torch.int64, device=DEV), torch.zeros(Q, dtype=torch.float32, device=DEV))
        before = gs._native.launch_count()
        gs.ops.rank_ip(Ed, Qd, tg, query_ids=qid, csr=csr, exclude="neighbours", splits=splits, workspace=ws, out=out)
        assert gs._native.launch_count() - before == 3                  # scan + filter + finish
        assert torch.equal(out[0], first[0]) and torch.equal(out[1], first[1]), splits
    assert int(first[0].min()) >= 1 and int(csr.err_flag.item()) == 0


def test_recorded_in_a_command_list_with_the_callers_workspace():
    gs = pkg()
    E, Qm, S = _integer(48)
    tg = np.random.RandomState(2).randint(0, 1001, size=33)
    want_rank, want_sc, _, _ = kr.rank_ref(E, Qm, tg, "bf16")
    Ed, Qd = _dev(E).to(torch.bfloat16), _dev(Qm).to(torch.bfloat16)
    nbytes, splits = gs.ops.rank_ip_workspace(33, 1001, 3)
    assert splits == 3
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = (torch.zeros(33, dtype=torch.int64, device=DEV), torch.zeros(33, dtype=torch.float32, device=DEV))
    tgd = _dev(tg)
    with gs._native.CommandList.record() as cl:
        gs.ops.rank_ip(Ed, Qd, tgd, splits=3, workspace=ws, out=out)
    assert len(cl) == 2 and int(out[0].abs().sum()) == 0                 # recorded, not run
    cl.replay(gs.ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(out[0].cpu(), torch.from_numpy(want_rank))
    assert torch.equal(out[1].cpu(), torch.from_numpy(want_sc.astype(np.float32)))


# ---- 4. agreement with gsage_topk_ip, bit for bit ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("exclude", ["none", "self"])
def test_rank_and_score_agree_with_topk_ip_bit_for_bit(exclude, mode):
    """Holds the bit-identity invariant: for every pair of rank r <= 128, top-k's entry r - 1 IS the target and carries
    the very same score bits.  Fails if any launch computes a score by another accumulator chain."""
    gs = pkg()
    gs.ops.set_compute_dtype(mode)
    N, D, Q = 5003, 256, 64
    E = rr.unit_rows(N, D, 3)
    nodes = np.random.RandomState(4).randint(0, N, size=Q)
    ref_ids, _, _, _ = rr.topk_ref(E, E[nodes], 128, mode, exclude, nodes)
    emb, nd = _dev(E), _dev(nodes)
    top_ids, top_sc = gs.ops.topk_ip(emb, emb[nd], 128, query_ids=nd, exclude=exclude)
    checked = 0
    for pos in (0, 1, 7, 63, 126, 127):                                 # targets at the reference's ranks 1 .. 128
        tg = _dev(ref_ids[:, pos].copy())
        rank, sc = gs.ops.rank_ip(emb, emb[nd], tg, query_ids=nd, exclude=exclude)
        near = rank <= 128
        assert int(near.sum()) >= Q - 8 and int(rank.min()) >= 1
        at = (rank[near] - 1).view(-1, 1)
        assert torch.equal(top_ids[near].gather(1, at).view(-1), tg[near])
        assert torch.equal(top_sc[near].gather(1, at).view(-1), sc[near])
        checked += int(near.sum())
    assert checked >= 6 * (Q - 8)


# ---- 5. the filter ---------------------------------------------------------------------------------------------------------
def _filter_case():
    N = 50
    rowptr, col = rr.hub_csr(N)
    ap, ac = kr.ascending_csr(rowptr, col)
    assert ap[3] - ap[2] == 39 and ap[6] == ap[5] and 9 in ac[ap[9]:ap[10]]      # hub, degree 0, self-loop
    E, _ = rr.integer_case(N, 1, 24, seed=4)
    hub = ac[ap[2]:ap[3]]
    outside = np.setdiff1d(np.arange(N), np.concatenate([hub, [2]]))
    # source 2 (the hub): a target below every excluded row (all of them beat it) and one above all (none does)
    low, high = outside[1], outside[2]
    E[low], E[high] = -E[2], E[2]
    S = rr.scores64(E, E, "fp32")
    assert S[2, low] < S[2, hub].min() and S[2, high] > np.delete(S[2], [2, high]).max()
    src = [2, 2, 2, 2, 5, 9, 9, 9, 2, 7, 2, 2]
    dst = [hub[0], hub[7], outside[0], 2, 5, 9, 30, 11, hub[0], 13, low, high]
    return N, E, S, rowptr, col, ap, ac, np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64), hub


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_filter_subtracts_exactly_the_excluded_rows_that_beat_the_target(mode):
    gs = pkg()
    gs.ops.set_compute_dtype(mode)
    N, E, S, rowptr, col, ap, ac, src, dst, hub = _filter_case()
    want_rank, want_sc, _, ok = kr.rank_ref(E, E[src], dst, mode, "neighbours", src, ap, ac)
    plain, _, _, _ = kr.rank_ref(E, E[src], dst, mode, "self", src)
    # the cases are what they claim to be: every column of the hub's row beats the target / none of them does
    assert plain[10] - want_rank[10] == np.setdiff1d(hub, [2]).size >= 38 and plain[11] == want_rank[11] == 1
    assert (plain - want_rank).max() >= 10 and want_rank[0] == want_rank[8]       # a duplicated pair
    emb = _dev(E)
    csr = gs.DeviceCSR(_dev(ap), _dev(ac), N, 40)
    before = gs._native.launch_count()
    rank, sc = gs.ops.rank_ip(emb, emb[_dev(src)], _dev(dst), query_ids=_dev(src), csr=csr, exclude="neighbours")
    assert gs._native.launch_count() - before == 3                      # scan + filter + finish
    assert torch.equal(rank.cpu(), torch.from_numpy(want_rank))
    assert torch.equal(sc.cpu(), torch.from_numpy(want_sc.astype(np.float32)))
    # the unsorted original with its duplicate column: refused by the kernel, handled by link_rank's own filter
    raw = gs.DeviceCSR(_dev(rowptr), _dev(col), N, 40)
    with pytest.raises(ValueError, match="strictly ascending"):
        gs.ops.rank_ip(emb, emb[_dev(src)], _dev(dst), query_ids=_dev(src), csr=raw, exclude="neighbours")
    assert int(raw.err_flag.item()) == 0                                # (the flag is back at rest)
    rank, sc = gs.link_rank(emb, src, dst, exclude="neighbours", adj=raw)
    assert torch.equal(rank.cpu(), torch.from_numpy(want_rank))
    assert torch.equal(sc.cpu(), torch.from_numpy(want_sc.astype(np.float32)))


# ---- 6. unranked -----------------------------------------------------------------------------------------------------------
def test_nan_targets_are_unranked_and_nan_rows_change_no_rank():
    gs = pkg()
    gs.ops.set_compute_dtype("fp32")
    E, Qm = rr.integer_case(100, 35, 16, seed=2)
    tg = np.random.RandomState(3).randint(0, 100, size=35)
    tg[[0, 33]] = 4
    tg[tg == 40] = 41
    tg[tg == 77] = 78
    clean, _, _, _ = kr.rank_ref(E, Qm, tg, "fp32")
    E[[4, 40, 77]] = np.nan
    want_rank, _, _, _ = kr.rank_ref(E, Qm, tg, "fp32")
    rank, sc = gs.ops.rank_ip(_dev(E), _dev(Qm), _dev(tg))
    assert torch.equal(rank.cpu(), torch.from_numpy(want_rank))
    rank, sc = rank.cpu().numpy(), sc.cpu().numpy()
    nan_t = tg == 4
    assert (rank[nan_t] == 0).all() and np.isnan(sc[nan_t]).all() and nan_t.sum() >= 2
    assert (rank[~nan_t] >= 1).all() and not np.isnan(sc[~nan_t]).any()
    # the three NaN rows beat nothing: every other rank is the clean table's minus the NaN rows that beat it there
    assert (rank[~nan_t] <= clean[~nan_t]).all() and (clean[~nan_t] - rank[~nan_t] <= 3).all()


# ---- 7. random unit rows: the derived interval -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_random_unit_rows_within_the_rank_interval(mode):
    gs = pkg()
    gs.ops.set_compute_dtype(mode)
    N, D = 5003, 256
    E = rr.unit_rows(N, D, 11)
    nodes = 7 * np.arange(64)
    emb = _dev(E)
    # near targets: the reference's ranks 1 .. 8 of each query, 512 pairs
    ref_ids, _, _, _ = rr.topk_ref(E, E[nodes], 8, mode, "self", nodes)
    src, dst = np.repeat(nodes, 8), ref_ids.reshape(-1)
    lo, hi, ref = kr.rank_interval(E, E[src], dst, mode, "self", src)
    assert np.array_equal(ref, np.tile(np.arange(1, 9), 64))
    rank, _ = gs.link_rank(emb, src, dst, exclude="self")
    rank = rank.cpu().numpy()
    sure = lo == hi
    print("%s near targets: %.3f have lo == hi; rank - reference in [%d, %d]"
          % (mode, sure.mean(), (rank - ref).min(), (rank - ref).max()))
    assert sure.mean() >= 0.9                                            # (a condition on the inputs)
    assert ((lo <= rank) & (rank <= hi)).all()
    assert np.array_equal(rank[sure], ref[sure])
    # random targets: one per query
    dst2 = np.random.RandomState(5).randint(0, N, size=64)
    lo2, hi2, ref2 = kr.rank_interval(E, E[nodes], dst2, mode, "self", nodes)
    rank2, _ = gs.link_rank(emb, nodes, dst2, exclude="self")
    rank2 = rank2.cpu().numpy()
    diff = rank2 - ref2
    rec = {"near_share_lo_eq_hi": sure.mean(), "near_rank_minus_ref_min": (rank - ref).min(),
           "near_rank_minus_ref_max": (rank - ref).max(), "random_width_max": (hi2 - lo2).max(),
           "random_width_mean": (hi2 - lo2).mean(), "random_rank_minus_ref_min": diff.min(),
           "random_rank_minus_ref_max": diff.max(), "random_rank_minus_ref_nonzero": (diff != 0).sum()}
    print("%s random targets: %r" % (mode, {k: float(v) for k, v in rec.items()}))
    note_parity("rank_interval/N%d_D%d_%s" % (N, D, mode), **rec)
    assert ((lo2 <= rank2) & (rank2 <= hi2)).all()


# ---- 8. public path ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_link_rank_over_a_models_embeddings(mode):
    gs = pkg()
    gs.ops.set_compute_dtype(mode)
    rng = np.random.RandomState(7)
    n, D = 699, 24
    adj, indptr, data = sparse_graph(n, rng)
    keep = rng.rand(data.size) < 0.7                                     # the training graph: 70 % of the stored edges
    from scipy import sparse
    tdeg = np.bincount(np.repeat(np.arange(n + 1), np.diff(indptr))[keep], minlength=n + 1)
    tptr = np.concatenate([[0], np.cumsum(tdeg)]).astype(np.int64)
    tcols = np.arange(tptr[-1]) - np.repeat(tptr[:-1], tdeg)
    train_adj = sparse.csr_matrix((data[keep], tcols, tptr), shape=(n + 1, max(int(tdeg.max()), 1)))
    feats = rng.normal(size=(n + 1, D)).astype(np.float32)
    feats[0] = 0
    model = make_model("mean", "identity", adj, D).to(DEV)
    store = gs.FeatureStore.from_array(feats, torch.device(DEV), dtype="fp32")
    emb = gs.embeddings(model, store)
    E = emb.cpu().numpy()
    full_d, seen_d = gs.DeviceCSR.from_scipy(adj, torch.device(DEV)), gs.DeviceCSR.from_scipy(train_adj, torch.device(DEV))
    full_h, seen_h = gs.DeviceCSR.from_scipy(adj, torch.device("cpu")), gs.DeviceCSR.from_scipy(train_adj, torch.device("cpu"))
    nodes = np.concatenate([rng.randint(1, n + 1, size=60), [17, 17]])
    src, dst = gs.held_out_edges(full_d, seen_d, nodes)
    src_h, dst_h = gs.held_out_edges(full_h, seen_h, nodes)
    assert src.is_cuda and torch.equal(src.cpu(), src_h) and torch.equal(dst.cpu(), dst_h) and src_h.numel() > 30
    rank, sc = gs.link_rank(emb, src, dst, exclude="neighbours", adj=full_d)
    ap, ac = kr.ascending_csr(indptr, data.astype(np.int32))
    s, d = src_h.numpy(), dst_h.numpy()
    lo, hi, ref = kr.rank_interval(E, E[s], d, mode, "neighbours", s, ap, ac)
    rank = rank.cpu().numpy()
    assert ((lo <= rank) & (rank <= hi)).all(), int(((rank < lo) | (rank > hi)).sum())
    m = gs.link_metrics(rank)
    assert m["n"] == rank.size and m["unranked"] == 0 and 0 < m["mrr"] <= 1
