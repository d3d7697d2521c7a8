"""-m gpu: gsage_sample_hops_temporal, every hop of a temporal frontier in one launch, against the serial restatement
of tests/temporal_ref.py and against the per-hop launches (torch.equal on ids and times: the frontier is defined bit for
bit) over the 14-row test graph whose degrees straddle 16 / 64 / 256 / 4096 and the 84 (row, query time) parents whose
times sit on every boundary kind; the call counter, the rank, the seed and time queues, out-of-range seeds, and the
launch in a command list under a device call counter."""
import ctypes

import numpy as np
import pytest
import torch

import temporal_engine_ref as ter
import temporal_ref as tr
from conftest import pkg

pytestmark = pytest.mark.gpu
gs = pkg()
ops, nat = gs.ops, gs._native
DEV = "cuda"
SEED = ter.SEED

# a lone parent; more than 16 samples per parent and a second hop of 125 parents; a second hop of 165; three hops; five
# hops; 17 samples per parent and a second hop of 34 parents; n = 1 over all 84 parents, every boundary kind
SHAPES = [(1, (3,)), (5, (25, 10)), (33, (5, 3)), (20, (4, 3, 2)), (3, (2, 2, 2, 2, 2)), (2, (17, 2)), (84, (1,))]


@pytest.fixture(autouse=True)
def _setup():
    ops.warmup(torch.device(DEV))
    yield


def _dev(a):
    return torch.from_numpy(np.asarray(a, dtype=np.int64)).to(DEV)


_ADJ = []


def _adj():
    if not _ADJ:
        _ADJ.append(tr.graph().csr(DEV))
    return _ADJ[0]


def _buffer(seeds, fans):
    B = len(seeds)
    ids = torch.full((sum(ter.sizes(B, fans)),), -7, dtype=torch.int64, device=DEV)
    ids[:B] = _dev(seeds)
    return ids


def _eq(got, ref):
    return torch.equal(got.cpu(), torch.from_numpy(ref))


@pytest.mark.parametrize("strategy,inherit", ter.PAIRS)
@pytest.mark.parametrize("B,fans", SHAPES)
def test_all_hops_equal_the_restatement_and_the_per_hop_launches(B, fans, strategy, inherit):
    adj = _adj()
    seeds, times = tr.parents(B)
    assert list(tr.graph().deg[seeds[:4]]) == [3, 300, 4097, 0][:min(B, 4)]    # one wave of the count phase
    before = nat.launch_count()
    ids, out_t = ops.sample_hops_temporal(adj, _buffer(seeds, fans), _dev(times), B, fans, {"seed": SEED, "call_base": 3},
                                          strategy=strategy, inherit=inherit)
    assert nat.launch_count() - before == 1                   # every hop in one launch
    ref, ref_t, err = ter.graph_frontier(seeds, times, fans, 3, strategy, inherit)
    assert err == 0 and _eq(ids, ref) and _eq(out_t, ref_t)
    cur, cur_t, off = ids[:B], out_t[:B], B
    assert torch.equal(cur_t, _dev(times))                    # hop 0 of out_times: the seeds' own times
    for k, n in enumerate(fans):
        nxt, nxt_t = ops.sample_csr_temporal(adj, cur, cur_t, n, {"seed": SEED, "call_base": 3 + k, "g0": 0},
                                             strategy=strategy, inherit=inherit)
        assert torch.equal(nxt, ids[off:off + nxt.numel()]) and torch.equal(nxt_t, out_t[off:off + nxt.numel()]), ("hop", k + 1)
        cur, cur_t, off = nxt, nxt_t, off + nxt.numel()
    assert off == ids.numel()
    adj.check()


@pytest.mark.parametrize("strategy", tr.STRATEGIES)
def test_edge_rule_times_strictly_decrease_along_every_path(strategy):
    adj = _adj()
    B, fans = 84, (3, 2, 2)
    seeds, times = tr.parents(B)
    ids, out_t = ops.sample_hops_temporal(adj, _buffer(seeds, fans), _dev(times), B, fans, {"seed": SEED},
                                          strategy=strategy, inherit="edge")
    ids, out_t = ids.cpu().numpy(), out_t.cpu().numpy()
    sz, off, walked = ter.sizes(B, fans), 0, 0
    for k, n in enumerate(fans):
        child, child_t = ids[off + sz[k]:off + sz[k] + sz[k + 1]], out_t[off + sz[k]:off + sz[k] + sz[k + 1]]
        parent_t = np.repeat(out_t[off:off + sz[k]], n)
        dummy = (child == 0) & (child_t == parent_t)            # (col never holds 0: a 0 is the dummy, its time the parent's)
        assert ((child_t < parent_t) | dummy).all(), ("hop", k + 1)
        walked += int((~dummy).sum())
        off += sz[k]
    assert walked > 100
    adj.check()


def test_out_times_none_gives_the_same_ids():
    adj = _adj()
    B, fans = 20, (4, 3, 2)
    seeds, times = tr.parents(B)
    with_t, _ = ops.sample_hops_temporal(adj, _buffer(seeds, fans), _dev(times), B, fans, {"seed": SEED}, inherit="edge")
    ids, d_times = _buffer(seeds, fans), _dev(times)
    d = _desc(adj, ids, B, fans)
    before = nat.launch_count()
    nat.check(nat.lib().gsage_sample_hops_temporal(ctypes.addressof(d), adj.etime.data_ptr(), d_times.data_ptr(), None, 0, 1,
                                                   None, None), "hops")
    assert nat.launch_count() - before == 1 and torch.equal(ids, with_t)
    adj.check()


def _desc(adj, ids, B, fans):
    d = nat.HopsDesc()
    d.rowptr, d.col, d.n_rows = adj.rowptr.data_ptr(), adj.col.data_ptr(), adj.n_rows
    d.ids, d.B, d.n_hops = ids.data_ptr(), B, len(fans)
    for k in range(5):
        d.fan[k] = fans[k] if k < len(fans) else 1
    d.max_deg, d.seed, d.err_flag = 0, SEED, adj.err_flag.data_ptr()          # (max_deg is ignored)
    return d


def test_call_counter_and_base():
    adj = _adj()
    B, fans = 3, (5, 3)
    seeds, times = (a[28:28 + B] for a in tr.parents())        # times inside a tie run
    ctr = torch.tensor([6], dtype=torch.int64, device=DEV)
    ids, out_t = ops.sample_hops_temporal(adj, _buffer(seeds, fans), _dev(times), B, fans,
                                          {"seed": SEED, "call_base": 2, "call_ctr": ctr}, inherit="edge")
    ref, ref_t, _ = ter.graph_frontier(seeds, times, fans, 8, "uniform", "edge")
    assert _eq(ids, ref) and _eq(out_t, ref_t) and int(ctr.item()) == 6


def test_rank_offsets_the_global_sample_index():
    """rank 1 with B seeds = rows [B, 2B) of every hop of a rank-0 run over 2B seeds whose second half they are"""
    adj = _adj()
    B, fans = 6, (4, 3, 2)
    ids2, times2 = (a[56:56 + 2 * B] for a in tr.parents())   # times above every edge: the draws decide the children
    one, one_t = ops.sample_hops_temporal(adj, _buffer(ids2[B:], fans), _dev(times2[B:]), B, fans,
                                          {"seed": SEED, "rank": 1}, inherit="edge")
    two, two_t = ops.sample_hops_temporal(adj, _buffer(ids2, fans), _dev(times2), 2 * B, fans, {"seed": SEED}, inherit="edge")
    o1 = o2 = 0
    for s in ter.sizes(B, fans):
        assert torch.equal(one[o1:o1 + s], two[o2 + s:o2 + 2 * s]) and torch.equal(one_t[o1:o1 + s], two_t[o2 + s:o2 + 2 * s])
        o1, o2 = o1 + s, o2 + 2 * s
    ref, ref_t, _ = ter.graph_frontier(ids2, times2, fans, 0, "uniform", "edge")
    assert _eq(two, ref) and _eq(two_t, ref_t)
    adj.check()


def test_seed_queue_and_time_queue():
    """n_batches = 3, *batch_idx = 4, batch_base = 1: batch (4 + 1) % 3 = 2 becomes hop 0 of ids and of out_times"""
    adj = _adj()
    B, fans = 14, (4, 3)
    allp, allt = tr.parents()
    queue = _dev(np.stack([allp[0:B], allp[28:28 + B][::-1].copy(), allp[56:56 + B]]))
    tqueue = _dev(np.stack([allt[0:B], allt[28:28 + B][::-1].copy(), allt[56:56 + B] - 7]))
    bidx = torch.tensor([4], dtype=torch.int64, device=DEV)
    ids = torch.full((sum(ter.sizes(B, fans)),), -7, dtype=torch.int64, device=DEV)
    out_t = torch.full_like(ids, -7)
    d = _desc(adj, ids, B, fans)
    d.seed_queue, d.batch_idx, d.batch_base, d.n_batches = queue.data_ptr(), bidx.data_ptr(), 1, 3
    before = nat.launch_count()
    nat.check(nat.lib().gsage_sample_hops_temporal(ctypes.addressof(d), adj.etime.data_ptr(), None, tqueue.data_ptr(), 0, 1,
                                                   out_t.data_ptr(), None), "hops")
    assert nat.launch_count() - before == 1
    ref, ref_t, err = ter.graph_frontier(queue[2].cpu().numpy(), tqueue[2].cpu().numpy(), fans, 0, "uniform", "edge")
    assert err == 0 and _eq(ids, ref) and _eq(out_t, ref_t)
    assert torch.equal(ids[:B], queue[2]) and torch.equal(out_t[:B], tqueue[2])      # hop 0 is published
    assert int(bidx.item()) == 4
    adj.check()


def test_out_of_range_and_negative_seeds():
    adj, g = _adj(), tr.graph()
    B, fans = 6, (4, 3)
    seeds = np.asarray([1, g.n, 9, -1, 2, 1 << 40], dtype=np.int64)
    times = np.asarray([tr.INT64_MAX, 5, tr.INT64_MAX, -9, tr.INT64_MAX, 11], dtype=np.int64)
    ids, out_t = ops.sample_hops_temporal(adj, _buffer(seeds, fans), _dev(times), B, fans, {"seed": SEED}, inherit="edge")
    ref, ref_t, err = ter.graph_frontier(seeds, times, fans, 0, "uniform", "edge")
    assert err == 1 and _eq(ids, ref) and _eq(out_t, ref_t)
    h1, t1 = ids[B:B + 4 * B].view(B, 4).cpu(), out_t[B:B + 4 * B].view(B, 4).cpu()
    for i in (1, 3, 5):                                       # zeros, with their own times
        assert not h1[i].any() and (t1[i] == int(times[i])).all()
    assert h1[0].all() and h1[2].all() and h1[4].all()
    assert int(adj.err_flag.item()) == 1
    adj.err_flag.zero_()


def test_the_recorded_launch_replays_under_a_device_call_counter():
    """recorded once with a device counter, replayed twice with the counter advanced by the number of hops between: the
    frontiers of calls c and c + L"""
    adj = _adj()
    B, fans, c = 20, (4, 3, 2), 4
    seeds, times = (a[56:56 + B] for a in tr.parents())
    ctr = torch.tensor([c], dtype=torch.int64, device=DEV)
    ids, out_t = _buffer(seeds, fans), torch.zeros(sum(ter.sizes(B, fans)), dtype=torch.int64, device=DEV)
    d_times = _dev(times)
    with nat.CommandList.record() as cl:
        ops.sample_hops_temporal(adj, ids, d_times, B, fans, {"seed": SEED, "call_base": 2, "call_ctr": ctr},
                                 strategy="uniform", inherit="edge", out_times=out_t)
        nat.check(nat.lib().gsage_counter_add(ctr.data_ptr(), len(fans), None), "counter_add")
    assert len(cl) == 2 and not out_t.any().item() and int(ids[B:].max().item()) == -7     # recorded, not launched
    for k in range(2):
        cl.replay(ops._stream())
        ref, ref_t, _ = ter.graph_frontier(seeds, times, fans, 2 + c + len(fans) * k, "uniform", "edge")
        assert _eq(ids, ref) and _eq(out_t, ref_t), k
    assert int(ctr.item()) == c + 2 * len(fans)
    adj.check()
