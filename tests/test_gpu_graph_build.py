"""-m gpu: graph construction on the device (csrc/gsage_build.hip) against host mode, which the CPU tests pin to the
serial restatement and to the reference's converter.  Every comparison is torch.equal: ids, offsets and times are
integers and a summed weight is a fixed-order fp32 chain.  Shapes: record counts either side of the sort's 2 048-entry
block, one above 1 024 blocks (the trip boundary of the sort's scan), key widths either side of the 8-bit pass
boundaries, a hub row spanning blocks next to rows of 0 and 1, and a run of duplicates spanning the window of 16."""
import numpy as np
import pytest
import torch

import graph_build_ref as gb
from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CPU = torch.device("cpu")
COMBOS = [(False, False, o, d) for o in ("insertion", "id") for d in ("first", "all")] + \
         [(True, False, o, d) for o in ("insertion", "id") for d in ("first", "sum", "all")] + \
         [(False, True, "time", "all")]


def _build(e, n, dev, **kw):
    """ops.edges_to_csr on `dev` from numpy arrays -> (rowptr, col, max_deg, payload) with CPU tensors"""
    ops = pkg().ops
    t = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    rowptr, col, max_deg, pay = ops.edges_to_csr(torch.from_numpy(e[:, 0].copy()).to(dev),
                                                 torch.from_numpy(e[:, 1].copy()).to(dev), n, **t)
    assert rowptr.device.type == col.device.type == dev.type
    return rowptr.cpu(), col.cpu(), max_deg, None if pay is None else pay.cpu()


def _same(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    assert a[1].dtype == torch.int32 and a[0].dtype == torch.int64
    assert (a[3] is None) == (b[3] is None)
    if a[3] is not None:
        assert a[3].dtype == b[3].dtype and torch.equal(a[3], b[3])


def _payloads(E, seed):
    rng = np.random.RandomState(seed)
    w = (rng.rand(E) * 4).astype(np.float32)
    t = rng.randint(-20, 20, size=E).astype(np.int64) * (1 << 33)       # equal times inside rows, beyond 32 bits
    return w, t


def _csr(got, n_rows):
    return pkg().DeviceCSR(got[0], got[1], n_rows, got[2])


@pytest.mark.parametrize("E", [1023, 1024, 1025])
def test_either_side_of_the_sort_block(E):
    """2E = 2 046, 2 048, 2 050 records; the default build is also the restatement's"""
    n = 300
    e = gb.edge_list(n, E, seed=E)
    before = pkg()._native.launch_count()
    got = _build(e, n, DEV)
    assert pkg()._native.launch_count() > before
    _same(got, _build(e, n, CPU))
    ref = gb.build(e, n)
    assert np.array_equal(got[0].numpy(), ref[0]) and np.array_equal(got[1].numpy(), ref[1]) and got[2] == ref[2]
    _same(_build(e, n, DEV, order="id"), _build(e, n, CPU, order="id"))


@pytest.mark.parametrize("n", [3, 255, 256, 70000])
def test_key_widths_either_side_of_a_pass(n):
    """4, 16, 18 and 34 key bits: one, two, three and five 8-bit passes"""
    e = gb.edge_list(n, 1500, seed=n, isolated_tail=0 if n == 3 else 3)
    if n > 3:
        e[5] = (n - 4, 0)                                            # the largest id the list may hold
    w, t = _payloads(1500, n)
    for kw in (dict(), dict(order="id"), dict(weight=w, duplicates="sum"), dict(time=t), dict(directed=True)):
        _same(_build(e, n, DEV, **kw), _build(e, n, CPU, **kw))
    a = _csr(_build(e, n, DEV, duplicates="all"), n + 1)
    for got, ref in ((a.transpose(), a_cpu(a).transpose()), (a.symmetrized(), a_cpu(a).symmetrized())):
        assert torch.equal(got.rowptr.cpu(), ref.rowptr) and torch.equal(got.col.cpu(), ref.col)
        assert got.max_deg == ref.max_deg


def a_cpu(csr):
    return pkg().DeviceCSR(csr.rowptr.cpu(), csr.col.cpu(), csr.n_rows, csr.max_deg)


def test_above_1024_blocks():
    """2.1e6 records: the sort's scan takes a second trip.  Against host mode only."""
    n, E = 70000, 1050000
    rng = np.random.RandomState(9)
    e = rng.randint(0, n - 3, size=(E, 2)).astype(np.int64)
    e[1000:1200] = e[:200][:, ::-1]                                   # reversed duplicates
    e[5000:5100, 1] = e[5000:5100, 0]                                 # self-loops
    _same(_build(e, n, DEV), _build(e, n, CPU))
    got, ref = _build(e, n, DEV, order="id"), _build(e, n, CPU, order="id")
    _same(got, ref)
    a, h = _csr(tuple(t.to(DEV) if torch.is_tensor(t) else t for t in got), n + 1), _csr(ref, n + 1)
    for x, y in ((a.transpose(), h.transpose()), (a.symmetrized(), h.symmetrized())):     # 2.1e6 and 4.2e6 records
        assert torch.equal(x.rowptr.cpu(), y.rowptr) and torch.equal(x.col.cpu(), y.col) and x.max_deg == y.max_deg


def _hub():
    n = 6000
    hub = np.stack([np.full(5000, 7), np.arange(10, 5010)], 1)        # row 7: 5 000 neighbours, spanning blocks
    e = np.concatenate([hub[:2500], [[8, 9]], hub[2500:], hub[:50]]).astype(np.int64)   # rows 8, 9: 1; row 6: 0
    return e, n


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "%s%s-%s-%s" % ("w" if c[0] else "", "t" if c[1] else "", c[2], c[3]))
def test_a_hub_row_next_to_rows_of_0_and_1(combo):
    e, n = _hub()
    w, t = _payloads(e.shape[0], 1)
    kw = dict(order=combo[2], duplicates=combo[3])
    if combo[0]:
        kw["weight"] = w
    if combo[1]:
        kw["time"] = t
    got = _build(e, n, DEV, **kw)
    _same(got, _build(e, n, CPU, **kw))
    deg = np.diff(got[0].numpy())
    assert deg[8] == (5050 if combo[3] == "all" else 5000) and deg[7] == 0 and deg[9] == deg[10] == 1
    sel = np.ones(n, dtype=bool)
    sel[7] = False                                                    # a sel that removes the hub
    got = _build(e, n, DEV, sel=sel, **kw)
    _same(got, _build(e, n, CPU, sel=sel, **kw))
    assert got[1].numel() == 2 and got[2] == 1


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "%s%s-%s-%s" % ("w" if c[0] else "", "t" if c[1] else "", c[2], c[3]))
@pytest.mark.parametrize("directed", [False, True])
def test_every_order_and_duplicates_pair(combo, directed):
    n, E = 300, 1025
    e = gb.edge_list(n, E, seed=77)
    w, t = _payloads(E, 2)
    rng = np.random.RandomState(4)
    sel = rng.rand(n) < 0.7
    kw = dict(order=combo[2], duplicates=combo[3], directed=directed)
    if combo[0]:
        kw["weight"] = w
    if combo[1]:
        kw["time"] = t
    _same(_build(e, n, DEV, **kw), _build(e, n, CPU, **kw))
    _same(_build(e, n, DEV, sel=sel, **kw), _build(e, n, CPU, sel=sel, **kw))
    ref = gb.build(e, n, sel=sel, weight=kw.get("weight"), time=kw.get("time"), directed=directed, order=combo[2],
                   duplicates=combo[3])
    got = _build(e, n, DEV, sel=sel, **kw)
    assert np.array_equal(got[0].numpy(), ref[0]) and np.array_equal(got[1].numpy(), ref[1])
    assert ref[3] is None or np.array_equal(got[3].numpy(), ref[3])


@pytest.mark.parametrize("order", ["insertion", "id"])
def test_sum_over_a_run_of_40(order):
    """the run spans the window of 16; the fp32 sum depends on the order of the additions"""
    e = np.array([[0, 1]] * 40 + [[1, 0]] * 3 + [[2, 1]], dtype=np.int64)
    w = (np.float32(1e8) * (np.arange(44) % 3 == 0) + np.arange(44)).astype(np.float32)
    got = _build(e, 3, DEV, weight=w, duplicates="sum", order=order)
    _same(got, _build(e, 3, CPU, weight=w, duplicates="sum", order=order))
    ref = gb.build(e, 3, weight=w, duplicates="sum", order=order)
    assert np.array_equal(got[3].numpy(), ref[3]) and ref[3][0] != np.float32(np.sum(w[:43].astype(np.float64)))


@pytest.mark.parametrize("E", [1023, 1024, 1025])
def test_transpose_and_symmetrized(E):
    gs = pkg()
    n = 300
    e = gb.edge_list(n, E, seed=E + 1)
    s, d = torch.from_numpy(e[:, 0].copy()), torch.from_numpy(e[:, 1].copy())
    for directed in (False, True):
        a = gs.DeviceCSR.from_edges(s, d, n, DEV, directed=directed, duplicates="all")
        h = gs.DeviceCSR.from_edges(s, d, n, CPU, directed=directed, duplicates="all")
        assert torch.equal(a.col.cpu(), h.col) and a.max_deg == h.max_deg
        for got, ref in ((a.transpose(), h.transpose()), (a.symmetrized(), h.symmetrized()),
                         (a.transpose().transpose(), h.transpose().transpose())):
            assert got.device.type == "cuda" and got.n_rows == ref.n_rows and got.max_deg == ref.max_deg
            assert torch.equal(got.rowptr.cpu(), ref.rowptr) and torch.equal(got.col.cpu(), ref.col)
    tref = gb.transpose(h.rowptr.numpy(), h.col.numpy(), h.n_rows)
    assert np.array_equal(a.transpose().col.cpu().numpy(), tref[1])


def test_transpose_and_symmetrized_of_the_hub():
    """a directed hub: its transpose has 5 000 rows of one entry (two where the duplicates are kept) and one empty hub row"""
    gs = pkg()
    e, n = _hub()
    s, d = torch.from_numpy(e[:, 0].copy()), torch.from_numpy(e[:, 1].copy())
    a = gs.DeviceCSR.from_edges(s, d, n, DEV, directed=True, duplicates="all")
    h = gs.DeviceCSR.from_edges(s, d, n, CPU, directed=True, duplicates="all")
    for x, y in ((a.transpose(), h.transpose()), (a.symmetrized(), h.symmetrized())):
        assert torch.equal(x.rowptr.cpu(), y.rowptr) and torch.equal(x.col.cpu(), y.col) and x.max_deg == y.max_deg
    assert a.transpose().max_deg == 2 and a.symmetrized().max_deg == 5000


def test_two_runs_give_the_same_bits():
    e, n = _hub()
    w, _ = _payloads(e.shape[0], 3)
    for kw in (dict(weight=w, duplicates="sum"), dict(weight=w, duplicates="sum", order="id"), dict()):
        _same(_build(e, n, DEV, **kw), _build(e, n, DEV, **kw))


def test_an_id_outside_the_graph_is_an_indexerror():
    gs = pkg()
    n = 300
    e = gb.edge_list(n, 1025, seed=5)
    s, d = torch.from_numpy(e[:, 0].copy()).to(DEV), torch.from_numpy(e[:, 1].copy()).to(DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    for bad in (n, -1, 1 << 40):
        d2 = d.clone()
        d2[700] = bad
        with pytest.raises(IndexError):
            gs.ops.edges_to_csr(s, d2, n, err_flag=flag)
        assert int(flag.item()) == 0                                  # left clear
        with pytest.raises(IndexError):
            gs.DeviceCSR.from_edges(s, d2, n, DEV, order="id")
    good = gs.ops.edges_to_csr(s, d, n, err_flag=flag)
    assert int(flag.item()) == 0 and good[1].numel() > 0
    csr = gs.DeviceCSR(torch.tensor([0, 1, 2], device=DEV), torch.tensor([1, 2], dtype=torch.int32, device=DEV), 2, 1)
    for fn in (csr.transpose, csr.symmetrized):
        with pytest.raises(IndexError):
            fn()
        csr.check()                                                   # the flag is clear again


def test_the_launch_count_does_not_depend_on_E():
    nat = pkg()._native
    n = 300                                                           # equal key bits
    counts = {}
    for kw in (dict(), dict(order="id"), dict(duplicates="all")):
        for E in (1024, 1025):
            e = gb.edge_list(n, E, seed=1)
            before = nat.launch_count()
            _build(e, n, DEV, **kw)
            counts[E] = nat.launch_count() - before
        assert counts[1024] == counts[1025] and counts[1024] >= 5, counts


def test_graph_from_edges_builds_on_the_gpu():
    gs = pkg()
    n = 300
    e = gb.edge_list(n, 1025, seed=8)
    before = gs._native.launch_count()
    got = gs.graph_from_edges(e, n)                                   # device=None: the GPU
    assert gs._native.launch_count() > before
    ref = gs.graph_from_edges(e, n, device=CPU)
    assert got.shape == ref.shape and np.array_equal(got.indptr, ref.indptr) and np.array_equal(got.data, ref.data)
    assert np.array_equal(got.indices, ref.indices)
