"""Retrieval over embeddings without a GPU: host mode of ops.topk_ip / gs.nearest against tests/retrieve_ref.py on
integer data (exact), the argument refusals of the C entry point, the workspace arithmetic and the train.py flag."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import retrieve_ref as rr
from conftest import pkg


@pytest.fixture(autouse=True)
def _dtype():
    gs = pkg()
    yield
    gs.ops.set_compute_dtype("bf16")


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("k", [1, 10, 128])
def test_host_mode_equals_the_reference_on_integer_data(mode, k):
    gs = pkg()
    gs.ops.set_compute_dtype(mode)
    E, Qm = rr.integer_case(301, 9, 40)
    ids, sc = gs.ops.topk_ip(torch.from_numpy(E), torch.from_numpy(Qm), k)
    want_ids, want_sc, _, _ = rr.topk_ref(E, Qm, k, mode)
    assert ids.dtype == torch.int64 and sc.dtype == torch.float32
    assert np.array_equal(ids.numpy(), want_ids) and np.array_equal(sc.numpy(), want_sc.astype(np.float32))


@pytest.mark.parametrize("exclude", ["none", "self", "neighbours"])
def test_nearest_host_exclusions_and_padding(exclude):
    gs = pkg()
    gs.ops.set_compute_dtype("fp32")
    N, k = 50, 64
    E, _ = rr.integer_case(N, 1, 24, seed=4)
    rowptr, col = rr.hub_csr(N)
    nodes = np.array([2, 5, 9, 2, 7], dtype=np.int64)
    adj = gs.DeviceCSR(torch.from_numpy(rowptr), torch.from_numpy(col), N, 40)
    ids, sc = gs.nearest(torch.from_numpy(E), nodes, k=k, exclude=exclude, adj=adj)
    want_ids, want_sc, _, ok = rr.topk_ref(E, E[nodes], k, "fp32", exclude, nodes, rowptr, col)
    assert np.array_equal(ids.numpy(), want_ids) and np.array_equal(sc.numpy(), want_sc.astype(np.float32))
    assert ((ids.numpy() == -1).sum(1) == k - np.minimum(ok.sum(1), k)).all()
    assert torch.equal(ids[0], ids[3])                                   # a duplicate is answered again
    # nodes=None: every row is a query
    all_ids, _ = gs.nearest(torch.from_numpy(E), None, k=3, exclude=exclude, adj=adj)
    want_all, _, _, _ = rr.topk_ref(E, E, 3, "fp32", exclude, np.arange(N), rowptr, col)
    assert np.array_equal(all_ids.numpy(), want_all)


def test_nearest_refusals():
    gs = pkg()
    E = torch.from_numpy(rr.integer_case(20, 1, 8)[0])
    with pytest.raises(ValueError, match="needs adj"):
        gs.nearest(E, [1, 2], k=3, exclude="neighbours")
    with pytest.raises(ValueError, match="DenseAdj"):
        gs.nearest(E, [1, 2], k=3, exclude="neighbours", adj=gs.DenseAdj(torch.zeros(20, 4, dtype=torch.int64)))
    with pytest.raises(IndexError):
        gs.nearest(E, [1, 20], k=3)
    with pytest.raises(ValueError, match="k must"):
        gs.nearest(E, [1], k=129)
    with pytest.raises(ValueError, match="query_ids"):
        gs.ops.topk_ip(E, E[:2], 3, exclude="self")
    with pytest.raises(ValueError, match="csr"):
        gs.ops.topk_ip(E, E[:2], 3, query_ids=[0, 1], exclude="neighbours")


def test_bad_arguments_return_einval_without_gpu():
    L = pkg()._native.lib()
    P = ctypes.c_void_p(4096)

    def call(N=100, ldt=16, ldq=16, Q=4, D=16, qids=None, rowptr=None, col=None, exclude=0, k=5, splits=0):
        return L.gsage_topk_ip(P, 0, ldt, N, P, 0, ldq, Q, D, qids, rowptr, col, exclude, k, splits, None, 0, P, P, None)

    for kw, name in (({"k": 0}, b"k must"), ({"k": 129}, b"k must"), ({"D": 1025, "ldt": 2048, "ldq": 2048}, b"D must"),
                     ({"ldt": 15}, b"ld ("), ({"ldq": 8}, b"ld ("), ({"N": 2 ** 31}, b"N must"),
                     ({"splits": -1}, b"splits"), ({"exclude": 1}, b"query_ids"),
                     ({"exclude": 2, "qids": P}, b"rowptr"), ({"exclude": 2, "qids": P, "rowptr": P}, b"col")):
        assert call(**kw) == -1, kw
        assert name in L.gsage_last_error(), (kw, L.gsage_last_error())
    # everything else in order: the workspace is what is missing
    assert call() == -1 and b"workspace" in L.gsage_last_error()


def test_workspace_is_host_arithmetic_and_monotone():
    gs = pkg()
    L = gs._native.lib()
    used = ctypes.c_int64(0)

    def ws(Q, k, splits, N=232965):
        return int(L.gsage_topk_ip_workspace(Q, N, k, splits, ctypes.byref(used)))

    assert ws(1, 1, 1) == 8 and used.value == 1
    assert ws(1, 10, 1) < ws(2, 10, 1) < ws(33, 10, 1) < ws(232965, 10, 1)              # in Q
    assert ws(70, 1, 3) < ws(70, 10, 3) < ws(70, 128, 3)                                # in k
    assert ws(70, 10, 1) < ws(70, 10, 3) < ws(70, 10, 7) < ws(70, 10, 1024)             # in splits
    # splits = 0: the library's choice for (Q, N), reported, and the bytes are those of that count
    for Q in (1, 512, 32768, 232965):
        b0 = ws(Q, 10, 0)
        s = used.value
        assert 1 <= s <= 1024 and b0 == ws(Q, 10, s) == Q * s * 10 * 8
    ws(1, 10, 0)
    many = used.value
    ws(232965, 10, 0)
    assert many > 1 and used.value == 1        # one query is split over the chip; the k-NN graph needs no split
    assert ws(0, 10, 1) == -1 and ws(1, 0, 1) == -1 and ws(1, 129, 1) == -1 and ws(1, 1, -1) == -1
    assert ws(1, 1, 1, N=2 ** 31) == -1
    assert gs.ops.topk_ip_workspace(70, 5003, 20, 3) == (70 * 3 * 20 * 8, 3)


def test_train_refuses_neighbour_nodes_without_save_neighbours(tmp_path):
    train = importlib.import_module("pytorch-graphsage_amd.train")
    ids = str(tmp_path / "ids.npy")
    np.save(ids, np.array([1, 2]))
    with pytest.raises(SystemExit, match="--neighbour-nodes goes with --save-neighbours"):
        train.main(["--problem-path", "<memory>", "--neighbour-nodes", ids])
