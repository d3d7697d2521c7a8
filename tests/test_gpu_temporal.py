"""-m gpu: the temporal sampler.  gsage_sample_csr_temporal, gsage_temporal_count and gsage_temporal_compact against
host mode (torch.equal: ids and times are defined bit for bit; the host tests hold host mode to the serial restatement
of tests/temporal_ref.py) on the test graph whose rows sit on either side of every search-round boundary, with rows of
3, 300, 4097 and 0 edges in one wave; error handling; the launch in a command list under a device call counter; the
module path's frontier; and the sampled forward as of T against full-neighbourhood inference over snapshot(T)."""
import numpy as np
import pytest
import torch

import temporal_ref as tr
from conftest import pkg
from util import close

pytestmark = pytest.mark.gpu
gs = pkg()
ops, nat = gs.ops, gs._native
DEV = "cuda"
SEED = 0x0123456789ABCDEF
EINVAL = -1                         # GSAGE_EINVAL (include/gsage.h)
INT64_MAX = tr.INT64_MAX


@pytest.fixture(autouse=True)
def _setup():
    ops.set_compute_dtype("bf16")
    ops.warmup(torch.device(DEV))
    yield
    ops.set_compute_dtype("bf16")


def _dev(a):
    return torch.from_numpy(np.asarray(a, dtype=np.int64)).to(DEV)


_ADJ = {}


def _graphs():
    """(the test graph, its device CSR, its host CSR), built once"""
    if not _ADJ:
        g = tr.graph()
        _ADJ["g"] = (g, g.csr(DEV), g.csr("cpu"))
    return _ADJ["g"]


# ---- the hop kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inherit", tr.RULES)
@pytest.mark.parametrize("strategy", tr.STRATEGIES)
@pytest.mark.parametrize("n", [1, 3, 10, 25])
def test_hop_kernel_equals_host_mode(n, strategy, inherit):
    """all 84 (row, query time) pairs -- M = 84 is no multiple of 16 -- adjacent parents of different rows, the first
    wave holding rows of 3, 300, 4097 and 0 edges"""
    g, adj, host = _graphs()
    ids, times = tr.parents()
    assert len(ids) % 16 != 0 and list(g.deg[ids[:4]]) == [3, 300, 4097, 0]
    ctr = torch.tensor([6], dtype=torch.int64, device=DEV)
    for g0, base, c in ((0, 0, None), (21 * n, 5, None), (21 * n, 2, ctr)):
        ph = {"seed": SEED, "call_base": base, "g0": g0}
        if c is not None:
            ph["call_ctr"] = c
        before = nat.launch_count()
        got, got_t = ops.sample_csr_temporal(adj, _dev(ids), _dev(times), n, ph, strategy=strategy, inherit=inherit)
        assert nat.launch_count() - before == 1
        if c is not None:
            ph["call_ctr"] = c.cpu()
        ref, ref_t = ops.sample_csr_temporal(host, torch.from_numpy(ids), torch.from_numpy(times), n, ph,
                                             strategy=strategy, inherit=inherit)
        assert torch.equal(got.cpu(), ref) and torch.equal(got_t.cpu(), ref_t), (g0, base)
    assert int(ctr.item()) == 6                               # read, not advanced
    adj.check()


@pytest.mark.parametrize("M", [1, 2, 17, 257])
def test_hop_kernel_other_parent_counts(M):
    """M = 1 (one team of one wave), M = 2, and M beyond one workgroup's sixteen teams; the long rows lead"""
    g, adj, host = _graphs()
    ids, times = tr.parents()
    lead = [i for i in range(len(ids)) if g.deg[ids[i]] == 4097 and times[i] == INT64_MAX]
    order = (lead + list(range(len(ids)))) * (M // len(ids) + 1)
    ids, times = ids[order[:M]], times[order[:M]]
    ph = {"seed": SEED, "call_base": 3, "g0": 5}
    for strategy, inherit in (("uniform", "edge"), ("recent", "seed")):
        got, got_t = ops.sample_csr_temporal(adj, _dev(ids), _dev(times), 10, ph, strategy=strategy, inherit=inherit)
        ref, ref_t = ops.sample_csr_temporal(host, torch.from_numpy(ids), torch.from_numpy(times), 10, ph,
                                             strategy=strategy, inherit=inherit)
        assert torch.equal(got.cpu(), ref) and torch.equal(got_t.cpu(), ref_t), (strategy, inherit)
    adj.check()


def test_hop_kernel_equals_the_restatement_directly():
    """the first wave's four parents and the PAIRED rows' 64-bit comparisons, against the serial restatement itself"""
    g, adj, _ = _graphs()
    ids, times = tr.parents()
    pick = list(range(4)) + [i for i in range(len(ids)) if times[i] == tr.BIG + 1]
    ids, times = ids[pick], times[pick]
    got, got_t = ops.sample_csr_temporal(adj, _dev(ids), _dev(times), 3, {"seed": SEED, "call_base": 1},
                                         strategy="uniform", inherit="edge")
    ref, ref_t, err = tr.sample(g.rowptr, g.col, g.etime, g.n, ids, times, 3, SEED, 1, 0, "uniform", "edge")
    assert err == 0 and np.array_equal(got.cpu().numpy(), ref) and np.array_equal(got_t.cpu().numpy(), ref_t)


def test_count_and_snapshot_equal_host_mode():
    g, adj, host = _graphs()
    ids, times = tr.parents()
    before = nat.launch_count()
    cnt = ops.temporal_count(adj, _dev(ids), _dev(times))
    assert nat.launch_count() - before == 1
    assert torch.equal(cnt.cpu(), ops.temporal_count(host, torch.from_numpy(ids), torch.from_numpy(times)))
    every = ops.temporal_count(adj, times=_dev(times[:g.n]))
    assert torch.equal(every.cpu(), ops.temporal_count(host, times=torch.from_numpy(times[:g.n])))
    for t in (-tr.BIG - 5, -40, -37, 11, 12, 2000, tr.BIG, tr.BIG + 1, INT64_MAX - 1, INT64_MAX):
        assert torch.equal(ops.temporal_count(adj, t=t).cpu(), ops.temporal_count(host, t=t)), t
        before = nat.launch_count()
        snap, ref = adj.snapshot(t), host.snapshot(t)
        assert nat.launch_count() - before == (2 if ref.nnz else 1)        # count and compact
        assert snap.n_rows == ref.n_rows and snap.max_deg == ref.max_deg and snap.device.type == "cuda"
        assert torch.equal(snap.rowptr.cpu(), ref.rowptr) and torch.equal(snap.col.cpu(), ref.col), t
        assert torch.equal(snap.etime.cpu(), ref.etime), t
    whole = adj.snapshot(INT64_MAX)
    assert torch.equal(whole.col, adj.col) and torch.equal(whole.etime, adj.etime) and torch.equal(whole.rowptr, adj.rowptr)
    adj.check()


def test_with_times_checks_on_the_device():
    g, adj, _ = _graphs()
    plain = gs.DeviceCSR(adj.rowptr, adj.col, adj.n_rows, adj.max_deg)
    bad = adj.etime.clone()
    bad[int(g.rowptr[1]) + 7] += 100                          # one edge of the 300-row out of order
    with pytest.raises(ValueError, match="TemporalAdj"):
        plain.with_times(bad)
    assert plain.with_times(adj.etime.clone()).etime.is_cuda


# ---- error handling ------------------------------------------------------------------------------------------------
def test_out_of_range_ids_raise_the_flag_and_yield_zeros():
    g, adj, _ = _graphs()
    ids = np.asarray([1, g.n, 2, -1, 0, 1 << 40], dtype=np.int64)
    times = np.asarray([INT64_MAX, 5, INT64_MAX, 6, INT64_MAX, 7], dtype=np.int64)
    got, got_t = ops.sample_csr_temporal(adj, _dev(ids), _dev(times), 3, {"seed": SEED}, inherit="edge")
    ref, ref_t, err = tr.sample(g.rowptr, g.col, g.etime, g.n, ids, times, 3, SEED, 0, 0, "uniform", "edge")
    assert err == 1 and np.array_equal(got.cpu().numpy(), ref) and np.array_equal(got_t.cpu().numpy(), ref_t)
    assert not got.view(-1, 3)[[1, 3, 5]].any().item() and got_t.view(-1, 3)[[1, 3, 5]].cpu().tolist() == [[5] * 3, [6] * 3, [7] * 3]
    with pytest.raises(IndexError):
        adj.check()
    cnt = ops.temporal_count(adj, _dev(ids), _dev(times))
    assert cnt.cpu().tolist() == [300, 0, 4097, 0, 3, 0]
    with pytest.raises(IndexError):
        adj.check()
    assert int(adj.err_flag.item()) == 0                      # check() cleared it


def test_einval_returns_without_a_launch():
    g, adj, _ = _graphs()
    lib = nat.lib()
    ids, tm = _dev([1, 2]), _dev([5, 5])
    out, out_t = torch.zeros(8, dtype=torch.int64, device=DEV), torch.zeros(8, dtype=torch.int64, device=DEV)
    rp, col, et = adj.rowptr.data_ptr(), adj.col.data_ptr(), adj.etime.data_ptr()
    torch.cuda.synchronize()
    before = nat.launch_count()

    def hop(n=3, strategy=0, inherit=0, etime=et, M=2):
        return lib.gsage_sample_csr_temporal(rp, col, etime, adj.n_rows, ids.data_ptr(), tm.data_ptr(), M, n, strategy,
                                             inherit, SEED, None, 0, 0, out.data_ptr(), out_t.data_ptr(), None, None)

    assert hop(n=0) == EINVAL and hop(strategy=7) == EINVAL and hop(inherit=-1) == EINVAL
    assert hop(etime=None) == EINVAL and hop(M=-2) == EINVAL and hop(M=0) == 0
    assert lib.gsage_temporal_count(rp, None, adj.n_rows, ids.data_ptr(), 2, tm.data_ptr(), 0, out.data_ptr(), None,
                                    None) == EINVAL
    assert lib.gsage_temporal_compact(rp, col, et, adj.n_rows, None, out.data_ptr(), None, None, 0, None) == EINVAL
    assert nat.launch_count() == before and not out.any().item()


# ---- command lists -------------------------------------------------------------------------------------------------
def test_the_recorded_launch_replays_under_a_device_call_counter():
    """recorded once with a device counter, replayed twice with the counter advanced between: the frontiers of calls
    c and c + 1"""
    g, adj, host = _graphs()
    ids, times = tr.parents()
    n, c = 10, 4
    ctr = torch.tensor([c], dtype=torch.int64, device=DEV)
    d_ids, d_times = _dev(ids), _dev(times)
    out = torch.zeros(len(ids) * n, dtype=torch.int64, device=DEV)
    out_t = torch.zeros_like(out)
    ph = {"seed": SEED, "call_base": 2, "call_ctr": ctr}
    before = nat.launch_count()
    with nat.CommandList.record() as cl:
        ops.sample_csr_temporal(adj, d_ids, d_times, n, ph, strategy="uniform", inherit="edge", out=out, out_time=out_t)
        nat.check(nat.lib().gsage_counter_add(ctr.data_ptr(), 1, None), "counter_add")
    assert len(cl) == 2 and not out.any().item()              # recorded, not launched
    for k in range(2):
        cl.replay(ops._stream())
        ref, ref_t = ops.sample_csr_temporal(host, torch.from_numpy(ids), torch.from_numpy(times), n,
                                             {"seed": SEED, "call_base": 2 + c + k}, strategy="uniform", inherit="edge")
        assert torch.equal(out.cpu(), ref) and torch.equal(out_t.cpu(), ref_t), k
    assert int(ctr.item()) == c + 2
    # the count and the compaction record too
    cnt = torch.zeros(adj.n_rows, dtype=torch.int64, device=DEV)
    with nat.CommandList.record() as cl2:
        nat.check(nat.lib().gsage_temporal_count(adj.rowptr.data_ptr(), adj.etime.data_ptr(), adj.n_rows, None,
                                                 adj.n_rows, None, 12, cnt.data_ptr(), adj.err_flag.data_ptr(), None),
                  "temporal_count")
    assert len(cl2) == 1 and not cnt.any().item()
    cl2.replay(ops._stream())
    assert torch.equal(cnt.cpu(), ops.temporal_count(host, t=12))
    adj.check()


# ---- the module path -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy,inherit", [("uniform", "edge"), ("recent", "seed")])
def test_module_path_frontier_equals_host_mode(strategy, inherit):
    p = tr.problem()
    fans = (5, 3)
    dev_model = tr.model(p, (8, 8), fans, strategy=strategy, inherit=inherit).to(DEV)
    host_model = tr.model(p, (8, 8), fans, strategy=strategy, inherit=inherit)
    dev_model.train_sampler.seed = host_model.train_sampler.seed = 77
    ids = torch.tensor([5, 9, 32, 1, 60, 17, 0], dtype=torch.int64)
    times = torch.tensor([tr.T_SNAP, tr.T_SNAP + 1, 3, INT64_MAX, -100, 500, tr.T_SNAP + 60], dtype=torch.int64)
    a, at, b, bt = ids.to(DEV), times.to(DEV), ids, times
    for fd, fh in zip(dev_model.train_sample_fns, host_model.train_sample_fns):
        a, at = fd(ids=a, times=at)
        b, bt = fh(ids=b, times=bt)
        assert torch.equal(a.cpu(), b) and torch.equal(at.cpu(), bt)
    store = gs.FeatureStore.from_array(p["feats"], torch.device(DEV), dtype="bf16")
    tg = torch.from_numpy(p["targets"][ids.numpy()]).to(DEV)
    preds = dev_model.train_step(ids=ids.to(DEV), feats=store, targets=tg, loss_fn=gs.ProblemLosses.classification,
                                 times=times.to(DEV))
    assert tuple(preds.shape) == (7, p["C"]) and bool(torch.isfinite(preds.float()).all())
    assert dev_model.train_sampler.calls == 4
    dev_model.train_sampler.csr(DEV).check()


# ---- train.py ------------------------------------------------------------------------------------------------------
def test_train_cli_engine_auto_takes_the_module_path(capsys, tmp_path):
    import importlib
    import json
    train = importlib.import_module("pytorch-graphsage_amd.train")
    p = tr.problem()
    folds = np.array(["train"] * 40 + ["val"] * 11 + ["test"] * 10)
    problem = gs.NodeProblem.from_arrays("classification", p["C"], p["adj"], p["adj"], p["feats"], folds, p["targets"],
                                         cuda=True, adj_time=p["time"], train_adj_time=p["time"],
                                         node_time=np.full(p["n"] + 1, tr.T_SNAP))
    emb = str(tmp_path / "emb.npy")
    try:
        train.main(["--problem-path", "<memory>", "--epochs", "2", "--batch-size", "16", "--n-train-samples", "3,2",
                    "--n-val-samples", "3,2", "--output-dims", "8,8", "--show-test", "--rng", "philox", "--sampler-class",
                    "sparse_temporal_neighbor_sampler", "--temporal-inherit", "edge", "--engine", "auto", "--eval-as-of",
                    str(tr.T_SNAP), "--save-embeddings", emb], problem=problem)
        cap = capsys.readouterr()
        said = [l for l in cap.err.splitlines() if "using the module path" in l]
        assert len(said) == 1 and "SparseTemporalNeighborSampler" in said[0] and "train_step runs on" not in cap.err
        assert "--eval-as-of %d" % tr.T_SNAP in cap.err
        lines = [json.loads(l) for l in cap.out.splitlines() if l.startswith("{")]
        assert lines and lines[-1]["test_f1"] is not None and np.load(emb).shape == (61, 16)
    finally:
        gs.nn_modules.SparseUniformNeighborSampler.rng_default = "compat"
        gs.nn_modules.SparseTemporalNeighborSampler.inherit_default = "seed"
        ops.set_compute_dtype("bf16")


# ---- the point of the feature --------------------------------------------------------------------------------------
def test_sampled_forward_as_of_T_is_full_neighbour_inference_over_the_snapshot():
    """tests/test_temporal_host.py's test of the same name on the device, at the same 2e-5"""
    ops.set_compute_dtype("fp32")
    p = tr.problem()
    store = gs.FeatureStore.from_array(p["feats"], torch.device(DEV), dtype="fp32")
    ids = torch.arange(0, 61, device=DEV)
    times = torch.full((61,), tr.T_SNAP, device=DEV)
    model = tr.model(p, (16, 8), (6, 6), strategy="recent", inherit="seed").to(DEV)
    snap = model.val_sampler.csr(DEV).snapshot(tr.T_SNAP)
    assert np.array_equal(np.diff(snap.rowptr.cpu().numpy()), p["early"])
    with torch.no_grad():
        sampled = model(ids, store, train=False, times=times)
    full = gs.full_neighbour(model, store, adj=snap)
    close(sampled.cpu().numpy(), full.cpu().numpy(), "temporal sampler vs full neighbourhood over the snapshot", 2e-5, 2e-5)
    old = gs.nn_modules.SparseUniformNeighborSampler.rng_default
    gs.nn_modules.SparseUniformNeighborSampler.rng_default = "philox"
    try:
        uniform = tr.model(p, (16, 8), (6, 6), sampler="sparse_uniform_neighbor_sampler", adj=p["adj"]).to(DEV)
    finally:
        gs.nn_modules.SparseUniformNeighborSampler.rng_default = old
    uniform.load_state_dict(model.state_dict())
    with torch.no_grad():
        noisy = uniform(ids, store, train=False)
    with pytest.raises(AssertionError):
        close(noisy.cpu().numpy(), full.cpu().numpy(), "uniform sampler on the timeless graph vs the snapshot", 2e-5, 2e-5)
    model.val_sampler.csr(DEV).check()
