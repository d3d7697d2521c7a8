"""-m gpu: the LSTM aggregator on this library's own recurrence kernels (csrc/gsage_lstm.hip) -- no torch.nn.LSTM
forward on a CUDA tensor, both compute modes against the float64 oracle of tests/lstm_ref.py (rounding-aware in bf16
mode), lazy rows equal to materialised rows, command-list capture of the forward, and two train steps of a two-layer
model against the same model stepped on the CPU."""
import numpy as np
import pytest
import torch
from scipy import sparse
from torch.nn import functional as F

import lstm_harness
import lstm_ref
from conftest import load_golden, pkg
from util import ACTS, SelReplay, close, weights

pytestmark = pytest.mark.gpu
gs = pkg()
ops = gs.ops
nat = gs._native
DEV = "cuda"


@pytest.fixture(autouse=True)
def _warm():
    ops.warmup(torch.device(DEV))
    yield
    ops.set_compute_dtype("bf16")


@pytest.fixture
def no_stock_lstm(monkeypatch):
    def refuse(self, *a, **kw):
        raise AssertionError("torch.nn.LSTM.forward was called on the GPU path")
    monkeypatch.setattr(torch.nn.LSTM, "forward", refuse)


def test_golden_vectors_without_the_stock_lstm(no_stock_lstm):
    ops.set_compute_dtype("fp32")
    g = load_golden("lstm_kat.npz")
    assert int(g["n_cases"]) == 4
    for c in range(int(g["n_cases"])):
        p = "c%d_" % c
        M, n, D, h, hid, bidir = [int(v) for v in g[p + "dims"]]
        agg = gs.aggregator_lookup["lstm"](input_dim=D, output_dim=h, activation=ACTS[str(g[p + "act"])],
                                           hidden_dim=hid, bidirectional=bool(bidir))
        agg.load_state_dict(weights(g, p + "w_"))
        agg = agg.to(DEV)
        x = torch.from_numpy(g[p + "x"].copy()).to(DEV).requires_grad_(True)
        nb = torch.from_numpy(g[p + "neibs"].copy()).to(DEV).requires_grad_(True)
        before = nat.launch_count()
        out = agg(x, nb)
        close(out.detach().float().cpu().numpy(), g[p + "out"], (c, "lstm out"), 2e-4, 2e-5)
        (out.float() * torch.from_numpy(g[p + "G"]).to(DEV)).sum().backward()
        assert nat.launch_count() - before >= 4, (c, nat.launch_count() - before)
        close(x.grad.cpu().numpy(), g[p + "dx"], (c, "dx"), 2e-4, 2e-5)
        close(nb.grad.cpu().numpy(), g[p + "dneibs"], (c, "dneibs"), 2e-4, 2e-5)
        for k, v in agg.named_parameters():
            close(v.grad.cpu().numpy(), g[p + "g_" + k], (c, k), 2e-4, 2e-5)
        if bidir:
            assert not agg.lstm.weight_hh_l0_reverse.grad.any()        # exact zeros, not None


# (M, n, D, hidden_dim, bidirectional)
SWEEP = [(1, 1, 7, 2, True), (17, 3, 602, 40, False), (33, 2, 100, 40, True), (64, 10, 602, 512, False),
         (64, 25, 256, 512, True), (50, 16, 128, 128, False), (257, 5, 64, 64, True)]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("case", range(len(SWEEP)))
def test_shape_sweep_against_the_float64_oracle(case, mode, no_stock_lstm):
    """ops.lstm_last, output and every gradient.  fp32 mode: close(2e-4, 2e-5).  bf16 mode against the rounding-aware
    oracle: output at TOL["bf16"], gradients at 3e-2 relative Frobenius (no ReLU in the recurrence: no mask flips)."""
    r = lstm_harness.run(SWEEP[case], mode, case, "lstm_sweep_case%d_%s" % (case + 1, mode))
    lstm_harness.compare(r, mode, case)


def _agg(D, h, hid, bidir):
    torch.manual_seed(1)
    return gs.aggregator_lookup["lstm"](input_dim=D, output_dim=h, activation=torch.relu, hidden_dim=hid,
                                        bidirectional=bidir).to(DEV)


@pytest.mark.parametrize("bidir", [False, True])
def test_rowref_equals_tensor_path(bidir, no_stock_lstm, monkeypatch):
    rng = np.random.RandomState(0)
    R, D, h, M, n = 300, 50, 16, 40, 7
    feats_np = rng.normal(size=(R, D)).astype(np.float32)
    idx = torch.from_numpy(rng.randint(0, R, size=M)).to(DEV)
    idn = torch.from_numpy(rng.randint(0, R, size=M * n)).to(DEV)
    # fp32 store, fp32 mode: the tolerance of test_aggregator_rowref_equals_tensor_path
    ops.set_compute_dtype("fp32")
    feats = torch.from_numpy(feats_np).to(DEV)
    store = gs.FeatureStore.from_array(feats_np, torch.device(DEV), dtype="fp32")
    agg = _agg(D, h, 24, bidir)
    a = agg(store[idx], store[idn])
    b = agg(feats[idx], feats[idn])
    close(a.detach().float().cpu().numpy(), b.detach().float().cpu().numpy(), "fp32 rowref", 1e-5, 1e-6)
    # bf16 store, bf16 mode: both routes round the same rows -- bitwise
    ops.set_compute_dtype("bf16")
    store16 = gs.FeatureStore.from_array(feats_np, torch.device(DEV), dtype="bf16")
    rows16 = store16.data[:, :D]
    a = agg(store16[idx], store16[idn])
    b = agg(rows16[idx], rows16[idn])
    assert a.dtype == b.dtype and torch.equal(a, b)
    # the RowRef route computes no d neibs: no input-gradient GEMM of width D runs in its backward
    widths = []
    real = ops._dgrad

    def spy(gc, wa, K):
        widths.append(int(K))
        return real(gc, wa, K)
    monkeypatch.setattr(ops, "_dgrad", spy)
    agg.zero_grad()
    agg(store16[idx], store16[idn]).float().sum().backward()
    assert D not in widths, widths
    lazy = {k: v.grad.clone() for k, v in agg.named_parameters()}
    assert all(v is not None for v in lazy.values())
    widths.clear()
    agg.zero_grad()
    nb = rows16[idn].clone().requires_grad_(True)
    agg(rows16[idx], nb).float().sum().backward()
    assert D in widths and nb.grad is not None and nb.grad.shape == (M * n, D)
    for k, v in agg.named_parameters():                     # same rows, same kernels: same parameter gradients
        assert torch.equal(v.grad, lazy[k]), k


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_forward_is_recorded_into_a_command_list(mode, no_stock_lstm):
    ops.set_compute_dtype(mode)
    cdt = ops.torch_dtype()
    M, n, D, hid = 70, 6, 64, 96
    torch.manual_seed(3)
    lstm = torch.nn.LSTM(D, hid // 2, bidirectional=True, batch_first=True).to(DEV)
    names = list(lstm_ref.PARAMS) + [k + "_reverse" for k in lstm_ref.PARAMS]
    params = [getattr(lstm, k) for k in names]
    gen = torch.Generator(device=DEV).manual_seed(0)
    buf = torch.randn(M * n, D, device=DEV, generator=gen).to(cdt)
    with nat.CommandList.record() as cl:
        out = ops.lstm_last(buf, M, *params[:4], reverse=params[4:])      # (out's graph keeps every operand alive)
    assert len(cl) >= 4               # two projections, the W_hh packing, two recurrence launches: recorded, not run
    stream = torch.cuda.current_stream().cuda_stream
    for k in range(2):
        buf.copy_(torch.randn(M * n, D, device=DEV, generator=gen).to(cdt))
        torch.cuda.synchronize()
        cl.replay(stream)
        torch.cuda.synchronize()
        direct = ops.lstm_last(buf.clone(), M, *params[:4], reverse=params[4:])
        assert torch.equal(out.detach(), direct.detach()), (mode, k)
        assert float(direct.detach().float().abs().max()) > 0


def test_two_train_steps_match_the_cpu_model(monkeypatch):
    """Two-layer GSSupervised with the LSTM aggregator on the tiny synthetic problem (the recipe of
    test_host_mode._tiny_problem): GPU (fp32 mode, no stock LSTM) against the same model stepped on the CPU from the
    same weights and the same replayed samples.  The model is as tiny as the problem (9 features, 16 hidden units in two
    directions, 8 outputs per half): Adam's first steps move every weight by ~lr * g / (|g| + 1e-8), which turns fp32
    summation-order noise on an entry whose gradient cancels to ~1e-8 into a fraction of lr (util.close_update); the
    fewer entries, the less the element-wise tolerance of test_full_model_host_mode_train_steps depends on none of them
    being such an entry."""
    ops.set_compute_dtype("fp32")
    rng = np.random.RandomState(0)
    n = 150
    degs = rng.randint(1, 9, size=n + 1)
    degs[0] = 0
    rows = np.repeat(np.arange(n + 1), degs)
    cols = np.concatenate([np.arange(d) for d in degs])
    vals = rng.randint(1, n + 1, size=rows.shape[0])
    adj = sparse.csr_matrix((vals, (rows, cols)))
    feats = rng.normal(size=(n + 1, 9)).astype(np.float32)
    B, fan, C = 24, (4, 3), 4
    ids = rng.randint(1, n + 1, size=B)
    tg = rng.randint(0, C, size=(B, 1))
    sels = [[rng.randint(0, adj.shape[1], size=(B, fan[0])), rng.randint(0, adj.shape[1], size=(B * fan[0], fan[1]))]
            for _ in range(2)]

    import functools
    lstm16 = functools.partial(gs.aggregator_lookup["lstm"], hidden_dim=16, bidirectional=True)

    def make():
        torch.manual_seed(7)
        return gs.GSSupervised(
            sampler_class=gs.sampler_lookup["sparse_uniform_neighbor_sampler"], adj=adj, train_adj=adj,
            prep_class=gs.prep_lookup["identity"], aggregator_class=lstm16, input_dim=9, n_nodes=n + 1, n_classes=C,
            layer_specs=[{"n_train_samples": fan[0], "n_val_samples": fan[0], "output_dim": 8, "activation": F.relu},
                         {"n_train_samples": fan[1], "n_val_samples": fan[1], "output_dim": 8,
                          "activation": lambda x: x}])

    cpu = make()
    w0 = {k: v.clone() for k, v in cpu.state_dict().items()}
    gpu = make()
    gpu.load_state_dict(w0)
    gpu = gpu.to(DEV)
    cpu.optimizer = torch.optim.Adam(cpu.parameters(), lr=0.01)
    gpu.optimizer = torch.optim.Adam(gpu.parameters(), lr=0.01)
    store = gs.FeatureStore.from_array(feats, torch.device(DEV), dtype="fp32")
    loss_fn = gs.ProblemLosses.classification
    stock = torch.nn.LSTM.forward

    def refuse(self, *a, **kw):
        raise AssertionError("torch.nn.LSTM.forward was called on the GPU path")
    for step in range(2):
        monkeypatch.setattr(torch.nn.LSTM, "forward", refuse)
        with SelReplay([s.copy() for s in sels[step]]):
            pg = gpu.train_step(ids=torch.from_numpy(ids).to(DEV), feats=store, targets=torch.from_numpy(tg).to(DEV),
                                loss_fn=loss_fn)
        monkeypatch.setattr(torch.nn.LSTM, "forward", stock)            # (the CPU model is the stock path)
        with SelReplay([s.copy() for s in sels[step]]):
            pc = cpu.train_step(ids=torch.from_numpy(ids), feats=torch.from_numpy(feats),
                                targets=torch.from_numpy(tg), loss_fn=loss_fn)
        close(pg.detach().float().cpu().numpy(), pc.detach().numpy(), (step, "preds"), 1e-4, 1e-5)
        sc = cpu.state_dict()
        for k, v in gpu.state_dict().items():
            close(v.detach().cpu().numpy(), sc[k].numpy(), (step, "w", k), 1e-4, 1e-5)
    assert max(float((v - w0[k]).abs().max()) for k, v in cpu.state_dict().items()) > 1e-3      # the steps moved them
