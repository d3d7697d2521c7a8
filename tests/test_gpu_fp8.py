"""-m gpu: the FP8 (e4m3fn, power-of-two column scales) feature table on the MI355X.

Everything is an equality: the quantiser kernel against the host mode byte for byte, every FP8 gather against the same
entry point on the bf16 table of the decoded values with torch.equal (an e4m3 value times a power of two is a bf16
number, and a power-of-two scale commutes with fp32 rounding), the mean engine on an FP8 store against the same engine
on the decoded bf16 store -- predictions after every step, weights after the last."""
import importlib
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from scipy import sparse

from conftest import pkg

pytestmark = pytest.mark.gpu
gs = pkg()
ops = gs.ops
DEV = "cuda"
DIMS = [1, 15, 16, 17, 100, 602, 1433]
FANS = [1, 5, 10, 15, 25]


@pytest.fixture(autouse=True)
def _warm():
    ops.warmup(torch.device(DEV))
    ops.set_compute_dtype("bf16")
    yield
    ops.set_compute_dtype("bf16")


def table(rows, D, seed):
    rng = np.random.RandomState(seed)
    x = (rng.randn(rows, D) * rng.uniform(1e-3, 50.0, size=D)).astype(np.float32)
    x[0] = 0.0
    if D > 2:
        x[:, 2] = 0.0                                        # an all-zero column
    x[3, 0] = 1.0e30                                         # one huge value
    return x


def bytes_of(store):
    return store.data.view(torch.uint8)


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("src", ["fp32", "bf16"])
def test_quantiser_kernel_equals_host_mode(D, src):
    x = table(1037, D, D)
    host = gs.FeatureStore.from_array(x, "cpu", dtype=src)
    dev = gs.FeatureStore.from_array(x, DEV, dtype=src)
    assert torch.equal(dev.data.cpu(), host.data)
    qh, qd = host.quantize(), dev.quantize()
    assert qd.is_fp8 and qd.is_cuda and qd.ld == qh.ld and qd.ld % 128 == 0
    assert torch.equal(qd.scale.cpu(), qh.scale)
    diff = (bytes_of(qd).cpu() != bytes_of(qh)).nonzero()
    assert diff.numel() == 0, (diff[:5], bytes_of(qd).cpu()[tuple(diff[0])], bytes_of(qh)[tuple(diff[0])])
    again = dev.quantize()                                   # deterministic
    assert torch.equal(bytes_of(again), bytes_of(qd)) and torch.equal(again.scale, qd.scale)
    if src == "fp32":                                        # from_array(dtype="fp8") is the same thing
        direct = gs.FeatureStore.from_array(x, DEV, dtype="fp8")
        assert torch.equal(bytes_of(direct), bytes_of(qd)) and torch.equal(direct.scale, qd.scale)
        # a wrapped fp32 tensor whose rows are NOT padded (ld == D)
        q2, s2 = ops.quantize_fp8(torch.from_numpy(x).to(DEV), D, qd.ld)
        assert torch.equal(q2.view(torch.uint8), bytes_of(qd)) and torch.equal(s2, qd.scale)


def _stores(D, seed=0, rows=700):
    st = gs.FeatureStore.from_array(table(rows, D, 100 + seed + D), DEV, dtype="fp8")
    dec = st.decoded("bf16")
    assert dec.dtype == torch.bfloat16 and torch.equal(dec.dense(), st.dense())
    assert torch.equal(st.dense().cpu(), gs.FeatureStore(st.data.cpu(), st.dim, st.scale.cpu()).dense())
    return st, dec


def _ids(rows, count, seed):
    ids = torch.from_numpy(np.random.RandomState(seed).randint(0, rows, size=count))
    ids[:2] = 0                                              # row 0
    if count > 4:
        ids[3] = ids[4]                                      # duplicates
        ids[-1] = ids[0]
    return ids.to(DEV)


@pytest.mark.parametrize("D", DIMS)
def test_row_gather_and_gather_mean_equal_the_decoded_bf16_table(D):
    st, dec = _stores(D)
    M = 37
    for out_dtype in (torch.bfloat16, torch.float32):
        for n in FANS:
            ids = _ids(700, M * n, n)
            for out_ld in (None, D + 3, dec.ld):
                a = ops.gather_mean(st, ids, M, n, out_dtype=out_dtype, out_ld=out_ld)
                b = ops.gather_mean(dec, ids, M, n, out_dtype=out_dtype, out_ld=out_ld)
                assert a.shape == b.shape and torch.equal(a, b), (D, n, out_dtype, out_ld)
            a = ops.gather_rows(st, ids, out_dtype=out_dtype)
            b = ops.gather_rows(dec, ids, out_dtype=out_dtype)
            assert torch.equal(a, b), (D, n, out_dtype)
            assert torch.equal(st[ids].materialize(out_dtype), b)
    # the C entry point of the row gather itself, into a slice of a wider buffer
    ids = _ids(700, 50, 9)
    out = torch.zeros(60, dec.ld, dtype=torch.bfloat16, device=DEV)
    gs._native.check(gs._native.lib().gsage_gather_rows_fp8(
        st.data.data_ptr(), st.ld, st.scale.data_ptr(), ids.data_ptr(), 50, D, out[5:].data_ptr(), gs._native.BF16,
        dec.ld, ops._stream()), "gather_rows_fp8")
    assert torch.equal(out[5:55], dec.data[ids]) and not out[:5].any() and not out[55:].any()


@pytest.mark.parametrize("D", DIMS)
def test_gather_mean_multi_equals_the_decoded_bf16_table(D):
    st, dec = _stores(D, seed=1)
    old = dec.ld
    for out_dtype in (torch.bfloat16, torch.float32):
        for n in FANS:
            shapes = [(23, n), (41, 1), (9, 25 if n != 25 else 10), (11, n)]       # the last one without a row list
            idl = [_ids(700, m * k, 7 * i + n) for i, (m, k) in enumerate(shapes)]
            idl[-1] = None
            outs_a = [torch.zeros(m, old, dtype=out_dtype, device=DEV) for m, _ in shapes]
            outs_b = [torch.zeros(m, old, dtype=out_dtype, device=DEV) for m, _ in shapes]
            ops.gather_mean_multi([(st.data, i, o, m, k) for i, o, (m, k) in zip(idl, outs_a, shapes)],
                                  st.ld, D, old, scale=st.scale)
            if out_dtype == torch.bfloat16:
                ops.gather_mean_multi([(dec.data, i, o, m, k) for i, o, (m, k) in zip(idl, outs_b, shapes)],
                                      dec.ld, D, old)
            else:
                # (the bf16 multi launch writes bf16 only: its single-problem form, which it is defined by, per segment)
                for i, o, (m, k) in zip(idl, outs_b, shapes):
                    ops._gather_mean_raw(dec.data, D, i, m, k, out_dtype, old, out=o)
            for a, b in zip(outs_a, outs_b):
                assert torch.equal(a, b), (D, n, out_dtype)


def test_bad_arguments_are_refused():
    st, dec = _stores(100)
    L, nat = gs._native.lib(), gs._native
    ids = _ids(700, 8, 0)
    out = torch.zeros(8, 104, dtype=torch.bfloat16, device=DEV)
    rc = L.gsage_gather_mean_fp8(st.data.data_ptr(), 100, st.scale.data_ptr(), ids.data_ptr(), 8, 1, 100,
                                 out.data_ptr(), nat.BF16, 104, None)
    assert rc == -1 and b"16-byte chunks" in L.gsage_last_error()
    with pytest.raises(RuntimeError):        # the bf16 / fp32 entry point never reads FP8 bytes
        ops._gather_mean_raw(st.data, 100, ids, 8, 1, torch.bfloat16)
    with pytest.raises(AssertionError):
        ops.gather_mean_multi([(st.data, ids, out, 8, 1)], st.ld, 100, 104)


# ---- module path -------------------------------------------------------------------------------------------------
def _graph(n_nodes, deg, seed):
    rng = np.random.RandomState(seed)
    r = np.repeat(np.arange(1, n_nodes), deg)
    c = np.tile(np.arange(deg), n_nodes - 1)
    v = rng.randint(1, n_nodes, size=r.shape[0])
    return sparse.csr_matrix((v, (r, c)), shape=(n_nodes, deg))


def _model(agg, prep, adj, D, n_nodes, fans=(5, 3), dims=(64, 64), C=5, rng="philox"):
    specs = [{"n_train_samples": f, "n_val_samples": f, "output_dim": d,
              "activation": F.relu if i < len(fans) - 1 else (lambda x: x)} for i, (f, d) in enumerate(zip(fans, dims))]
    torch.manual_seed(0)
    m = gs.GSSupervised(sampler_class=gs.sampler_lookup["sparse_uniform_neighbor_sampler"], adj=adj, train_adj=adj,
                        prep_class=gs.prep_lookup[prep], aggregator_class=gs.aggregator_lookup[agg],
                        input_dim=D, n_nodes=n_nodes, n_classes=C, layer_specs=specs)
    for s in (m.train_sampler, m.val_sampler):
        s.rng = rng
    return m


@pytest.mark.parametrize("agg", ["mean", "max_pool", "mean_pool", "lstm", "attention"])
@pytest.mark.parametrize("prep", ["identity", "linear"])
def test_module_path_on_an_fp8_store_equals_the_decoded_bf16_store(agg, prep):
    """Forward / backward / evaluate for every prep x aggregator: the FP8 store's rows reach every kernel as the very
    bf16 numbers the decoded store holds, so two train steps leave identical predictions and weights."""
    n, D = 400, 40
    adj = _graph(n, 7, 3)
    st, dec = _stores(D, seed=5, rows=n)
    ids = torch.arange(1, 65, device=DEV)
    tg = (torch.arange(64, device=DEV) % 5).view(-1, 1)
    res = []
    for feats in (st, dec):
        m = _model(agg, prep, adj, D, n).to(DEV)
        preds = []
        for step in range(2):
            for s in (m.train_sampler, m.val_sampler):
                s.seed, s.calls = 77, 10 * step              # the same Philox draws for both stores
            np.random.seed(step)
            torch.manual_seed(step)
            preds.append(m.train_step(ids, feats, tg, gs.ProblemLosses.classification).detach().clone())
        m.eval()
        np.random.seed(9)
        with torch.no_grad():
            preds.append(m(ids, feats, train=False).clone())
        res.append((preds, [p.detach().clone() for p in m.parameters()]))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    for a, b in zip(res[0][1], res[1][1]):
        assert torch.equal(a, b)


def test_full_neighbour_on_an_fp8_store():
    n, D = 400, 40
    adj = _graph(n, 7, 4)
    st, dec = _stores(D, seed=6, rows=n)
    m = _model("mean", "identity", adj, D, n).to(DEV)
    assert torch.equal(gs.full_neighbour(m, st), gs.full_neighbour(m, dec))


# ---- the mean engine ---------------------------------------------------------------------------------------------
def _engine_problem(n, D, C, seed):
    rng = np.random.RandomState(seed)
    deg = rng.randint(0, 30, size=n + 1)
    deg[0], deg[7] = 0, 0
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    data = rng.randint(1, n + 1, size=int(indptr[-1]))
    adj = sparse.csr_matrix((data, gs.store.row_positions(indptr), indptr), shape=(n + 1, int(deg.max())))
    feats = (rng.normal(size=(n + 1, D)) * rng.uniform(0.1, 4.0, size=D)).astype(np.float32)
    feats[0] = 0
    return adj, feats, rng


def _engine_model(adj, D, C, dims, fans):
    m = _model("mean", "identity", adj, D, adj.shape[0], fans=fans, dims=dims, C=C)
    m.train_sampler.seed = m.val_sampler.seed = 77
    return m.to(DEV)


def _engine_case(fans, dims, D, B, C, queued, capture):
    adj, feats, rng = _engine_problem(3000, D, C, seed=len(fans))
    st = gs.FeatureStore.from_array(feats, torch.device(DEV), dtype="fp8")
    dec = st.decoded("bf16")
    ids_all = torch.from_numpy(rng.randint(1, adj.shape[0], size=(3, B))).to(DEV)
    tg_all = torch.from_numpy(rng.randint(0, C, size=(3, B, 1))).to(DEV)
    res = []
    for store in (st, dec):
        model = _engine_model(adj, D, C, dims, fans)
        assert gs.engine.fused_engine_for(model, store) is gs.engine.FusedMeanTrainStep
        eng = gs.engine.FusedMeanTrainStep(model, store, gs.ProblemLosses.classification, ids_all[0], tg_all[0],
                                           capture=capture)
        assert eng.fp8 == store.is_fp8 and eng.tdt == torch.bfloat16 and eng.sdt == store.dtype
        preds = []
        if queued:
            eng.load_epoch(ids_all, tg_all)
            preds = [eng.step_queue().clone() for _ in range(3)]
            assert not (store.is_fp8 and eng._tail_rows)     # no gather role reads FP8 bytes
        else:
            preds = [eng(ids_all[k], tg_all[k]).clone() for k in range(3)]
        torch.cuda.synchronize()
        gs.store.DeviceCSR.check(eng.csr)
        # the evaluator follows the training engine: the forward launches over the validation sampler
        ev = gs.engine.FusedMeanTrainStep(model, store, gs.ProblemLosses.classification, ids_all[0], tg_all[0],
                                          eval_only=True)
        assert ev.fp8 == store.is_fp8
        res.append((preds, eng.flat_p.clone(), [p.detach().clone() for p in model.parameters()]))
        eng.close()
    for k, (a, b) in enumerate(zip(res[0][0], res[1][0])):
        assert torch.isfinite(a).all() and torch.equal(a, b), "predictions differ after step %d" % (k + 1)
    assert torch.equal(res[0][1], res[1][1])
    assert all(torch.equal(a, b) for a, b in zip(res[0][2], res[1][2]))
    assert not torch.equal(res[0][0][0], res[0][0][2])


@pytest.mark.parametrize("queued,capture", [(False, False), (False, "cmdlist"), (True, "cmdlist")])
def test_mean_engine_headline_like_shape_equals_the_decoded_bf16_store(queued, capture):
    """B = 64, fan-out 25/10, D = 602, 41 classes: three steps, same seeds, same Philox stream."""
    _engine_case((25, 10), (128, 128), 602, 64, 41, queued, capture)


@pytest.mark.parametrize("queued,capture", [(False, False), (True, "cmdlist")])
def test_mean_engine_papers_shape_equals_the_decoded_bf16_store(queued, capture):
    """Three layers, fan-out 15/10/5, D = 128."""
    _engine_case((15, 10, 5), (128, 128, 128), 128, 64, 41, queued, capture)


def test_other_engines_and_fp32_compute_refuse_an_fp8_store():
    adj, feats, _ = _engine_problem(500, 40, 5, seed=9)
    st = gs.FeatureStore.from_array(feats, torch.device(DEV), dtype="fp8")
    for agg, eng in (("max_pool", "FusedPoolTrainStep"), ("attention", "FusedAttnTrainStep")):
        m = _model(agg, "identity", adj, 40, adj.shape[0]).to(DEV)
        assert gs.engine.fused_engine_for(m, st) is None
        assert "FP8" in gs.engine.why_no_fused_engine(m, st)[eng]
    m = _model("mean", "identity", adj, 40, adj.shape[0]).to(DEV)
    assert gs.engine.fused_engine_for(m, st) is gs.engine.FusedMeanTrainStep
    ops.set_compute_dtype("fp32")
    assert gs.engine.fused_engine_for(m, st) is None
    assert "FP8" in gs.engine.why_no_fused_engine(m, st)["FusedMeanTrainStep"]
    ops.set_compute_dtype("bf16")
    m = _model("mean", "node_embedding", adj, 40, adj.shape[0]).to(DEV)
    assert gs.engine.fused_engine_for(m, st) is None


# ---- CLI -----------------------------------------------------------------------------------------------------------
def _cli_problem():
    rng = np.random.RandomState(5)
    n, D, C = 600, 24, 4
    adj, _, _ = _engine_problem(n, D, C, seed=21)
    feats = rng.normal(size=(n + 1, D)).astype(np.float32)
    feats[0] = 0
    folds = np.array(["train"] * 400 + ["val"] * 100 + ["test"] * (n + 1 - 500))
    folds[0] = "dummy"
    return gs.NodeProblem.from_arrays("classification", C, adj, adj, feats, folds,
                                      feats[:, :C].argmax(1).reshape(-1, 1), cuda=True)


@pytest.mark.parametrize("agg", ["mean", "max_pool"])
def test_cli_feature_dtype_fp8(agg, capsys):
    train = importlib.import_module("pytorch-graphsage_amd.train")
    prob = _cli_problem()
    train.main(["--problem-path", "<memory>", "--epochs", "6", "--batch-size", "64", "--sampler-class",
                "sparse_uniform_neighbor_sampler", "--n-train-samples", "5,3", "--n-val-samples", "5,3",
                "--output-dims", "128,128", "--feature-dtype", "fp8", "--aggregator-class", agg, "--lr-init", "0.01"],
               problem=prob)
    cap = capsys.readouterr()
    assert prob.feats.is_fp8
    assert "quantised to FP8" in cap.err and "MB ->" in cap.err and "largest absolute error" in cap.err
    if agg == "mean":
        assert "train_step runs on FusedMeanTrainStep" in cap.err
    else:
        assert "FP8" in cap.err and "using the module path" in cap.err
    lines = [json.loads(l) for l in cap.out.splitlines() if l.startswith("{") and "train_metric" in l]
    first = next(l["train_metric"] for l in lines if l.get("train_metric") is not None)
    last = lines[-1]["train_metric"]
    assert last["micro"] > first["micro"], (first, last)      # it trains
    assert lines[-1]["val_metric"] is not None
