"""Weighted graphs on the GPU (csrc/gsage_weighted.hip, the WEIGHTED_MEAN mode of csrc/gsage_fullgraph.hip) against the
restatements of tests/weighted_ref.py: the table and the sampler bit for bit, the weight-normalised mean against float64
within a derived bound (weighted_ref.compare) that is shown to catch a dropped edge and ignored weights, the weighted
sampler through GSSupervised.train_step against the same model on CPU tensors, and infer.embeddings against host mode."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

import segment_reduce_ref as sr
import weighted_ref as wr
from conftest import pkg
from util import close, note_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x0123456789ABCDEF
WIDTHS_256 = {"bf16": [7, 64, 136, 520], "fp32": [3, 33, 130, 260]}     # as tests/test_gpu_segment_reduce.py

_ADJ = {}


def _adj():
    if "adj" not in _ADJ:
        _ADJ["adj"] = wr.graph().csr(DEV)
    return _ADJ["adj"]


def test_cdf_build_equals_the_restatement():
    gs = pkg()
    g = wr.graph()
    before = gs._native.launch_count()
    adj = g.csr(DEV)
    assert gs._native.launch_count() - before == 2
    assert adj.edge_cdf.dtype == torch.int64 and adj.edge_cdf.is_cuda
    assert torch.equal(adj.edge_cdf.cpu(), torch.from_numpy(g.cdf.view(np.int64)))
    assert torch.equal(adj.edge_cdf.cpu(), g.csr("cpu").edge_cdf)         # host mode: the same bits
    again = g.csr(DEV)
    assert torch.equal(again.edge_cdf, adj.edge_cdf)
    with pytest.raises(ValueError, match="finite and >= 0"):
        w = torch.from_numpy(g.weight.copy()).to(DEV)
        w[5] = float("nan")
        g.csr(DEV, weighted=False).with_weights(w)


# ---- the sampler -------------------------------------------------------------------------------------------------
_SAMPLES = {}


def _ids(M):
    g = wr.graph()
    ids = np.random.RandomState(100 + M).randint(0, g.n, size=M)
    ids[0] = wr.ROWS[1000]
    if M > 8:
        ids[1:8] = [wr.ROWS[k] for k in ("degree 0", "all zero", "all denormal", "maximum 3.4e38", 257, 300,
                                         "one drawable of 20")]
    return ids


def _ref(M, n, call, g0):
    """the restatement's draw, computed once per argument set"""
    key = (M, n, call, g0)
    if key not in _SAMPLES:
        g = wr.graph()
        out, err = wr.sample(g.rowptr, g.col, g.cdf, g.n, _ids(M), n, SEED, call, g0)
        assert err == 0
        _SAMPLES[key] = out
    return _SAMPLES[key]


def _draw(adj, ids, n, **ph):
    gs = pkg()
    return gs.ops.sample_csr_weighted(adj, torch.as_tensor(ids).to(DEV), n, dict(seed=SEED, **ph))


@pytest.mark.parametrize("n", [1, 10, 25])
@pytest.mark.parametrize("M", [1, 37, 600])
def test_sampler_equals_the_restatement(M, n):
    adj, ids = _adj(), _ids(M)
    # g0 even and odd (a Philox block holds two draws), small and beyond 2^32; the call index beyond 2^32 too
    for call, g0 in ((0, 0), (3, 2 * M * n + 1), ((1 << 40) + 3, (1 << 33) + 6)):
        if M == 600 and n == 25 and call > 3:
            continue                                                    # (the largest case: two restatements are enough)
        got = _draw(adj, ids, n, call_base=call, g0=g0)
        assert np.array_equal(got.cpu().numpy(), _ref(M, n, call, g0)), (M, n, call, g0)
    # the call index as a device counter and as a host base
    ctr = torch.tensor([2], dtype=torch.int64, device=DEV)
    a = _draw(adj, ids, n, call_base=1, call_ctr=ctr, g0=2 * M * n + 1)
    assert np.array_equal(a.cpu().numpy(), _ref(M, n, 3, 2 * M * n + 1))
    # two calls with the same arguments
    assert torch.equal(a, _draw(adj, ids, n, call_base=3, g0=2 * M * n + 1))
    assert int(adj.err_flag.item()) == 0


@pytest.mark.parametrize("M,n", [(37, 10), (600, 25), (37, 1)])
def test_two_ranks_shards_are_the_one_rank_draw(M, n):
    adj, ids = _adj(), _ids(M)
    h = M // 2                                                          # (h * n odd for (37, 1): rank 1 starts mid-block)
    whole = _draw(adj, ids, n, call_base=0, g0=0)
    parts = torch.cat([_draw(adj, ids[:h], n, call_base=0, g0=0), _draw(adj, ids[h:], n, call_base=0, g0=h * n)])
    assert torch.equal(whole, parts)
    assert np.array_equal(whole.cpu().numpy(), _ref(M, n, 0, 0))


def test_out_of_range_id_yields_zero_and_raises():
    g = wr.graph()
    adj = g.csr(DEV)
    ids = _ids(37).copy()
    ids[5], ids[20] = g.n, -1
    got = _draw(adj, ids, 10, call_base=0, g0=0).cpu().numpy()
    ref, err = wr.sample(g.rowptr, g.col, g.cdf, g.n, ids, 10, SEED, 0, 0)
    assert err == 1 and np.array_equal(got, ref) and (got[50:60] == 0).all() and (got[200:210] == 0).all()
    with pytest.raises(IndexError):
        adj.check()
    adj.check()


def test_sampler_class_on_the_gpu():
    gs = pkg()
    p = wr.weighted_problem()
    wa = gs.WeightedAdj(p["adj"], p["weight"])
    s = gs.find_sampler("sparse_weighted_neighbor_sampler")(adj=wa, seed=5)
    h = gs.find_sampler("sparse_weighted_neighbor_sampler")(adj=wa, seed=5)
    ids = torch.arange(0, 201)
    for n in (3, 7):
        assert torch.equal(s(ids.to(DEV), n).cpu(), h(ids, n))
    assert torch.equal(s.csr(DEV).edge_cdf.cpu(), h.csr("cpu").edge_cdf)
    ctr = torch.tensor([2], dtype=torch.int64, device=DEV)
    s.begin_capture(ctr)
    a = s(ids.to(DEV), 3)
    assert s.calls_in_capture() == 1 and torch.equal(a.cpu(), h(ids, 3))
    s.csr(DEV).check()


# ---- the weight-normalised mean --------------------------------------------------------------------------------------
_MEANS = {}


def _mean_ref(D, tdt):
    key = (D, tdt)
    if key not in _MEANS:
        g = wr.graph()
        table, _ = sr.inputs(g.n, D, tdt, seed=3000 + D)
        _MEANS[key] = (table,) + wr.weighted_mean(g.rowptr, g.col, g.cdf, table)
    return _MEANS[key]


def _plan(adj, slice_len):
    gs = pkg()
    p = dict(gs.infer.plan(adj) if slice_len == gs.infer.SLICE_LEN else gs.infer.plan(adj, slice_len=slice_len))
    assert p["slice_len"] == slice_len
    return p


def _launch(adj, plan, table, D, out, act):
    gs = pkg()
    nat, ops = gs._native, gs.ops
    ldp = int(nat.lib().gsage_segment_reduce_ldp(D))
    partials = torch.empty(max(plan["n_slices"], 1), ldp, dtype=torch.float32, device=table.device)
    nat.check(nat.lib().gsage_segment_reduce_weighted(
        ops._ptr(table), ops._code(table.dtype), table.stride(0), D, ops._ptr(adj.rowptr), ops._ptr(adj.col),
        ops._ptr(adj.edge_cdf), adj.n_rows, ops._ptr(plan["order"]), plan["n_short"], ops._ptr(plan["slices"]),
        plan["n_slices"], ops._ptr(plan["long_rows"]), plan["n_long"], plan["slice_len"], ops._ptr(partials), ldp,
        ops._ptr(out), ops._code(out.dtype), out.stride(0), nat.ACT_RELU if act == "relu" else nat.ACT_NONE,
        ops._ptr(adj.err_flag), ops._stream()), "segment_reduce_weighted")


def _run(adj, plan, values, D, tdt, odt, act, wide=False, use_infer=False):
    gs = pkg()
    g = wr.graph()
    table = sr.device_table(values, tdt, wide, DEV)
    buf, out = sr.out_buffer(g.n, D, odt, DEV)
    if use_infer:
        nat = gs._native
        gs.infer.segment_reduce(adj, table[:, :D], nat.SEG_WEIGHTED_MEAN, out, nat.ACT_RELU if act == "relu" else nat.ACT_NONE)
    else:
        _launch(adj, plan, table, D, out, act)
    host = buf.cpu()
    assert bool((sr.bits(host[:, D:]) == sr.bits(torch.full_like(host[:, D:], sr.OUT_PAD))).all()), \
        ("columns at and beyond D were written", tdt, odt, D, act)
    return host[:, :D].contiguous()


@pytest.mark.parametrize("slice_len", [256, 8])
@pytest.mark.parametrize("tdt,D", [(t, D) for t in ("bf16", "fp32") for D in WIDTHS_256[t]])
def test_weighted_mean_against_float64(tdt, D, slice_len):
    g, adj = wr.graph(), _adj()
    plan = _plan(adj, slice_len)
    long_rows = {int(v) for v in plan["long_rows"][:, 0].cpu()}
    if slice_len == 256:
        assert long_rows == {wr.ROWS[257], wr.ROWS[300], wr.ROWS[1000], wr.ROWS["all zero, 300 edges"]}
    else:
        assert {wr.ROWS["all zero, 12 edges"], wr.ROWS["one drawable of 20"], wr.ROWS[63]} <= long_rows
        assert plan["n_short"] > 20
    values, ref, S, k = _mean_ref(D, tdt)
    assert k[wr.ROWS["one drawable of 20"]] == 1 and k[wr.ROWS["degree 1"]] == 1 and k[wr.ROWS["all zero"]] == 1
    for odt in ("fp32", "bf16"):
        for act in ("none", "relu"):
            for wide in (False, True):
                what = ("table " + tdt, "out " + odt, "D %d" % D, act, "slice_len %d" % slice_len, "wide" if wide else "")
                got = _run(adj, plan, values, D, tdt, odt, act, wide, use_infer=(slice_len == 256 and not wide))
                worst = wr.compare(got, ref, S, k, odt, what, act)
                if act == "none" and not wide:
                    note_parity("weighted/L%d/%s-%s/D%d" % (slice_len, tdt, odt, D), kernel=worst,
                                bound_units_of_2m24=float((k.max() + 2)))
    assert int(adj.err_flag.item()) == 0


@pytest.mark.parametrize("slice_len", [256, 8])
def test_comparison_sees_a_dropped_edge_and_ignored_weights(slice_len):
    """fp32 in and out: the kernel passes the comparison; the same comparison fails against a reference that lost one
    edge (of a short row, and the last edge of the degree-1000 row's last slice) or that weighs the edges equally"""
    g, adj = wr.graph(), _adj()
    D = 33
    values, ref, S, k = _mean_ref(D, "fp32")
    got = _run(adj, _plan(adj, slice_len), values, D, "fp32", "fp32", "none")
    wr.compare(got, ref, S, k, "fp32", "intact reference")
    short = next(v for v in range(21, g.n) if 3 <= k[v] and g.deg[v] <= 8)
    quanta = lambda v: np.diff(np.concatenate([[0], g.cdf[g.rowptr[v]:g.rowptr[v + 1]].astype(np.int64)]))
    last = int(np.flatnonzero(quanta(wr.ROWS[1000]))[-1])              # the last drawable edge of the last slice
    assert last >= 992
    for v, e in ((short, int(np.argmax(quanta(short)))), (wr.ROWS[1000], last)):
        r2, S2, _ = wr.weighted_mean(g.rowptr, g.col, g.cdf, values, drop=(v, e))
        with pytest.raises(AssertionError, match="row %d " % v):
            wr.compare(got, r2, S2, k, "fp32", "dropped edge")
    r3, S3, _ = wr.weighted_mean(g.rowptr, g.col, g.cdf, values, equal=True)
    with pytest.raises(AssertionError, match="beyond the bound"):
        wr.compare(got, r3, S3, k, "fp32", "equal weights")


def test_weighted_mean_two_calls_are_bit_equal():
    adj = _adj()
    values = _mean_ref(136, "bf16")[0]
    for slice_len in (256, 8):
        plan = _plan(adj, slice_len)
        a = _run(adj, plan, values, 136, "bf16", "fp32", "none")
        assert torch.equal(sr.bits(a), sr.bits(_run(adj, plan, values, 136, "bf16", "fp32", "none")))


# ---- through the model -----------------------------------------------------------------------------------------------
def _model(gs, p, agg, prep="identity", dims=(16, 16), fan=(4, 3), seed=0):
    torch.manual_seed(seed)
    specs = [{"n_train_samples": f, "n_val_samples": f, "output_dim": h,
              "activation": (lambda x: x) if i == len(dims) - 1 else F.relu} for i, (f, h) in enumerate(zip(fan, dims))]
    wa = gs.WeightedAdj(p["adj"], p["weight"])
    return gs.GSSupervised(sampler_class=gs.find_sampler("sparse_weighted_neighbor_sampler"), adj=wa, train_adj=wa,
                           prep_class=gs.prep_lookup[prep], aggregator_class=gs.aggregator_lookup[agg],
                           input_dim=p["feats"].shape[1], n_nodes=201, n_classes=p["C"], layer_specs=specs)


def test_train_step_equals_the_cpu_model():
    """mean aggregator, two steps, fp32: host mode draws the same frontiers (both are Philox); predictions and updated
    weights at the bounds tests/test_gpu_model.py applies to module-path steps in fp32"""
    gs = pkg()
    gs.ops.set_compute_dtype("fp32")
    try:
        p = wr.weighted_problem()
        host, dev = _model(gs, p, "mean"), _model(gs, p, "mean").to(DEV)
        for m in (host, dev):
            m.optimizer = torch.optim.Adam(m.parameters(), lr=0.01)
        store = gs.FeatureStore.from_array(p["feats"], torch.device(DEV), dtype="fp32")
        feats = torch.from_numpy(p["feats"])
        rng = np.random.RandomState(1)
        before = gs._native.launch_count()
        for step in range(2):
            ids = torch.from_numpy(rng.randint(1, 201, size=48))
            tg = torch.from_numpy(p["targets"][ids.numpy()])
            a = host.train_step(ids, feats, tg, gs.ProblemLosses.classification)
            b = dev.train_step(ids.to(DEV), store, tg.to(DEV), gs.ProblemLosses.classification)
            close(b.detach().cpu().numpy(), a.detach().numpy(), ("preds", step), 1e-4, 1e-5)
        assert gs._native.launch_count() - before >= 12
        assert dev.train_sampler.calls == host.train_sampler.calls == 4
        hs = host.state_dict()
        for name, v in dev.state_dict().items():
            close(v.cpu().numpy(), hs[name].numpy(), ("weights", name), 2e-4, 2e-5)
        dev.train_sampler.csr(DEV).check()
    finally:
        gs.ops.set_compute_dtype("bf16")


@pytest.mark.parametrize("agg", ["mean", "mean_pool"])
def test_embeddings_equal_host_mode(agg):
    gs = pkg()
    gs.ops.set_compute_dtype("fp32")
    try:
        p = wr.weighted_problem()
        host, dev = _model(gs, p, agg, "linear", seed=3), _model(gs, p, agg, "linear", seed=3).to(DEV)
        ref = gs.embeddings(host, torch.from_numpy(p["feats"]))
        got = gs.embeddings(dev, torch.from_numpy(p["feats"]).to(DEV))
        close(got.cpu().numpy(), ref.numpy(), "gpu vs host", 2e-5, 2e-5)
        ref64 = wr.dense_reference(host, p["feats"], p["indptr"], p["data"], p["w"])[1]
        close(got.cpu().numpy(), ref64, "gpu vs float64", 2e-5, 2e-5)
        with pytest.raises(ValueError, match="max-pool and attention"):
            gs.embeddings(_model(gs, p, "max_pool").to(DEV), torch.from_numpy(p["feats"]).to(DEV))
    finally:
        gs.ops.set_compute_dtype("bf16")
