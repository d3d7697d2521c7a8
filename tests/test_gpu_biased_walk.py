"""-m gpu: biased walks on the MI355X (include/gsage.h, "Biased walks").  gsage_unsup_batch_biased and
gsage_importance_walks_biased against the restatement of tests/biased_walk_ref.py, every comparison torch.equal: the
membership scan at the edges of its 64-column trips, a step that exhausts its 32 rounds, the builder over batch sizes,
lengths, uniform and weighted proposals, shards, the call counter and the error flag, neutral parameters against the
three legacy entries, importance walks over the size classes of the sorts with restarts, GSUnsupervised(walk_p, walk_q),
both fused unsupervised engines against the module path (ids and frontiers bit for bit, one step at the tolerances of
tests/test_gpu_unsup_engine.py: bf16 loss 3e-2, gradients 0.1, first-step weights 0.05), and host mode."""
import numpy as np
import pytest
import torch

import biased_walk_ref as br
import unsup_engine_ref as uref
import unsup_ref
import unsup_weighted_ref as ur
import weighted_ref as wr
from conftest import pkg

pytestmark = pytest.mark.gpu
gs = pkg()
ops = gs.ops
nat = gs._native
DEV = "cuda"
SEED = br.SEED
P, Q_ = 0.5, 4.0                   # theta = (2^32, 2^31, 2^29): three classes, and a band only the scan decides


@pytest.fixture(autouse=True)
def _warm():
    ops.set_compute_dtype("bf16")
    ops.warmup(torch.device(DEV))
    yield
    ops.set_compute_dtype("bf16")


_G = {}


def _walk_graph():
    if "walk" not in _G:
        rowptr, col = unsup_ref.walk_graph()
        _G["walk"] = wr.Graph(rowptr, col, np.ones(len(col), dtype=np.float32))
    return _G["walk"]


def _setup(g, weighted):
    """(device adjacency, the negatives' table on the device and as the restatement's input), once per (graph, mode)"""
    key = (id(g), weighted)
    if key not in _G:
        csr = g.csr(DEV, weighted=weighted)
        cdf = ops.neg_cdf(csr, weighted=weighted)
        _G[key] = (csr, cdf, cdf.cpu().numpy(), g)
    return _G[key][:3]


def _equal(got, ref):
    return torch.equal(got[0].cpu(), torch.from_numpy(ref[0])) and torch.equal(got[1].cpu(), torch.from_numpy(ref[1]))


# ---- 1. the membership scan ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [4.0, 0.25])
@pytest.mark.parametrize("weighted", [False, True])
def test_membership_scan_edges(weighted, q):
    """previous-node rows of degree 1, 63 .. 65, 128, 129, 255 .. 257 and 1000 with the candidate first, last, absent or repeated
    (biased_walk_ref.gadget_graph): p = 1, so theta_near != theta_far and three words in four fall between them"""
    g, cases = br.gadget_graph()
    assert {d for _, d, _ in cases} == set(br.GADGET_DEGREES) and {s for _, _, s in cases} == set(br.PLACEMENTS)
    csr, cdf, cdf_np = _setup(g, weighted)
    seeds = np.repeat(np.array([t for t, _, _ in cases], dtype=np.int64), 40)
    trace = []
    ref = br.build_batch(g.rowptr, g.col, g.cdf if weighted else None, g.n, seeds, 16, 1, cdf_np, SEED, 1, 1.0, q,
                         trace=trace)
    got = ops.unsup_batch(csr, torch.from_numpy(seeds).to(DEV), 16, 1, cdf, {"seed": SEED, "call_base": 1},
                          weighted=weighted, p=1.0, q=q)
    assert ref[2] == 0 and int(csr.err_flag.item()) == 0
    assert sum(1 for _, _, scanned in trace if scanned) >= 4 * len(cases)    # (final rounds only: the trace's unit is a step)
    assert _equal(got, ref)
    # the class decides where walks end: the candidate x is taken more often where row t stores it, or less (q < 1)
    B = len(seeds)
    pos = ref[0][B:2 * B]
    share = {}
    for k, (t, d, place) in enumerate(cases):
        mine = pos[40 * k:40 * (k + 1)]
        share.setdefault(place == "absent", []).append(float((mine == t + 2).sum()) / max(1, int((mine >= t + 2).sum())))
    near, far = np.mean(share[False]), np.mean(share[True])
    assert (near > far + 0.15) if q > 1 else (near < far - 0.15), (near, far)


# ---- 2. a step that exhausts its rounds -----------------------------------------------------------------------------------------
def test_exhausted_rounds_take_the_last_proposal():
    g = br.star_graph()
    csr, cdf, cdf_np = _setup(g, False)
    B = 2048
    seeds = np.zeros(B, dtype=np.int64)                        # every walk starts on the hub; a leaf's only neighbour is t
    trace = []
    ref = br.build_batch(g.rowptr, g.col, None, g.n, seeds, 4, 1, cdf_np, SEED, 2, 8.0, 1.0, trace=trace)
    assert any(n == br.ROUNDS and not ok for n, ok, _ in trace)               # on the reference: some step ran out
    assert not any(scanned for _, _, scanned in trace)                         # q = 1: no row is ever read
    got = ops.unsup_batch(csr, torch.from_numpy(seeds).to(DEV), 4, 1, cdf, {"seed": SEED, "call_base": 2}, p=8.0, q=1.0)
    assert _equal(got, ref) and int(csr.err_flag.item()) == 0


# ---- 3. the builder ---------------------------------------------------------------------------------------------------------------
def _seeds(g, B, weighted):
    rng = np.random.RandomState(B)
    if weighted:
        return ur.seeds_on_rows(g, B, rng) if B > 1 else np.asarray([wr.ROWS[1000]], dtype=np.int64)
    return rng.randint(0, g.n, size=B).astype(np.int64)


@pytest.mark.parametrize("Q", [1, 20])
@pytest.mark.parametrize("walk_len", [1, 2, 16])
@pytest.mark.parametrize("B", [1, 4, 5, 257])
@pytest.mark.parametrize("weighted", [False, True])
def test_builder_bit_exact(weighted, B, walk_len, Q):
    g = wr.graph() if weighted else _walk_graph()              # weighted: rows of <= 64 and > 64 edges, quanta 0, T_v = 0
    csr, cdf, cdf_np = _setup(g, weighted)
    seeds = _seeds(g, B, weighted)
    if weighted and B == 257:
        assert set(wr.ROWS.values()) <= set(seeds.tolist())
    ref = br.build_batch(g.rowptr, g.col, g.cdf if weighted else None, g.n, seeds, walk_len, Q, cdf_np, SEED, 2, P, Q_)
    sd = torch.from_numpy(seeds).to(DEV)
    before = nat.launch_count()
    got = ops.unsup_batch(csr, sd, walk_len, Q, cdf, {"seed": SEED, "call_base": 2}, weighted=weighted, p=P, q=Q_)
    assert nat.launch_count() - before == 1
    assert ref[2] == 0 and int(csr.err_flag.item()) == 0
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and _equal(got, ref)
    plain = ops.unsup_batch(csr, sd, walk_len, Q, cdf, {"seed": SEED, "call_base": 2}, weighted=weighted)
    assert torch.equal(got[0][2 * B:], plain[0][2 * B:])      # the negatives' role is shared
    if walk_len == 1:                                          # a walk's first step is first-order
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    elif B == 257:
        assert not torch.equal(got[0], plain[0])


@pytest.mark.parametrize("weighted", [False, True])
def test_builder_shards_counter_and_errors(weighted):
    g = wr.graph() if weighted else _walk_graph()
    csr, cdf, cdf_np = _setup(g, weighted)
    ecdf = g.cdf if weighted else None
    B, wl, Q = 37, 16, 20
    seeds = torch.from_numpy(_seeds(g, B, weighted)).to(DEV)
    kw = dict(weighted=weighted, p=P, q=Q_)
    ph = {"seed": SEED, "call_base": 4}
    ids, pw = ops.unsup_batch(csr, seeds, wl, Q, cdf, ph, **kw)
    sid, spw = ops.unsup_batch(csr, seeds[13:37], wl, Q, cdf, dict(ph, g0=13), **kw)
    assert torch.equal(sid[:24], ids[13:37]) and torch.equal(sid[24:48], ids[B + 13:B + 37])
    assert torch.equal(sid[48:], ids[2 * B:]) and torch.equal(spw, pw[13:37])
    hid, hpw = ops.unsup_batch(csr, seeds[:13], wl, Q, cdf, ph, **kw)
    assert torch.equal(torch.cat([hid[:13], sid[:24]]), ids[:B]) and torch.equal(torch.cat([hid[13:26], sid[24:48]]),
                                                                                 ids[B:2 * B])
    assert torch.equal(torch.cat([hpw, spw]), pw)
    # a device word advances the stream
    ctr = torch.ones(1, dtype=torch.int64, device=DEV)
    cid, cpw = ops.unsup_batch(csr, seeds, wl, Q, cdf, {"seed": SEED, "call_base": 3, "call_ctr": ctr}, **kw)
    assert torch.equal(cid, ids) and torch.equal(cpw, pw)
    ctr.fill_(2)
    nid, npw = ops.unsup_batch(csr, seeds, wl, Q, cdf, {"seed": SEED, "call_base": 3, "call_ctr": ctr}, **kw)
    ref = br.build_batch(g.rowptr, g.col, ecdf, g.n, seeds.cpu().numpy(), wl, Q, cdf_np, SEED, 5, P, Q_)
    assert _equal((nid, npw), ref) and not torch.equal(nid[B:2 * B], ids[B:2 * B])
    # a seed outside the graph raises the flag and yields 0
    for outside in (g.n, -1):
        bad = seeds.clone()
        bad[3] = outside
        got = ops.unsup_batch(csr, bad, wl, Q, cdf, ph, **kw)
        ref = br.build_batch(g.rowptr, g.col, ecdf, g.n, bad.cpu().numpy(), wl, Q, cdf_np, SEED, 4, P, Q_)
        assert ref[2] == 1 and int(csr.err_flag.item()) == 1
        csr.err_flag.zero_()
        assert _equal(got, ref) and int(got[0][3]) == 0 and int(got[0][B + 3]) == 0 and float(got[1][3]) == 0
    # a stored column outside the graph: the walk that proposes it ends at 0, the seed stays
    col = g.col.copy()
    rows = [v for v in range(g.n) if g.deg[v] >= 1 and (not weighted or int(g.cdf[g.rowptr[v + 1] - 1]) > 0)][:6]
    for k, v in enumerate(rows):
        e = int(g.rowptr[v]) + int(np.argmax(g.weight[g.rowptr[v]:g.rowptr[v + 1]]))
        col[e] = g.n if k % 2 == 0 else -5
    broken = gs.DeviceCSR(torch.from_numpy(g.rowptr).to(DEV), torch.from_numpy(col).to(DEV), g.n, int(g.deg.max()))
    if weighted:
        broken = broken.with_weights(torch.from_numpy(g.weight).to(DEV))
    start = seeds.clone()
    start[:6] = torch.tensor(rows)
    got = ops.unsup_batch(broken, start, wl, Q, cdf, ph, **kw)
    ref = br.build_batch(g.rowptr, col, ecdf, g.n, start.cpu().numpy(), wl, Q, cdf_np, SEED, 4, P, Q_)
    assert ref[2] == 1 and int(broken.err_flag.item()) == 1 and int(csr.err_flag.item()) == 0
    assert _equal(got, ref)
    hit = np.flatnonzero((ref[0][B:2 * B] == 0) & (ref[1] == 1.0))
    assert hit.size >= 1 and all(int(got[0][i]) == int(start[i]) for i in hit)


# ---- 4. neutral parameters through the biased entries -----------------------------------------------------------------------------
def test_neutral_parameters_reproduce_the_legacy_entries():
    for weighted in (False, True):
        g = wr.graph() if weighted else _walk_graph()
        csr, cdf, _ = _setup(g, weighted)
        for B, wl in ((257, 16), (5, 2)):
            seeds = torch.from_numpy(_seeds(g, B, weighted)).to(DEV)
            ph = {"seed": SEED, "call_base": 7, "g0": 3}
            legacy = ops.unsup_batch(csr, seeds, wl, 20, cdf, ph, weighted=weighted)
            forced = ops.unsup_batch(csr, seeds, wl, 20, cdf, ph, weighted=weighted, p=1.0, q=1.0, _biased=True)
            assert torch.equal(legacy[0], forced[0]) and torch.equal(legacy[1], forced[1]), (weighted, B)
    g = wr.graph()
    for weighted in (False, True):
        csr = _setup(g, weighted)[0]
        ids = torch.arange(g.n, device=DEV)
        for R, L, T in ((10, 2, 3), (50, 16, 64), (65, 16, 16)):
            legacy = ops.importance_walks(csr, ids, R, L, T, SEED)
            forced = ops.importance_walks(csr, ids, R, L, T, SEED, _biased=True)
            assert all(torch.equal(a, b) for a, b in zip(legacy, forced)), (weighted, R, L, T)


# ---- 5. importance ------------------------------------------------------------------------------------------------------------------
SOURCES = np.array([wr.ROWS[1000], wr.ROWS["degree 1"], wr.ROWS["degree 0"], wr.ROWS["all zero"], 30, 45, 71, wr.ROWS[65]],
                   dtype=np.int64)


@pytest.mark.parametrize("restart", [0.0, 0.15, 0.9])
@pytest.mark.parametrize("L", [1, 2, 16])
@pytest.mark.parametrize("R", [1, 50, 65])                     # R * L: 1 .. 130 (256 slots), 800 (1024), 1040 (4096)
@pytest.mark.parametrize("weighted", [False, True])
def test_importance_bit_exact(weighted, R, L, restart):
    g = wr.graph()
    csr = _setup(g, weighted)[0]
    ids = torch.from_numpy(SOURCES).to(DEV)
    for T in (1, 16, 64):
        col, w, deg, err = br.rows(g, weighted, SOURCES, R, L, T, P, Q_, restart)
        before = nat.launch_count()
        got = ops.importance_walks(csr, ids, R, L, T, SEED, p=P, q=Q_, restart=restart)
        assert nat.launch_count() - before == 1
        assert err == 0 and int(csr.err_flag.item()) == 0
        assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32 and got[2].dtype == torch.int32
        assert torch.equal(got[0].cpu(), torch.from_numpy(col)), (R, L, T)
        assert torch.equal(got[1].cpu(), torch.from_numpy(w)), (R, L, T)
        assert torch.equal(got[2].cpu(), torch.from_numpy(deg)), (R, L, T)


@pytest.mark.parametrize("weighted", [False, True])
def test_importance_rows_do_not_depend_on_the_launch(weighted):
    g = wr.graph()
    csr = _setup(g, weighted)[0]
    ids = torch.arange(g.n, device=DEV)
    kw = dict(p=P, q=Q_, restart=0.15)
    whole = ops.importance_walks(csr, ids, 50, 5, 16, SEED, **kw)
    again = ops.importance_walks(csr, ids, 50, 5, 16, SEED, **kw)
    assert all(torch.equal(a, b) for a, b in zip(whole, again))                # two calls, equal bits
    perm = torch.from_numpy(np.random.RandomState(1).permutation(g.n)).to(DEV)
    mixed = ops.importance_walks(csr, ids[perm], 50, 5, 16, SEED, **kw)
    assert all(torch.equal(a[perm], b) for a, b in zip(whole, mixed))
    parts = [ops.importance_walks(csr, ids[o:o + 7].flip(0), 50, 5, 16, SEED, **kw) for o in range(0, g.n, 7)]
    for k in range(3):
        assert torch.equal(torch.cat([p_[k].flip(0) for p_ in parts]), whole[k])
    a, b = csr.importance(50, 5, 16, seed=SEED, **kw), csr.importance(50, 5, 16, seed=SEED, chunk=7, **kw)
    assert torch.equal(a.rowptr, b.rowptr) and torch.equal(a.col, b.col) and torch.equal(a.edge_cdf, b.edge_cdf)
    plain = csr.importance(50, 5, 16, seed=SEED)
    assert not (torch.equal(a.rowptr, plain.rowptr) and torch.equal(a.edge_cdf, plain.edge_cdf))
    csr.check()


def test_importance_entry_records_into_a_command_list():
    g = wr.graph()
    csr = _setup(g, True)[0]
    ids = torch.arange(g.n, device=DEV)
    kw = dict(p=P, q=Q_, restart=0.15)
    want = ops.importance_walks(csr, ids, 50, 5, 16, SEED, **kw)
    torch.cuda.synchronize()
    with nat.CommandList.record() as cl:
        got = ops.importance_walks(csr, ids, 50, 5, 16, SEED, **kw)
    assert len(cl) == 1
    for _ in range(2):
        for t in got:
            t.fill_(-1)
        cl.replay(ops._stream())
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(want, got))
    csr.check()


# ---- 6. GPU equals host mode ---------------------------------------------------------------------------------------------------------
def test_gpu_equals_host_mode():
    g = wr.graph()
    for weighted in (False, True):
        csr, cdf, _ = _setup(g, weighted)
        host = g.csr("cpu", weighted=weighted)
        seeds = torch.from_numpy(_seeds(g, 70, True))
        ph = {"seed": SEED, "call_base": 6, "g0": 9}
        a = ops.unsup_batch(csr, seeds.to(DEV), 16, 5, cdf, ph, weighted=weighted, p=4.0, q=0.25)
        b = ops.unsup_batch(host, seeds, 16, 5, cdf.cpu(), ph, weighted=weighted, p=4.0, q=0.25)
        assert torch.equal(a[0].cpu(), b[0]) and torch.equal(a[1].cpu(), b[1])
        ids = torch.arange(g.n)
        c = ops.importance_walks(csr, ids.to(DEV), 65, 5, 16, SEED, p=4.0, q=0.25, restart=0.15)
        d = ops.importance_walks(host, ids, 65, 5, 16, SEED, p=4.0, q=0.25, restart=0.15)
        assert all(torch.equal(x.cpu(), y) for x, y in zip(c, d))


# ---- 7. the model and the engines ------------------------------------------------------------------------------------------------------
WP, WQ = 4.0, 0.25
TRAIN_SEED = 77


def test_model_builds_the_restatements_batches():
    adj, feats, _ = uref.problem()
    model = uref.make_model(gs, adj, feats.shape[1], (16, 8), (5, 3), 20, 1.0, DEV)
    model.walk_p, model.walk_q = WP, WQ
    assert model.biased_walks
    indptr, data = np.asarray(adj.indptr, dtype=np.int64), np.asarray(adj.data)
    seeds = torch.from_numpy(np.random.RandomState(4).randint(1, adj.shape[0], size=64)).to(DEV)
    cdf = model._walk_graph(True, torch.device(DEV))[1].cpu().numpy()
    for call in range(2):
        got = model.build_batch(seeds)
        ref = br.build_batch(indptr, data, None, adj.shape[0], seeds.cpu().numpy(), 5, 20, cdf, TRAIN_SEED, call, WP, WQ)
        assert ref[2] == 0 and _equal(got, ref)
    model.train_sampler.csr(DEV).check()


_WPROBLEM = []


def _weighted_problem():
    if not _WPROBLEM:
        _WPROBLEM.append(wr.weighted_problem())
    return _WPROBLEM[0]


def _twins(weighted, dims, fans, Q, dtype="bf16"):
    """(store, reference model, engine's model, engine class, node count): identical weights, walk_p = 4, walk_q = 0.25"""
    if weighted:
        p = _weighted_problem()
        feats, n = p["feats"], 201

        def mk():
            torch.manual_seed(3)
            m = gs.GSUnsupervised(sampler_class=gs.find_sampler("sparse_weighted_neighbor_sampler"),
                                  adj=gs.WeightedAdj(p["adj"], p["w"]), train_adj=gs.WeightedAdj(p["adj"], p["w"]),
                                  prep_class=gs.prep_lookup["identity"], aggregator_class=gs.aggregator_lookup["mean"],
                                  input_dim=feats.shape[1], n_nodes=n, layer_specs=uref.specs(dims, fans), n_negatives=Q,
                                  walk_len=5, lr_init=0.01, weight_decay=1e-4, weighted_walks=True, walk_p=WP, walk_q=WQ)
            m.train_sampler.seed, m.val_sampler.seed = TRAIN_SEED, 78
            return m.to(DEV)
        cls = gs.engine.FusedUnsupWeightedMeanTrainStep
    else:
        adj, feats, _ = uref.problem()
        n = adj.shape[0]

        def mk():
            m = uref.make_model(gs, adj, feats.shape[1], dims, fans, Q, 1.0, DEV)
            m.walk_p, m.walk_q = WP, WQ
            return m
        cls = gs.engine.FusedUnsupMeanTrainStep
    store = gs.FeatureStore.from_array(feats, torch.device(DEV), dtype=dtype)
    ref_model, eng_model = mk(), mk()
    eng_model.load_state_dict(ref_model.state_dict())
    return store, ref_model, eng_model, cls, n


@pytest.mark.parametrize("B,Q", [(16, 20), (8, 3)])             # R = 2 B + Q = 52 and 19 rows
@pytest.mark.parametrize("capture", [False, "cmdlist"])
@pytest.mark.parametrize("weighted", [False, True])
def test_engines_build_the_module_paths_batches_and_frontiers(weighted, capture, B, Q):
    dims, fans = (16, 8), (5, 3)
    L = len(fans)
    store, ref_model, eng_model, cls, n = _twins(weighted, dims, fans, Q)
    assert cls.why_not(eng_model, store) is None
    rng = np.random.RandomState(B)
    batches = [torch.from_numpy(rng.randint(1, n, size=B)).to(DEV) for _ in range(3)]
    eng = cls(eng_model, store, batches[0], capture=capture)
    R = 2 * B + Q
    csr = eng_model.train_sampler.csr(DEV)
    plain_differs = False
    for t, seeds in enumerate(batches):
        eng(seeds)
        rid, rpw = ref_model.build_batch(seeds)
        assert torch.equal(eng.ids_set[0][:R], rid) and torch.equal(eng.pair_w, rpw), t
        cur, hops = rid, [rid]
        for k, fan in enumerate(fans):
            ph = {"seed": TRAIN_SEED, "call_base": L * t + k}
            cur = ops.sample_csr_weighted(csr, cur, fan, ph) if weighted else ops.sample_csr(csr, cur, fan, philox=ph)
            hops.append(cur)
        assert torch.equal(eng.ids_set[0], torch.cat(hops)), ("frontier", t)
        plain = ops.unsup_batch(csr, seeds, 5, Q, eng.cdf, {"seed": TRAIN_SEED, "call_base": t}, weighted=weighted)
        plain_differs = plain_differs or not torch.equal(plain[0], rid)
        assert torch.equal(plain[0][2 * B:], rid[2 * B:])
    if B == 16:                                                # (24 walks of B = 8 can agree with the plain ones)
        assert plain_differs                                   # the engine did record the biased builder
    assert eng_model._batch_calls[1] == ref_model._batch_calls[1] == 3
    csr.check()


@pytest.mark.parametrize("weighted", [False, True])
def test_engine_step_matches_train_step(weighted):
    dims, fans, B, Q = (16, 8), (5, 3), 17, 5
    store, ref_model, eng_model, cls, n = _twins(weighted, dims, fans, Q)
    ref_model.optimizer = torch.optim.Adam(ref_model.parameters(), lr=0.01, weight_decay=1e-4)
    seeds = torch.from_numpy(np.random.RandomState(2).randint(1, n, size=B)).to(DEV)
    eng = cls(eng_model, store, seeds, capture="cmdlist")
    ref_model.load_state_dict(eng_model.state_dict())
    l_ref = float(ref_model.train_step(seeds, store))
    l_eng = float(eng(seeds))
    fro = lambda a, b: float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-12))           # noqa: E731
    print("biased %s: loss %.6f vs %.6f" % ("weighted" if weighted else "uniform", l_eng, l_ref))
    assert np.isfinite(l_eng) and abs(l_eng - l_ref) / max(1.0, abs(l_ref)) <= 3e-2, (l_eng, l_ref)
    for (k, a), (_, b) in zip(eng_model.named_parameters(), ref_model.named_parameters()):
        ge = fro(a.grad.double().cpu().numpy(), b.grad.double().cpu().numpy())
        we = fro(a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy())
        print("  %s: gradient %.3g, weight %.3g" % (k, ge, we))
        assert ge <= 0.1, ("grad", k, ge)
        assert we <= 0.05, ("weight", k, we)
    eng_model.train_sampler.csr(DEV).check()
