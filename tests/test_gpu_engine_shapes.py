"""-m gpu: every fused train-step engine (engine/mean.py, pool.py, attn.py) against the float64 oracle at the shapes where
it sends a level down another kernel, or another template instance of one.  The engines pick their kernels by the
input width D, the hidden widths, the fan-outs, the class count and the storage type; test_gpu_kernels.py checks those
kernels one launch at a time, this file checks whole engine steps that reach them.

Each case runs two steps the way bench.py does (command lists, device-resident batch queue; per-call steps where the
model has no fused head) on a small synthetic graph in the reference's convention (1-based ids, dummy row 0, empty
rows, rows with fewer neighbours than the fan-out), then oracle.torch_ref.train_step in float64 on the frontier's rows
relabelled to a compact table, from the same initial weights.  bf16 engines are checked against the rounding-aware
oracle (rounding="bf16": rounded exactly where the engine stores bf16, every sum in float64), fp32 engines against the
plain one.  Measured errors go to GSAGE_PARITY_LOG (profiles/engine_shapes_parity.jsonl)."""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch
from scipy import sparse
from torch.nn import functional as F

from conftest import pkg
from util import close, close_fro, close_update, note_parity, oracle_train_step, philox_frontier

pytestmark = pytest.mark.gpu
gs = pkg()
ops, nat = gs.ops, gs._native
DEV = "cuda"
N_NODES, SEED, N_STEPS = 4000, 77, 2

# relative Frobenius bound on the two-step Adam update of the bf16 engines: test_gpu_headline.UPDATE_BOUND (mean pool
# takes max pool's: its ReLU-mask flips move whole routes as argmax flips do)
UPDATE_BOUND = {"mean": 5e-3, "max_pool": 5e-2, "mean_pool": 5e-2, "attention": 0.13}
# ... except where a case measures above it (1.5 x the measured error; the step-0 gradients of these cases agree to
# 1.3e-2 / 3.4e-4 / 9.5e-3 in norm, so the excess is the Adam update's conditioning, not a wrong gradient):
#   A7  att.0.weight of level 0 0.134: the fused hop at ks 20 rounds the hidden layer of a 640-term dot product to bf16
#       (an ulp away from the separate launches on some rows, test_gpu_round6), and Adam's second step turns the tiny
#       attention-MLP gradients' differences into whole-lr moves
#   M6  fc_neib.weight of level 0 0.0103: three levels, two of them bf16 hidden levels whose ReLU masks can flip
#   P2  mlp.0.weight of level 0 0.0516: argmax flips over 64 seeds' short segments (fan-outs 7 and 3)
UPDATE_BOUND_CASE = {"A7": 0.2, "M6": 1.5e-2, "P2": 7.5e-2}
FP32_BOUND = 2e-5                       # fp32 engines: predictions, and the gradient norm relative to max(1, norm)
# relative Frobenius bound on each step-0 gradient (same weights, same samples: well conditioned).  fp32 measures at most
# 1.2e-6; bf16 at most 1.3e-2 (A7), inside the fused hop's own norm bound on d a / d hid (test_gpu_round6: 3e-2)
GRAD_BOUND = {"fp32": FP32_BOUND, "bf16": 3e-2}

Case = namedtuple("Case", "agg prec D dims fans B C hm tail path")
# tail: the levels whose last 16-byte input chunk gets the column-tail check (fc_neib / mlp.0 columns it alone feeds)
# path: what the engine must report having chosen -- attention: (fuse per level, wide K4 per level); mean: (fused_head,
# fused_tail, tail on the matrix cores); pool: fused_head
CASES = {
    # level 0: 602 fp32 columns = 151 chunks > 32 * ATTN_TMAX (attn_group_lanes) -> k_attn_aggregate_wide<float, 4> and
    # k_attn_bwd_wide<float, 4, 32>; the fused K4 is bf16 only (gsage_attn_fused_ok)
    "A1": Case("attention", "fp32", 602, (128, 128), (10, 5), 64, 7, None, (0,), ((False, False), (True, False))),
    # 384 fp32 columns = exactly 96 chunks at both levels: grouped K4, 32 lanes x 3 chunks (attn_group_lanes' last bin)
    "A2": Case("attention", "fp32", 384, (192, 192), (10, 5), 64, 7, None, (), ((False, False), (False, False))),
    # level 1 reads 2h = 512 fp32 columns = 128 chunks: the wide K4 / K4' at a hidden level
    "A3": Case("attention", "fp32", 40, (256, 64), (8, 4), 64, 7, None, (1,), ((False, False), (False, True))),
    # 776 bf16 columns = 97 chunks: not grouped, not fused (af_ksteps(776) = 0: 25 k-steps) -> k_attn_aggregate_wide<
    # uint16_t, 8>; level 1 (D = 128, last hop 12 <= AF_NMAX) takes the fused K4 at ks 4
    "A4": Case("attention", "bf16", 776, (64, 64), (12, 6), 64, 7, None, (0,), ((False, True), (True, False))),
    # 768 bf16 columns = 96 chunks at both levels: grouped; af_ksteps(768) = 0 (24 k-steps): not fused
    "A5": Case("attention", "bf16", 768, (384, 64), (10, 5), 64, 7, None, (), ((False, False), (False, False))),
    # level 0: last hop (16 <= AF_NMAX) fused at ks 4 with D = 100 not a multiple of 32; hop 0 (n = 17) grouped;
    # level 1 reads D = 1024 bf16 columns = 128 chunks: wide (and n = 17 > AF_NMAX: not fused)
    "A6": Case("attention", "bf16", 100, (512, 64), (17, 16), 48, 7, None, (1,), ((True, False), (False, True))),
    # level 0 fused at ks 20 (af_ksteps' top bin, 32 * 20 = ld = 640); level 1 fused at fan-out 2 (the lower bound)
    "A7": Case("attention", "bf16", 640, (64, 64), (2, 16), 64, 7, None, (), ((True, True), (False, False))),
    # ks 19 would fuse, but level 0's last hop 17 > AF_NMAX: grouped (75 chunks); level 1 fused (n = 5)
    "A8": Case("attention", "bf16", 600, (64, 64), (5, 17), 64, 7, None, (), ((False, True), (False, False))),
    # the fan-out would fuse, but af_ksteps(648) = 0 (21 k-steps): grouped (81 chunks); level 1 fused (n = 5)
    "A10": Case("attention", "bf16", 648, (64, 64), (5, 16), 64, 7, None, (), ((False, True), (False, False))),
    # three levels, six K4 hops: every level's last hop fused (ks 2, fan-outs 2, 3, 4), the other three grouped
    "A9": Case("attention", "bf16", 64, (32, 32, 32), (4, 3, 2), 40, 5, None, (), ((True, True, True), (False,) * 3)),
    # k_mean_tail_mfma<15, 5> (fan-out 15 specialised, gather role over the last hop's 5), B = 50 not a multiple of 16,
    # C = 64 (the fused head's largest); level 0 projection weight-stationary (K = 128)
    "M1": Case("mean", "bf16", 128, (128, 128), (15, 5), 50, 64, None, (), (True, True, True)),
    # fp32 storage: the VALU seed level k_mean_tail_ce<float, ...> (_tail_on_mfma: bf16 only)
    "M2": Case("mean", "fp32", 128, (128, 128), (15, 5), 50, 64, None, (), (True, True, False)),
    # fan-outs without a specialisation: the generic tail k_mean_tail_mfma<0, 0> (n 7; 3 not in 5/10/15: no gather role)
    "M3": Case("mean", "bf16", 602, (128, 128), (7, 3), 64, 41, None, (0,), (True, True, True)),
    # C = 65 > 64: no fused head (_will_fuse_head), hence no fused tail: K2 + K5 and the stock head, per-call steps
    "M4": Case("mean", "bf16", 602, (128, 128), (10, 5), 64, 65, None, (0,), (False, False, True)),
    # 2h = 128 != 256 at level 0: no fused tail (_will_fuse_tail)
    "M5": Case("mean", "bf16", 40, (64, 256), (10, 10), 64, 7, None, (), (True, False, True)),
    # three levels with the fused tail (2h = 256 at the two top levels)
    "M6": Case("mean", "bf16", 256, (128, 128, 128), (5, 5, 5), 40, 7, None, (), (True, True, True)),
    # register-pooled K3: k_pool_mlp_packed<4, 20> (level 0's hop 0) and <4, 5> (gsage_pool_mlp_packed: max, no mask)
    "P1": Case("max_pool", "bf16", 602, (128, 128), (20, 5), 64, 7, None, (0,), True),
    # fan-outs 7 and 3: the generic k_pool_mlp_packed<4, 0>; Hm = 640, 640 % 256 = 128: a partial column block
    "P2": Case("max_pool", "bf16", 128, (64, 64), (7, 3), 64, 7, 640, (), True),
    # mean pool passes the ReLU mask: k_pool_mlp_packed<4, 0>, the LDS pooling epilogue
    "P3": Case("mean_pool", "bf16", 602, (128, 128), (25, 10), 64, 7, None, (0,), True),
    # the headline shape at fp32 (gsage_pool_mlp: the packed K3 is bf16 only), on the small graph
    "P4": Case("max_pool", "fp32", 602, (128, 128), (25, 10), 64, 41, None, (0,), True),
    # three levels at fp32
    "P5": Case("mean_pool", "fp32", 40, (64, 64, 64), (4, 3, 2), 40, 5, None, (), True),
}


@pytest.fixture(scope="module")
def graph():
    """~4000 nodes, ids 1..N, dummy row 0: degrees 0..39 (fan-outs up to 25: many rows sample with duplicates), a
    run of empty rows"""
    rng = np.random.RandomState(1)
    deg = rng.randint(0, 40, size=N_NODES + 1)
    deg[0] = 0
    deg[rng.randint(1, N_NODES + 1, size=200)] = 0
    deg[1:4] = (0, 1, 2)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    data = rng.randint(1, N_NODES + 1, size=int(indptr[-1]))
    return sparse.csr_matrix((data, gs.store.row_positions(indptr), indptr), shape=(N_NODES + 1, int(deg.max())))


@pytest.fixture(autouse=True)
def _setup():
    yield
    ops.set_compute_dtype("bf16")
    gs.nn_modules.SparseUniformNeighborSampler.rng_default = "compat"


def _model(adj, c):
    torch.manual_seed(3)
    gs.nn_modules.SparseUniformNeighborSampler.rng_default = "philox"
    agg_cls = gs.aggregator_lookup[c.agg]
    if c.hm is not None:
        agg_cls = functools.partial(gs.nn_modules.MaxPoolAggregator, hidden_dim=c.hm)
    specs = [{"n_train_samples": f, "n_val_samples": f, "output_dim": h,
              "activation": (lambda x: x) if i == len(c.dims) - 1 else F.relu}
             for i, (h, f) in enumerate(zip(c.dims, c.fans))]
    m = gs.GSSupervised(sampler_class=gs.sampler_lookup["sparse_uniform_neighbor_sampler"], adj=adj,
                        train_adj=adj, prep_class=gs.prep_lookup["identity"], aggregator_class=agg_cls, input_dim=c.D,
                        n_nodes=adj.shape[0], n_classes=c.C, layer_specs=specs, lr_init=0.01, weight_decay=1e-4)
    gs.nn_modules.SparseUniformNeighborSampler.rng_default = "compat"
    m.train_sampler.seed = m.val_sampler.seed = SEED
    return m.to(DEV)


def _inputs(adj, c):
    """(feature store, ids [4, B], targets [4, B, 1]) of a case"""
    ops.set_compute_dtype(c.prec)
    ops.warmup(torch.device(DEV))
    rng = np.random.RandomState(c.D)
    feats = rng.normal(size=(adj.shape[0], c.D)).astype(np.float32)
    feats[0] = 0
    store = gs.FeatureStore.from_array(feats, torch.device(DEV), dtype=c.prec)
    ids = torch.from_numpy(rng.randint(1, adj.shape[0], size=(N_STEPS + 2, c.B))).to(DEV)
    tg = torch.from_numpy(rng.randint(0, c.C, size=(N_STEPS + 2, c.B, 1))).to(DEV)
    return store, ids, tg


def _check_path(eng, c):
    if c.agg == "attention":
        fuse, wide = c.path
        assert eng.fused_head and list(eng.fuse) == list(fuse), (eng.fuse, fuse)
        assert [a is not None for a in eng.agg32] == list(wide), "levels on the wide K4"
    elif c.agg == "mean":
        head, tail, mfma = c.path
        assert (eng.fused_head, eng.fused_tail) == (head, tail)
        assert not tail or eng._tail_on_mfma() == mfma
    else:
        assert eng.fused_head == c.path
        assert eng.Hm == [c.hm or 512] * len(c.dims)


def _run(adj, name, edit=None):
    """two engine steps and two float64 oracle steps of case `name` -> dict of both sides' results.  edit: a change to
    the oracle's input rows only (the sensitivity tests)."""
    from oracle import torch_ref as tref
    c = CASES[name]
    store, ids, tg = _inputs(adj, c)
    model = _model(adj, c)
    w0 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    csr = model.train_sampler.csr(DEV)
    cls = gs.engine.fused_engine_for(model, store, explain=True)
    want = {"mean": gs.engine.FusedMeanTrainStep, "attention": gs.engine.FusedAttnTrainStep}.get(
        c.agg, gs.engine.FusedPoolTrainStep)
    assert cls is not None and cls is want, (cls, gs.engine.why_no_fused_engine(model, store))
    eng = cls(model, store, gs.ProblemLosses.classification, ids[0], tg[0], capture="cmdlist")
    _check_path(eng, c)
    preds, norms = [], []
    if eng.fused_head:
        eng.load_epoch(ids, tg)
    for s in range(N_STEPS):
        if eng.fused_head:
            p = eng.step_queue()
        else:
            p = eng(ids[s], tg[s])
            torch.cuda.synchronize()
            hops = philox_frontier(ops, csr, ids[s], c.fans, SEED, s)
            assert torch.equal(eng.ids_set[0][c.B:], torch.cat(hops)), ("frontier", s)
        preds.append(p.detach().float().cpu().numpy().copy())
        norms.append(float(eng.gnorm.item()))
        if s == 0:
            grads0 = {k: v.grad.detach().cpu().double().clone() for k, v in model.named_parameters()}
        if s == 0 and eng.fused_head:
            # the queue pipeline's frontier buffers: batch 1 sampled by the prime launch, batch 2 inside step 0
            torch.cuda.synchronize()
            for b, buf in ((1, eng.ids_q[1]), (2, eng.ids_q[2 % eng.P])):
                hops = philox_frontier(ops, csr, ids[b], c.fans, SEED, b)
                assert torch.equal(buf[c.B:], torch.cat(hops)), ("frontier", b)
    torch.cuda.synchronize()
    csr.check()
    got = {k: v.detach().cpu().double() for k, v in model.named_parameters()}

    w = {k: v.double() for k, v in w0.items()}
    opt = tref.Adam(weight_decay=1e-4)
    ref = []
    for s in range(N_STEPS):
        hops = [h.cpu().numpy() for h in philox_frontier(ops, csr, ids[s], c.fans, SEED, s)]
        ref.append(oracle_train_step(tref, w, opt, store, ids[s].cpu().numpy(), tg[s].cpu(), hops, c.fans, c.agg,
                                     "bf16" if c.prec == "bf16" else None, dtype=torch.float64, edit=edit))
    return dict(case=c, name=name, preds=preds, norms=norms, got=got, w0=w0, want=w, ref=ref, grads0=grads0)


def _compare(r):
    """predictions and gradient norm of each step, weights after the last one"""
    c, name = r["case"], r["name"]
    bf = c.prec == "bf16"
    p_tol = ((1e-3, 1e-3) if c.agg == "mean" else (3e-3, 3e-3)) if bf else (FP32_BOUND, 0.0)
    g_tol = (1e-3 if c.agg == "mean" else 5e-3) if bf else FP32_BOUND
    for s in range(N_STEPS):
        want, gn = r["ref"][s]["preds"].numpy(), r["ref"][s]["gradnorm"]
        perr, gerr = np.abs(r["preds"][s] - want).max(), abs(r["norms"][s] - gn) / max(1.0, gn)
        note_parity("shapes/%s/%s/%s/step%d" % (name, c.agg, c.prec, s), preds=perr, gnorm_rel=gerr)
        close(r["preds"][s], want, ("preds", name, s), *p_tol)
        assert gerr <= g_tol, ("gradient norm", name, s, r["norms"][s], gn)
    gworst = {}
    for k, g in r["grads0"].items():
        g_ref = r["ref"][0]["grads"][k]
        gworst[k] = float((g - g_ref).norm() / g_ref.norm().clamp_min(1e-30))
    kmax = max(gworst, key=gworst.get)
    note_parity("shapes/%s/%s/%s/grad0/%s" % (name, c.agg, c.prec, kmax), grad_fro=gworst[kmax])
    assert gworst[kmax] <= GRAD_BOUND[c.prec], ("step-0 gradient", name, kmax, gworst[kmax])
    worst = 0.0
    for k, v in r["got"].items():
        d, d_ref = v - r["w0"][k].double(), r["want"][k] - r["w0"][k].double()
        worst = max(worst, float((d - d_ref).norm() / d_ref.norm().clamp_min(1e-12)))
        if bf:
            close_fro(d.numpy(), d_ref.numpy(), ("Adam updates", name, k), UPDATE_BOUND_CASE.get(name, UPDATE_BOUND[c.agg]))
        else:
            close_update(v.numpy(), r["want"][k].numpy(), r["w0"][k].numpy(), ("weights after 2 steps", name, k))
    note_parity("shapes/%s/%s/%s/update" % (name, c.agg, c.prec), upd_fro=worst)


def _tail_columns(r, l):
    """(parameter name, columns) that only the last 16-byte chunk of level l's input rows feeds"""
    c = r["case"]
    D = c.D if l == 0 else 2 * c.dims[l - 1]
    vec = 8 if c.prec == "bf16" else 4
    key = "agg_layers.%d.%s.weight" % (l, "mlp.0" if c.agg in ("max_pool", "mean_pool") else "fc_neib")
    return key, slice((-(-D // vec) - 1) * vec, D)


def _column_tail(r):
    """the two-step Adam update of the weight columns the last chunk of an input row alone feeds: a kernel that dropped
    that chunk leaves them with no gradient (relative error 1), which the whole-tensor norms may not see at bf16
    bounds"""
    c, name = r["case"], r["name"]
    tol = UPDATE_BOUND_CASE.get(name, UPDATE_BOUND[c.agg]) if c.prec == "bf16" else 5e-3   # (fp32: close_update's)
    for l in c.tail:
        key, cols = _tail_columns(r, l)
        d = (r["got"][key] - r["w0"][key].double())[:, cols]
        d_ref = (r["want"][key] - r["w0"][key].double())[:, cols]
        note_parity("shapes/%s/%s/%s/tail%d" % (name, c.agg, c.prec, l),
                    upd_fro=float((d - d_ref).norm() / d_ref.norm().clamp_min(1e-12)))
        close_fro(d.numpy(), d_ref.numpy(), ("column tail", name, key, cols), tol)


@pytest.mark.parametrize("name", list(CASES))
def test_engine_step_matches_fp64_oracle(graph, name):
    r = _run(graph, name)
    _compare(r)
    _column_tail(r)


def _zero_cols(n):
    def edit(rows):
        rows = rows.clone()
        rows[:, -n:] = 0
        return rows
    return edit


@pytest.mark.parametrize("name", ["A1", "P4"])
def test_comparison_sees_a_dropped_last_column(graph, name):
    """the fp32 comparison fails when the oracle's input loses its last feature column"""
    r = _run(graph, name, edit=_zero_cols(1))
    with pytest.raises(AssertionError):
        _compare(r)


def test_column_tail_sees_a_dropped_last_chunk(graph):
    """bf16, 776 columns: the column-tail check fails when the oracle's input loses its last 8-column chunk"""
    r = _run(graph, "A4", edit=_zero_cols(8))
    with pytest.raises(AssertionError):
        _column_tail(r)


@pytest.mark.parametrize("name", ["A1", "A4"])
def test_wide_attention_evaluation_matches_fp64_oracle(graph, name):
    """the forward-only engine (eval_only: train.FusedEvaluator) shares the training engine's K4 stage: on the wide path
    its predictions over the validation sampler's frontier equal the oracle's forward"""
    from oracle import torch_ref as tref
    from util import compact_rows
    c = CASES[name]
    store, ids, tg = _inputs(graph, c)
    model = _model(graph, c)
    w = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    eng = gs.engine.FusedAttnTrainStep(model, store, gs.ProblemLosses.classification, ids[0], tg[0],
                                       capture="cmdlist", eval_only=True)
    assert [a is not None for a in eng.agg32] == list(c.path[1])
    got = eng.evaluate_fold(ids[:1], [c.B]).cpu().numpy()
    torch.cuda.synchronize()
    hops = philox_frontier(ops, model.val_sampler.csr(DEV), ids[0], c.fans, SEED, 0)
    assert torch.equal(eng.ids_set[0][c.B:], torch.cat(hops))
    rows, seeds, frontier = compact_rows(store, ids[0].cpu().numpy(), [h.cpu().numpy() for h in hops], torch.float64)
    with torch.no_grad():
        want = tref.forward(w, seeds, rows, None, None, c.fans, None, "attention", "identity",
                            int(store.data.shape[0]), rounding="bf16" if c.prec == "bf16" else None,
                            frontier=frontier).numpy()
    note_parity("shapes/%s/eval" % name, preds=np.abs(got - want).max())
    close(got, want, ("eval preds", name), *((3e-3, 3e-3) if c.prec == "bf16" else (FP32_BOUND, 0.0)))
