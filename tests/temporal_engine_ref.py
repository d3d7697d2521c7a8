"""What the tests of the all-hops temporal launch and of FusedTemporalMeanTrainStep share, on top of
tests/temporal_ref.py: the frontier buffer's layout, the restatement of a whole frontier as two flat arrays, and the
engine tests' problem (60 nodes, half of them at T_SNAP and half at times of their own, a validation adjacency of
another structure)."""
import numpy as np

import temporal_ref as tr

SEED = 0x0123456789ABCDEF
PAIRS = [(s, r) for s in tr.STRATEGIES for r in tr.RULES]
COUNTS = {}                         # (row, t) -> cnt of the restatement over tr.graph(), shared by every test


def sizes(B, fans):
    out = [B]
    for n in fans:
        out.append(out[-1] * n)
    return out


def frontier(rowptr, col, etime, n_rows, seeds, times, fans, seed, call0, strategy, inherit, counts=None):
    """-> (ids [hop 0 | hop 1 | ...], times of the same layout, err): temporal_ref.sample_hops, concatenated"""
    hops, err = tr.sample_hops(rowptr, col, etime, n_rows, seeds, times, fans, seed, call0, strategy, inherit, counts)
    return np.concatenate([h[0] for h in hops]), np.concatenate([h[1] for h in hops]), err


def graph_frontier(seeds, times, fans, call0, strategy, inherit, seed=SEED):
    g = tr.graph()
    return frontier(g.rowptr, g.col, g.etime, g.n, seeds, times, fans, seed, call0, strategy, inherit, COUNTS)


TRAIN_SEED, VAL_SEED = 77, 78


def model(p, dims, fans, strategy="uniform", inherit="seed", seed=3, val=None):
    """temporal_ref.model over (train_adj = p's adjacency, adj = the validation one), the two samplers under seeds of
    their own; val: (strategy, inherit) of the validation sampler when it is to differ"""
    from functools import partial

    import torch
    from torch.nn import functional as F

    from conftest import pkg
    gs = pkg()
    torch.manual_seed(seed)
    specs = [{"n_train_samples": f, "n_val_samples": f, "output_dim": h,
              "activation": (lambda x: x) if i == len(dims) - 1 else F.relu} for i, (f, h) in enumerate(zip(fans, dims))]
    cls = partial(gs.find_sampler("sparse_temporal_neighbor_sampler"), strategy=strategy, inherit=inherit)
    m = gs.GSSupervised(sampler_class=cls, adj=p["val_tadj"], train_adj=p["tadj"], prep_class=gs.prep_lookup["identity"],
                        aggregator_class=gs.aggregator_lookup["mean"], input_dim=p["feats"].shape[1], n_nodes=p["n"] + 1,
                        n_classes=p["C"], layer_specs=specs, lr_init=0.01, weight_decay=1e-4)
    m.train_sampler.seed, m.val_sampler.seed = TRAIN_SEED, VAL_SEED
    if val is not None:
        m.val_sampler.strategy, m.val_sampler.inherit = val
    return m


_PROBLEM = []


def problem():
    """temporal_ref.problem(n=60) with node_time = T_SNAP for the even nodes and a time of their own for the odd ones
    (some before every edge of theirs, some between, some past T_SNAP); val_*: problem(seed=8)'s adjacency"""
    if not _PROBLEM:
        from conftest import pkg
        gs = pkg()
        p = dict(tr.problem(n=60))
        q = tr.problem(n=60, seed=8)
        node_time = np.full(p["n"] + 1, tr.T_SNAP, dtype=np.int64)
        odd = np.arange(1, p["n"] + 1, 2)
        node_time[odd] = np.random.RandomState(12).randint(-60, tr.T_SNAP + 60, size=odd.shape[0])
        p["node_time"] = node_time
        p["tadj"] = gs.TemporalAdj(p["adj"], p["time"], node_time=node_time)
        p["val_tadj"] = gs.TemporalAdj(q["adj"], q["time"], node_time=node_time)
        p["val_indptr"], p["val_data"], p["val_etime"] = q["indptr"], q["data"], q["etime"]
        _PROBLEM.append(p)
    return _PROBLEM[0]
