"""Unsupervised GraphSAGE without a GPU: the host-mode batch builder against the restatement of tests/unsup_ref.py
(bit-exact), the host-mode overfit of GSUnsupervised on the model tests' fixed batch, and GSSupervised.forward after
its frontier / stacking loop moved into the shared _encode."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

import unsup_ref
from conftest import pkg


def _host_csr(gs, rowptr, col):
    return gs.DeviceCSR(torch.from_numpy(rowptr), torch.from_numpy(col), len(rowptr) - 1, int(np.diff(rowptr).max()))


@pytest.mark.parametrize("B,walk_len,Q", [(1, 1, 1), (37, 5, 20), (64, 16, 64)])
def test_host_builder_equals_the_restatement(B, walk_len, Q):
    gs = pkg()
    rowptr, col = unsup_ref.walk_graph()
    csr = _host_csr(gs, rowptr, col)
    cdf = gs.ops.neg_cdf(csr)
    assert np.array_equal(cdf.numpy(), unsup_ref.degree_cdf(rowptr))
    rng = np.random.RandomState(B)
    seeds = rng.randint(0, 60, size=B)
    seeds[0] = 7                                           # a seed without edges
    if B > 2:
        seeds[1], seeds[2] = 5, 10                         # the self-loop, the chain
    for call, g0 in ((0, 0), (3, 13)):
        ids, pw = gs.ops.unsup_batch(csr, torch.from_numpy(seeds), walk_len, Q, cdf,
                                     {"seed": 0x1234567887654321, "call_base": call, "g0": g0})
        rid, rpw, err = unsup_ref.build_batch(rowptr, col, 60, seeds, walk_len, Q, cdf.numpy(), 0x1234567887654321,
                                              call, g0)
        assert err == 0
        assert np.array_equal(ids.numpy(), rid) and np.array_equal(pw.numpy(), rpw)
        assert ids[B] == 7 and pw[0] == 0                  # the walk of a degree-0 seed stays put
        if B > 2:
            assert ids[B + 1] == 5 and pw[1] == 0
        deg = np.diff(rowptr)
        assert (deg[ids[2 * B:].numpy()] > 0).all()
    with pytest.raises(IndexError):
        gs.ops.unsup_batch(csr, torch.tensor([60]), walk_len, Q, cdf, {"seed": 0})
    with pytest.raises(ValueError):
        gs.ops.unsup_batch(csr, torch.from_numpy(seeds), walk_len, Q, torch.zeros(60, dtype=torch.float64), {"seed": 0})


def _specs(fan=(5, 3), dims=(32, 32)):
    return [{"n_train_samples": fan[0], "n_val_samples": fan[0], "output_dim": dims[0], "activation": F.relu},
            {"n_train_samples": fan[1], "n_val_samples": fan[1], "output_dim": dims[1], "activation": lambda x: x}]


def make_unsup_model(gs, prob, device="cpu"):
    torch.manual_seed(0)
    model = gs.GSUnsupervised(
        sampler_class=lambda adj: gs.nn_modules.SparseUniformNeighborSampler(adj, rng="philox"),
        adj=prob["adj"], train_adj=prob["adj"], prep_class=gs.prep_lookup["identity"],
        aggregator_class=gs.aggregator_lookup["mean"], input_dim=16, n_nodes=200, layer_specs=_specs(),
        n_negatives=20, walk_len=5)
    return model.to(device)


def test_host_overfit_of_a_fixed_batch():
    gs = pkg()
    prob = unsup_ref.model_problem()
    model = make_unsup_model(gs, prob)
    assert not any(k.startswith("fc.") for k in model.state_dict())
    feats = torch.from_numpy(prob["feats"])
    batch = (torch.from_numpy(prob["batch_ids"]), torch.from_numpy(prob["pair_w"]))
    losses = [float(model.train_step(None, feats, batch=batch)) for _ in range(40)]
    print("host overfit: first %.5f last %.5f" % (losses[0], losses[-1]))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    res = model.evaluate(batch[0][:64], feats)
    assert np.isfinite(res["loss"]) and 0 < res["mrr"] <= 1
    out = model(batch[0][:64], feats, train=False)
    assert out.shape == (64, 64) and torch.allclose(out.norm(dim=1), torch.ones(64), atol=1e-5)
    emb = gs.embeddings(model, feats)
    assert emb.shape == (200, 64)


def test_skipgram_host_expression_equals_float64():
    gs = pkg()
    torch.manual_seed(1)
    B, Q, D = 17, 20, 24
    E = torch.randn(2 * B + Q, D)
    pw = (torch.rand(B) > 0.2).float()
    Eg = E.clone().requires_grad_(True)
    loss = gs.ops.skipgram_loss(Eg, B, Q, pw, 0.25)
    loss.backward()
    rl, raff, rdE = unsup_ref.head(E, B, Q, pw, 0.25)
    assert abs(float(loss.detach()) - float(rl)) <= 1e-5 * abs(float(rl))
    assert float((Eg.grad.double() - rdE).abs().max()) <= 1e-5 * float(rdE.abs().max())
    assert float((gs.ops._skipgram_host(E, B, Q, pw, 0.25)[1].double() - raff).abs().max()) <= 1e-5


def test_supervised_forward_is_what_it_was():
    """GSSupervised.forward = normalise(_encode) -> fc, with the frontier loop restated here as it stood in forward."""
    gs = pkg()
    prob = unsup_ref.model_problem()
    torch.manual_seed(0)
    model = gs.GSSupervised(
        sampler_class=lambda adj: gs.nn_modules.SparseUniformNeighborSampler(adj, rng="compat"),
        adj=prob["adj"], train_adj=prob["adj"], prep_class=gs.prep_lookup["identity"],
        aggregator_class=gs.aggregator_lookup["mean"], input_dim=16, n_nodes=200, n_classes=3, layer_specs=_specs())
    assert [k for k in model.state_dict() if k.startswith("fc.")] == ["fc.weight", "fc.bias"]
    feats = torch.from_numpy(prob["feats"])
    ids = torch.arange(1, 41)
    for train in (True, False):
        np.random.seed(9)
        got = model(ids, feats, train=train)
        np.random.seed(9)
        fns = model.train_sample_fns if train else model.val_sample_fns
        cur, hops = ids, [model.prep(ids, feats[ids], layer_idx=0)]
        for hop, sample in enumerate(fns):
            cur = sample(ids=cur).contiguous().view(-1)
            hops.append(model.prep(cur, feats[cur], layer_idx=hop + 1))
        for layer in model.agg_layers.children():
            hops = [layer(hops[k], hops[k + 1]) for k in range(len(hops) - 1)]
        want = model.fc(F.normalize(hops[0].float(), dim=1))
        assert torch.equal(got, want)
