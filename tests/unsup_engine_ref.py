"""Restatements the unsupervised-engine tests compare against (test infrastructure):

  masked_loss   the skip-gram loss of a batch whose seeds b .. B-1 are padding (include/gsage.h,
                gsage_head_skipgram_live), as a differentiable torch expression in the dtype of its input
  masked_head   float64 autograd of it -> (loss, aff, dE)
  problem / make_model   the 600-node problem of the engine tests (rows of degree 0) and a GSUnsupervised over it
"""
import numpy as np
import torch
from scipy import sparse
from torch.nn import functional as F


def masked_loss(E, B, Q, pair_w, neg_weight, b):
    """(1/b) sum_{i < b} [pair_w_i softplus(-a_i) + neg_weight sum_q softplus(n_iq)] on the rows
    E = [seeds (B) | positives (B) | negatives (Q)];  -> (loss, aff [B, 1 + Q])"""
    z = E / E.norm(dim=1, keepdim=True).clamp(min=1e-12)
    a = (z[:B] * z[B:2 * B]).sum(1)
    n = z[:B] @ z[2 * B:2 * B + Q].t()
    # (written smooth, as unsup_ref.head: the derivative at an affinity of exactly 0 is sigmoid(0) = 1/2)
    softplus = lambda x: torch.log1p(torch.exp(x))                                # noqa: E731
    live = (torch.arange(B, device=E.device) < b).to(E.dtype)
    per_seed = pair_w.to(E.dtype) * softplus(-a) + neg_weight * softplus(n).sum(1)
    return (live * per_seed).sum() / b, torch.cat([a.unsqueeze(1), n], 1)


def masked_head(E, B, Q, pair_w, neg_weight, b):
    """float64 autograd of masked_loss -> (loss, aff [B, 1 + Q], dE), float64 tensors"""
    E = E.detach().double().clone().requires_grad_(True)
    loss, aff = masked_loss(E, B, Q, pair_w.detach().double(), neg_weight, b)
    loss.backward()
    return loss.detach(), aff.detach(), E.grad.detach()


def problem(n=600, D=40, seed=0, max_deg=30):
    """as tests/test_gpu_engine.py::_problem: n + 1 rows in the reference's sparse convention, rows 0 and 7 of degree 0"""
    rng = np.random.RandomState(seed)
    deg = rng.randint(0, max_deg, size=n + 1)
    deg[0], deg[7], deg[n] = 0, 0, 3
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    data = rng.randint(1, n + 1, size=int(indptr[-1]))
    cols = np.arange(indptr[-1]) - np.repeat(indptr[:-1], deg)
    adj = sparse.csr_matrix((data, cols, indptr), shape=(n + 1, int(deg.max())))
    feats = rng.normal(size=(n + 1, D)).astype(np.float32)
    feats[0] = 0
    return adj, feats, rng


def specs(dims, fans):
    return [{"n_train_samples": f, "n_val_samples": f, "output_dim": h,
             "activation": (lambda x: x) if i == len(dims) - 1 else F.relu}
            for i, (h, f) in enumerate(zip(dims, fans))]


def make_model(gs, adj, D, dims=(32, 32), fans=(5, 3), Q=20, neg_weight=1.0, device="cpu", seed=3, rng="philox",
               agg="mean", prep="identity", sampler=None, n_nodes=None):
    """GSUnsupervised after the pattern of test_unsup_host.make_unsup_model"""
    torch.manual_seed(seed)
    sampler = sampler or (lambda adj: gs.nn_modules.SparseUniformNeighborSampler(adj, rng=rng, seed=77))
    model = gs.GSUnsupervised(
        sampler_class=sampler, adj=adj, train_adj=adj, prep_class=gs.prep_lookup[prep],
        aggregator_class=gs.aggregator_lookup[agg], input_dim=D, n_nodes=n_nodes or adj.shape[0],
        layer_specs=specs(dims, fans), n_negatives=Q, walk_len=5, neg_weight=neg_weight, lr_init=0.01,
        weight_decay=1e-4)
    return model.to(device)
