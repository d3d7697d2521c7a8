"""
models.py -- GSSupervised, the layer-stacking loop and train_step (reference models.py:21-104), and
GSUnsupervised, the same encoder under a skip-gram loss (no reference counterpart).  GSSupervised is
kept drop-in: same constructor keywords (as passed at train.py:94-123), same methods
(`forward(ids, feats, train)`, `set_progress`, `train_step`), same parameter names.

What changes underneath: the frontier is built on the device by K1, the
per-hop `feats[ids]` gathers are row *references* consumed inside the aggregator kernels
(K2-K5) instead of materialised [B*f1*f2, D] tensors, and `train_step` has a gradient-sync
hook between backward and clip for data-parallel runs (one flat RCCL all-reduce, dist.py).
"""
from functools import partial

import torch
from torch import nn
from torch.nn import functional as F

import os

from . import ops
from .lr import LRSchedule
from .nn_modules import UniformNeighborSampler
from .optim import FlatAdam
from .store import DenseAdj, DeviceCSR, FeatureStore


class _SageModel(nn.Module):
    """What GSSupervised and GSUnsupervised share: samplers, prep, the aggregator stack (_build_encoder), the frontier
    and layer-stacking loop (_encode), the learning-rate schedule and the optimizer route."""

    def _build_encoder(self, input_dim, n_nodes, layer_specs, aggregator_class, prep_class, sampler_class, adj,
                       train_adj):
        """-> the width of the top-level rows"""
        # samplers: training walks train_adj, evaluation the full graph (models.py:41-44)
        self.train_sampler = sampler_class(adj=train_adj)
        self.val_sampler = sampler_class(adj=adj)
        self.train_sample_fns = [partial(self.train_sampler, n_samples=spec['n_train_samples'])
                                 for spec in layer_specs]
        self.val_sample_fns = [partial(self.val_sampler, n_samples=spec['n_val_samples'])
                               for spec in layer_specs]

        self.prep = prep_class(input_dim=input_dim, n_nodes=n_nodes)
        width = self.prep.output_dim

        stack = []
        for spec in layer_specs:
            layer = aggregator_class(input_dim=width, output_dim=spec['output_dim'],
                                     activation=spec['activation'])
            stack.append(layer)
            width = layer.output_dim          # 2 * output_dim for the concat (models.py:59)
        self.agg_layers = nn.Sequential(*stack)
        return width

    def _build_optimizer(self, lr_init, weight_decay, lr_schedule):
        # schedule is a function of progress only: `epochs` is not forwarded (models.py:67)
        self.lr_scheduler = partial(getattr(LRSchedule, lr_schedule), lr_init=lr_init)
        self.lr = self.lr_scheduler(0.0)
        self.optimizer = torch.optim.Adam(self.parameters(), lr=self.lr, weight_decay=weight_decay)
        self._init_optimizer = self.optimizer

        self.grad_sync = None                 # set by dist.attach(): called after backward
        self._wrapped = {}

    # ------------------------------------------------------------------------------------
    def _rows_of(self, feats):
        """What `feats[ids]` should index: FeatureStore as is; a CUDA tensor is wrapped zero-copy
        so its gathers are fused too; CPU tensors keep stock indexing (host mode)."""
        if feats is None or isinstance(feats, FeatureStore) or not feats.is_cuda:
            return feats
        key = (feats.data_ptr(), tuple(feats.shape), feats.dtype)
        if key not in self._wrapped:
            self._wrapped = {key: FeatureStore.wrap(feats)}
        return self._wrapped[key]

    def _encode(self, ids, feats, train=True, times=None):
        """The un-normalised top-level rows [len(ids), width] (fp32) of `ids`: frontier, prep, layer stack.
        times: int64 [len(ids)], the seeds' query times under a temporal sampler (nn_modules.
        SparseTemporalNeighborSampler) -- they flow hop by hop beside the ids; None: node_time[ids] of the sampler's
        adjacency, or INT64_MAX without one.  With any other sampler `times` must be None."""
        # a fused engine that defers the embedding table's zero-gradient Adam updates (engine.sync_rows)
        # settles them HERE: the prep reads `embedding.weight` directly, not through the nn.Embedding
        # module, so a hook on that module would never fire
        settle = getattr(self, "_settle_rows", None)
        if settle is not None:
            settle()
        sample_fns = self.train_sample_fns if train else self.val_sample_fns
        table = self._rows_of(feats)
        rows = (lambda i: table[i]) if table is not None else (lambda i: None)

        # frontier: [B], [B*f1], [B*f1*f2], ...  (models.py:75-81)
        sampler = self.train_sampler if train else self.val_sampler
        temporal = bool(getattr(sampler, "temporal", False))
        if temporal:
            times = sampler.default_times(ids) if times is None else times.to(ids.device).contiguous().view(-1)
        elif times is not None:
            raise ValueError("times were given, but %s is not a temporal sampler (sparse_temporal_neighbor_sampler)"
                             % type(sampler).__name__)
        hops = [self.prep(ids, rows(ids), layer_idx=0)]
        for hop, sample in enumerate(sample_fns):
            if temporal:
                ids, times = sample(ids=ids, times=times)
            else:
                ids = sample(ids=ids).contiguous().view(-1)
            hops.append(self.prep(ids, rows(ids), layer_idx=hop + 1))

        # layer l maps every adjacent pair of hop representations; shared weights (models.py:85-86)
        for layer in self.agg_layers.children():
            hops = [layer(hops[k], hops[k + 1]) for k in range(len(hops) - 1)]
        assert len(hops) == 1, "len(all_feats) != 1"
        return hops[0].float()

    def __getstate__(self):
        # per-process handles of a fused engine (a weakref and a bound method) do not pickle / deep-copy
        state = dict(self.__dict__)
        state.pop("_engine", None)
        state.pop("_settle_rows", None)
        return state

    def set_progress(self, progress):
        self.lr = self.lr_scheduler(progress)
        LRSchedule.set_lr(self.optimizer, self.lr)

    def _clip_and_step(self, flat):
        if self.grad_sync is not None:
            self.grad_sync(self)
        if flat is not None:
            flat.clip_and_step(5.0)               # models.py:101-102 in two launches
        else:
            torch.nn.utils.clip_grad_norm_(self.parameters(), 5)
            self.optimizer.step()

    def _flat_optimizer(self):
        """On the GPU the optimizer built in __init__ (torch.optim.Adam, never stepped yet) is replaced,
        on the first train_step, by optim.FlatAdam (its state_dict keeps torch.optim.Adam's format, so
        checkpoints interchange; a reference to the ORIGINAL optimizer object taken before the first step
        goes stale -- hold `model.optimizer` instead): same arithmetic, Parameters and gradients become
        views of flat buckets, clip + Adam become two launches.  An optimizer assigned from outside,
        one that has state already, CPU parameters or GSAGE_TORCH_ADAM=1 keep the stock route."""
        opt = self.optimizer
        settle = getattr(self, "_settle_rows", None)
        if settle is not None:                    # a fused engine with deferred embedding-table rows
            settle()
        eng = getattr(self, "_engine", None)
        eng = eng() if eng is not None else None
        trained = eng is not None and eng.holds_parameters()     # a fused engine trained them last
        if isinstance(opt, FlatAdam):
            if not opt.owns():                    # somebody re-pointed the Parameters (e.g. a fused engine):
                opt._attach()                     # take them back WITH their current values ...
                if trained:
                    eng.export_optimizer_state(opt)   # ... and the engine's exp_avg / exp_avg_sq / step count
            return opt
        if opt is not self._init_optimizer or opt.state or os.environ.get("GSAGE_TORCH_ADAM", "0") == "1":
            if trained and getattr(self, "_handed_over", None) != id(eng):
                # the stock route takes over from a fused engine: Adam continues from the engine's exp_avg /
                # exp_avg_sq / step count when this optimizer has no state of its own, else say what is lost
                self._handed_over = id(eng)
                try:
                    if opt.state:
                        raise RuntimeError("the optimizer already holds state of its own")
                    opt.load_state_dict(eng.optimizer_state_dict())
                except Exception as e:
                    import warnings
                    warnings.warn("gsage: %s -- Adam's moments of the fused engine's steps are NOT carried over "
                                  "into model.optimizer" % (e,))
            return None
        params = [p for p in self.parameters() if p.requires_grad]
        if not params or not all(p.is_cuda and p.dtype == torch.float32 for p in params):
            return None
        g = opt.param_groups[0]
        self.optimizer = FlatAdam(params, lr=g["lr"], weight_decay=g.get("weight_decay", 0.0),
                                  betas=g.get("betas", (0.9, 0.999)), eps=g.get("eps", 1e-8))
        if trained:
            eng.export_optimizer_state(self.optimizer)
        return self.optimizer

    def optimizer_state_dict(self):
        """torch.optim.Adam-format state of whoever trained last: the fused engine's buckets when one holds
        the Parameters (`model.optimizer` is then still the never-stepped optimizer of __init__), else
        `model.optimizer.state_dict()`.  Loads into the torch.optim.Adam the reference builds (models.py:69)."""
        eng = getattr(self, "_engine", None)
        eng = eng() if eng is not None else None
        if eng is not None and eng.holds_parameters():
            return eng.optimizer_state_dict()
        return self.optimizer.state_dict()


class GSSupervised(_SageModel):
    def __init__(self, input_dim, n_nodes, n_classes, layer_specs, aggregator_class, prep_class,
                 sampler_class, adj, train_adj, lr_init=0.01, weight_decay=0.0,
                 lr_schedule='constant', epochs=10):
        super(GSSupervised, self).__init__()
        width = self._build_encoder(input_dim, n_nodes, layer_specs, aggregator_class, prep_class, sampler_class,
                                    adj, train_adj)
        self.fc = nn.Linear(width, n_classes, bias=True)
        self._build_optimizer(lr_init, weight_decay, lr_schedule)

    def forward(self, ids, feats, train=True, times=None):
        out = F.normalize(self._encode(ids, feats, train, times=times), dim=1)
        if out.is_cuda:
            # the head's projection on K5 in exact fp32 (models.py:91 is an nn.Linear: a library GEMM on the GPU
            # otherwise -- the last one of the module path, forward and backward)
            return ops.linear(out, self.fc.weight, self.fc.bias, compute_dtype="fp32")
        return self.fc(out)

    def train_step(self, ids, feats, targets, loss_fn, times=None):
        flat = self._flat_optimizer()
        self.optimizer.zero_grad()
        preds = self(ids, feats, train=True) if times is None else self(ids, feats, train=True, times=times)
        loss = loss_fn(preds, targets.squeeze())
        loss.backward()
        self._clip_and_step(flat)
        return preds


class GSUnsupervised(_SageModel):
    """The same encoder trained without labels: random-walk co-occurrence positives, degree^0.75 negatives and a
    skip-gram loss on the cosines of the embeddings (include/gsage.h, "Unsupervised GraphSAGE").  Constructor keywords
    of GSSupervised minus n_classes; no `fc`: the model's output IS the embedding, F.normalize of the top-level rows
    (what infer.embeddings / train.py --save-embeddings export for every node).

    A step encodes [seeds (B) | positives (B) | negatives (Q)] in ONE pass of the module path.  The walks run on the
    adjacency the step's sampler walks (train_adj for training, adj for evaluation) and draw from Philox under the
    neighbour sampler's seed with role tags of their own, whatever --rng the neighbour sampler uses.

    weighted_walks=True (a sampler over a weighted adjacency: SparseWeightedNeighborSampler): every step of a walk is
    drawn in proportion to the edge weights (gsage_unsup_batch_weighted), so the positives follow the neighbourhoods the
    encoder aggregates over, in training and in evaluate alike, and a row without a drawable edge is never a negative.
    False: uniform steps over the stored edges, whatever the sampler.

    walk_p, walk_q (in [1/8, 8]): node2vec's return and in-out parameters -- every step of a walk after its first is a
    second-order step (include/gsage.h, "Biased walks", gsage_unsup_batch_biased); composes with weighted_walks (the
    proposals are then drawn by edge weight).  1, 1: the plain walks, the entries and the bits of before.

    temporal_walks=True (both samplers SparseTemporalNeighborSampler): the walks respect time (include/gsage.h, "Temporal
    walks", gsage_unsup_batch_temporal) -- every step is drawn among the edges before the seed's query time (the sampler's
    inherit "seed") or before the edge just walked ("edge"), and the query times travel with [seeds | positives |
    negatives] into the temporal sampler: build_batch returns (ids, pair_w, times), and build_batch / train_step /
    evaluate take `times` (None: the sampler's default_times).  Not with weighted_walks or walk_p / walk_q.  False:
    nothing changes."""

    def __init__(self, input_dim, n_nodes, layer_specs, aggregator_class, prep_class, sampler_class, adj, train_adj,
                 lr_init=0.01, weight_decay=0.0, lr_schedule='constant', epochs=10, walk_len=5, n_negatives=20,
                 neg_weight=1.0, weighted_walks=False, walk_p=1.0, walk_q=1.0, temporal_walks=False):
        super(GSUnsupervised, self).__init__()
        assert 1 <= walk_len <= 16 and 1 <= n_negatives <= 64, "GSUnsupervised: walk_len in 1..16, n_negatives in 1..64"
        self.output_dim = self._build_encoder(input_dim, n_nodes, layer_specs, aggregator_class, prep_class,
                                              sampler_class, adj, train_adj)
        self.walk_len, self.n_negatives, self.neg_weight = int(walk_len), int(n_negatives), float(neg_weight)
        self.weighted_walks = bool(weighted_walks)
        self.walk_p, self.walk_q, _ = ops.walk_bias_check(walk_p, walk_q, 0.0, "GSUnsupervised")
        self.temporal_walks = bool(temporal_walks)
        if self.temporal_walks:
            for s in (self.train_sampler, self.val_sampler):
                if not getattr(s, "temporal", False):
                    raise ValueError("GSUnsupervised: temporal_walks=True needs the temporal sampler "
                                     "(SparseTemporalNeighborSampler) for training and validation, not %s"
                                     % type(s).__name__)
            if self.weighted_walks:
                raise ValueError("GSUnsupervised: temporal_walks=True does not combine with weighted_walks=True "
                                 "(weights and times together are not covered)")
            if self.biased_walks:
                raise ValueError("GSUnsupervised: temporal_walks=True does not combine with walk_p / walk_q other than 1 "
                                 "(biased temporal walks are not covered)")
        if self.weighted_walks:
            for s in (self.train_sampler, self.val_sampler):
                host = None if isinstance(s, UniformNeighborSampler) else s.csr("cpu")
                if getattr(host, "edge_cdf", None) is None:
                    raise ValueError("GSUnsupervised: weighted_walks=True needs a sampler over a weighted adjacency "
                                     "(SparseWeightedNeighborSampler), not %s" % type(s).__name__)
        self._build_optimizer(lr_init, weight_decay, lr_schedule)
        self._walk = {}                       # (train, device) -> (DeviceCSR, negatives' table)
        self._batch_calls = [0, 0]            # Philox call index of the next batch: evaluation, training

    def extra_repr(self):
        bias = ", walk_p=%g, walk_q=%g" % (self.walk_p, self.walk_q) if self.biased_walks else ""
        return "walk_len=%d, n_negatives=%d, neg_weight=%g%s%s%s" % (
            self.walk_len, self.n_negatives, self.neg_weight, ", weighted_walks=True" if self.weighted_walks else "", bias,
            ", temporal_walks=True" if getattr(self, "temporal_walks", False) else "")

    @property
    def biased_walks(self):
        return (self.walk_p, self.walk_q) != (1.0, 1.0)

    def forward(self, ids, feats, train=True):
        return F.normalize(self._encode(ids, feats, train), dim=1)

    def _walk_graph(self, train, device):
        key = (bool(train), str(device))
        if key not in self._walk:
            sampler = self.train_sampler if train else self.val_sampler
            csr = sampler.csr(device)
            if isinstance(csr, DenseAdj):     # the dense sampler's [n, K] table read as K edges per row
                rowptr = torch.arange(csr.n_rows + 1, dtype=torch.int64, device=csr.device) * csr.K
                csr = DeviceCSR(rowptr, csr.adj.reshape(-1).to(torch.int32), csr.n_rows, csr.K)
            if self.weighted_walks and getattr(csr, "edge_cdf", None) is None:
                raise ValueError("GSUnsupervised: weighted_walks=True, but the sampler's adjacency carries no edge "
                                 "weights")
            self._walk[key] = (csr, ops.neg_cdf(csr, weighted=self.weighted_walks))
        return self._walk[key]

    def build_batch(self, ids, train=True, times=None):
        """-> (ids [2B + Q] = [seeds | positives | negatives], pair_w [B]) for the seeds `ids` (ops.unsup_batch).
        temporal_walks=True: -> (ids, pair_w, times [2B + Q]) (ops.unsup_batch_temporal) for the seeds' query times
        `times` (int64 [B]; None: the sampler's default_times(ids)), the walk's rule the sampler's `inherit`."""
        ids = ids.contiguous().view(-1)
        csr, cdf = self._walk_graph(train, ids.device)
        sampler = self.train_sampler if train else self.val_sampler
        rank, _ = getattr(sampler, "shard", (0, 1))
        ph = {"seed": int(getattr(sampler, "seed", 0)), "call_base": self._batch_calls[int(train)],
              "g0": rank * int(ids.shape[0])}
        if not getattr(self, "temporal_walks", False):
            if times is not None:
                raise ValueError("GSUnsupervised: times were given, but the walks are not temporal (temporal_walks=True)")
        else:
            times = sampler.default_times(ids) if times is None else times.to(ids.device).contiguous().view(-1)
            self._batch_calls[int(train)] += 1
            return ops.unsup_batch_temporal(csr, ids, times, self.walk_len, self.n_negatives, cdf, ph,
                                            inherit=sampler.inherit)
        self._batch_calls[int(train)] += 1
        return ops.unsup_batch(csr, ids, self.walk_len, self.n_negatives, cdf, ph, weighted=self.weighted_walks,
                               p=self.walk_p, q=self.walk_q)

    def _loss_inputs(self, ids, feats, batch, train, times=None):
        all_times = None
        if batch is None:
            batch = self.build_batch(ids, train=train, times=times)
        elif times is not None:
            raise ValueError("GSUnsupervised: an explicit batch carries its own times (batch = (ids, pair_w, times))")
        if getattr(self, "temporal_walks", False):
            if len(batch) != 3:
                raise ValueError("GSUnsupervised: with temporal_walks=True a batch is (ids [2B + Q], pair_w [B], "
                                 "times [2B + Q])")
            all_ids, pair_w, all_times = batch
        else:
            all_ids, pair_w = batch
        B = int(pair_w.shape[0])
        Q = int(all_ids.shape[0]) - 2 * B
        assert Q >= 1, "GSUnsupervised: a batch is [seeds (B) | positives (B) | negatives (Q >= 1)]"
        return self._encode(all_ids, feats, train=train, times=all_times), B, Q, pair_w

    def train_step(self, ids, feats, batch=None, times=None):
        """One optimisation step on the seeds `ids` (or on an explicit batch = (ids [2B + Q], pair_w [B])): the loss.
        temporal_walks=True: `times` are the seeds' query times (None: the sampler's default_times), an explicit batch
        is (ids, pair_w, times [2B + Q])."""
        flat = self._flat_optimizer()
        self.optimizer.zero_grad()
        E, B, Q, pair_w = self._loss_inputs(ids, feats, batch, True, times)
        loss = ops.skipgram_loss(E, B, Q, pair_w, self.neg_weight)
        loss.backward()
        self._clip_and_step(flat)
        return loss.detach()

    def evaluate(self, ids, feats, batch=None, times=None):
        """{"loss", "mrr"} of the seeds `ids` on the evaluation graph: mrr = mean of 1 / rank of a_i among
        [a_i, n_i1 .. n_iQ] (rank 1: the positive is closer than every negative).  times: as for train_step."""
        with torch.no_grad():
            E, B, Q, pair_w = self._loss_inputs(ids, feats, batch, False, times)
            if E.is_cuda:
                loss, aff, _ = ops.skipgram_head(E, B, Q, pair_w, self.neg_weight)
            else:
                loss, aff = ops._skipgram_host(E, B, Q, pair_w, self.neg_weight)
            rank = 1 + (aff[:, 1:] > aff[:, :1]).sum(dim=1)
            mrr = (1.0 / rank.double()).mean()
        return {"loss": float(loss), "mrr": float(mrr)}
