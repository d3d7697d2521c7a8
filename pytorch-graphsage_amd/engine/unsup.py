"""
engine/unsup.py -- FusedUnsupMeanTrainStep: GSUnsupervised.train_step (models.py) for mean aggregators as ONE
recorded list of launches: batch builder, frontier sampler, level-0 gathers, the encoder of FusedMeanTrainStep without
its fused seed level, the skip-gram head with a live-seed count, backward, finalise, clip + Adam.

The encoder sees one batch of R = 2B + Q rows [seeds | positives | negatives]: that IS the base engine's batch
(self.B = R; size / off / fan follow), so every launch between the sampler and the update is the mean engine's own.

FusedUnsupWeightedMeanTrainStep: the same step over a weighted adjacency (GSUnsupervised(weighted_walks=True)): the
builder's steps and every hop of the frontier are drawn from the adjacency's per-edge table.

FusedUnsupTemporalMeanTrainStep: the same step over a temporal adjacency (GSUnsupervised(temporal_walks=True)): the
builder's walks respect time and hand the frontier sampler (gsage_sample_hops_temporal) a query time per row.

The first two record gsage_unsup_batch_biased as their builder when the model's walk_p / walk_q are not neutral (include/gsage.h,
"Biased walks"): the same buffers and call index; nothing else of the step changes.
"""
import ctypes

import torch

from .. import _native as nat
from .. import ops
from ..nn_modules import MeanAggregator, NodeEmbeddingPrep, SparseTemporalNeighborSampler, \
    SparseUniformNeighborSampler, SparseWeightedNeighborSampler, UniformNeighborSampler, _split_activation
from ..store import FeatureStore
from .mean import FusedMeanTrainStep
from .temporal import FusedTemporalMeanTrainStep
from .weighted import FusedWeightedMeanTrainStep


class FusedUnsupMeanTrainStep(FusedMeanTrainStep):
    """`eng = FusedUnsupMeanTrainStep(model, feats, example_seeds)`; `eng(seeds)` has the contract of
    `GSUnsupervised.train_step(seeds, feats)`: one optimisation step, the loss as a device scalar (a view of a static
    buffer: the next step overwrites it).  One step:

        builder       gsage_unsup_batch: the seed buffer -> [seeds | positives | negatives] + pair_w
        K1            every hop of the frontier of those R rows
        gather        level-0 neighbour means
        K2 / K5       per level (no fused seed-level kernel: the head is not a classifier)
        head          gsage_head_skipgram_live, two launches: loss, aff, d loss / d rows; padded seeds take nothing
        backward      K5 + merge per level, K5b, finalise (which also ticks the builder's call index)
        update        clip + Adam + refresh of the operand copies

    Step t builds the batch `model.build_batch` would build at that point of the model's stream: the call index is
    model._batch_calls[1] at construction plus a device word the finalisation launch advances, so a recorded list
    replays unchanged; every real call also advances model._batch_calls[1], so the module path or another engine
    continues the same stream.  Short batches (2 <= b < B seeds) are padded with their first seed.
    Per-call, sequential, single process only: load_epoch / step_queue raise."""

    TIMED = dict(FusedMeanTrainStep.TIMED, builder=(10, 11), head=(12, 13))      # head: marks around its two launches

    # ---- coverage -------------------------------------------------------------------------------------------------
    @classmethod
    def why_not(cls, model, feats, ddp=None, pipelined=False, eval_only=False):
        """None, or one sentence: what of (model, feats, mode) this engine does not cover.  What can be said of the
        model alone comes first (so it can be said without a device), the feature store last."""
        from ..models import GSUnsupervised
        if not isinstance(model, GSUnsupervised):
            return "a model that is not GSUnsupervised (%s: the supervised engines train it)" % type(model).__name__
        layers = list(model.agg_layers.children())
        if not layers or any(type(l) is not MeanAggregator for l in layers):
            return ("aggregators other than mean (%s): the pool, attention and LSTM aggregators have no unsupervised "
                    "engine" % ", ".join(sorted({type(l).__name__ for l in layers})))
        if isinstance(model.prep, NodeEmbeddingPrep):
            return "the node_embedding prep (a trainable table under the skip-gram loss has no fused form)"
        s = model.train_sampler
        if isinstance(s, SparseWeightedNeighborSampler):
            return "the weighted sampler (SparseWeightedNeighborSampler): the fused K1 draws uniformly"
        if isinstance(s, UniformNeighborSampler):
            return "the dense sampler (UniformNeighborSampler): the batch builder walks a CSR"
        if not isinstance(s, SparseUniformNeighborSampler):
            return "a sampler class the fused K1 does not know (%s)" % type(s).__name__
        if s.rng != "philox":
            return ("the sampler's rng mode %r: padded rows sit in the middle of the id batch and the reference's draw "
                    "order has no place for them (use --rng philox)" % (s.rng,))
        if ddp is not None:
            return "a data-parallel handle: the unsupervised engine runs in one process"
        if pipelined:
            return "pipelined=True: the unsupervised engine runs one batch at a time"
        if eval_only:
            return "eval_only=True: there is no evaluation engine for the unsupervised model (model.evaluate runs it)"
        why = cls._why_not_common(model, feats, (MeanAggregator,), "mean") or \
            cls._why_not_input(model, feats, None, concat_ok=False, fp8_ok=False)
        if why:
            return why
        if not all(l.output_dim_ % 8 == 0 for l in layers):
            return "output dims that are not multiples of 8"
        post = _split_activation(layers[-1].activation)[1]
        probe = torch.linspace(-2.0, 2.0, 12).view(3, 4)
        if post is not None and not torch.equal(post(probe), probe):
            return "an activation on the last layer other than the identity"
        if int(model.output_dim) > 1024 or not 1 <= int(model.n_negatives) <= 64:
            return "an embedding wider than 1024 or more than 64 negatives (the skip-gram head's limits)"
        return None

    @classmethod
    def head_why_not(cls, model, loss_fn, example_targets, batch, padded, world=1):
        """The skip-gram head ignores padded seeds itself: nothing about the head stops this engine."""
        return None

    def __init__(self, model, feats, example_seeds, capture=True, warmup=2, pipelined=False, eval_only=False, ddp=None):
        why = type(self).why_not(model, feats, ddp, pipelined=pipelined, eval_only=eval_only)
        if why is not None:
            raise ValueError("%s does not cover this (model, feature store): %s" % (type(self).__name__, why))
        if not (torch.is_tensor(example_seeds) and example_seeds.is_cuda and example_seeds.dtype == torch.int64
                and example_seeds.dim() == 1 and int(example_seeds.shape[0]) >= 1):
            raise ValueError("example_seeds must be a CUDA int64 vector of seed ids (one batch)")
        self.Bs, self.Q = int(example_seeds.shape[0]), int(model.n_negatives)
        R = 2 * self.Bs + self.Q
        self._example_seeds = example_seeds
        ids = torch.zeros(R, dtype=torch.int64, device=example_seeds.device)
        ids[:self.Bs] = example_seeds
        # (the base engine keeps one target per row of ITS batch: nothing reads them here)
        super(FusedUnsupMeanTrainStep, self).__init__(model, feats, None, ids, torch.zeros(R, device=ids.device),
                                                      ddp=None, capture=capture, warmup=warmup)
        del self._example_seeds

    # ---- the head's hooks (common.py) ------------------------------------------------------------------------------
    def _will_fuse_head(self, example_targets):
        return False                              # (no classifier: so no fused seed level either, _will_fuse_tail)

    def _head_recordable(self):
        return True

    def _head_reduce_descs(self):
        return []                                 # no fc: the head owns no parameter

    def _init_head(self, loss_fn, example_targets):
        model, dev, Bs, Q = self.model, self.dev, self.Bs, self.Q
        self.fused_head = self.fused_l1 = self.fused_tail = self.fused_wide = False
        self.D = int(model.output_dim)
        assert self.D == int(self.hout[self.L - 1].shape[1])
        f32 = torch.float32
        self.seeds = self._example_seeds.clone().contiguous()
        self.pair_w = torch.zeros(Bs, dtype=f32, device=dev)
        self.loss = torch.zeros(1, dtype=f32, device=dev)
        self.aff = torch.zeros(Bs, 1 + Q, dtype=f32, device=dev)
        self.head_scratch = torch.zeros(max(int(nat.lib().gsage_head_skipgram_scratch(Bs, Q, self.D)), 1), dtype=f32,
                                        device=dev)
        # live seeds of the batch (the base engine's n_valid counts ITS rows, all R of them)
        self.n_live = torch.full((1,), Bs, dtype=torch.int32, device=dev)
        self._live_host = Bs
        # the builder's graph and table are the model's own (GSUnsupervised._walk_graph): same walks, same negatives
        self.walk_csr, self.cdf = model._walk_graph(True, dev)
        # call index of step t = _call_base + *batch_ctr; the finalisation launch advances the word (_stage_finalize),
        # the warm-up's steps are taken back (_warm_reset), model._batch_calls moves in __call__ only
        self._call_base = int(model._batch_calls[1])
        self.batch_ctr = torch.zeros(1, dtype=torch.int64, device=dev)
        self._ctr_host = 0
        self._warm_reset = tuple(self._warm_reset) + (self.batch_ctr,)

    # ---- stages ----------------------------------------------------------------------------------------------------
    def _stage_batch_biased(self, s, edge_cdf):
        """gsage_unsup_batch_biased (the model's walk_p / walk_q are not neutral): the same buffers, the same stream"""
        csr, cdf, m = self.walk_csr, self.cdf, self.model
        self._time_next(*self.TIMED["builder"])
        nat.check(nat.lib().gsage_unsup_batch_biased(
            csr.rowptr.data_ptr(), csr.col.data_ptr(), edge_cdf, csr.n_rows, self.seeds.data_ptr(), self.Bs, m.walk_len,
            self.Q, cdf.data_ptr(), cdf._gsage_total, int(getattr(self.sampler, "seed", 0)), self.batch_ctr.data_ptr(),
            self._call_base, 0, float(m.walk_p), float(m.walk_q), self.ids_set[s].data_ptr(), self.pair_w.data_ptr(),
            csr.err_flag.data_ptr(), ops._stream()), "unsup_batch_biased")

    def _stage_batch(self, s):
        """gsage_unsup_batch: the seed buffer -> the first R ids of the frontier buffer + pair_w"""
        csr, cdf, m = self.walk_csr, self.cdf, self.model
        if getattr(m, "biased_walks", False):
            return self._stage_batch_biased(s, None)
        self._time_next(*self.TIMED["builder"])
        nat.check(nat.lib().gsage_unsup_batch(
            csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.n_rows, self.seeds.data_ptr(), self.Bs, m.walk_len, self.Q,
            cdf.data_ptr(), cdf._gsage_total, int(getattr(self.sampler, "seed", 0)), self.batch_ctr.data_ptr(),
            self._call_base, 0, self.ids_set[s].data_ptr(), self.pair_w.data_ptr(), csr.err_flag.data_ptr(),
            ops._stream()), "unsup_batch")

    def _stage_sample_gather(self, s):
        self._stage_batch(s)
        super(FusedUnsupMeanTrainStep, self)._stage_sample_gather(s)

    def _stage_head(self, s):
        """normalize + cosines + skip-gram loss + d loss / d rows (two launches); rows of padded seeds come out zero"""
        L = self.L
        E, dE = self.hout[L - 1], self.dc[L - 1]
        marks = self._marks and self._in_list
        if marks:
            nat.check(nat.lib().gsage_cmdlist_mark(self.TIMED["head"][0]), "cmdlist_mark")
        nat.check(nat.lib().gsage_head_skipgram_live(
            E.data_ptr(), E.stride(0), self.Bs, self.Q, self.D, self.pair_w.data_ptr(), float(self.model.neg_weight),
            self.n_live.data_ptr(), dE.data_ptr(), self.code, dE.stride(0), self.loss.data_ptr(), self.aff.data_ptr(),
            self.head_scratch.data_ptr(), ops._stream()), "head_skipgram_live")
        if marks:
            nat.check(nat.lib().gsage_cmdlist_mark(self.TIMED["head"][1]), "cmdlist_mark")

    def _stage_finalize(self, s):
        """the mean engine's finalisation; its second tick advances the builder's call index"""
        assert not self._fold_finalize()
        nat.check(nat.lib().gsage_finalize_grads(self.rdescs.data_ptr(), self.n_rdesc, self.r_max,
                                                 self.flat_g.data_ptr(), self.partial.data_ptr(), self.step.data_ptr(),
                                                 self.counter.data_ptr(), self.L, self.batch_ctr.data_ptr(), 1,
                                                 ops._stream()), "finalize_grads")

    # ---- entry points ----------------------------------------------------------------------------------------------
    def load_epoch(self, *a, **k):
        raise ValueError("FusedUnsupMeanTrainStep runs one batch per call: there is no queue mode")

    def step_queue(self, *a, **k):
        raise ValueError("FusedUnsupMeanTrainStep runs one batch per call: there is no queue mode")

    def __call__(self, seeds):
        """One train step on `seeds` (int64, 2 <= len <= the recorded batch) -> the loss (device scalar)."""
        self._rows_tick()
        seeds = seeds.contiguous().view(-1)
        b = int(seeds.shape[0])
        if b != self.Bs:
            if not 2 <= b < self.Bs:
                raise ValueError("this engine was recorded for batches of %d seeds (got %d)" % (self.Bs, b))
            seeds = torch.cat([seeds, seeds[:1].expand(self.Bs - b)])
        if b != self._live_host:
            self._live_host = b
            self.n_live.fill_(b)
        # the model's stream may have moved without us (a module-path step, evaluate on the training graph)
        want = int(self.model._batch_calls[1]) - self._call_base
        if want != self._ctr_host:
            self.batch_ctr.fill_(want)
        self.seeds.copy_(seeds.to(self.dev), non_blocking=True)
        self.n_calls += 1
        if self.g_main is None:
            self._run_sequential(0)
        else:
            self.g_main[0].replay()
        self.model._batch_calls[1] += 1
        self._ctr_host = want + 1
        return self.loss.view(())


class FusedUnsupWeightedMeanTrainStep(FusedUnsupMeanTrainStep):
    """FusedUnsupMeanTrainStep for a GSUnsupervised(weighted_walks=True) whose samplers are
    SparseWeightedNeighborSampler: same constructor, same `__call__(seeds)`.  Two launches differ:

        builder       gsage_unsup_batch_weighted: every step of a walk drawn from the adjacency's edge_cdf
        K1w           gsage_sample_hops_weighted, a launch of its own (as in FusedWeightedMeanTrainStep)

    Step t builds the batch the model's `build_batch` would build at that point of its stream and draws hop k with the
    call index a SparseWeightedNeighborSampler consumes on the module path, so both paths see the same id batch, the
    same pair_w and the same frontier.  Opt-in (train.py --unsupervised --weighted-walks --engine fused): not one of
    engine.ENGINES."""

    TIMED = dict(FusedUnsupMeanTrainStep.TIMED, sampler=(14, 15))

    @classmethod
    def why_not(cls, model, feats, ddp=None, pipelined=False, eval_only=False):
        """None, or one sentence: what of (model, feats, mode) this engine does not cover -- the sentences of
        FusedUnsupMeanTrainStep and FusedWeightedMeanTrainStep, the model's first, the feature store's last."""
        from ..models import GSUnsupervised
        if not isinstance(model, GSUnsupervised):
            return "a model that is not GSUnsupervised (%s: the supervised engines train it)" % type(model).__name__
        if not getattr(model, "weighted_walks", False):
            return ("a GSUnsupervised with weighted_walks=False: its walks take uniform steps "
                    "(FusedUnsupMeanTrainStep runs them over a uniform sampler)")
        layers = list(model.agg_layers.children())
        if not layers or any(type(l) is not MeanAggregator for l in layers):
            return ("aggregators other than mean (%s): the pool, attention and LSTM aggregators have no unsupervised "
                    "engine" % ", ".join(sorted({type(l).__name__ for l in layers})))
        if isinstance(model.prep, NodeEmbeddingPrep):
            return "the node_embedding prep (a trainable table under the skip-gram loss has no fused form)"
        for s in (model.train_sampler, model.val_sampler):
            if not isinstance(s, SparseWeightedNeighborSampler):
                return ("a train / validation sampler that is not SparseWeightedNeighborSampler (%s: "
                        "FusedUnsupMeanTrainStep covers the uniform sparse sampler)" % type(s).__name__)
        if ddp is not None:
            return "a data-parallel handle: the unsupervised engine runs in one process"
        if pipelined:
            return "pipelined=True: the unsupervised engine runs one batch at a time"
        if eval_only:
            return "eval_only=True: there is no evaluation engine for the unsupervised model (model.evaluate runs it)"
        why = cls._why_not_common(model, feats, (MeanAggregator,), "mean", sampler=False)
        if why:
            return why
        if not all(l.output_dim_ % 8 == 0 for l in layers):
            return "output dims that are not multiples of 8"
        post = _split_activation(layers[-1].activation)[1]
        probe = torch.linspace(-2.0, 2.0, 12).view(3, 4)
        if post is not None and not torch.equal(post(probe), probe):
            return "an activation on the last layer other than the identity"
        if int(model.output_dim) > 1024 or not 1 <= int(model.n_negatives) <= 64:
            return "an embedding wider than 1024 or more than 64 negatives (the skip-gram head's limits)"
        return cls._why_not_input(model, feats, None, concat_ok=False, fp8_ok=False)

    # ---- stages ----------------------------------------------------------------------------------------------------
    def _stage_batch(self, s):
        """gsage_unsup_batch_weighted: the seed buffer -> the first R ids of the frontier buffer + pair_w"""
        csr, cdf, m = self.walk_csr, self.cdf, self.model
        if getattr(m, "biased_walks", False):
            return self._stage_batch_biased(s, csr.edge_cdf.data_ptr())
        self._time_next(*self.TIMED["builder"])
        nat.check(nat.lib().gsage_unsup_batch_weighted(
            csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.edge_cdf.data_ptr(), csr.n_rows, self.seeds.data_ptr(),
            self.Bs, m.walk_len, self.Q, cdf.data_ptr(), cdf._gsage_total, int(getattr(self.sampler, "seed", 0)),
            self.batch_ctr.data_ptr(), self._call_base, 0, self.ids_set[s].data_ptr(), self.pair_w.data_ptr(),
            csr.err_flag.data_ptr(), ops._stream()), "unsup_batch_weighted")

    def _stage_sample(self, s, ids=None, ahead=False, counters=None):
        """K1w: every hop in one launch, drawn from the adjacency's edge_cdf (FusedWeightedMeanTrainStep's stage)"""
        d = self._hops_desc(self.ids_set[s] if ids is None else ids, ahead, counters)
        self._time_next(*self.TIMED["sampler"])
        nat.check(nat.lib().gsage_sample_hops_weighted(ctypes.addressof(d), self.csr.edge_cdf.data_ptr(), ops._stream()),
                  "sample_hops_weighted")

    _k1_own_launch = FusedWeightedMeanTrainStep._k1_own_launch
    _k1_in_k5 = FusedWeightedMeanTrainStep._k1_in_k5
    _k1_in_tail = FusedWeightedMeanTrainStep._k1_in_tail
    _k1_early = FusedWeightedMeanTrainStep._k1_early

    def load_epoch(self, *a, **k):
        raise ValueError("FusedUnsupWeightedMeanTrainStep runs one batch per call: there is no queue mode")

    def step_queue(self, *a, **k):
        raise ValueError("FusedUnsupWeightedMeanTrainStep runs one batch per call: there is no queue mode")


class FusedUnsupTemporalMeanTrainStep(FusedUnsupMeanTrainStep):
    """FusedUnsupMeanTrainStep for a GSUnsupervised(temporal_walks=True) whose samplers are
    SparseTemporalNeighborSampler: the same constructor plus `example_times` / `keep_times`, and `__call__(seeds,
    times=None)`.  Two launches differ:

        builder       gsage_unsup_batch_temporal: walks that respect time; beside the first R ids of the frontier buffer
                      it writes an int64 times buffer of R entries (negative q: the time of live seed q % b, b the live
                      count)
        K1t           gsage_sample_hops_temporal, a launch of its own (as in FusedTemporalMeanTrainStep), with that
                      buffer as hop 0's times

    times=None means the sampler's default_times(seeds); a batch short of the recorded one pads its times with the first
    seed's, as its seeds are padded.  The walk's rule and the sampler's strategy / rule are the train sampler's.
    keep_times=True makes K1t write the whole frontier's times to `times_set[s]`, laid out like `ids_set[s]` (tests).
    Step t builds the batch the model's `build_batch` would build at that point of its stream and draws hop k with the
    call index a fresh SparseTemporalNeighborSampler consumes on the module path.  Opt-in (train.py --unsupervised
    --temporal-walks --engine fused): not one of engine.ENGINES."""

    TIMED = dict(FusedUnsupMeanTrainStep.TIMED, sampler=(14, 15))

    @classmethod
    def why_not(cls, model, feats, ddp=None, pipelined=False, eval_only=False):
        """None, or one sentence: what of (model, feats, mode) this engine does not cover -- the sentences of
        FusedUnsupMeanTrainStep and FusedTemporalMeanTrainStep, the model's first, the feature store's last."""
        from ..models import GSUnsupervised
        if not isinstance(model, GSUnsupervised):
            return "a model that is not GSUnsupervised (%s: the supervised engines train it)" % type(model).__name__
        if not getattr(model, "temporal_walks", False):
            return ("a GSUnsupervised with temporal_walks=False: its walks know no time "
                    "(FusedUnsupMeanTrainStep runs them over a uniform sampler)")
        layers = list(model.agg_layers.children())
        if not layers or any(type(l) is not MeanAggregator for l in layers):
            return ("aggregators other than mean (%s): the pool, attention and LSTM aggregators have no unsupervised "
                    "engine" % ", ".join(sorted({type(l).__name__ for l in layers})))
        if isinstance(model.prep, NodeEmbeddingPrep):
            return "the node_embedding prep (a trainable table under the skip-gram loss has no fused form)"
        for s in (model.train_sampler, model.val_sampler):
            if not isinstance(s, SparseTemporalNeighborSampler):
                return ("a train / validation sampler that is not SparseTemporalNeighborSampler (%s: "
                        "FusedUnsupMeanTrainStep covers the uniform sparse sampler)" % type(s).__name__)
        if ddp is not None:
            return "a data-parallel handle: the unsupervised engine runs in one process"
        if pipelined:
            return "pipelined=True: the unsupervised engine runs one batch at a time"
        if eval_only:
            return "eval_only=True: there is no evaluation engine for the unsupervised model (model.evaluate runs it)"
        if isinstance(feats, FeatureStore) and feats.is_fp8:
            return "an FP8 feature store (the temporal engine reads bf16 / fp32 rows)"
        why = cls._why_not_common(model, feats, (MeanAggregator,), "mean", sampler=False)
        if why:
            return why
        if not all(l.output_dim_ % 8 == 0 for l in layers):
            return "output dims that are not multiples of 8"
        post = _split_activation(layers[-1].activation)[1]
        probe = torch.linspace(-2.0, 2.0, 12).view(3, 4)
        if post is not None and not torch.equal(post(probe), probe):
            return "an activation on the last layer other than the identity"
        if int(model.output_dim) > 1024 or not 1 <= int(model.n_negatives) <= 64:
            return "an embedding wider than 1024 or more than 64 negatives (the skip-gram head's limits)"
        return cls._why_not_input(model, feats, None, concat_ok=False, fp8_ok=False)

    def __init__(self, model, feats, example_seeds, capture=True, warmup=2, pipelined=False, eval_only=False, ddp=None,
                 example_times=None, keep_times=False):
        self._example_times, self.keep_times = example_times, bool(keep_times)
        super(FusedUnsupTemporalMeanTrainStep, self).__init__(model, feats, example_seeds, capture=capture, warmup=warmup,
                                                              pipelined=pipelined, eval_only=eval_only, ddp=ddp)
        del self._example_times

    _batch_times = FusedTemporalMeanTrainStep._batch_times

    def _init_head(self, loss_fn, example_targets):
        super(FusedUnsupTemporalMeanTrainStep, self)._init_head(loss_fn, example_targets)
        # the seeds' query times (the builder's input) and the R times it writes (hop 0's times of K1t)
        self.seed_times = self._batch_times(self._example_seeds, self._example_times, self.Bs).clone()
        self.times_in = torch.zeros(2 * self.Bs + self.Q, dtype=torch.int64, device=self.dev)
        # keep_times: the frontier's times beside every frontier buffer, keyed by the buffer the launch writes
        self.times_set = [torch.zeros_like(t) if self.keep_times else None for t in self.ids_set]
        self._times_of = {t.data_ptr(): tt for t, tt in zip(self.ids_set, self.times_set)}

    # ---- stages ----------------------------------------------------------------------------------------------------
    def _stage_batch(self, s):
        """gsage_unsup_batch_temporal: seeds + their times -> the first R ids of the frontier buffer, R times, pair_w"""
        csr, cdf, m = self.walk_csr, self.cdf, self.model
        self._time_next(*self.TIMED["builder"])
        nat.check(nat.lib().gsage_unsup_batch_temporal(
            csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.etime.data_ptr(), csr.n_rows, self.seeds.data_ptr(),
            self.seed_times.data_ptr(), self.Bs, m.walk_len, self.Q, cdf.data_ptr(), cdf._gsage_total,
            int(getattr(self.sampler, "seed", 0)), self.batch_ctr.data_ptr(), self._call_base, 0,
            ops.TEMPORAL_INHERIT[self.sampler.inherit], self.n_live.data_ptr(), self.ids_set[s].data_ptr(),
            self.times_in.data_ptr(), self.pair_w.data_ptr(), csr.err_flag.data_ptr(), ops._stream()),
            "unsup_batch_temporal")

    def _stage_sample(self, s, ids=None, ahead=False, counters=None):
        """K1t: every hop in one launch, among the edges before the builder's times (FusedTemporalMeanTrainStep's stage)"""
        ids = self.ids_set[s] if ids is None else ids
        d = self._hops_desc(ids, ahead, counters)
        kept = self._times_of.get(ids.data_ptr()) if self.keep_times else None
        self._time_next(*self.TIMED["sampler"])
        nat.check(nat.lib().gsage_sample_hops_temporal(
            ctypes.addressof(d), self.csr.etime.data_ptr(), self.times_in.data_ptr(), None,
            ops.TEMPORAL_STRATEGIES[self.sampler.strategy], ops.TEMPORAL_INHERIT[self.sampler.inherit],
            kept.data_ptr() if kept is not None else None, ops._stream()), "sample_hops_temporal")

    _k1_own_launch = FusedTemporalMeanTrainStep._k1_own_launch
    _k1_in_k5 = FusedTemporalMeanTrainStep._k1_in_k5
    _k1_in_tail = FusedTemporalMeanTrainStep._k1_in_tail
    _k1_early = FusedTemporalMeanTrainStep._k1_early

    def load_epoch(self, *a, **k):
        raise ValueError("FusedUnsupTemporalMeanTrainStep runs one batch per call: there is no queue mode")

    def step_queue(self, *a, **k):
        raise ValueError("FusedUnsupTemporalMeanTrainStep runs one batch per call: there is no queue mode")

    def __call__(self, seeds, times=None):
        """One train step on `seeds` (int64, 2 <= len <= the recorded batch) and their query times (int64, one per
        seed; None: the sampler's default_times(seeds)) -> the loss (device scalar)."""
        seeds = seeds.contiguous().view(-1)
        if 2 <= int(seeds.shape[0]) <= self.Bs:                # (any other length: the base class says so)
            self.seed_times.copy_(self._batch_times(seeds, times, self.Bs), non_blocking=True)
        return super(FusedUnsupTemporalMeanTrainStep, self).__call__(seeds)
