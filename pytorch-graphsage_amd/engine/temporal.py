"""
engine/temporal.py -- FusedTemporalMeanTrainStep: the mean engine over the temporal sampler (include/gsage.h, "Temporal
neighbours").  Only where the frontier comes from differs from FusedMeanTrainStep: every hop is drawn among the edges
before the query time by gsage_sample_hops_temporal, a launch of its own; every launch behind the sampler is the mean
engine's.  The sampler has a second input per seed, the query time: it reaches the launch from a static buffer per call,
from a device-resident time queue beside the seed queue in queue mode and in evaluation.
"""
import ctypes

import torch

from .. import _native as nat
from .. import ops
from ..nn_modules import NodeEmbeddingPrep, SparseTemporalNeighborSampler
from ..store import FeatureStore
from .mean import FusedMeanTrainStep


class FusedTemporalMeanTrainStep(FusedMeanTrainStep):
    """FusedMeanTrainStep for a model whose samplers are SparseTemporalNeighborSampler: the same constructor plus
    `example_times` / `keep_times`, `__call__(ids, targets, times=None)`, `load_epoch(..., times_epoch=None)` /
    `step_queue` and `eval_only=True` / `evaluate_fold(ids, live, times=None)`, same heads.  One step:

        per call      K1t (gsage_sample_hops_temporal: all hops) -> gather -> K5 -> seed level -> K5b -> finalise -> Adam
        queue mode    K5 -> seed level [|| part of the next batch's last-hop means] -> K5b -> finalise ->
                      gather of the next batch || Adam -> K1t of the batch after the next

    Times.  times=None everywhere means the sampler's default_times: node_time[ids], or INT64_MAX without one -- what
    GSSupervised._encode does.  Per call they are copied into a static int64 [B] buffer before the recorded list replays
    (a batch short of B pads them with its first seed's time, as its ids are padded); in queue mode the sampler launches
    read `times_epoch` int64 [n_batches, B] at the batch index their seed queue uses (batch_base included: the launch that
    samples batch i+2 ahead of the counters reads batch i+2's times); in evaluation a time queue sits beside the id queue.
    The frontier's times live only inside the sampler launch (the gathers read ids); keep_times=True makes the launch
    write them to `times_set[s]` (queue mode: `times_q[par]`), laid out like `ids_set[s]` -- for tests and debugging.

    Strategy and inheritance rule are read from the sampler a launch walks: a training engine takes the train sampler's,
    an eval_only engine the validation sampler's (with its adjacency and seed), so the two may differ.

    The frontier is never a role of another launch, so the ring of frontier buffers stays two deep.  Step t of a fresh
    engine draws hop k with call index L * t + k - 1 under the sampler's seed and g0 = 0: the indices a fresh
    SparseTemporalNeighborSampler consumes on the module path, so both paths see the same frontiers.  Opt-in (train.py
    --engine fused with the temporal sampler): not one of engine.ENGINES.
    Single process, sequential, identity prep over a bf16 / fp32 FeatureStore."""

    TIMED = dict(FusedMeanTrainStep.TIMED, sampler=(10, 11))

    @classmethod
    def why_not(cls, model, feats, ddp=None, pipelined=False):
        """None, or one sentence: what of (model, feats, mode) this engine does not cover.  What can be said of the
        model alone comes first (so it can be said without a device), the feature store last."""
        for s in (model.train_sampler, model.val_sampler):
            if not isinstance(s, SparseTemporalNeighborSampler):
                return ("a train / validation sampler that is not SparseTemporalNeighborSampler (%s: "
                        "FusedMeanTrainStep covers the uniform samplers)" % type(s).__name__)
        if ddp is not None:
            return "a data-parallel handle: the temporal engine runs in one process"
        if pipelined:
            return "pipelined=True: the temporal engine runs one batch at a time (queue mode is its pipeline)"
        if isinstance(model.prep, NodeEmbeddingPrep):
            return "the node_embedding prep (the temporal engine reads an identity prep over a feature store)"
        if isinstance(feats, FeatureStore) and feats.is_fp8:
            return "an FP8 feature store (the temporal engine reads bf16 / fp32 rows)"
        return cls._why_not_mean(model, feats, None, sampler=False)

    def __init__(self, model, feats, loss_fn, example_ids, example_targets, ddp=None, capture=True, warmup=2,
                 pipelined=False, eval_only=False, wide_head=False, example_times=None, keep_times=False):
        why = type(self).why_not(model, feats, ddp, pipelined=pipelined)
        if why is not None:
            raise ValueError("%s does not cover this (model, feature store): %s" % (type(self).__name__, why))
        self._example_times, self.keep_times = example_times, bool(keep_times)
        super(FusedTemporalMeanTrainStep, self).__init__(model, feats, loss_fn, example_ids, example_targets, ddp=None,
                                                         capture=capture, warmup=warmup, pipelined=False,
                                                         eval_only=eval_only, wide_head=wide_head)

    def _init_common(self, model, feats, loss_fn, example_ids, example_targets, ddp, pipelined):
        super(FusedTemporalMeanTrainStep, self)._init_common(model, feats, loss_fn, example_ids, example_targets, ddp,
                                                             pipelined)
        # the seeds' query times of the batch a per-call step samples, and the queue the other modes read instead
        self.times_in = self._batch_times(example_ids, self._example_times, self.B).clone()
        self.time_queue, self.q_times = None, None
        # keep_times: the frontier's times beside every frontier buffer, keyed by the buffer the launch writes
        self.times_set = [torch.zeros_like(t) if self.keep_times else None for t in self.ids_set]
        self._times_of = {t.data_ptr(): tt for t, tt in zip(self.ids_set, self.times_set)}

    def _batch_times(self, ids, times, rows):
        """int64 query times of `ids` on the engine's device (None: the sampler's defaults), padded to `rows` entries
        with the first seed's time"""
        if times is None:
            times = self.sampler.default_times(ids)
        times = times.to(device=self.dev, dtype=torch.int64).contiguous().view(-1)
        if int(times.shape[0]) != int(ids.numel()):
            raise ValueError("times must hold one int64 query time per seed (%d seeds, %d times)"
                             % (int(ids.numel()), int(times.shape[0])))
        pad = rows - int(times.shape[0])
        return torch.cat([times, times[:1].expand(pad)]) if pad > 0 else times

    @property
    def times_q(self):
        """(queue mode, keep_times=True) the kept times of the ring's frontier buffers, times_q[par] beside ids_q[par]"""
        return [self._times_of.get(t.data_ptr()) for t in self.ids_q]

    # ---- the sampler: a launch of its own, always -------------------------------------------------------------------
    def _stage_sample(self, s, ids=None, ahead=False, counters=None):
        """K1t: every hop in one launch, among the edges before the query times (same descriptor as the uniform K1)."""
        ids = self.ids_set[s] if ids is None else ids
        d = self._hops_desc(ids, ahead, counters)
        queued = bool(self.queue)
        kept = self._times_of.get(ids.data_ptr()) if self.keep_times else None
        self._time_next(10, 11)
        nat.check(nat.lib().gsage_sample_hops_temporal(
            ctypes.addressof(d), self.csr.etime.data_ptr(), None if queued else self.times_in.data_ptr(),
            self.time_queue.data_ptr() if queued else None, ops.TEMPORAL_STRATEGIES[self.sampler.strategy],
            ops.TEMPORAL_INHERIT[self.sampler.inherit], kept.data_ptr() if kept is not None else None, ops._stream()),
            "sample_hops_temporal")

    def _k1_own_launch(self):
        return True

    def _k1_in_k5(self):
        return False

    def _k1_in_tail(self):
        return False

    def _k1_early(self):
        return False

    # ---- per call ---------------------------------------------------------------------------------------------------
    def __call__(self, ids, targets, times=None):
        """FusedTrainStep.__call__ with the seeds' query times (None: the sampler's default_times(ids))."""
        if int(ids.shape[0]) <= self.B:                        # (a longer batch: the base class says so)
            self.times_in.copy_(self._batch_times(ids, times, self.B), non_blocking=True)
        return super(FusedTemporalMeanTrainStep, self).__call__(ids, targets)

    # ---- queue mode -------------------------------------------------------------------------------------------------
    def load_epoch(self, ids_epoch, targets_epoch, sel_epoch=None, n_valid=None, times_epoch=None):
        """FusedTrainStep.load_epoch with the epoch's query times: times_epoch int64 [n_batches, B] on the device (None:
        the sampler's default_times of the whole epoch, computed once).  sel_epoch is refused: the temporal sampler
        draws from Philox."""
        if sel_epoch is not None:
            raise ValueError("load_epoch: sel_epoch is not supported (the temporal sampler draws from Philox)")
        if times_epoch is None and torch.is_tensor(ids_epoch) and ids_epoch.dtype == torch.int64:
            times_epoch = self.sampler.default_times(ids_epoch.reshape(-1)).view(ids_epoch.shape)
        if not (torch.is_tensor(times_epoch) and times_epoch.dtype == torch.int64 and times_epoch.is_cuda and
                tuple(times_epoch.shape) == tuple(ids_epoch.shape)):
            raise ValueError("times_epoch must be int64 [n_batches, %d] on the device, one query time per seed of "
                             "ids_epoch" % self.B)
        torch.cuda.synchronize()             # (the previous epoch's last sampler launches still read its time queue)
        self.time_queue = times_epoch.contiguous()
        return super(FusedTemporalMeanTrainStep, self).load_epoch(ids_epoch, targets_epoch, None, n_valid)

    def _record_queue(self):
        if self.keep_times:
            for t in self.ids_q:
                if self._times_of.get(t.data_ptr()) is None:
                    self._times_of[t.data_ptr()] = torch.zeros_like(t)
        super(FusedTemporalMeanTrainStep, self)._record_queue()

    # ---- evaluation -------------------------------------------------------------------------------------------------
    def _finish_init_eval(self, capture, warmup):
        self.q_times = self.times_in.view(1, -1).repeat(self.EVAL_BATCHES, 1)      # the time queue beside q_ids
        self.time_queue = self.q_times
        super(FusedTemporalMeanTrainStep, self)._finish_init_eval(capture, warmup)

    def evaluate_fold(self, ids, live, times=None):
        """FusedTrainStep.evaluate_fold with the seeds' query times: times int64 [n_batches, B], padded like ids (None:
        the validation sampler's default_times(ids))."""
        assert self.eval_only and ids.dim() == 2 and int(ids.shape[1]) == self.B and len(live) == int(ids.shape[0])
        nb, nbuf = int(ids.shape[0]), self.EVAL_BATCHES
        times = self._batch_times(ids, times, nb * self.B).view(nb, self.B)
        outs = []
        for b0 in range(0, nb, nbuf):        # (the queue's buffers hold EVAL_BATCHES batches: longer folds in pieces)
            n = min(nbuf, nb - b0)
            self.q_times[:n].copy_(times[b0:b0 + n])
            outs.append(super(FusedTemporalMeanTrainStep, self).evaluate_fold(ids[b0:b0 + n], live[b0:b0 + n]))
        return outs[0] if len(outs) == 1 else torch.cat(outs)
