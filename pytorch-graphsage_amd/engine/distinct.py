"""
engine/distinct.py -- FusedDistinctMeanTrainStep: the mean engine over the distinct-draw sampler (include/gsage.h,
"Distinct neighbours").  Only where the frontier comes from differs from FusedMeanTrainStep: every hop is drawn without
replacement by gsage_sample_hops_distinct, a launch of its own; every launch behind the sampler is the mean engine's.
"""
import ctypes

from .. import _native as nat
from .. import ops
from ..nn_modules import NodeEmbeddingPrep, SparseDistinctNeighborSampler
from ..store import FeatureStore
from .mean import FusedMeanTrainStep


class FusedDistinctMeanTrainStep(FusedMeanTrainStep):
    """FusedMeanTrainStep for a model whose samplers are SparseDistinctNeighborSampler: same constructor, `__call__(ids,
    targets)`, `load_epoch` / `step_queue` and `eval_only=True` / `evaluate_fold`, same heads.  One step:

        per call      K1d (gsage_sample_hops_distinct: all hops) -> gather -> K5 -> seed level -> K5b -> finalise -> Adam
        queue mode    K5 -> seed level [|| part of the next batch's last-hop means] -> K5b -> finalise ->
                      gather of the next batch || Adam -> K1d of the batch after the next

    The frontier is never a role of another launch (the roles draw with replacement), so the ring of frontier buffers
    stays two deep.  Step t of a fresh engine draws hop k with call index L * t + k - 1 under the sampler's seed and
    g0 = 0: the indices a fresh SparseDistinctNeighborSampler consumes on the module path, so both paths see the same
    frontiers.  Opt-in (train.py --engine fused with the distinct sampler): not one of engine.ENGINES.
    Single process, sequential, identity prep over a bf16 / fp32 FeatureStore."""

    TIMED = dict(FusedMeanTrainStep.TIMED, sampler=(10, 11))

    @classmethod
    def why_not(cls, model, feats, ddp=None, pipelined=False):
        """None, or one sentence: what of (model, feats, mode) this engine does not cover.  What can be said of the
        model alone comes first (so it can be said without a device), the feature store last."""
        for s in (model.train_sampler, model.val_sampler):
            if not isinstance(s, SparseDistinctNeighborSampler):
                return ("a train / validation sampler that is not SparseDistinctNeighborSampler (%s: "
                        "FusedMeanTrainStep covers the uniform samplers)" % type(s).__name__)
        if ddp is not None:
            return "a data-parallel handle: the distinct engine runs in one process"
        if pipelined:
            return "pipelined=True: the distinct engine runs one batch at a time (queue mode is its pipeline)"
        if isinstance(model.prep, NodeEmbeddingPrep):
            return "the node_embedding prep (the distinct engine reads an identity prep over a feature store)"
        if isinstance(feats, FeatureStore) and feats.is_fp8:
            return "an FP8 feature store (the distinct engine reads bf16 / fp32 rows)"
        return cls._why_not_mean(model, feats, None, sampler=False)

    def __init__(self, model, feats, loss_fn, example_ids, example_targets, ddp=None, capture=True, warmup=2,
                 pipelined=False, eval_only=False, wide_head=False):
        why = type(self).why_not(model, feats, ddp, pipelined=pipelined)
        if why is not None:
            raise ValueError("%s does not cover this (model, feature store): %s" % (type(self).__name__, why))
        super(FusedDistinctMeanTrainStep, self).__init__(model, feats, loss_fn, example_ids, example_targets, ddp=None,
                                                         capture=capture, warmup=warmup, pipelined=False,
                                                         eval_only=eval_only, wide_head=wide_head)

    # ---- the sampler: a launch of its own, always -------------------------------------------------------------------
    def _stage_sample(self, s, ids=None, ahead=False, counters=None):
        """K1d: every hop in one launch, drawn without replacement (same descriptor as the uniform K1)."""
        d = self._hops_desc(self.ids_set[s] if ids is None else ids, ahead, counters)
        self._time_next(10, 11)
        nat.check(nat.lib().gsage_sample_hops_distinct(ctypes.addressof(d), ops._stream()), "sample_hops_distinct")

    def _k1_own_launch(self):
        return True

    def _k1_in_k5(self):
        return False

    def _k1_in_tail(self):
        return False

    def _k1_early(self):
        return False
