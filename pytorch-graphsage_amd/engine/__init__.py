"""
engine -- the whole train_step (reference models.py:97-104) as recorded launches.

  captured.CapturedTrainStep   GSSupervised.train_step under autograd, captured once as hipGraphs
  common.FusedTrainStep        what the fused engines share (buckets, sampler descriptor, head, finalise + Adam,
                               command lists / graphs, batch queue + software pipeline, data-parallel order)
  mean.FusedMeanTrainStep      mean aggregators (BASELINE configs[1], [4])
  pool.FusedPoolTrainStep      max-pool / mean-pool aggregators (configs[2])
  attn.FusedAttnTrainStep      attention aggregators, optionally over trainable node embeddings (configs[3])
  unsup.FusedUnsupMeanTrainStep  GSUnsupervised under mean aggregators: builder, encoder, skip-gram head, update
                               (opt-in: train.py --unsupervised --engine fused; not one of ENGINES, whose call takes targets)
  unsup.FusedUnsupWeightedMeanTrainStep  FusedUnsupMeanTrainStep over a weighted adjacency: the builder's walk steps
                               (gsage_unsup_batch_weighted) and every hop (gsage_sample_hops_weighted) drawn from the
                               per-edge cdf table (opt-in: train.py --unsupervised --weighted-walks --engine fused; not
                               one of ENGINES)
  unsup.FusedUnsupTemporalMeanTrainStep  FusedUnsupMeanTrainStep over a temporal adjacency: walks that respect time
                               (gsage_unsup_batch_temporal) and every hop drawn among the edges before the batch's
                               query times (gsage_sample_hops_temporal) (opt-in: train.py --unsupervised --temporal-walks
                               --engine fused; not one of ENGINES)
  weighted.FusedWeightedMeanTrainStep  the mean engine over a weighted adjacency: every hop drawn from the per-edge
                               cdf table by one sampler launch of its own (gsage_sample_hops_weighted), everything
                               behind it the mean engine's (opt-in: train.py --engine fused with the weighted sampler;
                               not one of ENGINES: fused_engine_for / why_no_fused_engine answer as without it)
  distinct.FusedDistinctMeanTrainStep  the mean engine over the distinct-draw sampler: every hop drawn without
                               replacement by one sampler launch of its own (gsage_sample_hops_distinct), everything
                               behind it the mean engine's (opt-in: train.py --engine fused with the distinct sampler;
                               not one of ENGINES)
  temporal.FusedTemporalMeanTrainStep  the mean engine over the temporal sampler: every hop drawn among the edges before
                               the query time by one sampler launch of its own (gsage_sample_hops_temporal), the seeds'
                               query times per call, from the epoch queue and in evaluation; everything behind it the
                               mean engine's (opt-in: train.py --engine fused with the temporal sampler; not one of ENGINES)

`fused_engine_for(model, feats)` picks the engine that covers a model, or explains why none does.
"""
import sys

from .captured import CapturedTrainStep                      # noqa: F401
from .common import FusedTrainStep, _PrepDesc, _ReduceDesc   # noqa: F401
from .mean import FusedMeanTrainStep
from .pool import FusedPoolTrainStep
from .attn import FusedAttnTrainStep
from .unsup import FusedUnsupMeanTrainStep, FusedUnsupTemporalMeanTrainStep, FusedUnsupWeightedMeanTrainStep   # noqa: F401
from .weighted import FusedWeightedMeanTrainStep             # noqa: F401
from .distinct import FusedDistinctMeanTrainStep             # noqa: F401
from .temporal import FusedTemporalMeanTrainStep             # noqa: F401

ENGINES = (FusedMeanTrainStep, FusedPoolTrainStep, FusedAttnTrainStep)


def why_no_fused_engine(model, feats, ddp=None):
    """{engine name: what it does not cover} for every fused engine (empty when one covers the model)."""
    out = {}
    for cls in ENGINES:
        why = cls.why_not(model, feats, ddp)
        if why is None:
            return {}
        out[cls.__name__] = why
    return out


def fused_engine_for(model, feats, explain=False, ddp=None):
    """The fused train-step engine that covers (model, feats), or None (callers then fall back to
    GSSupervised.train_step, optionally captured by CapturedTrainStep).  explain=True: when none does, say on
    stderr what each engine misses, so nobody lands on the slow path without knowing.  ddp: the data-parallel handle
    the engine will be built with (dist.DataParallel), so that what an engine cannot do under it is said HERE."""
    for cls in ENGINES:
        if cls.supports(model, feats, ddp):
            return cls
    if explain:
        why = why_no_fused_engine(model, feats, ddp)
        print("gsage: no fused train-step engine covers this model -- " +
              "; ".join("%s: %s" % kv for kv in why.items()), file=sys.stderr)
    return None
