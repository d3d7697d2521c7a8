"""
pytorch-graphsage_amd -- MI355X (gfx950) native GraphSAGE training hot path behind the plugin
surface of bkj/pytorch-graphsage.  Directory name has a hyphen: import it with
`importlib.import_module("pytorch-graphsage_amd")`, or run `pytorch-graphsage_amd/train.py`.

    csrc/ + libgsage_hip.so   hand-written HIP kernels behind the C ABI of include/gsage.h
    _native.py                ctypes binding (fails loudly when the library is missing)
    ops.py / store.py         tensor-level operators, HBM data layouts
    nn_modules.py, models.py, problem.py, helpers.py, lr.py, train.py
                              same names and interfaces as the reference's files
    dist.py                   RCCL data-parallel gradient sync
    infer.py                  layer-wise full-neighbourhood inference, node-embedding export; for a query set, over
                              its k-hop closure blocks (infer.closure / infer.query); infer.nearest: the k nearest
                              rows of an embedding table (ops.topk_ip, csrc/gsage_retrieve.hip); infer.link_rank /
                              link_metrics / held_out_edges: the exact (filtered) rank of an edge's other endpoint
                              among all rows, MRR and hits@k (ops.rank_ip, csrc/gsage_rank.hip); infer.linear_probe /
                              probe_eval: a linear classifier fitted on the frozen embeddings, micro / macro F1 of
                              the val / test folds (ops.probe_pass, csrc/gsage_probe.hip); infer.kmeans /
                              cluster_metrics / cluster_eval: Lloyd's k-means on the frozen embeddings, NMI and
                              purity against the labels (ops.kmeans_pass / kmeans_update, csrc/gsage_kmeans.hip)
    propagate.py              propagation over the graph after the encoder has run: gs.propagate (one fused step of
                              csrc/gsage_propagate.hip per iteration), gs.label_propagation, gs.correct_and_smooth,
                              gs.correct_smooth_eval
    store.WeightedAdj         edge weights: sparse_weighted_neighbor_sampler, weight-normalised full-neighbourhood mean
    store.importance_adj      any adjacency -> its importance-weighted one: visit counts of short random walks, the
                              top-T most-visited nodes per row (DeviceCSR.importance, csrc/gsage_importance.hip);
                              p=, q=, restart=: node2vec-biased walks with restarts (gsage_importance_walks_biased)
    store.graph_from_edges    an edge list -> the adjacency (scipy matrix / WeightedAdj / TemporalAdj), built on the GPU:
                              DeviceCSR.from_edges / .transpose() / .symmetrized() (ops.edges_to_csr, ops.csr_transpose,
                              csrc/gsage_build.hip); gs.problem_from_edges: a NodeProblem from an edge list;
                              `convert edges`: the problem file
    models.GSUnsupervised     label-free training: random-walk positives, degree^0.75 negatives, skip-gram head;
                              weighted_walks=True: over a weighted adjacency the walks draw every step by edge weight
                              (ops.unsup_batch(weighted=True), gsage_unsup_batch_weighted); walk_p=, walk_q=: node2vec's
                              return / in-out parameters (ops.unsup_batch(p=, q=), gsage_unsup_batch_biased);
                              temporal_walks=True: over the temporal sampler the walks respect time and the query times
                              travel with the batch (ops.unsup_batch_temporal, gsage_unsup_batch_temporal)
    nn_modules.SparseDistinctNeighborSampler   neighbours WITHOUT replacement (sparse_distinct_neighbor_sampler in
                              sampler_extensions; ops.sample_csr_distinct, csrc/gsage_distinct.hip): every neighbour of a
                              short row, n distinct ones of a long row
    nn_modules.SparseTemporalNeighborSampler   neighbours among the edges BEFORE a query time (sparse_temporal_neighbor_
                              sampler in sampler_extensions; ops.sample_csr_temporal, csrc/gsage_temporal.hip) over a
                              store.TemporalAdj; store.DeviceCSR.snapshot(t): the graph "as of t" for everything in
                              infer.py and propagate.py
    engine/                   the whole train_step as recorded launches (captured autograd path; fused mean /
                              pool / attention engines on a shared base; opt-in: the weighted mean engine, the
                              distinct-draw mean engine FusedDistinctMeanTrainStep and the unsupervised engines,
                              FusedUnsupMeanTrainStep / FusedUnsupWeightedMeanTrainStep / FusedUnsupTemporalMeanTrainStep)
"""
from . import _native, dist, engine, helpers, infer, nn_modules, ops, optim, problem, store        # noqa: F401
from .helpers import set_seeds, to_numpy                            # noqa: F401
from .infer import (KMeans, LinearProbe, cluster_eval, cluster_metrics, embeddings, full_neighbour,   # noqa: F401
                    held_out_edges, kmeans, linear_probe, link_metrics, link_rank, nearest, probe_eval, query)
from .lr import LRSchedule                                          # noqa: F401
from .models import GSSupervised, GSUnsupervised                                # noqa: F401
from .nn_modules import aggregator_lookup, find_sampler, prep_lookup, sampler_extensions, sampler_lookup   # noqa: F401
# (gs.propagate is the FUNCTION; its module is sys.modules[gs.propagate.__module__])
from .propagate import correct_and_smooth, correct_smooth_eval, label_propagation, propagate   # noqa: F401
from .problem import DeviceMetrics, NodeProblem, ProblemLosses, ProblemMetrics, batch_metric   # noqa: F401
from .store import (DenseAdj, DeviceCSR, FeatureStore, RowRef, TemporalAdj, WeightedAdj, graph_from_edges,  # noqa: F401
                    importance_adj)
from .convert import problem_from_edges                             # noqa: F401

__all__ = ["GSSupervised", "GSUnsupervised", "NodeProblem", "aggregator_lookup", "prep_lookup", "sampler_lookup",
           "set_seeds", "to_numpy", "LRSchedule", "FeatureStore", "DeviceCSR", "RowRef", "ops", "full_neighbour",
           "embeddings", "query", "nearest", "link_rank", "link_metrics", "held_out_edges", "LinearProbe", "linear_probe",
           "probe_eval", "KMeans", "kmeans", "cluster_metrics", "cluster_eval", "WeightedAdj", "TemporalAdj", "find_sampler", "sampler_extensions", "importance_adj",
           "propagate", "label_propagation", "correct_and_smooth", "correct_smooth_eval", "graph_from_edges",
           "problem_from_edges"]
