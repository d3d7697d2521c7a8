#!/usr/bin/env python
"""
train.py -- command-line driver, drop-in for the reference's train.py: every flag of
train.py:44-66 with the same defaults, the same seeding order (train.py:81,133), the same
per-batch / final / test JSON lines on stdout (train.py:151-157,165-170,174-176) and the
model repr on stderr, so run.sh / utils/pokec.sh work unchanged.

Additions (all optional): --rng {compat,philox}, --precision {bf16,fp32}, data-parallel execution
when launched under torch.distributed.run (one process per GPU, RCCL grad all-reduce), and --engine:

  auto (default)  a fused engine (engine.Fused{Mean,Pool,Attn}TrainStep: a handful of kernel launches per step
                  instead of one framework op per tensor expression) whenever one covers the model, else the
                  module path -- with one stderr line saying which engine runs or why none does.  The run is
                  the reference's run: the epoch is shuffled with numpy's legacy stream and cut into the
                  reference's near-equal `array_split` chunks (problem.py:141-153; a recorded step has one
                  geometry, so chunks one seed short are padded and the head ignores the padding), the sampler
                  consumes the SAME generators in the SAME order (--rng compat: numpy's stream, on the device;
                  dense sampler: torch.randperm), so the sampled frontiers are bit-identical to the module
                  path's and to the reference's, and one JSON line is printed per batch (train.py:150-158).
  fused           the same engines, asked for explicitly: a model none covers is an error, and a line is printed
                  every --log-interval batches only (the reference parses that flag and ignores it,
                  train.py:64) -- the per-batch readback is the one thing left that costs a host sync per step.
  eager           the module path (GSSupervised.train_step), one launch per operator.
Data-parallel runs keep batches of one fixed size (--batch-size / world per rank, counter-based sampler).

--feature-dtype {native,fp8} (default native: nothing changes): fp8 quantises the problem's feature table after
loading to one OCP e4m3 byte per element with a power-of-two scale per column (store.FeatureStore.quantize) and says
on stderr how large the table was and is and the largest absolute error.  The mean engine reads the FP8 table through
the FP8 gather launch; every other model takes the module path (said on stderr, as for every uncovered model).

--wide-head (default off: nothing changes): the multilabel head (2..128 labels) and cross-entropy over 65..128 classes
run on gsage_head_wide inside the engine's step (engine wide_head=True).  That head ignores padded seeds, so such a
problem gets a fused engine whatever the sizes of the reference's chunks, training and evaluation both as native
command lists; one stderr line names the head that runs.  One batch per call (no device-resident queue); one process;
refused with --unsupervised.

Layer-wise full-neighbourhood inference (infer.py, opt-in; the default output is unchanged):
  --full-neighbour-eval   val_metric / test_f1 come from infer.full_neighbour on the val / test folds (deterministic:
                          every neighbour of every node, no sampling) instead of the sampled forward
  --save-embeddings PATH  after training, F.normalize(H^L) of every row of the adjacency, in node-id order, as one
                          .npy (rank 0)
  --eval-closure          with --full-neighbour-eval: each fold is answered from its nodes' k-hop closure alone
                          (infer.query: the same numbers; the cost follows the closure of the fold, about 1 % of the
                          nodes, instead of the graph)
  --embed-nodes IDS.npy   with --save-embeddings: only the rows of the node ids in IDS.npy, in that order (duplicates
                          repeat), computed from their closure (infer.query_embeddings)

Retrieval over the embeddings (infer.nearest, opt-in):
  --save-neighbours PATH  after training, the k nearest rows (inner product of the unit embeddings = cosine) of every
                          row of the adjacency, as one .npz with `ids` int64 [rows, k] and `scores` fp32 [rows, k],
                          best first, ties by ascending id (rank 0).  With --save-embeddings (and no --embed-nodes)
                          the embeddings are computed once for both files.
  --link-eval             after training (sharing the one embedding pass with --save-embeddings / --save-neighbours):
                          filtered link ranking of the held-out edges of the validation fold -- the edges stored in the
                          evaluation adjacency whose source is in the fold and that the training adjacency does not
                          store.  Each edge's target is ranked among ALL rows by gs.link_rank (exact; the source's known
                          edges in the evaluation adjacency do not count against it) and one line
                          {"link_eval": {"fold": "val", "n", "unranked", "mrr", "mean_rank", "hits@k"...}} is printed;
                          with --show-test a second one for the test fold.  The embeddings come from the EVALUATION
                          graph: the held-out edge takes part in message passing, as in GraphSAGE's inductive protocol;
                          call gs.link_rank on embeddings of your own for anything else.  Sparse problems, one process.
  --probe                 after training (sharing the one embedding pass with --save-embeddings / --link-eval): the
                          GraphSAGE paper's judgement of the embeddings.  A linear classifier is fitted on the frozen
                          embeddings of the train fold (gs.linear_probe: zero start, full-batch Adam, every iteration a
                          fused loss / gradient pass of csrc/gsage_probe.hip) and scored on the validation fold with the
                          problem's F1 metric; one line {"probe": {"fold": "val", "task", "micro", "macro", "loss_first",
                          "loss_last"}} is printed, with --show-test a second one for the test fold.  Classification
                          and multilabel problems, with and without --unsupervised; a regression problem exits with
                          one sentence.
  --probe-iters N         Adam iterations (default 100)     --probe-lr F   learning rate (default 0.1)
  --probe-l2 F            Adam's L2 term (default 0).  The defaults reach the toy results of the tests; nobody has
                          tuned them on a real graph.
  --cluster K             after training (sharing the one embedding pass with --save-embeddings / --link-eval / --probe):
                          node clustering.  Lloyd's k-means with K clusters on the frozen embeddings of every node of the
                          three folds (gs.kmeans: every iteration a fused assign / accumulate pass and an update launch of
                          csrc/gsage_kmeans.hip), scored against the labels of the validation fold; one line {"cluster":
                          {"fold": "val", "k", "iters", "inertia", "nmi", "purity"}} is printed, with --show-test a second
                          one for the test fold.  With and without --unsupervised.  A problem without class labels
                          (multilabel, regression) prints the line without nmi and purity: clustering needs no labels.
  --cluster-iters N       Lloyd iterations at most (default 50)   --cluster-init ++|random   (default ++: k-means++)
  --cluster-n-init R      fits with seeds S, S + 1, ..; the lowest inertia is kept (default 1)   --cluster-seed S (0)
  --cluster-spherical     unit-length centroids, assignment by inner product
  --save-clusters PATH    .npz of nodes (the ids that were clustered), labels (theirs) and centroids
  --correct-smooth        after training: Correct and Smooth (gs.correct_smooth_eval, propagate.py) -- the logits of EVERY row by
                          full-neighbourhood inference over the evaluation adjacency, the train fold's residual errors
                          propagated over the graph and added back, the result smoothed with the train labels held
                          (each iteration one fused step of csrc/gsage_propagate.hip); one line {"correct_smooth":
                          {"fold": "val", "task", "base", "corrected", "smoothed"}}, each score {"micro", "macro"}, is
                          printed, with --show-test a second one for the test fold.  "base" is what
                          --full-neighbour-eval prints for the fold.  Supervised classification / multilabel problems
                          with a sparse unweighted adjacency, one process; --unsupervised is refused (no logits).
  --cs-iters 50,50        correct, smooth iterations      --cs-alpha 0.8,0.8   their alpha
  --cs-no-autoscale       hold the labelled residuals instead of rescaling the propagated ones
  --label-prop            with --correct-smooth: also {"label_prop": {"fold", "task", "micro", "macro"}}, plain label
                          propagation from the train labels (--cs-iters' / --cs-alpha's second values).  The defaults are
                          the common published ones; nobody has tuned them on a graph of this project.
  --link-eval-edges M     at most M edges per fold (default 100000), a subsample seeded by --seed when there are more
  --link-eval-ks 1,10,50  the k of hits@k
  --neighbours-k K        how many (default 10, at most 128)
  --neighbour-nodes IDS.npy   with --save-neighbours: only for the node ids in IDS.npy, in that order
  --neighbours-exclude none|self|neighbours   rows a node is never answered with (default self; neighbours: nor a
                          node it already has an edge to in the evaluation adjacency -- link recommendation)

--unsupervised (with --walk-len, --n-negatives, --neg-weight): train the encoder without labels (models.GSUnsupervised:
random-walk positives, degree^0.75 negatives, skip-gram loss on the HIP head).  Targets are ignored; every batch
prints one JSON line with its loss, every epoch the validation fold's loss and mean reciprocal rank ("mrr").  The
module path runs it (said on stderr) under --engine auto / eager; data-parallel launches are refused.  --engine fused
(opt-in, with --rng philox, mean aggregators, the identity prep and the sparse sampler) runs every step as one recorded
list of launches on engine.FusedUnsupMeanTrainStep -- batch builder, sampler, encoder, skip-gram head, backward,
update -- and is an error, with the engine's sentence, where that engine does not cover the run.

--sampler-class sparse_weighted_neighbor_sampler: neighbours drawn in proportion to edge weights (a problem file with
`adj_weight` / `train_adj_weight`; include/gsage.h, "Weighted adjacency").  Always Philox; under --engine auto / eager
the module path runs it (said on stderr, with the name of the engine --engine fused would select); --engine fused (opt-in,
mean aggregators, the identity prep over a bf16 / fp32 table, one process) runs training on
engine.FusedWeightedMeanTrainStep -- the mean engine behind one sampler launch that draws every hop from the edge
weights (gsage_sample_hops_weighted), queue mode included -- and the validation / test folds on the same class; what
that engine does not cover is an error with its sentence.  --full-neighbour-eval / --save-embeddings compute the
weight-normalised mean (mean and mean-pool models); --unsupervised is refused unless --weighted-walks is given (its
walks would otherwise take uniform steps over a graph the encoder reads by weight).

--sampler-class sparse_distinct_neighbor_sampler: neighbours drawn WITHOUT replacement (include/gsage.h, "Distinct
neighbours"; sparse problems): a node with no more neighbours than the fan-out gets every one of them, balanced -- its
sampled mean is its exact mean whenever its degree divides the fan-out -- and a node with more gets that many distinct
ones.  Edge weights, if the problem has any, are ignored, as under the uniform sampler.  Always Philox; fan-outs of at
most 256.  Under --engine auto / eager the module path runs it (said on stderr, with the name of the engine --engine
fused would select); --engine fused (opt-in, mean aggregators, the identity prep over a bf16 / fp32 table, one process)
runs training on engine.FusedDistinctMeanTrainStep -- the mean engine behind one sampler launch that draws every hop
(gsage_sample_hops_distinct), queue mode included -- and the validation / test folds on the same class; what that
engine does not cover is an error with its sentence.  --unsupervised runs on the module path (the sampler only supplies
the frontier; --engine fused exits with the unsupervised engine's sentence); --importance-walks is refused (that run is
a weighted one).

--sampler-class sparse_temporal_neighbor_sampler [--temporal-strategy uniform|recent] [--temporal-inherit seed|edge]:
neighbours drawn among the edges that happened strictly BEFORE the seed's query time (a problem file with `adj_time` /
`train_adj_time`, int64, and optionally `node_time`, the seeds' query times; include/gsage.h, "Temporal neighbours").
Always Philox.  Under --engine auto / eager the module path runs it (said on stderr, with the name of the engine --engine
fused would select); --engine fused (opt-in, mean aggregators, the identity prep over a bf16 / fp32 table, one process,
a GPU) runs training on engine.FusedTemporalMeanTrainStep -- the mean engine behind one sampler launch that draws every
hop with the times beside the ids (gsage_sample_hops_temporal), queue mode included, the seeds' query times the
problem's `node_time` as on the module path -- and the validation / test folds on the same class; what that engine does
not cover is an error with its sentence.
Refused with a sentence: a problem without edge times, a dense problem, --unsupervised without --temporal-walks (the
walks are not temporal) and --importance-walks.  --eval-as-of T: --full-neighbour-eval, --save-embeddings and the exports built on the embeddings
run over the snapshot of the evaluation adjacency as of T (store.DeviceCSR.snapshot: the edges with time < T).

--temporal-walks (default off: nothing changes; with --unsupervised and the temporal sampler): the positives come from
walks that respect time (models.GSUnsupervised(temporal_walks=True), gsage_unsup_batch_temporal; include/gsage.h,
"Temporal walks"): every step is drawn uniformly among the edges before the seed's query time (--temporal-inherit seed)
or before the edge just walked (edge), and the query times -- the problem's `node_time` -- travel with [seeds |
positives | negatives] into the temporal sampler, in training and in the validation / test lines.  The module path runs
it under --engine auto / eager; --engine fused --rng philox runs engine.FusedUnsupTemporalMeanTrainStep -- the temporal
builder and gsage_sample_hops_temporal in front of the unsupervised mean engine -- or exits with that engine's sentence.
Errors: without --unsupervised, without the temporal sampler, with --weighted-walks, --walk-p / --walk-q other than 1 or
--importance-walks.
--link-eval-future (with --link-eval and --eval-as-of T): the ranked edges are those stored in the evaluation adjacency
that its snapshot as of T does not store -- the edges that first happen at or after T -- ranked on the embeddings as of
T, filtered as --link-eval filters; the JSON line gains "future": true and "as_of": T.

--weighted-walks (default off: nothing changes; with --unsupervised and the weighted sampler, asked for by name or
reached through --importance-walks): the positives' random walks draw every step in proportion to the edge weights
(models.GSUnsupervised(weighted_walks=True), gsage_unsup_batch_weighted), on the training graph and -- in the
validation / test lines -- on the evaluation graph, and a row without a drawable edge is never a negative.  The module
path runs it under --engine auto / eager; --engine fused runs engine.FusedUnsupWeightedMeanTrainStep -- the weighted
builder and gsage_sample_hops_weighted in front of the unsupervised mean engine -- or exits with that engine's
sentence.  --save-embeddings / --save-neighbours / --link-eval / --probe then compute the weight-normalised mean, as
after a supervised weighted run.  Without --unsupervised, or with a sampler that is not the weighted one, the flag is
an error.

--importance-walks R (with --importance-len L, --importance-top T, --importance-seed S; default off: nothing changes):
after the problem is loaded, the training and the evaluation adjacency are each replaced by gs.importance_adj of
THEMSELVES (include/gsage.h, "Importance neighbourhoods": R random walks of L steps from every node, its T most-visited
nodes as neighbours, the visit counts as edge weights; the training graph's walks never see evaluation edges), and the
run is a weighted one: --sampler-class sparse_uniform_neighbor_sampler is switched to the weighted sampler (said on
stderr), the dense sampler is refused, and everything the weighted sampler refuses or redirects stays as it is.  The
defaults of L and T (2, 16) reach the toy results of the tests; nobody has tuned them on a real graph.

--walk-p P / --walk-q Q (with --unsupervised; default 1, 1: nothing changes) and --importance-p P / --importance-q Q /
--importance-restart A (with --importance-walks; default 1, 1, 0: nothing changes): biased walks (include/gsage.h,
"Biased walks").  P and Q, each in [1/8, 8], are node2vec's return and in-out parameters: every step of a walk after its
first is drawn in second order -- back to the previous node with weight 1/P, to a node the previous node stores as a
neighbour with weight 1, elsewhere with weight 1/Q (gsage_unsup_batch_biased for the positives, under --weighted-walks
on top of the edge weights, on the module path and on the fused unsupervised engines alike;
gsage_importance_walks_biased for the neighbourhoods).  A in [0, 1) sends a neighbourhood's walk back to its source
before a step with that probability (personalised-PageRank visit counts).  Values outside the limits, --walk-p / --walk-q
without --unsupervised and --importance-p / -q / -restart without --importance-walks are errors.
"""
from __future__ import division, print_function

import argparse
import importlib
import json
import os
import sys
from time import time

import numpy as np
import torch
from torch.nn import functional as F

if __package__ in (None, ""):                       # executed as a script: ./train.py
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    gs = importlib.import_module(os.path.basename(os.path.dirname(os.path.abspath(__file__))))
else:
    gs = importlib.import_module(__package__)

GSSupervised, NodeProblem = gs.GSSupervised, gs.NodeProblem
set_seeds, to_numpy, batch_metric = gs.set_seeds, gs.to_numpy, gs.batch_metric
aggregator_lookup, prep_lookup, sampler_lookup = gs.aggregator_lookup, gs.prep_lookup, gs.sampler_lookup


def _round5(obj):
    """ujson.dumps(..., double_precision=5) of the reference: floats printed with 5 decimals."""
    if isinstance(obj, float):
        return round(obj, 5)
    if isinstance(obj, dict):
        return {k: _round5(v) for k, v in obj.items()}
    return obj


def dumps(obj):
    return json.dumps(_round5(obj), separators=(",", ":"))


def check_samplers(model):
    """The GPU sampler maps an id outside the adjacency to the dummy node and raises a device flag
    instead of synchronising per call; the reference (and host mode) raise IndexError on the spot.  Read
    the flags here -- once per evaluation, so no sync is added to a train step."""
    for s in (model.train_sampler, model.val_sampler):
        for csr in getattr(s, "_dev", {}).values():          # the device copies a sparse sampler has made
            csr.check()


def evaluate(model, problem, mode='val'):
    assert mode in ['test', 'val']
    preds, acts = [], []
    # every rank evaluates the WHOLE fold: draw the samples a single process would (rank offset off)
    shard = getattr(model.val_sampler, "shard", None)
    if shard is not None:
        model.val_sampler.shard = (0, 1)
    try:
        for (ids, targets, _) in problem.iterate(mode=mode, shuffle=False):
            preds.append(model(ids, problem.feats, train=False).detach())
            acts.append(targets.reshape(targets.shape[0], -1))
    finally:
        if shard is not None:
            model.val_sampler.shard = shard
    check_samplers(model)
    if preds and preds[0].is_cuda:
        # scored on the device (problem.DeviceMetrics): the fold's predictions never travel to the host
        return batch_metric(problem.task, torch.cat(acts), torch.cat(preds))
    return problem.metric_fn(np.vstack([to_numpy(a) for a in acts]), np.vstack([to_numpy(p) for p in preds]))


def full_neighbour_evaluate(model, problem, mode='val', closure=False):
    """evaluate() by layer-wise full-neighbourhood inference (infer.full_neighbour) of the fold's nodes; every rank
    computes the whole fold.  No random draw is consumed.  closure: over the fold's k-hop closure (--eval-closure)."""
    assert mode in ['test', 'val']
    nodes = problem.nodes[mode]
    _, acts = problem._batch(nodes, problem.targets[nodes])
    dev = problem.feats.device
    preds = gs.full_neighbour(model, problem.feats, nodes=torch.from_numpy(nodes).to(dev), closure=closure,
                              adj=as_of_adj(problem))
    return batch_metric(problem.task, acts.reshape(acts.shape[0], -1), preds)


def as_of_adj(problem):
    """--eval-as-of T: the snapshot of the evaluation adjacency that full-neighbourhood evaluation and the embedding
    pass run over (set_as_of), or None: the adjacency evaluation samples from."""
    return getattr(problem, "_as_of_adj", None)


def set_as_of(args, problem):
    """--eval-as-of T: build snapshot(T) of the evaluation adjacency once, on the device of the feature table."""
    if not isinstance(problem.adj, gs.store.TemporalAdj):
        raise SystemExit('gsage: --eval-as-of: this problem has no edge times (adj_time) to take a snapshot by')
    if not (args.full_neighbour_eval or args.save_embeddings or args.save_neighbours or args.link_eval or args.probe
            or args.cluster):
        raise SystemExit('gsage: --eval-as-of goes with --full-neighbour-eval, --save-embeddings or an export built on '
                         'the embeddings (the sampled evaluation takes its times from node_time)')
    if args.correct_smooth:
        raise SystemExit('gsage: --eval-as-of: --correct-smooth propagates over every stored edge and is not covered')
    dev = torch.device('cuda' if args.cuda else 'cpu')
    full = gs.DeviceCSR.from_scipy(problem.adj, dev)
    problem._as_of_adj = full.snapshot(args.eval_as_of)
    print('gsage: --eval-as-of %d: full-neighbourhood evaluation and the embedding pass run over %d of the %d '
          'evaluation edges' % (args.eval_as_of, problem._as_of_adj.nnz, full.nnz), file=sys.stderr)


def save_embeddings(model, problem, path, nodes=None):
    """F.normalize(H^L) of every row, node-id order, one .npy; nodes (--embed-nodes): of these rows only, in their order."""
    if nodes is not None:
        ids = torch.from_numpy(np.asarray(np.load(nodes), dtype=np.int64).reshape(-1)).to(problem.feats.device)
        np.save(path, gs.infer.query_embeddings(model, problem.feats, ids, adj=as_of_adj(problem)).cpu().numpy())
        return
    np.save(path, gs.embeddings(model, problem.feats, adj=as_of_adj(problem)).cpu().numpy())


def link_eval(model, problem, args, emb):
    """--link-eval: filtered MRR / hits@k of the held-out edges of the validation fold (and, with --show-test, of the
    test fold) over `emb`, one JSON line per fold.  Held out = stored in the evaluation adjacency with its source in
    the fold, not stored in the training adjacency; filtered by the evaluation adjacency (gs.link_rank)."""
    dev = emb.device
    adj, train_adj = model.val_sampler.csr(dev), model.train_sampler.csr(dev)
    ks = tuple(int(v) for v in args.link_eval_ks.split(','))
    if args.link_eval_future:                      # the edges that first happen at or after T, on the embeddings as of T
        train_adj = as_of_adj(problem)
    for i, fold in enumerate(['val', 'test'] if args.show_test else ['val']):
        src, dst = gs.held_out_edges(adj, train_adj, torch.from_numpy(np.asarray(problem.nodes[fold], dtype=np.int64)))
        n = int(src.shape[0])
        if n > args.link_eval_edges:              # a seeded subsample, in the edges' order
            pick = np.sort(np.random.RandomState(args.seed + i).choice(n, args.link_eval_edges, replace=False))
            pick = torch.from_numpy(pick).to(dev)
            src, dst = src[pick], dst[pick]
        ranks, _ = gs.link_rank(emb, src, dst, exclude='neighbours', adj=adj)
        res = {"fold": fold, "held_out_edges": n}
        if args.link_eval_future:
            res["future"], res["as_of"] = True, int(args.eval_as_of)
        res.update(gs.link_metrics(ranks, ks))
        print(dumps({"link_eval": res}))
        sys.stdout.flush()


def probe_eval(problem, args, emb):
    """--probe: micro / macro F1 of a linear classifier fitted on the train fold's rows of `emb` (gs.probe_eval), one
    JSON line for the validation fold and, with --show-test, one for the test fold."""
    try:
        res = gs.probe_eval(emb, problem, iters=args.probe_iters, lr=args.probe_lr, weight_decay=args.probe_l2)
    except (ValueError, IndexError) as e:
        raise SystemExit('gsage: --probe: %s' % e)
    for fold in (['val', 'test'] if args.show_test else ['val']):
        f1 = res[fold] or {"micro": None, "macro": None}
        print(dumps({"probe": {"fold": fold, "task": res["task"], "micro": f1["micro"], "macro": f1["macro"],
                               "loss_first": res["loss_first"], "loss_last": res["loss_last"]}}))
        sys.stdout.flush()


def cluster_eval(problem, args, emb):
    """--cluster K: k-means on the embeddings of every node of the three folds (gs.cluster_eval), one JSON line for the
    validation fold and, with --show-test, one for the test fold; NMI and purity where the problem has class labels.
    --save-clusters: the nodes, their labels and the centroids as an .npz."""
    try:
        res = gs.cluster_eval(emb, problem, k=args.cluster, iters=args.cluster_iters, init=args.cluster_init,
                              n_init=args.cluster_n_init, seed=args.cluster_seed, spherical=args.cluster_spherical)
    except (ValueError, IndexError) as e:
        raise SystemExit('gsage: --cluster: %s' % e)
    for fold in (['val', 'test'] if args.show_test else ['val']):
        line = {"fold": fold, "k": res["k"], "iters": res["iters"], "inertia": res["inertia"]}
        if res[fold] is not None:
            line["nmi"], line["purity"] = res[fold]["nmi"], res[fold]["purity"]
        print(dumps({"cluster": line}))
        sys.stdout.flush()
    if args.save_clusters:
        with open(args.save_clusters, 'wb') as f:
            np.savez(f, nodes=res["nodes"], labels=res["labels"].cpu().numpy(), centroids=res["centroids"].cpu().numpy())


def cs_settings(args):
    """(iters, alpha) of --cs-iters / --cs-alpha, or SystemExit with a sentence."""
    try:
        iters = tuple(int(v) for v in args.cs_iters.split(','))
        alpha = tuple(float(v) for v in args.cs_alpha.split(','))
        ok = len(iters) == 2 and len(alpha) == 2 and all(v >= 0 for v in iters) and all(0.0 <= v <= 1.0 for v in alpha)
    except ValueError:
        ok = False
    if not ok:
        raise SystemExit('gsage: --cs-iters must be two counts >= 0 (correct,smooth) and --cs-alpha two values in [0, 1]')
    return iters, alpha


def correct_smooth(model, problem, args):
    """--correct-smooth (and --label-prop) after training: one JSON line per fold (gs.correct_smooth_eval)."""
    iters, alpha = cs_settings(args)
    folds = ['val', 'test'] if args.show_test else ['val']
    try:
        res = gs.correct_smooth_eval(model, problem, iters=iters, alpha=alpha, autoscale=not args.cs_no_autoscale,
                                     label_prop=args.label_prop, folds=folds)
    except (ValueError, IndexError) as e:
        raise SystemExit('gsage: --correct-smooth: %s' % e)
    for fold in folds:
        f1 = res[fold] or {}
        print(dumps({"correct_smooth": {"fold": fold, "task": res["task"], "base": f1.get("base"),
                                        "corrected": f1.get("corrected"), "smoothed": f1.get("smoothed")}}))
        if args.label_prop:
            lp = f1.get("label_prop") or {"micro": None, "macro": None}
            print(dumps({"label_prop": {"fold": fold, "task": res["task"], "micro": lp["micro"], "macro": lp["macro"]}}))
        sys.stdout.flush()


def export(model, problem, args):
    """--save-embeddings, --save-neighbours, --link-eval and --probe after training: one embedding pass serves all."""
    emb = None
    if args.save_embeddings:
        if args.embed_nodes:
            save_embeddings(model, problem, args.save_embeddings, args.embed_nodes)
        else:
            emb = gs.embeddings(model, problem.feats, adj=as_of_adj(problem))
            np.save(args.save_embeddings, emb.cpu().numpy())
    if args.save_neighbours:
        if emb is None:
            emb = gs.embeddings(model, problem.feats, adj=as_of_adj(problem))
        nodes = None
        if args.neighbour_nodes:
            nodes = torch.from_numpy(np.asarray(np.load(args.neighbour_nodes), dtype=np.int64).reshape(-1))
        adj = model.val_sampler.csr(emb.device) if args.neighbours_exclude == 'neighbours' else None
        try:
            ids, scores = gs.nearest(emb, nodes, k=args.neighbours_k, exclude=args.neighbours_exclude, adj=adj)
        except ValueError as e:
            raise SystemExit('gsage: --save-neighbours: %s' % e)
        with open(args.save_neighbours, 'wb') as f:
            np.savez(f, ids=ids.cpu().numpy(), scores=scores.cpu().numpy())
    if args.link_eval or args.probe or args.cluster:
        emb = emb if emb is not None else gs.embeddings(model, problem.feats, adj=as_of_adj(problem))
    if args.link_eval:
        link_eval(model, problem, args, emb)
    if args.probe:
        probe_eval(problem, args, emb)
    if args.cluster:
        cluster_eval(problem, args, emb)


class FusedEvaluator(object):
    """evaluate() on a fused engine's FORWARD launches (engine.FusedTrainStep(eval_only=True).evaluate_fold): the
    fold cut into the reference's chunks (problem.py:141-153 with shuffle=False, batch_size 512 as train.py:32 calls
    it), the validation sampler's frontier drawn from the generator -- and in the order -- the reference's evaluation
    would draw from, no autograd, no per-op launches, the metric on the device.  One engine per fold (their chunk
    sizes differ), built on first use; a model / store no engine covers keeps the module path (said once) --
    strict=True (an engine the run asked for by name: the weighted one): what the engine refuses is an error."""

    def __init__(self, cls, model, problem, wide_head=False, strict=False):
        self.cls, self.model, self.problem, self.wide_head = cls, model, problem, bool(wide_head)
        self.engines, self.off, self.strict = {}, False, bool(strict)

    def _fold(self, mode, batch_size=512):
        nodes = self.problem.nodes[mode]
        chunks = np.array_split(np.arange(nodes.shape[0]), nodes.shape[0] // batch_size + 1)
        B = max(int(c.shape[0]) for c in chunks)
        mids = np.stack([np.concatenate([nodes[c], np.repeat(nodes[c[:1]], B - c.shape[0])]) for c in chunks])
        return torch.from_numpy(mids).cuda(), [int(c.shape[0]) for c in chunks]

    def prepare(self, mode='val'):
        """build the fold's engine now (part of a run's set-up, not of its first epoch)"""
        if not self.off and self.problem.nodes[mode].shape[0] >= 2:
            ids, live = self._fold(mode)
            if min(live) >= 2:
                self._engine(mode, ids)
        return self

    def _engine(self, mode, ids):
        model, problem = self.model, self.problem
        eng = self.engines.get(mode)
        if eng is None and not self.off:
            try:
                tg = torch.zeros(ids.shape[1], 1, dtype=torch.int64, device=ids.device) \
                    if problem.task == 'classification' else \
                    torch.zeros((ids.shape[1],) + tuple(np.asarray(problem.targets[:1]).shape[1:]), dtype=torch.float32,
                                device=ids.device)
                kw = {"wide_head": True} if self.wide_head else {}
                eng = self.engines[mode] = self.cls(model, problem.feats, problem.loss_fn, ids[0], tg, eval_only=True,
                                                    **kw)
            except Exception as e:
                if self.strict:
                    raise SystemExit('gsage: --engine fused: evaluation on %s: %s' % (self.cls.__name__, e))
                self.off = True
                print('gsage: evaluation stays on the module path (%s: %s)' % (type(e).__name__, e), file=sys.stderr)
        return eng

    def __call__(self, mode='val'):
        assert mode in ['test', 'val']
        model, problem = self.model, self.problem
        if self.off or problem.nodes[mode].shape[0] < 2:
            return evaluate(model, problem, mode=mode)
        ids, live = self._fold(mode)
        if min(live) < 2:
            return evaluate(model, problem, mode=mode)
        eng = self._engine(mode, ids)
        if eng is None:
            return evaluate(model, problem, mode=mode)
        try:
            preds = eng.evaluate_fold(ids, live)
        except Exception as e:            # (e.g. a validation fan-out the forward-only engine's kernels refuse)
            if self.strict:
                raise SystemExit('gsage: --engine fused: evaluation on %s: %s' % (self.cls.__name__, e))
            self.off = True
            self.engines.pop(mode, None)
            print('gsage: evaluation falls back to the module path (%s: %s)' % (type(e).__name__, e), file=sys.stderr)
            return evaluate(model, problem, mode=mode)
        nodes = problem.nodes[mode]
        _, acts = problem._batch(nodes, problem.targets[nodes])
        check_samplers(model)
        eng.csr.check()
        return batch_metric(problem.task, acts.reshape(acts.shape[0], -1), preds)


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--problem-path', type=str, required=True)
    parser.add_argument('--no-cuda', action="store_true")
    # optimization
    parser.add_argument('--batch-size', type=int, default=512)
    parser.add_argument('--epochs', type=int, default=10)
    parser.add_argument('--lr-init', type=float, default=0.01)
    parser.add_argument('--lr-schedule', type=str, default='constant')
    parser.add_argument('--weight-decay', type=float, default=0.0)
    # architecture
    parser.add_argument('--sampler-class', type=str, default='uniform_neighbor_sampler')
    parser.add_argument('--aggregator-class', type=str, default='mean')
    parser.add_argument('--prep-class', type=str, default='identity')
    parser.add_argument('--n-train-samples', type=str, default='25,10')
    parser.add_argument('--n-val-samples', type=str, default='25,10')
    parser.add_argument('--output-dims', type=str, default='128,128')
    # logging
    parser.add_argument('--log-interval', default=10, type=int)
    parser.add_argument('--seed', default=123, type=int)
    parser.add_argument('--show-test', action="store_true")
    # build-specific (not in the reference)
    parser.add_argument('--rng', type=str, default='compat', choices=['compat', 'philox'])
    parser.add_argument('--precision', type=str, default='bf16', choices=['bf16', 'fp32'])
    parser.add_argument('--engine', type=str, default='auto', choices=['auto', 'eager', 'fused'],
                        help='auto: a fused engine where one covers the run, else the module path (said on stderr); '
                             'eager: the module path; fused: an engine or an error.  --unsupervised runs on the module '
                             'path unless --engine fused asks for FusedUnsupMeanTrainStep (needs --rng philox; with '
                             '--weighted-walks: FusedUnsupWeightedMeanTrainStep, with --temporal-walks: '
                             'FusedUnsupTemporalMeanTrainStep).  The weighted, distinct and temporal '
                             'samplers run on the module path unless --engine fused asks for their engine '
                             '(FusedWeightedMeanTrainStep / FusedDistinctMeanTrainStep / FusedTemporalMeanTrainStep)')
    parser.add_argument('--feature-dtype', type=str, default='native', choices=['native', 'fp8'])
    parser.add_argument('--wide-head', action="store_true",
                        help='fuse the multilabel head (2..128 labels) and cross-entropy over 65..128 classes '
                             '(gsage_head_wide): such a problem then runs on a fused engine whatever its chunk sizes')
    parser.add_argument('--full-neighbour-eval', action="store_true")
    parser.add_argument('--save-embeddings', type=str, default=None)
    parser.add_argument('--eval-closure', action="store_true")
    parser.add_argument('--embed-nodes', type=str, default=None)
    parser.add_argument('--save-neighbours', type=str, default=None)
    parser.add_argument('--neighbours-k', type=int, default=10)
    parser.add_argument('--neighbour-nodes', type=str, default=None)
    parser.add_argument('--neighbours-exclude', type=str, default='self', choices=['none', 'self', 'neighbours'])
    parser.add_argument('--link-eval', action="store_true")
    parser.add_argument('--link-eval-edges', type=int, default=100000)
    parser.add_argument('--link-eval-ks', type=str, default='1,10,50')
    parser.add_argument('--probe', action="store_true")
    parser.add_argument('--probe-iters', type=int, default=100)
    parser.add_argument('--probe-lr', type=float, default=0.1)
    parser.add_argument('--probe-l2', type=float, default=0.0)
    parser.add_argument('--cluster', type=int, default=0)
    parser.add_argument('--cluster-iters', type=int, default=50)
    parser.add_argument('--cluster-init', type=str, default='++', choices=['++', 'random'])
    parser.add_argument('--cluster-n-init', type=int, default=1)
    parser.add_argument('--cluster-seed', type=int, default=0)
    parser.add_argument('--cluster-spherical', action="store_true")
    parser.add_argument('--save-clusters', type=str, default=None)
    parser.add_argument('--correct-smooth', action="store_true")
    parser.add_argument('--cs-iters', type=str, default='50,50')
    parser.add_argument('--cs-alpha', type=str, default='0.8,0.8')
    parser.add_argument('--cs-no-autoscale', action="store_true")
    parser.add_argument('--label-prop', action="store_true")
    parser.add_argument('--unsupervised', action="store_true")
    parser.add_argument('--walk-len', type=int, default=5)
    parser.add_argument('--n-negatives', type=int, default=20)
    parser.add_argument('--neg-weight', type=float, default=1.0)
    parser.add_argument('--weighted-walks', action="store_true",
                        help='with --unsupervised and the weighted sampler: the walks draw every step in proportion to '
                             'the edge weights (gsage_unsup_batch_weighted)')
    parser.add_argument('--importance-walks', type=int, default=0,
                        help='rebuild both adjacencies from this many random walks per node (gs.importance_adj) and '
                             'train with the weighted sampler; 0 (default): off')
    parser.add_argument('--importance-len', type=int, default=2)
    parser.add_argument('--importance-top', type=int, default=16)
    parser.add_argument('--importance-seed', type=int, default=0)
    parser.add_argument('--walk-p', type=float, default=1.0,
                        help='with --unsupervised: node2vec return parameter of the walks, in [1/8, 8]')
    parser.add_argument('--walk-q', type=float, default=1.0,
                        help='with --unsupervised: node2vec in-out parameter of the walks, in [1/8, 8]')
    parser.add_argument('--importance-p', type=float, default=1.0)
    parser.add_argument('--importance-q', type=float, default=1.0)
    parser.add_argument('--importance-restart', type=float, default=0.0,
                        help='with --importance-walks: probability in [0, 1) that a step puts the walk back on its node')
    parser.add_argument('--temporal-strategy', type=str, default=None, choices=['uniform', 'recent'],
                        help='with --sampler-class sparse_temporal_neighbor_sampler: draw uniformly among the edges '
                             'before the query time (default), or take the most recent ones')
    parser.add_argument('--temporal-inherit', type=str, default=None, choices=['seed', 'edge'],
                        help='with the temporal sampler: the next hop looks before the seed\'s time (default) or before '
                             'the time of the edge just walked')
    parser.add_argument('--temporal-walks', action="store_true",
                        help='with --unsupervised and the temporal sampler: the positives come from walks that respect '
                             'time (gsage_unsup_batch_temporal) and the query times travel with the batch')
    parser.add_argument('--link-eval-future', action="store_true",
                        help='with --link-eval and --eval-as-of T: rank the edges that first happen at or after T on the '
                             'embeddings as of T')
    parser.add_argument('--eval-as-of', type=int, default=None,
                        help='--full-neighbour-eval, --save-embeddings and the exports built on them run over the '
                             'snapshot of the evaluation adjacency as of this time (edges with time < T)')

    args = parser.parse_args(argv)
    args.cuda = not args.no_cuda
    assert args.prep_class in prep_lookup.keys(), 'parse_args: prep_class not in %s' % str(prep_lookup.keys())
    assert args.aggregator_class in aggregator_lookup.keys(), \
        'parse_args: aggregator_class not in %s' % str(aggregator_lookup.keys())
    assert args.batch_size > 1, 'parse_args: batch_size must be > 1'
    assert 1 <= args.walk_len <= 16 and 1 <= args.n_negatives <= 64, \
        'parse_args: --walk-len must be in 1..16 and --n-negatives in 1..64'
    return args


def importance_graphs(args, problem):
    """--importance-walks: problem.train_adj and problem.adj become the importance-weighted adjacencies of themselves
    and the run a weighted one (args.sampler_class); one stderr line says what was built and which sampler draws."""
    if args.sampler_class == 'uniform_neighbor_sampler' or not gs.problem._is_sparse(problem.adj):
        raise SystemExit('gsage: --importance-walks: random walks need the stored edges of a sparse problem, not the dense '
                         'sampler\'s pre-sampled table (use --sampler-class sparse_uniform_neighbor_sampler)')
    if args.sampler_class == 'sparse_distinct_neighbor_sampler':
        raise SystemExit('gsage: --importance-walks: the run is a weighted one (the visit counts are the edge weights), '
                         'and the distinct sampler (sparse_distinct_neighbor_sampler) ignores edge weights')
    if args.sampler_class == 'sparse_uniform_neighbor_sampler':
        print('gsage: --importance-walks: --sampler-class sparse_uniform_neighbor_sampler becomes '
              'sparse_weighted_neighbor_sampler (the visit counts are the edge weights)', file=sys.stderr)
        args.sampler_class = 'sparse_weighted_neighbor_sampler'
    device = torch.device('cuda' if args.cuda else 'cpu')
    kw = dict(n_walks=args.importance_walks, walk_len=args.importance_len, top=args.importance_top,
              seed=args.importance_seed, device=device, p=args.importance_p, q=args.importance_q,
              restart=args.importance_restart)
    t0 = time()
    try:
        same = problem.train_adj is problem.adj
        problem.train_adj = gs.importance_adj(problem.train_adj, **kw)
        problem.adj = problem.train_adj if same else gs.importance_adj(problem.adj, **kw)
    except (ValueError, IndexError) as e:
        raise SystemExit('gsage: --importance-walks: %s' % e)
    print('gsage: --importance-walks: both adjacencies rebuilt from %d walks of %d steps per node, top %d (%d training '
          'edges, %d evaluation edges, %.2f s on %s)' % (args.importance_walks, args.importance_len, args.importance_top,
                                                         problem.train_adj.adj.nnz, problem.adj.adj.nnz, time() - t0,
                                                         device.type), file=sys.stderr)


TEMPORAL = 'sparse_temporal_neighbor_sampler'


def temporal_checks(args, problem):
    """--sampler-class sparse_temporal_neighbor_sampler: one sentence for each thing it does not cover, and the class-wide
    strategy / inheritance rule of the run."""
    if args.sampler_class != TEMPORAL:
        if args.temporal_strategy is not None or args.temporal_inherit is not None:
            raise SystemExit('gsage: --temporal-strategy / --temporal-inherit: they belong to the temporal sampler '
                             '(--sampler-class %s), not %s' % (TEMPORAL, args.sampler_class))
        return
    who = 'gsage: --sampler-class %s' % TEMPORAL
    if not gs.problem._is_sparse(problem.adj):
        raise SystemExit('%s: edge times need the stored edges of a sparse problem, not the dense sampler\'s pre-sampled '
                         'table' % who)
    if not (isinstance(problem.adj, gs.store.TemporalAdj) and isinstance(problem.train_adj, gs.store.TemporalAdj)):
        raise SystemExit('%s: this problem has no edge times (adj_time / train_adj_time)' % who)
    if args.unsupervised and not args.temporal_walks:
        raise SystemExit('%s: --unsupervised is not supported (the random walks are not temporal: their positives would '
                         'come from the future)' % who)
    if args.importance_walks:
        raise SystemExit('%s: --importance-walks is not supported (the walks are not temporal, and the rebuilt adjacency '
                         'carries no edge times)' % who)
    if args.engine == 'fused' and not args.cuda:       # (with a GPU: choose_engine builds FusedTemporalMeanTrainStep)
        raise SystemExit('%s: --engine fused: no fused engine covers the temporal sampler without a GPU (--no-cuda)' % who)
    cls = gs.nn_modules.SparseTemporalNeighborSampler
    cls.strategy_default = args.temporal_strategy or 'uniform'
    cls.inherit_default = args.temporal_inherit or 'seed'


def build_model(args, problem):
    n_train = [int(v) for v in args.n_train_samples.split(',')]
    n_val = [int(v) for v in args.n_val_samples.split(',')]
    dims = [int(v) for v in args.output_dims.split(',')]
    depth = len(dims)
    specs = []
    for li in range(depth):
        last = li == depth - 1
        specs.append({
            "n_train_samples": n_train[li],
            "n_val_samples": n_val[li],
            "output_dim": dims[li],
            "activation": (lambda x: x) if last else F.relu,     # train.py:105-118
        })
    common = dict(
        sampler_class=gs.find_sampler(args.sampler_class), adj=problem.adj, train_adj=problem.train_adj,
        prep_class=prep_lookup[args.prep_class], aggregator_class=aggregator_lookup[args.aggregator_class],
        input_dim=problem.feats_dim, n_nodes=problem.n_nodes,
        layer_specs=specs, lr_init=args.lr_init, lr_schedule=args.lr_schedule,
        weight_decay=args.weight_decay)
    if args.unsupervised:
        return gs.GSUnsupervised(walk_len=args.walk_len, n_negatives=args.n_negatives, neg_weight=args.neg_weight,
                                 weighted_walks=args.weighted_walks, walk_p=args.walk_p, walk_q=args.walk_q,
                                 **dict(common, **({"temporal_walks": True} if args.temporal_walks else {})))
    return GSSupervised(n_classes=problem.n_classes, **common)


def main(argv=None, problem=None):
    """problem: a NodeProblem already in memory (NodeProblem.from_arrays) instead of --problem-path's file."""
    args = parse_args(argv)
    if args.eval_closure and not args.full_neighbour_eval:
        raise SystemExit('gsage: --eval-closure goes with --full-neighbour-eval')
    if args.embed_nodes and not args.save_embeddings:
        raise SystemExit('gsage: --embed-nodes goes with --save-embeddings')
    if args.neighbour_nodes and not args.save_neighbours:
        raise SystemExit('gsage: --neighbour-nodes goes with --save-neighbours')
    if args.save_neighbours and not 1 <= args.neighbours_k <= gs.ops.TOPK_K_MAX:
        raise SystemExit('gsage: --neighbours-k must be in 1..%d' % gs.ops.TOPK_K_MAX)
    if args.link_eval:
        try:
            ok = args.link_eval_edges >= 1 and all(int(v) >= 1 for v in args.link_eval_ks.split(','))
        except ValueError:
            ok = False
        if not ok:
            raise SystemExit('gsage: --link-eval-edges must be >= 1 and --link-eval-ks a comma-separated list of k >= 1')
        if int(os.environ.get("WORLD_SIZE", "1")) > 1 or os.environ.get("GSAGE_FORCE_DDP", "0") == "1":
            raise SystemExit('gsage: --link-eval: data-parallel launches are not supported (run a single process)')
    if args.probe and (args.probe_iters < 1 or not args.probe_lr > 0 or args.probe_l2 < 0):
        raise SystemExit('gsage: --probe-iters must be >= 1, --probe-lr > 0 and --probe-l2 >= 0')
    if args.cluster < 0 or (args.cluster and (args.cluster_iters < 1 or args.cluster_n_init < 1)):
        raise SystemExit('gsage: --cluster must be a number of clusters >= 1, --cluster-iters >= 1 and --cluster-n-init >= 1')
    if args.save_clusters and not args.cluster:
        raise SystemExit('gsage: --save-clusters goes with --cluster K')
    if args.label_prop and not args.correct_smooth:
        raise SystemExit('gsage: --label-prop goes with --correct-smooth')
    if args.correct_smooth:
        cs_settings(args)
        if args.unsupervised:
            raise SystemExit('gsage: --correct-smooth: --unsupervised trains no classifier; there are no logits to correct')
        if int(os.environ.get("WORLD_SIZE", "1")) > 1 or os.environ.get("GSAGE_FORCE_DDP", "0") == "1":
            raise SystemExit('gsage: --correct-smooth: data-parallel launches are not supported (run a single process)')
    set_seeds(args.seed)
    gs.ops.set_compute_dtype(args.precision)
    gs.nn_modules.SparseUniformNeighborSampler.rng_default = args.rng
    # compat mode on the GPU: the sampler consumes numpy's legacy stream on the device (same words, same
    # order; helpers.LegacyStreamOnDevice) instead of drawing on the host and copying `sel` over
    gs.helpers.legacy_stream.enabled = bool(args.cuda and args.rng == 'compat' and
                                            os.environ.get("GSAGE_HOST_SEL", "0") != "1")

    if args.unsupervised and args.wide_head:
        raise SystemExit('gsage: --unsupervised: --wide-head fuses a supervised head; there is none')
    if args.weighted_walks and not args.unsupervised:
        raise SystemExit('gsage: --weighted-walks: the walks belong to --unsupervised training (add --unsupervised)')
    if args.temporal_walks:
        if not args.unsupervised:
            raise SystemExit('gsage: --temporal-walks: the walks belong to --unsupervised training (add --unsupervised)')
        if args.sampler_class != TEMPORAL:
            raise SystemExit('gsage: --temporal-walks: needs the temporal sampler (--sampler-class %s), not %s'
                             % (TEMPORAL, args.sampler_class))
        if args.weighted_walks or (args.walk_p, args.walk_q) != (1.0, 1.0) or args.importance_walks:
            raise SystemExit('gsage: --temporal-walks: does not combine with --weighted-walks, --walk-p / --walk-q other '
                             'than 1 or --importance-walks (weights and times together, and biased temporal walks, are '
                             'not covered)')
    if args.link_eval_future and not (args.link_eval and args.eval_as_of is not None):
        raise SystemExit('gsage: --link-eval-future: goes with --link-eval and --eval-as-of T (the edges at or after T are '
                         'ranked on the embeddings as of T)')
    if (args.walk_p, args.walk_q) != (1.0, 1.0) and not args.unsupervised:
        raise SystemExit('gsage: --walk-p / --walk-q: the walks belong to --unsupervised training (add --unsupervised)')
    if (args.importance_p, args.importance_q, args.importance_restart) != (1.0, 1.0, 0.0) and not args.importance_walks:
        raise SystemExit('gsage: --importance-p / --importance-q / --importance-restart: there are no walks to bias '
                         '(add --importance-walks R)')
    for flag, val in (('--walk-p', args.walk_p), ('--walk-q', args.walk_q), ('--importance-p', args.importance_p),
                      ('--importance-q', args.importance_q)):
        if not gs.ops.WALK_PQ_MIN <= val <= gs.ops.WALK_PQ_MAX:
            raise SystemExit('gsage: %s must be in [1/8, 8] (got %g)' % (flag, val))
    if not 0.0 <= args.importance_restart < 1.0:
        raise SystemExit('gsage: --importance-restart must be in [0, 1) (got %g)' % args.importance_restart)
    if args.unsupervised and (int(os.environ.get("WORLD_SIZE", "1")) > 1 or os.environ.get("GSAGE_FORCE_DDP", "0") == "1"):
        raise SystemExit('gsage: --unsupervised: data-parallel training is not supported (run a single process)')
    ddp = gs.dist.init_from_env(args.cuda)            # no-op outside torch.distributed.run
    if problem is None:
        problem = NodeProblem(problem_path=args.problem_path, cuda=args.cuda)
    if args.probe and problem.task not in gs.ops.PROBE_TASKS:
        raise SystemExit('gsage: --probe: a linear probe is a classifier; this problem\'s task is %s' % problem.task)
    if args.link_eval and not gs.problem._is_sparse(problem.adj):
        raise SystemExit('gsage: --link-eval: a dense problem file holds neighbour samples, not edges to hold out')
    temporal_checks(args, problem)
    if args.importance_walks:
        importance_graphs(args, problem)
    if args.eval_as_of is not None:
        set_as_of(args, problem)
    if args.correct_smooth:
        if problem.task not in ('classification', 'multilabel_classification'):
            raise SystemExit('gsage: --correct-smooth: labels are propagated as class scores; this problem\'s task is %s'
                             % problem.task)
        if not gs.problem._is_sparse(problem.adj):
            raise SystemExit('gsage: --correct-smooth: a dense problem file holds neighbour samples, not the edges to '
                             'propagate over')
        if isinstance(problem.adj, gs.store.WeightedAdj):
            raise SystemExit('gsage: --correct-smooth: a weighted adjacency is not supported (edge weights are out of '
                             'scope; importance neighbourhoods included)')
    weighted = args.sampler_class == 'sparse_weighted_neighbor_sampler'
    if weighted:
        if not (isinstance(problem.adj, gs.store.WeightedAdj) and isinstance(problem.train_adj, gs.store.WeightedAdj)):
            raise SystemExit('gsage: --sampler-class sparse_weighted_neighbor_sampler: this problem has no edge weights '
                             '(adj_weight / train_adj_weight)')
        if args.unsupervised and not args.weighted_walks:
            raise SystemExit('gsage: --unsupervised: the weighted sampler is not supported (random walks are unweighted; '
                             '--weighted-walks draws their steps from the edge weights)')
    elif args.weighted_walks:
        raise SystemExit('gsage: --weighted-walks: needs the weighted sampler (--sampler-class '
                         'sparse_weighted_neighbor_sampler, or --importance-walks), not %s' % args.sampler_class)
    if args.sampler_class == 'sparse_distinct_neighbor_sampler' and not gs.problem._is_sparse(problem.adj):
        raise SystemExit('gsage: --sampler-class sparse_distinct_neighbor_sampler: distinct draws need the stored edges '
                         'of a sparse problem, not the dense sampler\'s pre-sampled table')
    if args.feature_dtype == 'fp8':
        if problem.feats is None:
            raise SystemExit('gsage: --feature-dtype fp8: this problem has no feature table')
        before, after, err = problem.quantize_features()
        print('gsage: feature table quantised to FP8 (e4m3, power-of-two column scales): %.1f MB -> %.1f MB, '
              'largest absolute error %.4g' % (before / 1e6, after / 1e6, err), file=sys.stderr)
    model = build_model(args, problem)
    if args.cuda:
        model = model.cuda()
        gs.ops.warmup(torch.device("cuda"))
    if ddp is not None:
        gs.dist.attach(model, ddp, seed=args.seed)
    print(model, file=sys.stderr)
    if args.unsupervised:
        if args.full_neighbour_eval:
            raise SystemExit('gsage: --unsupervised: --full-neighbour-eval scores logits; there are none')
        if args.save_embeddings or args.save_neighbours or args.link_eval or args.probe or args.cluster:
            try:
                gs.infer.check_supported(model, model.val_sampler.csr('cpu') if weighted else None)
            except ValueError as e:
                raise SystemExit('gsage: --save-embeddings / --save-neighbours / --link-eval / --probe%s: %s'
                                 % (' / --cluster' if args.cluster else '', e))
        set_seeds(args.seed ** 2)
        return train_unsupervised(args, problem, model)
    if args.full_neighbour_eval or args.save_embeddings or args.save_neighbours or args.link_eval or args.probe or args.cluster or \
            args.correct_smooth:
        try:
            gs.infer.check_supported(model, model.val_sampler.csr('cpu') if weighted else None)
        except ValueError as e:
            flags = '--full-neighbour-eval / --save-embeddings / --save-neighbours / --link-eval / --probe'
            raise SystemExit('gsage: %s%s%s: %s' % (flags, ' / --correct-smooth' if args.correct_smooth else '',
                                                      ' / --cluster' if args.cluster else '', e))
    evaluate_fn = (lambda mode: full_neighbour_evaluate(model, problem, mode=mode, closure=args.eval_closure)) \
        if args.full_neighbour_eval else \
        (lambda mode: evaluate(model, problem, mode=mode))

    set_seeds(args.seed ** 2)                          # train.py:133
    start_time = time()
    val_metric = train_metric = None
    epoch = 0
    if args.engine in ('auto', 'fused') and args.cuda:
        cls = choose_engine(args, problem, model, ddp)
        if cls is not None:
            print('gsage: train_step runs on %s' % cls.__name__, file=sys.stderr)
            return train_fused(args, problem, model, ddp, start_time, cls)
    for epoch in range(args.epochs):
        model.train()
        for ids, targets, epoch_progress in problem.iterate(mode='train', shuffle=True,
                                                           batch_size=args.batch_size):
            if ddp is not None:
                ids, targets = ddp.shard(ids, targets)
            model.set_progress((epoch + epoch_progress) / args.epochs)
            preds = model.train_step(ids=ids, feats=problem.feats, targets=targets,
                                     loss_fn=problem.loss_fn)
            train_metric = batch_metric(problem.task, targets, preds)      # on the device when the batch is
            if ddp is None or ddp.rank == 0:
                print(dumps({"epoch": epoch, "epoch_progress": epoch_progress,
                             "train_metric": train_metric, "val_metric": val_metric,
                             "time": time() - start_time}))
                sys.stdout.flush()
        model.eval()
        val_metric = evaluate_fn('val')

    gs.helpers.legacy_stream.release()                 # hand numpy's stream back to the host
    print('-- done --', file=sys.stderr)
    if ddp is None or ddp.rank == 0:
        print(dumps({"epoch": epoch, "train_metric": train_metric, "val_metric": val_metric,
                     "time": time() - start_time}))
        sys.stdout.flush()
        if args.show_test:
            print(dumps({"test_f1": evaluate_fn('test')}))
        if args.save_embeddings or args.save_neighbours or args.link_eval or args.probe or args.cluster:
            export(model, problem, args)
        if args.correct_smooth:
            correct_smooth(model, problem, args)
    if ddp is not None:
        ddp.close()


def evaluate_unsupervised(model, problem, mode='val'):
    """{"loss", "mrr"} of a fold under GSUnsupervised.evaluate, seed-weighted over the fold's batches."""
    tot = {"loss": 0.0, "mrr": 0.0}
    count = 0
    for (ids, _, _) in problem.iterate(mode=mode, shuffle=False):
        res = model.evaluate(ids, problem.feats)
        n = int(ids.shape[0])
        count += n
        for k in tot:
            tot[k] += res[k] * n
    check_samplers(model)
    return {k: v / max(count, 1) for k, v in tot.items()}


def train_unsupervised(args, problem, model):
    """The --unsupervised run, one JSON line per batch: GSUnsupervised.train_step on the module path, or -- with
    --engine fused -- the same step on engine.FusedUnsupMeanTrainStep (--weighted-walks: FusedUnsupWeightedMeanTrainStep;
    the batches are the reference's chunks either way; the engine pads the short ones and gives the padding no loss)."""
    cls = choose_engine(args, problem, model, None)    # (None: says on stderr that the module path runs)
    eng = None
    if cls is not None:
        nodes = problem.nodes['train']
        n_batches = nodes.shape[0] // args.batch_size + 1
        B = -(-nodes.shape[0] // n_batches)            # the largest of the reference's array_split chunks
        example = torch.from_numpy(np.ascontiguousarray(nodes[:B])).long().to(torch.device('cuda'))
        eng = cls(model, problem.feats, example)
        print('gsage: train_step runs on %s' % cls.__name__, file=sys.stderr)
    start_time = time()
    val = {"loss": None, "mrr": None}
    loss = None
    epoch = 0
    for epoch in range(args.epochs):
        model.train()
        for ids, _, epoch_progress in problem.iterate(mode='train', shuffle=True, batch_size=args.batch_size):
            (eng if eng is not None else model).set_progress((epoch + epoch_progress) / args.epochs)
            loss = float(eng(ids) if eng is not None else model.train_step(ids=ids, feats=problem.feats))
            print(dumps({"epoch": epoch, "epoch_progress": epoch_progress, "loss": loss, "val_loss": val["loss"],
                         "val_mrr": val["mrr"], "time": time() - start_time}))
            sys.stdout.flush()
        model.eval()
        val = evaluate_unsupervised(model, problem, 'val')
        print(dumps({"epoch": epoch, "val_loss": val["loss"], "mrr": val["mrr"], "time": time() - start_time}))
        sys.stdout.flush()
    gs.helpers.legacy_stream.release()                 # hand numpy's stream back to the host
    print('-- done --', file=sys.stderr)
    print(dumps({"epoch": epoch, "loss": loss, "val_loss": val["loss"], "mrr": val["mrr"], "time": time() - start_time}))
    if args.show_test:
        print(dumps({"test": evaluate_unsupervised(model, problem, 'test')}))
    sys.stdout.flush()
    if eng is not None:
        eng.close()
    if args.save_embeddings or args.save_neighbours or args.link_eval or args.probe or args.cluster:
        export(model, problem, args)


def choose_engine(args, problem, model, ddp):
    """The fused engine this run gets, or None for the module path.  Everything that could stop an engine AFTER it
    has re-pointed the model's Parameters into its buckets is decided here: the model / feature store / process
    group (engine.why_not), the head (engine.head_why_not: only a fused head can ignore the padding of the
    reference's unequal chunks) and the batch geometry.  --engine auto: one stderr line says why the module path
    runs; --engine fused: the same sentence is an error."""
    def give_up(why):
        if args.unsupervised and args.engine != 'fused':
            print('gsage: unsupervised model: module path', file=sys.stderr)
            return None
        if args.engine == 'fused':
            raise SystemExit('gsage: --engine fused: %s (use --engine auto / eager)' % why)
        print('gsage: %s; using the module path' % why, file=sys.stderr)
        return None
    if args.unsupervised:                           # the engine is opt-in: --engine fused, or the module path
        if args.engine != 'fused':
            return give_up('unsupervised model')
        cls = gs.engine.FusedUnsupWeightedMeanTrainStep if args.weighted_walks else \
            gs.engine.FusedUnsupTemporalMeanTrainStep if args.temporal_walks else gs.engine.FusedUnsupMeanTrainStep
        why = cls.why_not(model, problem.feats, ddp)
        if why is not None:
            return give_up('%s: %s' % (cls.__name__, why) if args.weighted_walks or args.temporal_walks else why)
        nodes = problem.nodes['train']
        if nodes.shape[0] // (nodes.shape[0] // args.batch_size + 1) < 2:
            return give_up('chunks of fewer than two training nodes')
        return cls
    own = [(what, scls, cls) for what, scls, cls in
           (('weighted', gs.nn_modules.SparseWeightedNeighborSampler, gs.engine.FusedWeightedMeanTrainStep),
            ('distinct', gs.nn_modules.SparseDistinctNeighborSampler, gs.engine.FusedDistinctMeanTrainStep),
            ('temporal', gs.nn_modules.SparseTemporalNeighborSampler, gs.engine.FusedTemporalMeanTrainStep))
           if isinstance(model.train_sampler, scls)]
    if own:
        what, scls, cls = own[0]                       # opt-in: --engine fused, or the module path
        if args.engine != 'fused':
            return give_up('no fused engine covers the %s sampler (%s) (--engine fused selects %s)'
                           % (what, scls.__name__, cls.__name__))
        why = cls.why_not(model, problem.feats, ddp)
        if why is not None:
            return give_up('%s: %s' % (cls.__name__, why))
    else:
        cls = gs.engine.fused_engine_for(model, problem.feats, explain=True, ddp=ddp)
    if cls is None:
        return give_up('no fused engine covers this model')
    if ddp is not None and args.rng != 'philox':
        return give_up('data-parallel runs of the fused engines need --rng philox')
    nodes = problem.nodes['train']
    world = ddp.world if ddp is not None else 1
    if world > 1:
        B, padded = args.batch_size // world, False
        if B < 2 or nodes.shape[0] < B * world:
            return give_up('fewer training nodes (or a smaller --batch-size) than two seeds per rank')
    else:
        n_batches = nodes.shape[0] // args.batch_size + 1
        B = -(-nodes.shape[0] // n_batches)
        padded = nodes.shape[0] % n_batches != 0
        if nodes.shape[0] // n_batches < 2:           # the smallest of the reference's array_split chunks
            return give_up('chunks of fewer than two training nodes')
    example = torch.zeros(1, dtype=torch.int64 if problem.task == 'classification' else torch.float32)
    if args.wide_head:
        why = cls.head_why_not(model, problem.loss_fn, example, B, padded, world, wide=True)
    else:
        why = cls.head_why_not(model, problem.loss_fn, example, B, padded, world)
    if why is not None:
        return give_up(why)
    return cls


def epoch_chunks(nodes, batch_size):
    """The reference's batches of one epoch (problem.py:141-153): a permutation from numpy's legacy stream, cut
    into n // batch_size + 1 near-equal chunks (never all of one size: quirk 6).  -> list of index arrays."""
    gs.helpers.legacy_stream.release()               # the shuffle is a HOST draw from the shared stream
    order = np.random.permutation(np.arange(nodes.shape[0]))
    return np.array_split(order, order.shape[0] // batch_size + 1)


def train_fused(args, problem, model, ddp, start_time, cls):
    """The training run on a fused engine (see the module docstring)."""
    assert args.cuda
    world, rank = (ddp.world, ddp.rank) if ddp is not None else (1, 0)
    nodes = problem.nodes['train']
    dev = torch.device('cuda')
    cls_task = problem.task == 'classification'
    every = 1 if args.engine == 'auto' else max(args.log_interval, 1)

    def targets_of(mids, shape):
        tg = np.asarray(problem.targets[mids.reshape(-1)])
        if cls_task:
            return torch.from_numpy(tg.reshape(shape)).long().to(dev)
        return torch.from_numpy(tg.reshape(shape + (-1,)).astype(np.float32)).to(dev)   # multilabel / regression

    if world > 1:
        # data-parallel: batches of one fixed size (the < batch-size tail of an epoch is dropped)
        B = args.batch_size // world
        n_batches = nodes.shape[0] // (B * world)
        assert n_batches >= 1, 'fewer training nodes than one global batch'

        def epoch_batches():
            gs.helpers.legacy_stream.release()
            order = np.random.permutation(np.arange(nodes.shape[0]))[:n_batches * B * world]     # problem.py:146
            mids = nodes[order].reshape(n_batches, world, B)[:, rank]
            return torch.from_numpy(np.ascontiguousarray(mids)).to(dev), targets_of(mids, (n_batches, B)), None
    else:
        # the reference's own chunks, padded to the largest one with the chunk's first seed
        n_batches = nodes.shape[0] // args.batch_size + 1
        B = -(-nodes.shape[0] // n_batches)
        assert B >= 2, 'fewer than two training nodes per batch'

        def epoch_batches():
            chunks = epoch_chunks(nodes, args.batch_size)
            mids = np.stack([np.concatenate([nodes[c], np.repeat(nodes[c[:1]], B - c.shape[0])]) for c in chunks])
            return (torch.from_numpy(mids).to(dev), targets_of(mids, (n_batches, B)),
                    [int(c.shape[0]) for c in chunks])
    ids, tgs, live = epoch_batches()
    first = tgs[0].view(B, 1) if cls_task else tgs[0]
    step = cls(model, problem.feats, problem.loss_fn, ids[0], first, ddp=ddp, **({"wide_head": True} if args.wide_head else {}))
    if args.wide_head:
        print('gsage: --wide-head: the head runs on %s' % (
            'gsage_head_wide' if step.fused_wide else 'gsage_head_ce (at most 64 classes)' if step.fused_head else
            'gsage_head_l1' if step.fused_l1 else 'stock torch ops (not a case of the wide head)'), file=sys.stderr)
    # engines with the fused classification head walk a device-resident queue of the epoch's batches; the others
    # (regression: the fused L1 head; multilabel: stock torch ops inside the captured step) take one batch per call
    queued = bool(step.fused_head)
    # (choose_engine has made sure that a head without a fused kernel never meets padded chunks)
    assert live is None or step.fused_head or step.fused_l1 or step.fused_wide or min(live) == B
    val_metric = train_metric = None
    epoch = 0
    if args.full_neighbour_eval:
        fold_eval = lambda mode='val': full_neighbour_evaluate(model, problem, mode=mode,      # noqa: E731
                                                               closure=args.eval_closure)
    elif os.environ.get("GSAGE_FUSED_EVAL", "1") == "1":
        fold_eval = FusedEvaluator(cls, model, problem, wide_head=args.wide_head,
                                   strict=cls in (gs.engine.FusedWeightedMeanTrainStep,
                                                  gs.engine.FusedDistinctMeanTrainStep,
                                                  gs.engine.FusedTemporalMeanTrainStep)).prepare('val')
    else:
        fold_eval = lambda mode='val': evaluate(model, problem, mode=mode)                     # noqa: E731
    # The per-batch line (train.py:150-158) without a host sync per step: batch b is scored on the device right behind
    # its step into a small device ring (problem.MetricRing), and the ring is read back -- one copy -- every 32 batches
    # and at the end of every epoch: same lines, same order, same values, printed 32 at a time.
    # (the `time` of a line is taken when its batch is SUBMITTED, not when the ring is read back; GSAGE_METRIC_RING=1
    # makes the ring one slot deep: the reference's per-batch flush, one host sync per batch)
    ring = gs.problem.MetricRing(problem.task, dev, capacity=max(1, int(os.environ.get("GSAGE_METRIC_RING", "32"))))
    pending = []
    # (class ids outside [0, C) are scored the reference's way, on the host: the synchronous route)
    tg_ok = problem.task != 'classification' or (int(np.min(problem.targets)) >= 0 and
                                                 int(np.max(problem.targets)) < problem.n_classes)

    def flush():
        nonlocal train_metric
        for (prog, stamp), metric in zip(pending, ring.results()):
            train_metric = metric
            print(dumps({"epoch": epoch, "epoch_progress": prog, "train_metric": train_metric,
                         "val_metric": val_metric, "time": stamp}))
        del pending[:]
        sys.stdout.flush()
    # GSAGE_TRAIN_TIMING=1 (bench.py's CLI measurement): wall seconds of every epoch's batch loop, bracketed by device
    # synchronisations, in step.timing -- the log lines reach stdout a ring at a time, their `time` stamps do not
    # resolve single batches any more
    timing = os.environ.get("GSAGE_TRAIN_TIMING", "0") == "1"
    step.timing = []
    for epoch in range(args.epochs):
        model.train()
        t_epoch = time()
        if epoch > 0:
            ids, tgs, live = epoch_batches()
        if queued:
            step.load_epoch(ids, tgs, n_valid=live)          # (compat / dense sampler: draws the epoch's values)
        if timing:
            torch.cuda.synchronize()
        t_loop = time()
        try:
            for b in range(n_batches):
                nb = live[b] if live is not None else B
                step.set_progress((epoch + b / n_batches) / args.epochs)
                preds = step.step_queue() if queued else step(ids[b, :nb], tgs[b, :nb])
                if (b % every == 0 or b == n_batches - 1) and rank == 0:
                    if tg_ok and preds.dtype == torch.float32 and preds.is_contiguous():
                        # (a full batch costs one indexing op here: the loop's host time per batch is what bounds the CLI)
                        full = nb == B
                        ring.score(tgs[b] if full else tgs[b, :nb], preds if full else preds[:nb])
                        pending.append((b / n_batches, time() - start_time))
                        if ring.pending == ring.capacity:
                            flush()
                    else:
                        flush()
                        train_metric = batch_metric(problem.task, tgs[b, :nb].view(nb, -1), preds[:nb])
                        print(dumps({"epoch": epoch, "epoch_progress": b / n_batches, "train_metric": train_metric,
                                     "val_metric": val_metric, "time": time() - start_time}))
                        sys.stdout.flush()
        except BaseException:
            try:
                flush()                   # (a run that dies mid-epoch still prints the batches it scored ...
            except Exception:             #  ... but a failing read-back must not replace the error that ended it)
                pass
            raise
        flush()
        if timing:
            torch.cuda.synchronize()
            step.timing.append({"epoch": epoch, "batches": n_batches, "seeds": int(sum(live)) if live is not None
                                else n_batches * B * world, "loop_s": time() - t_loop, "with_draws_s": time() - t_epoch})
        model.eval()
        t_val = time()
        val_metric = fold_eval('val')
        if timing:
            torch.cuda.synchronize()
            step.timing[-1]["val_s"] = time() - t_val
            step.timing[-1]["epoch_s"] = time() - t_epoch            # draws + batch loop + validation
    if rank == 0 and args.show_test:
        test_metric = fold_eval('test')
    gs.helpers.legacy_stream.release()                 # hand numpy's stream back to the host
    print('-- done --', file=sys.stderr)
    if rank == 0:
        print(dumps({"epoch": epoch, "train_metric": train_metric, "val_metric": val_metric,
                     "time": time() - start_time}))
        sys.stdout.flush()
        if args.show_test:
            print(dumps({"test_f1": test_metric}))
        if args.save_embeddings or args.save_neighbours or args.link_eval or args.probe or args.cluster:
            export(model, problem, args)
        if args.correct_smooth:
            correct_smooth(model, problem, args)
    if ddp is not None:
        ddp.close()
    return step


if __name__ == "__main__":
    main()
