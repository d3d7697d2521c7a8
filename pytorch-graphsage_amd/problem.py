"""
problem.py -- NodeProblem: the data container the train loop iterates (reference
problem.py:74-153) plus the loss / metric tables (problem.py:26-64).

Same attributes (`adj, train_adj, feats, feats_dim, n_nodes, n_classes, loss_fn, metric_fn,
nodes, task`) and the same `iterate(mode, batch_size, shuffle)` generator, including its
chunking rule (n_chunks = len // batch_size + 1, np.array_split) and its draw from numpy's
global stream for the shuffle.  Differences:
  * the file may be the reference's HDF5 (needs h5py) or an .npz twin with the same keys
    (h5py is absent from the build image);
  * a sparse problem may carry edge weights: optional keys `adj_weight` / `train_adj_weight`, in the encoding of `adj`
    ((v, r, c) with v the weights); `adj` / `train_adj` then become store.WeightedAdj (what
    sparse_weighted_neighbor_sampler needs; the uniform samplers ignore the weights).  Files without them load as before;
  * a sparse problem may carry edge times: optional keys `adj_time` / `train_adj_time`, int64 in the encoding of `adj`
    ((v, r, c) with v the times), and `node_time`, int64 [n_nodes], the default query time of a seed; `adj` /
    `train_adj` then become store.TemporalAdj (what sparse_temporal_neighbor_sampler needs; the other samplers ignore
    the times).  A file with both weights and times loads as temporal.  Files without them load as before;
  * with cuda=True the feature matrix becomes a store.FeatureStore resident in HBM
    (bf16 rows padded to 128 B; fp32 when ops.config.compute_dtype == "fp32") instead of a
    FloatTensor, so per-batch gathers are fused into the aggregator kernels.
"""
from __future__ import division, print_function

import sys

import numpy as np
import torch
from scipy import sparse
from scipy.sparse import csr_matrix
from torch.nn import functional as F

from . import ops
from .store import FeatureStore, TemporalAdj, WeightedAdj


class ProblemLosses:
    """problem.py:26-38."""

    @staticmethod
    def multilabel_classification(preds, targets):
        return F.multilabel_soft_margin_loss(preds, targets)

    @staticmethod
    def classification(preds, targets):
        return F.cross_entropy(preds, targets)

    @staticmethod
    def regression_mae(preds, targets):
        # NB: called with targets.squeeze() (models.py:100): [B,1] vs [B] broadcasts to [B,B] in
        # the reference; kept as is (it is what the recorded Pokec result was trained with).
        return F.l1_loss(preds, targets)


class ProblemMetrics:
    """problem.py:44-64 (host-side sklearn, like the reference)."""

    @staticmethod
    def _f1(y_true, y_pred):
        from sklearn import metrics
        return {
            "micro": float(metrics.f1_score(y_true, y_pred, average="micro")),
            "macro": float(metrics.f1_score(y_true, y_pred, average="macro")),
        }

    @staticmethod
    def multilabel_classification(y_true, y_pred):
        return ProblemMetrics._f1(y_true, (y_pred > 0).astype(int))

    @staticmethod
    def classification(y_true, y_pred):
        return ProblemMetrics._f1(y_true, np.argmax(y_pred, axis=1))

    @staticmethod
    def regression_mae(y_true, y_pred):
        return float(np.abs(y_true - y_pred).mean())


class DeviceMetrics:
    """ProblemMetrics for CUDA tensors: the counting / reduction runs on the device
    (csrc/gsage_metrics.hip), 8 bytes come back for the log line instead of the [B, C] predictions
    going to the host and through sklearn on every batch (train.py:150)."""

    @staticmethod
    def _f1(y_true, preds, multilabel):
        from . import _native as nat
        preds = preds.detach().float().contiguous()
        B, C = preds.shape
        f32 = bool(multilabel and y_true.dtype.is_floating_point)
        y = y_true.detach().contiguous().float() if f32 else y_true.detach().contiguous().long()
        y = y.view(B, C) if multilabel else y.view(-1)
        assert y.shape[0] == B
        counts = torch.empty(3 * C + 1, dtype=torch.int32, device=preds.device)
        out = torch.empty(3, dtype=torch.float64, device=preds.device)
        nat.check(nat.lib().gsage_metric_f1(preds.data_ptr(), preds.stride(0), y.data_ptr(), int(multilabel),
                                            int(f32), C if multilabel else 0, B, C, counts.data_ptr(),
                                            out.data_ptr(), ops._stream()), "metric_f1")
        micro, macro, n_bad = out.tolist()
        if n_bad:
            # a class id outside [0, C): sklearn adds it to the label set (a false negative of a class that no
            # logit column stands for) -- score this batch exactly as the reference does, on the host
            fn = ProblemMetrics.multilabel_classification if multilabel else ProblemMetrics.classification
            return fn(y_true.detach().cpu().numpy(), preds.cpu().numpy())
        return {"micro": float(micro), "macro": float(macro)}

    @staticmethod
    def multilabel_classification(y_true, y_pred):
        return DeviceMetrics._f1(y_true, y_pred, True)

    @staticmethod
    def classification(y_true, y_pred):
        return DeviceMetrics._f1(y_true, y_pred, False)

    @staticmethod
    def regression_mae(y_true, y_pred):
        from . import _native as nat
        a = y_true.detach().float().contiguous().view(-1)
        b = y_pred.detach().float().contiguous().view(-1)
        assert a.shape == b.shape, "regression_mae: y_true and y_pred must have the same number of elements"
        out = torch.empty(1, dtype=torch.float64, device=a.device)
        nat.check(nat.lib().gsage_metric_mae(a.data_ptr(), b.data_ptr(), a.numel(), out.data_ptr(),
                                             ops._stream()), "metric_mae")
        return float(out.item())


class MetricRing(object):
    """problem.metric_fn of the batches of a training loop, scored on the device and read back a RING at a time.
    The reference scores every batch on the host (train.py:150-158); scoring on the device but reading the 24 bytes
    back per batch still costs a host sync per step (33 % of a Reddit-shaped run), and letting the metric kernel store
    straight into pinned host memory costs the step's stream ~15 us per batch (the kernel cannot retire before the
    PCIe write has).  So: `score()` launches ONE single-workgroup kernel that writes its three doubles into the next
    slot of a small device ring, `results()` -- called when `pending == capacity` or at the end of an epoch -- copies
    the ring once and returns the pending batches' metrics in order.  Same JSON lines, same order, same values; the
    lines reach stdout `capacity` at a time.  Targets with class ids outside [0, C) need the reference's host route
    (DeviceMetrics._f1): callers with such targets use batch_metric instead."""

    def __init__(self, task, device, capacity=32):
        self.task, self.capacity = task, int(capacity)
        self.ring = torch.zeros(self.capacity, 3, dtype=torch.float64, device=device)
        self.pending = 0
        self._counts = None

    def score(self, y_true, y_pred):
        from . import _native as nat
        assert self.pending < self.capacity, "MetricRing: call results() before the ring wraps"
        preds = y_pred.detach()
        assert preds.dtype == torch.float32 and preds.is_contiguous() and preds.is_cuda
        out = self.ring[self.pending]
        if self.task == "regression_mae":
            a = y_true.detach().float().contiguous().view(-1)
            b = preds.view(-1)
            assert a.shape == b.shape, "regression_mae: y_true and y_pred must have the same number of elements"
            nat.check(nat.lib().gsage_metric_mae(a.data_ptr(), b.data_ptr(), a.numel(), out.data_ptr(), ops._stream()),
                      "metric_mae")
        else:
            multilabel = self.task == "multilabel_classification"
            B, C = preds.shape
            f32 = bool(multilabel and y_true.dtype.is_floating_point)
            want = torch.float32 if f32 else torch.int64
            y = y_true                           # (the common case costs no tensor op: this runs once per batch)
            if y.dtype != want or not y.is_contiguous() or y.requires_grad:
                y = y.detach().contiguous().to(want)
            assert y.numel() == (B * C if multilabel else B)
            if self._counts is None:
                self._counts = torch.empty(3 * C + 1, dtype=torch.int32, device=preds.device)
            nat.check(nat.lib().gsage_metric_f1(preds.data_ptr(), preds.stride(0), y.data_ptr(), int(multilabel), int(f32),
                                                C if multilabel else 0, B, C, self._counts.data_ptr(), out.data_ptr(),
                                                ops._stream()), "metric_f1")
        self.pending += 1

    def results(self):
        """the metrics of the batches scored since the last call, in order (ONE device-to-host copy)"""
        n, self.pending = self.pending, 0
        if n == 0:
            return []
        vals = self.ring[:n].tolist()
        if self.task == "regression_mae":
            return [float(v[0]) for v in vals]
        return [{"micro": float(v[0]), "macro": float(v[1])} for v in vals]


def batch_metric(task, y_true, y_pred):
    """problem.metric_fn for a batch that may live on the GPU: CUDA tensors are scored by the device
    kernels, anything else by the reference's host route (ProblemMetrics on numpy copies)."""
    if torch.is_tensor(y_pred) and y_pred.is_cuda:
        return getattr(DeviceMetrics, task)(y_true.to(y_pred.device), y_pred)
    to_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return getattr(ProblemMetrics, task)(to_np(y_true), to_np(y_pred))


def parse_csr_matrix(x):
    """(v, r, c) triple -> csr_matrix with inferred shape (problem.py:70-72)."""
    v, r, c = x
    return csr_matrix((v, (r, c)))


def _weighted(adj, w):
    """adj with the weights of the problem file's (v, r, c) triple `w` (v: the weights), or adj itself without one"""
    if w is None:
        return adj
    if not sparse.issparse(adj):
        raise ValueError("edge weights need a sparse adjacency")
    if not sparse.issparse(w):
        v, r, c = np.asarray(w)
        w = csr_matrix((v.astype(np.float32), (r.astype(np.int64), c.astype(np.int64))), shape=adj.shape)
    return WeightedAdj(adj, w)


def _temporal(adj, tm, node_time, weight=None, key="adj", quiet=False):
    """adj with the edge times of the problem file's (v, r, c) triple `tm` (v: int64 times) as a store.TemporalAdj,
    or `adj` as it is without one.  Weights and times together are not supported: the weights are ignored, with one
    line on stderr (quiet: the line was said for the problem's other adjacency already)."""
    if tm is None:
        return adj
    if isinstance(adj, WeightedAdj) or weight is not None:
        if not quiet:
            print("gsage: the problem carries both edge weights and edge times (%s): loaded as temporal, the weights "
                  "are ignored" % key, file=sys.stderr)
        adj = adj.adj if isinstance(adj, WeightedAdj) else adj
    if not sparse.issparse(adj):
        raise ValueError("edge times need a sparse adjacency")
    if not sparse.issparse(tm):
        tm = np.asarray(tm)
        if tm.ndim == 2 and tm.shape[0] == 3:
            if tm.dtype.kind not in "iu":
                raise ValueError("edge times must be int64 (the %s_time key holds %s)" % (key, tm.dtype))
            v, r, c = tm
            tm = csr_matrix((v.astype(np.int64), (r.astype(np.int64), c.astype(np.int64))), shape=adj.shape)
    return TemporalAdj(adj, tm, node_time=node_time)


def _is_sparse(adj):
    return sparse.issparse(adj) or isinstance(adj, (WeightedAdj, TemporalAdj))


def _scalar(v):
    v = np.asarray(v)
    v = v.item() if v.shape == () else v
    return v.decode() if isinstance(v, bytes) else v


def _read_problem(path):
    """Returns a dict with the keys of utils/convert.py:192-202."""
    if path.endswith(".npz"):
        with np.load(path, allow_pickle=False) as f:
            return {k: f[k] for k in f.files}
    try:
        import h5py
    except ImportError:
        raise ImportError("reading %s needs h5py; convert it to the .npz twin "
                          "(same keys) with utils/h5_to_npz.py on a machine that has it" % path)
    with h5py.File(path, "r") as f:
        return {k: f[k][()] for k in f.keys()}


def save_problem_npz(path, problem):
    """Writes the .npz twin of the reference's problem.h5 (same keys; sparse adjacencies as the
    [3, nnz] (v, r, c) array of utils/convert.py:128-131)."""
    out = {}
    problem = dict(problem)
    for k in ("adj", "train_adj"):                  # a TemporalAdj's times travel under their own keys, in ITS order
        v = problem.get(k)
        if isinstance(v, TemporalAdj):
            coo = v.adj.tocoo()
            problem[k] = v.adj
            problem[k + "_time"] = np.vstack([v.time, coo.row.astype(np.int64), coo.col.astype(np.int64)])
            if v.node_time is not None and problem.get("node_time") is None:
                problem["node_time"] = v.node_time
    for k, v in problem.items():
        if v is None:
            continue
        if isinstance(v, WeightedAdj):              # (its weights travel under their own key: `adj_weight`)
            v = v.adj
        if sparse.issparse(v):
            coo = v.tocoo()
            v = np.vstack([coo.data, coo.row, coo.col])
        out[k] = np.asarray(v)
    np.savez(path, **out)


class NodeProblem(object):
    def __init__(self, problem_path, cuda=True):
        print('NodeProblem: loading started')
        f = _read_problem(problem_path)
        self.task = str(_scalar(f['task']))
        self.n_classes = int(_scalar(f['n_classes'])) if 'n_classes' in f else 1
        self.feats = f['feats'] if 'feats' in f else None
        self.folds = np.array([s.decode() if isinstance(s, bytes) else str(s) for s in f['folds']])
        self.targets = f['targets']
        self.node_time = None
        if 'sparse' in f and bool(_scalar(f['sparse'])):
            self.adj = _weighted(parse_csr_matrix(f['adj']), f.get('adj_weight'))
            self.train_adj = _weighted(parse_csr_matrix(f['train_adj']), f.get('train_adj_weight'))
            self.node_time = np.asarray(f['node_time']) if 'node_time' in f else None
            said = isinstance(self.adj, WeightedAdj) and 'adj_time' in f
            self.adj = _temporal(self.adj, f.get('adj_time'), self.node_time, key='adj')
            self.train_adj = _temporal(self.train_adj, f.get('train_adj_time'), self.node_time, key='train_adj',
                                       quiet=said)
        elif 'adj_time' in f or 'train_adj_time' in f:
            raise ValueError("edge times need a sparse adjacency")
        else:
            self.adj = f['adj']
            self.train_adj = f['train_adj']

        self.feats_dim = self.feats.shape[1] if self.feats is not None else None
        self.n_nodes = self.adj.shape[0]
        self.cuda = cuda
        self._to_device()

        self.nodes = {mode: np.where(self.folds == mode)[0] for mode in ("train", "val", "test")}
        self.loss_fn = getattr(ProblemLosses, self.task)
        self.metric_fn = getattr(ProblemMetrics, self.task)
        print('NodeProblem: loading finished')

    @classmethod
    def from_arrays(cls, task, n_classes, adj, train_adj, feats, folds, targets, cuda=True, adj_weight=None,
                    train_adj_weight=None, adj_time=None, train_adj_time=None, node_time=None):
        """The same object from arrays already in memory (the keys of utils/convert.py:192-202): adj / train_adj a
        scipy csr_matrix in the (v, r, c) convention (sparse problems) or an int array [n + 1, K] (dense), feats a
        float array / FeatureStore / None.  What bench.py's CLI measurements and the tests use instead of writing a
        multi-GB problem file first; everything downstream of the loader is the code path of `NodeProblem(path)`.
        adj_weight / train_adj_weight (sparse problems): edge weights as store.WeightedAdj takes them.
        adj_time / train_adj_time (sparse problems): int64 edge times as store.TemporalAdj takes them; node_time: int64
        [n_nodes], the seeds' default query times.  With both weights and times a problem is temporal."""
        self = object.__new__(cls)
        self.task, self.n_classes = str(task), int(n_classes) if n_classes is not None else 1
        self.feats, self.folds, self.targets = feats, np.asarray(folds), targets
        self.node_time = np.asarray(node_time) if node_time is not None else None
        self.adj = adj if adj_weight is None or adj_time is not None else WeightedAdj(adj, adj_weight)
        self.train_adj = train_adj if train_adj_weight is None or train_adj_time is not None \
            else WeightedAdj(train_adj, train_adj_weight)
        self.adj = _temporal(self.adj, adj_time, self.node_time, weight=adj_weight, key='adj')
        self.train_adj = _temporal(self.train_adj, train_adj_time, self.node_time, weight=train_adj_weight,
                                   key='train_adj', quiet=adj_weight is not None and adj_time is not None)
        self.feats_dim = feats.shape[1] if feats is not None else None
        self.n_nodes = self.adj.shape[0]
        self.cuda = cuda
        if isinstance(feats, FeatureStore):
            self.feats = None
            self._to_device()
            self.feats = feats
        else:
            self._to_device()
        self.nodes = {mode: np.where(self.folds == mode)[0] for mode in ("train", "val", "test")}
        self.loss_fn = getattr(ProblemLosses, self.task)
        self.metric_fn = getattr(ProblemMetrics, self.task)
        return self

    def _to_device(self):
        if not _is_sparse(self.adj):
            self.adj = torch.LongTensor(np.asarray(self.adj))
            self.train_adj = torch.LongTensor(np.asarray(self.train_adj))
            if self.cuda:
                self.adj, self.train_adj = self.adj.cuda(), self.train_adj.cuda()
        if self.feats is not None:
            if self.cuda:
                self.feats = FeatureStore.from_array(self.feats, torch.device("cuda"),
                                                     dtype=ops.config.compute_dtype)
            else:
                self.feats = torch.FloatTensor(np.asarray(self.feats, dtype=np.float32))

    def quantize_features(self):
        """Replace the features by their FP8 store (store.FeatureStore.quantize; a CPU problem's tensor becomes a
        CPU store: host mode).  Returns (bytes before, bytes after, largest absolute quantisation error)."""
        assert self.feats is not None, "quantize_features: this problem has no features"
        old = self.feats if isinstance(self.feats, FeatureStore) else FeatureStore.wrap(self.feats)
        if old.is_fp8:
            return old.nbytes(), old.nbytes(), 0.0
        new = old.quantize()
        err, rows = 0.0, int(old.data.shape[0])
        for o in range(0, rows, 1 << 20):                     # (chunks: two fp32 copies of a 28 GB table do not fit)
            ids = torch.arange(o, min(o + (1 << 20), rows), device=old.device)
            err = max(err, float((ops.gather_rows(new, ids) - ops.gather_rows(old, ids)).abs().max()))
        self.feats = new
        return old.nbytes(), new.nbytes(), err

    def _batch(self, mids, targets):
        mids = torch.LongTensor(mids)
        if self.task == 'classification':
            targets = torch.LongTensor(targets)
        elif self.task == 'multilabel_classification' or 'regression' in self.task:
            targets = torch.FloatTensor(np.asarray(targets, dtype=np.float32))
        else:
            raise Exception('NodeDataLoader: unknown task: %s' % self.task)
        if self.cuda:
            mids, targets = mids.cuda(), targets.cuda()
        return mids, targets

    def iterate(self, mode, batch_size=512, shuffle=False):
        nodes = self.nodes[mode]
        order = np.arange(nodes.shape[0])
        if shuffle:
            from .helpers import legacy_stream
            legacy_stream.release()                       # the shuffle is a HOST draw from the shared stream
            order = np.random.permutation(order)          # global legacy stream (problem.py:146)
        n_chunks = order.shape[0] // batch_size + 1       # never exactly batch_size (quirk 6)
        for chunk_id, chunk in enumerate(np.array_split(order, n_chunks)):
            mids = nodes[chunk]
            yield self._batch(mids, self.targets[mids]) + (chunk_id / n_chunks,)
