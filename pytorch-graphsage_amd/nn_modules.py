"""
nn_modules.py -- the reference's plugin surface, backed by the gfx950 kernels.

Same three lookup tables, class names, constructor keywords, parameter names/shapes (so
state_dicts interchange) and call signatures as the reference's nn_modules.py
(sampler_lookup :104-107, prep_lookup :169-173, aggregator_lookup :324-330); the bodies are
calls into ops.py (C ABI of libgsage_hip.so).  What differs on purpose:

  * `feats[ids]` may arrive as a store.RowRef instead of a materialised tensor; the aggregators
    then gather inside their kernels.  Plain tensors are accepted everywhere, as in the reference.
  * The sparse sampler never leaves the device: no D2H/H2D of ids, no scipy row slicing.
    rng="compat" draws `sel` from numpy's global legacy stream exactly like nn_modules.py:88
    (bit-identical samples for the same seed); rng="philox" draws it in-kernel (counter based).
"""
import sys

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import _native as nat
from . import ops
from .store import DenseAdj, DeviceCSR, RowRef, TemporalAdj, WeightedAdj


# --------------------------------------------------------------------------------------------
# Samplers
# --------------------------------------------------------------------------------------------
class UniformNeighborSampler(object):
    """Dense `[n_nodes+1, K]` LongTensor adjacency (reference nn_modules.py:19-49): every row was
    pre-sampled to exactly K neighbours offline; a call picks the same n random columns for the
    whole batch (ONE torch.randperm per call, from torch's global CPU generator -- SURVEY quirk 4).
    On the GPU one launch of gsage_sample_dense computes `adj[ids][:, perm][:, :n]` without the
    [M, K] intermediate; CPU tensors keep stock indexing (host mode)."""

    def __init__(self, adj):
        self.adj = adj
        self._dev = {}                                    # device -> store.DenseAdj (train.check_samplers reads it)

    def table(self, device=None):
        """store.DenseAdj over the adjacency on `device` (default: where `adj` lives)."""
        adj = self.adj if torch.is_tensor(self.adj) else torch.as_tensor(np.asarray(self.adj), dtype=torch.int64)
        device = adj.device if device is None else torch.device(device)
        key = (device.type, device.index if device.index is not None or device.type == "cpu"
               else torch.cuda.current_device())
        if key not in self._dev:
            self._dev[key] = DenseAdj(adj.to(device))
        return self._dev[key]

    csr = table                                           # what the fused engines ask a sampler for

    @staticmethod
    def draw_keep(K, n_samples):
        """The columns a call keeps: head of ONE permutation of the K columns, drawn exactly where the
        reference draws it (nn_modules.py:44); n_samples = -1: all but the last (python slicing)."""
        return torch.randperm(K)[:n_samples]

    def __call__(self, ids, n_samples=-1):
        keep = self.draw_keep(self.adj.size(1), n_samples)
        if not ids.is_cuda:
            return self.adj[ids][:, keep]
        tab = self.table(ids.device)
        ids = ids.contiguous().view(-1)
        M, n = int(ids.shape[0]), int(keep.shape[0])
        out = torch.empty(M, n, dtype=torch.int64, device=ids.device)
        keep = keep.to(ids.device, non_blocking=True)
        nat.check(nat.lib().gsage_sample_dense(tab.adj.data_ptr(), tab.K, tab.n_rows, ids.data_ptr(), M,
                                               keep.data_ptr(), n, out.data_ptr(), tab.err_flag.data_ptr(),
                                               ops._stream()), "sample_dense")
        return out


class SparseUniformNeighborSampler(object):
    """CSR uniform neighbour sampling with replacement (reference nn_modules.py:52-101) as the
    K1 kernel.  Contract: out[i*n+j] = row_i[sel[i,j] % deg_i], or the
    dummy node 0 when deg_i == 0, with sel ~ U[0, adj.shape[1]) -- modulo bias included."""

    rng_default = "compat"

    def __init__(self, adj, rng=None, seed=0):
        if isinstance(adj, (WeightedAdj, TemporalAdj)):    # under the uniform sampler the weights / times are ignored
            adj = adj.adj
        self.adj = adj
        self._host = DeviceCSR.from_scipy(adj, torch.device("cpu"))
        self._dev = {}
        self.rng = rng or SparseUniformNeighborSampler.rng_default
        assert self.rng in ("compat", "philox")
        self.seed = int(seed)
        self.calls = 0                # host-side call index (philox, eager)
        self.call_ctr = None          # device counter tensor (philox inside a captured graph)
        self.shard = (0, 1)           # (rank, world): offsets the global sample index

    @property
    def degrees(self):
        """nn_modules.py:76-78: stored-entry count per row == rowptr differences."""
        return np.diff(self._host.rowptr.numpy())

    def csr(self, device):
        device = torch.device(device)
        if device.type == "cpu":
            return self._host
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        if key not in self._dev:
            self._dev[key] = DeviceCSR(self._host.rowptr.to(device), self._host.col.to(device),
                                       self._host.n_rows, self._host.max_deg)
        return self._dev[key]

    def use_device_csr(self, csr):
        """Walk `csr` (a store.DeviceCSR already in HBM) on its device instead of uploading the scipy matrix this
        sampler was built with -- for graphs that only ever exist on the GPU (store.DeviceCSR.synthetic: a
        papers100M-sized CSR is 14 GB; the plugin API's scipy matrix is then a placeholder)."""
        dev = csr.device
        self._dev[(dev.type, dev.index if dev.index is not None else torch.cuda.current_device())] = csr
        return csr

    def __call__(self, ids, n_samples=128):
        assert n_samples > 0, 'SparseUniformNeighborSampler: n_samples must be set explicitly'
        ids = ids.contiguous().view(-1)
        csr = self.csr(ids.device)
        M = int(ids.shape[0])
        rank, world = self.shard
        if self.rng == "compat":
            # the reference's own draw (nn_modules.py:88).  Data-parallel: every rank draws the
            # whole job's matrix from the same stream and keeps its rows (dist.py).
            from .helpers import legacy_stream
            if ids.is_cuda and legacy_stream.enabled:
                # the same words, consumed on the device (gsage_mt_choice_device): no host draw, no H2D
                st = legacy_stream.acquire(ids.device)
                full = torch.empty(M * world * n_samples, dtype=torch.int32, device=ids.device)
                nat.check(nat.lib().gsage_mt_choice_device(st.data_ptr(), csr.max_deg, full.numel(),
                                                           full.data_ptr(), ops._stream()), "mt_choice_device")
                sel = full[rank * M * n_samples:(rank + 1) * M * n_samples]
                return ops.sample_csr(csr, ids, n_samples, sel=sel)
            legacy_stream.release()
            sel = np.random.choice(csr.max_deg, (M * world, n_samples))[rank * M:(rank + 1) * M]
            sel = torch.from_numpy(np.ascontiguousarray(sel, dtype=np.int32))
            if ids.is_cuda:
                sel = sel.to(ids.device, non_blocking=True)
            return ops.sample_csr(csr, ids, n_samples, sel=sel)
        ph = {"seed": self.seed, "g0": rank * M * n_samples}
        if self.call_ctr is not None:
            ph["call_ctr"] = self.call_ctr
            ph["call_base"] = self._static_calls
            self._static_calls += 1
        else:
            ph["call_base"] = self.calls
            self.calls += 1
        return ops.sample_csr(csr, ids, n_samples, philox=ph)

    # graph capture support: the call index lives in device memory and is advanced in-graph
    _static_calls = 0

    def begin_capture(self, counter):
        self.call_ctr = counter
        self._static_calls = 0

    def calls_in_capture(self):
        return self._static_calls


class SparseWeightedNeighborSampler(object):
    """CSR neighbour sampling with replacement in proportion to the edge weights (no reference counterpart;
    include/gsage.h, "Weighted adjacency"): out[i*n+j] = a neighbour of ids[i] drawn with probability q_e / T, the
    integer quanta of the adjacency's edge_cdf, or the dummy node 0 for a row without a drawable edge.  adj: a
    store.WeightedAdj (a bare scipy matrix carries no weights: ValueError).  Same call signature, `shard`,
    begin_capture / calls_in_capture, csr(device) and use_device_csr as SparseUniformNeighborSampler.  It always
    draws from Philox -- there is no legacy stream to be compatible with -- and says so once when the class-wide
    default asks for "compat"."""

    _said_philox = False

    def __init__(self, adj, rng=None, seed=0):
        if not isinstance(adj, WeightedAdj):
            raise ValueError("SparseWeightedNeighborSampler: the adjacency carries no edge weights "
                             "(wrap it in store.WeightedAdj, or add adj_weight / train_adj_weight to the problem)")
        if (rng or SparseUniformNeighborSampler.rng_default) != "philox" and not SparseWeightedNeighborSampler._said_philox:
            SparseWeightedNeighborSampler._said_philox = True
            print("gsage: the weighted sampler always draws from Philox (--rng compat has no meaning for it)",
                  file=sys.stderr)
        self.adj = adj
        self._weight = torch.from_numpy(adj.weight)
        self._host = DeviceCSR.from_scipy(adj.adj, torch.device("cpu")).with_weights(self._weight)
        self._dev = {}
        self.rng = "philox"
        self.seed = int(seed)
        self.calls = 0                # host-side call index (eager)
        self.call_ctr = None          # device counter tensor (inside a captured graph)
        self.shard = (0, 1)           # (rank, world): offsets the global sample index

    @property
    def degrees(self):
        return np.diff(self._host.rowptr.numpy())

    def csr(self, device):
        device = torch.device(device)
        if device.type == "cpu":
            return self._host
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        if key not in self._dev:
            # (the table is built where it lives: gsage_edge_cdf_build; the same bits as the host's)
            self._dev[key] = DeviceCSR(self._host.rowptr.to(device), self._host.col.to(device), self._host.n_rows,
                                       self._host.max_deg).with_weights(self._weight.to(device))
        return self._dev[key]

    def use_device_csr(self, csr):
        """Walk `csr` (a weighted store.DeviceCSR already in HBM) on its device, as the uniform sampler's."""
        if csr.edge_cdf is None:
            raise ValueError("SparseWeightedNeighborSampler: the adjacency carries no edge weights")
        dev = csr.device
        self._dev[(dev.type, dev.index if dev.index is not None else torch.cuda.current_device())] = csr
        return csr

    def __call__(self, ids, n_samples=128):
        assert n_samples > 0, 'SparseWeightedNeighborSampler: n_samples must be set explicitly'
        ids = ids.contiguous().view(-1)
        csr = self.csr(ids.device)
        rank, _ = self.shard
        ph = {"seed": self.seed, "g0": rank * int(ids.shape[0]) * n_samples}
        if self.call_ctr is not None:
            ph["call_ctr"] = self.call_ctr
            ph["call_base"] = self._static_calls
            self._static_calls += 1
        else:
            ph["call_base"] = self.calls
            self.calls += 1
        return ops.sample_csr_weighted(csr, ids, n_samples, ph)

    _static_calls = 0

    def begin_capture(self, counter):
        self.call_ctr = counter
        self._static_calls = 0

    def calls_in_capture(self):
        return self._static_calls


class SparseDistinctNeighborSampler(object):
    """CSR neighbour sampling WITHOUT replacement (no reference counterpart; include/gsage.h, "Distinct neighbours"): a
    row of degree <= n_samples returns every stored edge floor(n / deg) or ceil(n / deg) times -- the plain mean over
    the slots is the row's mean when deg divides n, and an unbiased estimate of it otherwise -- a longer row n_samples
    distinct stored edges, uniformly random; a row of degree 0 the dummy node 0.  adj: a scipy matrix in the
    reference's sparse convention, or a store.WeightedAdj whose weights are ignored (as the uniform sampler ignores
    them).  Same call signature, `shard`, begin_capture / calls_in_capture, csr(device) and use_device_csr as
    SparseUniformNeighborSampler, of which it is deliberately NOT a subclass: the engines accept a model by isinstance,
    and the uniform K1 must not run a model that asked for distinct draws.  It always draws from Philox and says so
    once when the class-wide default asks for "compat".  1 <= n_samples <= 256."""

    _said_philox = False

    def __init__(self, adj, rng=None, seed=0):
        if isinstance(adj, (WeightedAdj, TemporalAdj)):
            adj = adj.adj
        if (rng or SparseUniformNeighborSampler.rng_default) != "philox" and not SparseDistinctNeighborSampler._said_philox:
            SparseDistinctNeighborSampler._said_philox = True
            print("gsage: the distinct sampler always draws from Philox (--rng compat has no meaning for it)",
                  file=sys.stderr)
        self.adj = adj
        self._host = DeviceCSR.from_scipy(adj, torch.device("cpu"))
        self._dev = {}
        self.rng = "philox"
        self.seed = int(seed)
        self.calls = 0                # host-side call index (eager)
        self.call_ctr = None          # device counter tensor (inside a captured graph)
        self.shard = (0, 1)           # (rank, world): offsets the global sample index

    degrees = SparseUniformNeighborSampler.degrees
    csr = SparseUniformNeighborSampler.csr
    use_device_csr = SparseUniformNeighborSampler.use_device_csr

    def __call__(self, ids, n_samples=128):
        assert n_samples > 0, 'SparseDistinctNeighborSampler: n_samples must be set explicitly'
        ids = ids.contiguous().view(-1)
        csr = self.csr(ids.device)
        rank, _ = self.shard
        ph = {"seed": self.seed, "g0": rank * int(ids.shape[0]) * n_samples}
        if self.call_ctr is not None:
            ph["call_ctr"] = self.call_ctr
            ph["call_base"] = self._static_calls
            self._static_calls += 1
        else:
            ph["call_base"] = self.calls
            self.calls += 1
        return ops.sample_csr_distinct(csr, ids, n_samples, ph)

    _static_calls = 0

    def begin_capture(self, counter):
        self.call_ctr = counter
        self._static_calls = 0

    def calls_in_capture(self):
        return self._static_calls


class SparseTemporalNeighborSampler(object):
    """CSR neighbour sampling over the edges that happened strictly BEFORE a query time (no reference counterpart;
    include/gsage.h, "Temporal neighbours"): training node v "as of time t" on later edges would leak the future
    into the prediction.  adj: a store.TemporalAdj (a bare scipy matrix carries no times: ValueError).  strategy
    "uniform" draws with replacement among the eligible edges, "recent" takes the latest ones; inherit "seed" keeps the
    seed's time at every hop, "edge" hands the walked edge's time to the next hop (class-wide strategy_default /
    inherit_default, as rng_default).  The call takes and returns the times explicitly --
    (ids, times, n_samples) -> (ids, times) -- and keeps no frontier time between calls: two interleaved forwards
    cannot mix.  times=None asks for the adjacency's node_time (INT64_MAX without one: the whole row).  Same `shard`,
    begin_capture / calls_in_capture, csr(device) and use_device_csr as SparseUniformNeighborSampler, of which it is
    deliberately NOT a subclass (see SparseDistinctNeighborSampler).  It always draws from Philox and says so once when
    the class-wide default asks for "compat"."""

    _said_philox = False
    strategy_default = "uniform"
    inherit_default = "seed"
    temporal = True                   # what models.py asks a sampler: do the times flow beside the ids

    def __init__(self, adj, rng=None, seed=0, strategy=None, inherit=None):
        if not isinstance(adj, TemporalAdj):
            raise ValueError("SparseTemporalNeighborSampler: the adjacency carries no edge times "
                             "(wrap it in store.TemporalAdj, or add adj_time / train_adj_time to the problem)")
        self.strategy = strategy or SparseTemporalNeighborSampler.strategy_default
        self.inherit = inherit or SparseTemporalNeighborSampler.inherit_default
        if self.strategy not in ops.TEMPORAL_STRATEGIES:
            raise ValueError("SparseTemporalNeighborSampler: unknown strategy %r (known: uniform, recent)" % (self.strategy,))
        if self.inherit not in ops.TEMPORAL_INHERIT:
            raise ValueError("SparseTemporalNeighborSampler: unknown inherit rule %r (known: seed, edge)" % (self.inherit,))
        if (rng or SparseUniformNeighborSampler.rng_default) != "philox" and not SparseTemporalNeighborSampler._said_philox:
            SparseTemporalNeighborSampler._said_philox = True
            print("gsage: the temporal sampler always draws from Philox (--rng compat has no meaning for it)",
                  file=sys.stderr)
        self.adj = adj
        self._host = DeviceCSR.from_scipy(adj.adj, torch.device("cpu")).with_times(torch.from_numpy(adj.time))
        self._node_time = {}          # device -> int64 [n_rows]
        if adj.node_time is not None:
            self._node_time["cpu"] = torch.from_numpy(adj.node_time)
        self._dev = {}
        self.rng = "philox"
        self.seed = int(seed)
        self.calls = 0                # host-side call index (eager)
        self.call_ctr = None          # device counter tensor (inside a captured graph)
        self.shard = (0, 1)           # (rank, world): offsets the global sample index

    degrees = SparseUniformNeighborSampler.degrees

    def csr(self, device):
        device = torch.device(device)
        if device.type == "cpu":
            return self._host
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        if key not in self._dev:
            # (the host copy was checked when it was built: the same bytes need no second pass)
            self._dev[key] = DeviceCSR(self._host.rowptr.to(device), self._host.col.to(device), self._host.n_rows,
                                       self._host.max_deg, etime=self._host.etime.to(device))
        return self._dev[key]

    def use_device_csr(self, csr):
        """Walk `csr` (a temporal store.DeviceCSR already in HBM) on its device, as the uniform sampler's."""
        if csr.etime is None:
            raise ValueError("SparseTemporalNeighborSampler: the adjacency carries no edge times")
        dev = csr.device
        self._dev[(dev.type, dev.index if dev.index is not None else torch.cuda.current_device())] = csr
        return csr

    def default_times(self, ids):
        """The query times of seeds that come without any: node_time[ids], or INT64_MAX without a node_time."""
        ids = ids.contiguous().view(-1)
        if "cpu" not in self._node_time:
            return torch.full((int(ids.shape[0]),), ops.INT64_MAX, dtype=torch.int64, device=ids.device)
        key = str(ids.device)
        if key not in self._node_time:
            self._node_time[key] = self._node_time["cpu"].to(ids.device)
        return self._node_time[key][ids]

    def __call__(self, ids, times=None, n_samples=128):
        assert n_samples > 0, 'SparseTemporalNeighborSampler: n_samples must be set explicitly'
        ids = ids.contiguous().view(-1)
        if times is None:
            times = self.default_times(ids)
        csr = self.csr(ids.device)
        rank, _ = self.shard
        ph = {"seed": self.seed, "g0": rank * int(ids.shape[0]) * n_samples}
        if self.call_ctr is not None:
            ph["call_ctr"] = self.call_ctr
            ph["call_base"] = self._static_calls
            self._static_calls += 1
        else:
            ph["call_base"] = self.calls
            self.calls += 1
        return ops.sample_csr_temporal(csr, ids, times, n_samples, ph, strategy=self.strategy, inherit=self.inherit)

    _static_calls = 0

    def begin_capture(self, counter):
        self.call_ctr = counter
        self._static_calls = 0

    def calls_in_capture(self):
        return self._static_calls


sampler_lookup = {
    "uniform_neighbor_sampler": UniformNeighborSampler,
    "sparse_uniform_neighbor_sampler": SparseUniformNeighborSampler,
}

# samplers the reference does not have.  sampler_lookup stays the reference's table, name for name (the drop-in
# surface: tests/test_host_mode.py pins it); find_sampler() resolves a --sampler-class name over both
sampler_extensions = {
    "sparse_weighted_neighbor_sampler": SparseWeightedNeighborSampler,
    "sparse_distinct_neighbor_sampler": SparseDistinctNeighborSampler,
    "sparse_temporal_neighbor_sampler": SparseTemporalNeighborSampler,
}


def find_sampler(name):
    """The sampler class registered as `name`: the reference's table first, then this library's extensions."""
    if name in sampler_lookup:
        return sampler_lookup[name]
    if name in sampler_extensions:
        return sampler_extensions[name]
    raise KeyError("unknown sampler class %r (known: %s)" % (name, ", ".join(list(sampler_lookup) + list(sampler_extensions))))


# --------------------------------------------------------------------------------------------
# Preprocessers
# --------------------------------------------------------------------------------------------
def _as_tensor(feats):
    return feats.materialize() if isinstance(feats, RowRef) else feats


class IdentityPrep(nn.Module):
    """nn_modules.py:112-123: passes the (possibly lazy) feature rows through."""

    def __init__(self, input_dim, n_nodes=None):
        super(IdentityPrep, self).__init__()
        self.input_dim = input_dim

    @property
    def output_dim(self):
        return self.input_dim

    def forward(self, ids, feats, layer_idx=0):
        return feats


class NodeEmbeddingPrep(nn.Module):
    """nn_modules.py:126-155: trainable per-node embedding (+ affine), concatenated to the
    features when there are any.  Seeds (layer_idx 0) all read the spare row `n_nodes` so a node
    never sees its own embedding.  Gather = K2, dense gradient = K6 scatter-add."""

    def __init__(self, input_dim, n_nodes, embedding_dim=64):
        super(NodeEmbeddingPrep, self).__init__()
        self.n_nodes = n_nodes
        self.input_dim = input_dim
        self.embedding_dim = embedding_dim
        self.embedding = nn.Embedding(num_embeddings=n_nodes + 1, embedding_dim=embedding_dim)
        self.fc = nn.Linear(embedding_dim, embedding_dim)

    @property
    def output_dim(self):
        return (self.input_dim or 0) + self.embedding_dim

    def forward(self, ids, feats, layer_idx=0):
        rows = ids if layer_idx > 0 else torch.full_like(ids, self.n_nodes)
        embs = ops.embedding_rows(self.embedding.weight, rows)
        embs = ops.linear(embs, self.fc.weight, self.fc.bias)
        if self.input_dim:
            return torch.cat([_as_tensor(feats).float(), embs], dim=1)
        return embs


class LinearPrep(nn.Module):
    """nn_modules.py:158-166."""

    def __init__(self, input_dim, n_nodes, output_dim=32):
        super(LinearPrep, self).__init__()
        self.fc = nn.Linear(input_dim, output_dim, bias=False)
        self.output_dim = output_dim

    def forward(self, ids, feats, layer_idx=0):
        return ops.linear(_as_tensor(feats), self.fc.weight)


prep_lookup = {
    "identity": IdentityPrep,
    "node_embedding": NodeEmbeddingPrep,
    "linear": LinearPrep,
}


# --------------------------------------------------------------------------------------------
# Aggregators
# --------------------------------------------------------------------------------------------
def concat_combine(parts):
    return torch.cat(parts, dim=1)


def _split_activation(act):
    """(fusable code, leftover callable).  ReLU goes into the GEMM epilogue; anything else
    (e.g. the reference's `lambda x: x`, train.py:116) is applied afterwards."""
    if act is None:
        return nat.ACT_NONE, None
    if act in (F.relu, torch.relu) or isinstance(act, nn.ReLU):
        return nat.ACT_RELU, None
    return nat.ACT_NONE, act


class AggregatorMixin(object):
    @property
    def output_dim(self):
        """Width after combine_fn (nn_modules.py:178-182); 2 * output_dim_ for the concat."""
        probe = torch.zeros((1, self.output_dim_))
        return self.combine_fn([probe, probe]).size(1)

    def _project(self, x, agg):
        """combine_fn([fc_x(x), fc_neib(agg)]) + activation; one grouped MFMA launch for the
        stock concat."""
        code, post = _split_activation(self.activation)
        if self.combine_fn is concat_combine:
            hidden = code == nat.ACT_RELU and agg.is_cuda
            out = ops.sage_project(x, agg, self.fc_x.weight, self.fc_neib.weight, code,
                                   out_dtype=ops.torch_dtype() if hidden else torch.float32)
        else:
            xt = _as_tensor(x)
            out = self.combine_fn([ops.linear(xt, self.fc_x.weight),
                                   ops.linear(agg, self.fc_neib.weight)])
            if code == nat.ACT_RELU:
                out = torch.relu(out)
        return post(out) if post is not None else out


class MeanAggregator(nn.Module, AggregatorMixin):
    """nn_modules.py:185-204."""

    def __init__(self, input_dim, output_dim, activation, combine_fn=concat_combine):
        super(MeanAggregator, self).__init__()
        self.fc_x = nn.Linear(input_dim, output_dim, bias=False)
        self.fc_neib = nn.Linear(input_dim, output_dim, bias=False)
        self.output_dim_ = output_dim
        self.activation = activation
        self.combine_fn = combine_fn

    def forward(self, x, neibs):
        M = x.size(0)
        n = neibs.size(0) // M
        cdt = ops.torch_dtype() if neibs.is_cuda else torch.float32
        if isinstance(neibs, RowRef):
            same = isinstance(x, RowRef) and x.store is neibs.store and neibs.store.dtype == cdt
            agg = ops.gather_mean(neibs.store, neibs.ids, M, n, out_dtype=cdt,
                                  out_ld=neibs.store.ld if same else None)
        else:
            agg = ops.segment_mean(neibs, M, out_dtype=cdt)
        return self._project(x, agg)


class PoolAggregator(nn.Module, AggregatorMixin):
    """nn_modules.py:207-232.  pool_fn: "max" / "mean" run fused (K3: the [M*n, hidden] MLP
    output never reaches HBM); any other callable gets the unfused MLP output [M, n, hidden]."""

    def __init__(self, input_dim, output_dim, pool_fn, activation, hidden_dim=512,
                 combine_fn=concat_combine):
        super(PoolAggregator, self).__init__()
        self.mlp = nn.Sequential(nn.Linear(input_dim, hidden_dim, bias=True), nn.ReLU())
        self.fc_x = nn.Linear(input_dim, output_dim, bias=False)
        self.fc_neib = nn.Linear(hidden_dim, output_dim, bias=False)
        self.output_dim_ = output_dim
        self.activation = activation
        self.pool_fn = pool_fn
        self.combine_fn = combine_fn

    def forward(self, x, neibs):
        M = x.size(0)
        lin = self.mlp[0]
        if self.pool_fn in ("max", "mean"):
            mode = nat.POOL_MAX if self.pool_fn == "max" else nat.POOL_MEAN
            agg = ops.pool_mlp(neibs, lin.weight, lin.bias, M, mode)
        else:
            hid = ops.linear(_as_tensor(neibs), lin.weight, lin.bias, nat.ACT_RELU)
            agg = self.pool_fn(hid.view(M, -1, hid.size(1)))
        return self._project(x, agg)


class MaxPoolAggregator(PoolAggregator):
    """nn_modules.py:235-244."""

    def __init__(self, input_dim, output_dim, activation, hidden_dim=512, combine_fn=concat_combine):
        super(MaxPoolAggregator, self).__init__(input_dim=input_dim, output_dim=output_dim,
                                                pool_fn="max", activation=activation,
                                                hidden_dim=hidden_dim, combine_fn=combine_fn)


class MeanPoolAggregator(PoolAggregator):
    """nn_modules.py:247-256."""

    def __init__(self, input_dim, output_dim, activation, hidden_dim=512, combine_fn=concat_combine):
        super(MeanPoolAggregator, self).__init__(input_dim=input_dim, output_dim=output_dim,
                                                 pool_fn="mean", activation=activation,
                                                 hidden_dim=hidden_dim, combine_fn=combine_fn)


class LSTMAggregator(nn.Module, AggregatorMixin):
    """nn_modules.py:259-286: the output of a batch_first LSTM over each node's neighbour rows at the LAST position,
    then the concat projection.  On CUDA the recurrence and its backward run on this library's kernels
    (ops.lstm_last: K5 input projection with the neighbour gather fused for a RowRef, gsage_lstm_fwd / _bwd, K5b / K5
    for the gradients) in either compute mode; the reverse direction of a bidirectional LSTM is ONE cell evaluation on
    the last neighbour, which is all the reference's `[:, -1, :]` keeps of it.  `self.lstm` stays an nn.LSTM: it owns
    the parameters (state_dict keys, initialisation) and is what host mode (CPU tensors) calls."""

    _told = set()

    def __init__(self, input_dim, output_dim, activation, hidden_dim=512, bidirectional=False,
                 combine_fn=concat_combine):
        super(LSTMAggregator, self).__init__()
        assert not hidden_dim % 2, "LSTMAggregator: hiddem_dim % 2 != 0"
        self.lstm = nn.LSTM(input_dim, hidden_dim // (1 + bidirectional),
                            bidirectional=bidirectional, batch_first=True)
        self.fc_x = nn.Linear(input_dim, output_dim, bias=False)
        self.fc_neib = nn.Linear(hidden_dim, output_dim, bias=False)
        self.output_dim_ = output_dim
        self.activation = activation
        self.combine_fn = combine_fn

    def _why_stock(self, n):
        """None when the recurrence kernels take this shape, else the reason (said once per reason on stderr)."""
        H = self.lstm.hidden_size
        if ops.lstm_ok(H, n):
            return None
        why = ("LSTMAggregator: %d hidden units per direction over %d neighbours in %s mode is outside what "
               "gsage_lstm_ok covers (1..128 steps, up to 1024 units in bf16 / 512 in fp32); this call runs on "
               "torch.nn.LSTM instead" % (H, n, ops.config.compute_dtype))
        if why not in LSTMAggregator._told:
            LSTMAggregator._told.add(why)
            sys.stderr.write(why + "\n")
        return why

    def forward(self, x, neibs):
        M = x.size(0)
        if neibs.is_cuda and self._why_stock(neibs.size(0) // M) is None:
            l = self.lstm
            rev = (l.weight_ih_l0_reverse, l.weight_hh_l0_reverse, l.bias_ih_l0_reverse,
                   l.bias_hh_l0_reverse) if l.bidirectional else None
            agg = ops.lstm_last(neibs, M, l.weight_ih_l0, l.weight_hh_l0, l.bias_ih_l0, l.bias_hh_l0, rev)
            return self._project(x, agg)
        xt, nt = _as_tensor(x).float(), _as_tensor(neibs).float()
        seq, _ = self.lstm(nt.view(xt.size(0), -1, nt.size(1)))
        return self._project(xt, seq[:, -1, :].contiguous())


class AttentionAggregator(nn.Module, AggregatorMixin):
    """nn_modules.py:289-321: scores = att(neibs) . att(x), softmax over the fanout, weighted sum
    of the RAW neighbour rows.  The two tiny att GEMMs run on K5 (tanh fused), the weighting on
    K4 with the neighbour gather fused."""

    def __init__(self, input_dim, output_dim, activation, hidden_dim=32, combine_fn=concat_combine):
        super(AttentionAggregator, self).__init__()
        self.att = nn.Sequential(nn.Linear(input_dim, hidden_dim, bias=False), nn.Tanh(),
                                 nn.Linear(hidden_dim, hidden_dim, bias=False))
        self.fc_x = nn.Linear(input_dim, output_dim, bias=False)
        self.fc_neib = nn.Linear(input_dim, output_dim, bias=False)
        self.output_dim_ = output_dim
        self.activation = activation
        self.combine_fn = combine_fn

    @staticmethod
    def _rows(t):
        """Operand of the att MLP.  Lazy feature rows of a bf16 table are gathered ONCE, in storage
        precision and with the table's zero padding, i.e. already in the layout K5 wants (the generic
        route materialises fp32 rows and re-casts them: 3x the bytes and two extra passes)."""
        if isinstance(t, RowRef) and t.store.data.is_cuda and t.store.data.dtype == torch.bfloat16 \
                and ops.config.compute_dtype == "bf16":
            st = t.store
            ids = t.ids.contiguous().view(-1)
            buf = ops._gather_mean_raw(st.data, st.ld, ids, int(ids.shape[0]), 1, torch.bfloat16, st.ld)
            return ops.mark_zero_padded(buf[:, :st.dim])
        return _as_tensor(t)

    def _att(self, t):
        hid = ops.linear(t, self.att[0].weight, None, nat.ACT_TANH)
        return ops.linear(hid, self.att[2].weight)

    def forward(self, x, neibs):
        M = x.size(0)
        n = neibs.size(0) // M
        # the reference's bare .squeeze() (nn_modules.py:311) changes meaning for M == 1 or
        # fanout == 1 (train.py:75 forbids batch 1); refuse instead of silently diverging
        assert M > 1 and n > 1, "AttentionAggregator: needs batch > 1 and fanout > 1"
        xt, nt = self._rows(x), self._rows(neibs)
        agg = ops.attn_aggregate(self._att(nt), self._att(xt), neibs if isinstance(neibs, RowRef)
                                 else nt, M)
        return self._project(x, agg)


aggregator_lookup = {
    "mean": MeanAggregator,
    "max_pool": MaxPoolAggregator,
    "mean_pool": MeanPoolAggregator,
    "lstm": LSTMAggregator,
    "attention": AttentionAggregator,
}
