"""
store.py -- HBM-resident data layouts of the hot path.

  DeviceCSR     the adjacency the sampler walks: (rowptr int64 [n_rows+1], col int32 [nnz]) built
                once from the reference's scipy csr_matrix (problem.py:70-72: csr_matrix((v,(r,c)))
                in the convention of utils/convert.py:100-126 -- ids 1-based, row 0 the dummy,
                row i's neighbours in columns 0..deg_i-1).  Optionally weighted: `edge_cdf`, one
                uint64 per stored edge (include/gsage.h, "Weighted adjacency"), built by with_weights().
                from_edges() builds it from an edge list on the device, transpose() / symmetrized() from another
                DeviceCSR (include/gsage.h, "Graph construction"); graph_from_edges() is the same for the plugin
                surface, returned as scipy.
  WeightedAdj   the reference-convention scipy matrix plus one fp32 weight per stored edge: what a
                weighted problem hands to the samplers in place of the bare matrix.
  TemporalAdj   the reference-convention scipy matrix plus one int64 time per stored edge, rows reordered by
                time: what a temporal problem hands to the samplers.  DeviceCSR.with_times() carries the times
                (`etime`), DeviceCSR.snapshot(t) is the graph of the edges before t.
  FeatureStore  the node-feature table feats[N+1, D] (problem.py:118-121) kept in HBM as a
                row-major [n_rows, ld] matrix, bf16 (default on GPU) or fp32, rows padded with zeros
                to a multiple of 128 bytes so every row is a whole number of cache lines and
                16-byte lane loads are aligned.  Opt-in FP8 storage (dtype="fp8", .quantize()): one
                OCP e4m3fn byte per element (torch.float8_e4m3fn) plus `scale`, one power-of-two
                fp32 per column; value = e4m3(data[r, c]) * scale[c] (include/gsage.h, "FP8 feature
                table").  Its `dtype` says so: no consumer can mistake the bytes for bf16.
  RowRef        what `feats[ids]` (models.py:76,80) returns for a FeatureStore: a *reference* to
                rows, consumed by the fused gather kernels; the [B*f1*f2, D] frontier the reference
                materialises per batch never exists unless someone asks for `.materialize()`.
"""
import numpy as np
import torch


def _round_up(v, m):
    return (v + m - 1) // m * m


FP8 = torch.float8_e4m3fn
_DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp8": FP8}
_FP8_MAX = 448.0


def _ld_for(dim, tdt):
    """Leading dimension (elements) of a row padded to a multiple of 128 bytes."""
    return _round_up(int(dim), 128 // torch.empty(0, dtype=tdt).element_size())


def quantize_fp8_host(x):
    """Host-mode statement of gsage_quantize_fp8 in stock torch: x [R, D] fp32 / bf16 (CPU) -> (q [R, D]
    float8_e4m3fn, scale [D] fp32).  scale[c] = the smallest power of two s >= 2^-126 with max|x[:, c]| / s <= 448
    (1.0 for an all-zero column); q = x / s rounded to e4m3fn, nearest even, saturating (never a NaN byte).  A NaN
    input counts as 0, one beyond +-2^127 as +-2^127."""
    x = torch.nan_to_num(x.float(), nan=0.0).clamp(-2.0 ** 127, 2.0 ** 127)    # (every decoded value stays finite)
    amax = x.abs().amax(dim=0) if x.shape[0] else torch.zeros(x.shape[1])
    mant, exp = torch.frexp(amax)                            # amax = mant * 2^exp, mant in [0.5, 1): 448 = 0.875 * 2^9
    k = (exp - 9 + (mant > 0.875).to(exp.dtype)).clamp(-126, 119)
    scale = torch.where(amax > 0, torch.ldexp(torch.ones_like(amax), k), torch.ones_like(amax))
    q = (x / scale).clamp(-_FP8_MAX, _FP8_MAX).to(FP8)       # x / s is exact; the cast rounds to nearest even
    return q, scale


def row_positions(indptr):
    """[0..deg_0-1, 0..deg_1-1, ...] for a CSR row pointer, via one cumsum (np.repeat on 1e8
    entries is ~10x slower)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    nnz = int(indptr[-1])
    if nnz == 0:
        return np.zeros(0, dtype=np.int32)
    deg = np.diff(indptr)
    rows = np.flatnonzero(deg > 0)
    step = np.ones(nnz, dtype=np.int32)
    step[0] = 0
    step[indptr[rows[1:]]] -= deg[rows[:-1]].astype(np.int32)
    return np.cumsum(step, dtype=np.int32)


def _canonical_csr(adj):
    """adj as a scipy CSR with sorted indices (the order DeviceCSR.from_scipy stores the edges in)"""
    adj = adj.tocsr()
    return adj if adj.has_sorted_indices else adj.sorted_indices()


class WeightedAdj(object):
    """A sparse adjacency in the reference's convention with one fp32 weight per stored edge.  `weight`: a scipy
    matrix with the structure of `adj` (same indptr / indices once both are in canonical order) whose data are the
    weights, or a flat array aligned with the data of `adj` in canonical (row-major, sorted-column) order; anything
    else is a ValueError.  Forwards `.shape`, so whatever only asks an adjacency for its size takes it as is; the
    weighted sampler reads `.adj` and `.weight`, the uniform samplers `.adj` alone.  The values are validated where
    the table is built (DeviceCSR.with_weights)."""

    def __init__(self, adj, weight):
        from scipy import sparse
        if not sparse.issparse(adj):
            raise ValueError("WeightedAdj: the adjacency must be a scipy sparse matrix")
        self.adj = _canonical_csr(adj)
        if sparse.issparse(weight):
            w = _canonical_csr(weight)
            if w.shape[0] != self.adj.shape[0] or not np.array_equal(w.indptr, self.adj.indptr) or \
                    not np.array_equal(w.indices, self.adj.indices):
                raise ValueError("WeightedAdj: the weight matrix does not have the adjacency's structure")
            weight = w.data
        weight = np.asarray(weight)
        if weight.ndim != 1 or weight.shape[0] != self.adj.nnz:
            raise ValueError("WeightedAdj: %s weights for %d stored edges" % (weight.shape, self.adj.nnz))
        self.weight = np.ascontiguousarray(weight, dtype=np.float32)

    @property
    def shape(self):
        return self.adj.shape


INT64_MAX = (1 << 63) - 1


class TemporalAdj(object):
    """A sparse adjacency in the reference's convention with one int64 time per stored edge (include/gsage.h,
    "Temporal neighbours").  `time`: a scipy matrix with the structure of `adj` whose data are the times, or a flat
    array aligned with the data of `adj` in canonical (row-major, sorted-column) order, as WeightedAdj aligns weights;
    anything else, a time that is not an integer and a time equal to INT64_MAX are a ValueError.  On the host every row
    is reordered by time -- stably: edges of one time keep their order -- and its columns re-issued as 0..deg-1, so
    afterwards `.adj` is in time order (still in the reference's convention) and `.time` is aligned with its data.
    node_time: int64 [n_rows] or None, the default query time of a seed (None: INT64_MAX, the whole row).  Forwards
    `.shape`; the temporal sampler reads `.adj`, `.time` and `.node_time`, every other sampler `.adj` alone."""

    def __init__(self, adj, time, node_time=None):
        from scipy import sparse
        if not sparse.issparse(adj):
            raise ValueError("TemporalAdj: the adjacency must be a scipy sparse matrix")
        adj = _canonical_csr(adj)
        if sparse.issparse(time):
            tm = _canonical_csr(time)
            if tm.shape[0] != adj.shape[0] or not np.array_equal(tm.indptr, adj.indptr) or \
                    not np.array_equal(tm.indices, adj.indices):
                raise ValueError("TemporalAdj: the time matrix does not have the adjacency's structure")
            time = tm.data
        time = np.asarray(time)
        if time.ndim != 1 or time.shape[0] != adj.nnz:
            raise ValueError("TemporalAdj: %s times for %d stored edges" % (time.shape, adj.nnz))
        if time.dtype.kind not in "iu":
            raise ValueError("TemporalAdj: edge times must be integers (int64), not %s" % time.dtype)
        if time.size and int(time.max()) >= INT64_MAX:
            raise ValueError("TemporalAdj: edge times must be below INT64_MAX (the query time that sees every edge)")
        time = np.ascontiguousarray(time, dtype=np.int64)
        indptr = np.asarray(adj.indptr, dtype=np.int64)
        rows = np.repeat(np.arange(adj.shape[0], dtype=np.int64), np.diff(indptr))
        order = np.lexsort((time, rows))                   # by row, then by time; lexsort is stable
        self.adj = sparse.csr_matrix((np.asarray(adj.data)[order], row_positions(indptr), indptr), shape=adj.shape)
        self.time = time[order]
        if node_time is not None:
            node_time = np.asarray(node_time)
            if node_time.ndim != 1 or node_time.shape[0] != adj.shape[0] or node_time.dtype.kind not in "iu":
                raise ValueError("TemporalAdj: node_time must be int64 [%d] (one query time per row)" % adj.shape[0])
            node_time = np.ascontiguousarray(node_time, dtype=np.int64)
        self.node_time = node_time

    @property
    def shape(self):
        return self.adj.shape


class DeviceCSR(object):
    def __init__(self, rowptr, col, n_rows, max_deg, edge_cdf=None, etime=None):
        self.rowptr = rowptr          # int64 [n_rows + 1]
        self.col = col                # int32 [nnz]
        self.n_rows = int(n_rows)     # adj.shape[0]  (counts the dummy row)
        self.max_deg = int(max_deg)   # adj.shape[1]: the population `sel` is drawn from
        self.edge_cdf = edge_cdf      # weighted: int64 [nnz] holding the uint64 bits of the per-row running sums
        self.etime = etime            # temporal: int64 [nnz], non-decreasing inside every row (with_times)
        self.err_flag = torch.zeros(1, dtype=torch.int32, device=rowptr.device)

    @property
    def device(self):
        return self.rowptr.device

    @property
    def nnz(self):
        return int(self.col.shape[0])

    def with_weights(self, weight):
        """Make this adjacency weighted: weight = one fp32 per stored edge, aligned with `col`, finite and >= 0
        (ValueError otherwise -- checked here, once, by reductions on the adjacency's device).  Builds `edge_cdf`
        (gsage_edge_cdf_build on the GPU, the same integers in numpy on the CPU) and returns self.  An edge lighter
        than 2^-24 of its row's heaviest gets the quantum 0 and is never drawn."""
        from . import ops
        w = torch.as_tensor(weight).to(device=self.device, dtype=torch.float32).contiguous().view(-1)
        if int(w.shape[0]) != self.nnz:
            raise ValueError("with_weights: %d weights for %d stored edges" % (int(w.shape[0]), self.nnz))
        if w.numel() and not bool((torch.isfinite(w) & (w >= 0)).all()):
            raise ValueError("with_weights: edge weights must be finite and >= 0")
        self.edge_cdf = ops.edge_cdf(self.rowptr, w, self.n_rows)
        return self

    def with_times(self, etime):
        """Make this adjacency temporal: etime = one int64 per stored edge, aligned with `col`, non-decreasing inside
        every row and below INT64_MAX (ValueError otherwise -- checked here, once, by reductions on the adjacency's
        device).  Sets `.etime` and returns self."""
        t = torch.as_tensor(etime)
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError("with_times: edge times must be integers (int64), not %s" % t.dtype)
        t = t.to(device=self.device, dtype=torch.int64).contiguous().view(-1)
        if int(t.shape[0]) != self.nnz:
            raise ValueError("with_times: %d times for %d stored edges" % (int(t.shape[0]), self.nnz))
        if t.numel():
            if int(t.max()) >= INT64_MAX:
                raise ValueError("with_times: edge times must be below INT64_MAX (the query time that sees every edge)")
            if t.numel() > 1:
                down = t[1:] < t[:-1]                      # a step down is allowed only where a new row begins
                first = torch.zeros(self.nnz + 1, dtype=torch.bool, device=self.device)
                first[self.rowptr] = True
                if bool((down & ~first[1:self.nnz]).any()):
                    raise ValueError("with_times: the edges of a row are not in time order (store.TemporalAdj reorders "
                                     "the rows of a scipy adjacency by time)")
        self.etime = t
        return self

    def snapshot(self, t):
        """The graph "as of t": a new DeviceCSR over the same n_rows (max_deg unchanged, `.etime` kept) holding exactly
        the edges with etime < t -- the first cnt positions of every row.  Built on the device by
        gsage_temporal_count, one torch.cumsum and gsage_temporal_compact; on the CPU the same definition in numpy.
        Full-neighbourhood inference, closures, propagation, retrieval and ranking take it as any adjacency."""
        from . import ops
        if self.etime is None:
            raise ValueError("snapshot: the adjacency carries no edge times (DeviceCSR.with_times)")
        rowptr, col, etime = ops.temporal_snapshot(self, int(t))
        return DeviceCSR(rowptr, col, self.n_rows, self.max_deg, etime=etime)

    def _importance_rows(self, n_walks, walk_len, top, seed, chunk, p=1.0, q=1.0, restart=0.0):
        """(rowptr int64 [n_rows + 1], col int32 [nnz], counts fp32 [nnz]) of importance(), on this adjacency's device"""
        from . import ops
        ops.importance_check(int(n_walks), int(walk_len), int(top))
        ops.walk_bias_check(p, q, restart, "importance_walks_biased")
        chunk = max(int(chunk), 1)
        degs, cols, counts = [], [], []
        for o in range(0, self.n_rows, chunk):
            ids = torch.arange(o, min(o + chunk, self.n_rows), dtype=torch.int64, device=self.device)
            c, w, d = ops.importance_walks(self, ids, n_walks, walk_len, top, seed, p=p, q=q, restart=restart)
            c, w = ops.importance_compact(c, w, d)        # (the padded buffers of a chunk end here)
            degs.append(d)
            cols.append(c)
            counts.append(w)
        self.check()
        rowptr = torch.zeros(self.n_rows + 1, dtype=torch.int64, device=self.device)
        if not degs:
            return rowptr, torch.zeros(0, dtype=torch.int32, device=self.device), \
                torch.zeros(0, dtype=torch.float32, device=self.device)
        torch.cumsum(torch.cat(degs), 0, dtype=torch.int64, out=rowptr[1:])
        return rowptr, torch.cat(cols), torch.cat(counts)

    def importance(self, n_walks=50, walk_len=2, top=16, seed=0, chunk=1 << 20, p=1.0, q=1.0, restart=0.0):
        """The importance-weighted adjacency of this one (include/gsage.h, "Importance neighbourhoods"): from every
        row, n_walks random walks of walk_len steps (weighted steps when this adjacency carries an edge_cdf); the row's
        new neighbours are its `top` most-visited nodes, most visited first, and the visit counts are the edge weights.
        -> a new DeviceCSR over the same n_rows with max_deg = top and its edge_cdf (with_weights(counts)).  Built
        `chunk` rows at a time: the padded [chunk, top] buffers are all that exists beside the result.  IndexError
        (check()) when a stored neighbour id lies outside the graph.  n_walks in 1.., walk_len in 1..16, top in 1..64,
        n_walks * walk_len <= 4096.  p, q in [1/8, 8] and restart in [0, 1): node2vec's return and in-out parameters and
        a restart probability for the walks (include/gsage.h, "Biased walks"); 1, 1, 0 are the plain walks.  The
        defaults reach the toy results of the tests; nobody has tuned them on a real graph."""
        rowptr, col, counts = self._importance_rows(n_walks, walk_len, top, seed, chunk, p, q, restart)
        return DeviceCSR(rowptr, col, self.n_rows, int(top)).with_weights(counts)

    @staticmethod
    def from_scipy(adj, device, weight=None):
        """adj: scipy.sparse matrix in the reference convention.  Checks the convention instead
        of silently re-interpreting it: the reference indexes a row by COLUMN (nn_modules.py:90-93),
        which equals the position inside the row only when columns are 0..deg-1.  weight (optional): as
        for WeightedAdj; the result then carries its edge_cdf (with_weights)."""
        from scipy import sparse
        if isinstance(adj, WeightedAdj):
            adj = adj.adj
        if isinstance(adj, TemporalAdj):          # its rows are in time order already: the times ride along
            if weight is not None:
                raise ValueError("DeviceCSR.from_scipy: weights and times together are not supported")
            return DeviceCSR.from_scipy(adj.adj, device).with_times(adj.time)
        if weight is not None:
            wadj = WeightedAdj(adj, weight)
            return DeviceCSR.from_scipy(wadj.adj, device).with_weights(wadj.weight)
        assert sparse.issparse(adj), "SparseUniformNeighborSampler: not sparse.issparse(adj)"
        adj = adj.tocsr()
        if not adj.has_sorted_indices:
            adj = adj.sorted_indices()
        indptr = np.asarray(adj.indptr, dtype=np.int64)
        # columns 0..deg-1 in every row: strictly increasing columns (scipy's canonical-format flag: one C pass over the
        # indices, cached on the matrix) whose LAST one is deg - 1 -- an O(rows) look instead of building and comparing
        # an nnz-long position array (0.36 of the 0.47 s the reference's Reddit command line took, two adjacencies)
        deg = np.diff(indptr)
        rows = np.flatnonzero(deg > 0)
        indices = np.asarray(adj.indices)
        ok = bool(adj.has_canonical_format) and (rows.size == 0 or (
            np.array_equal(indices[indptr[rows + 1] - 1], deg[rows] - 1) and bool((indices[indptr[rows]] == 0).all())))
        if not ok:
            raise ValueError("adjacency is not in the reference's sparse convention "
                             "(row i must hold its neighbours in columns 0..deg_i-1)")
        data = np.asarray(adj.data)
        # (ids wider than 32 bits: both bounds BEFORE narrowing -- -(2**32) + 5 would wrap to 5 and pass a check made after)
        if data.size and data.dtype.itemsize > 4 and (data.max() >= 2 ** 31 or data.min() < 1):
            raise ValueError("neighbour ids must be 1-based positive int32 values")
        rowptr = torch.from_numpy(indptr).to(device)
        col = torch.from_numpy(data.astype(np.int32, copy=False)).to(device)
        # (the lower bound is looked at where the narrowed ids already are: one pass on the device, not on the host)
        if data.size and int(col.min()) <= 0:
            raise ValueError("neighbour ids must be 1-based positive int32 values")
        return DeviceCSR(rowptr, col, adj.shape[0], adj.shape[1])

    @staticmethod
    def from_edges(src, dst, n_nodes, device, sel=None, weight=None, time=None, directed=False, order=None,
                   duplicates=None):
        """The adjacency of an edge list, built on `device` (include/gsage.h, "Graph construction"; ops.edges_to_csr):
        src, dst int64 [E] node ids in 0..n_nodes-1 -> the reference's sparse convention (n_rows = n_nodes + 1, row
        u + 1 holds neighbour + 1, row 0 the empty dummy), bit-identical to convert.graph_from_edgelist +
        make_sparse_adjacency under the defaults.  sel: bool [n_nodes], only edges between selected nodes (the
        training graph).  weight fp32 [E] / time int64 [E]: the result carries its edge_cdf (with_weights) / etime
        (with_times).  directed: one record per edge instead of two.  duplicates: "first" (default), "sum" (weights),
        "all" (default with time); order: "insertion" (default), "id", "time" (with time).  ValueError for what the
        definition does not have (2^31 records or more among it: there is no chunked build), IndexError for an id
        outside the graph."""
        from . import ops
        device = torch.device(device)

        def dev(x, dtype):
            if x is None:
                return None
            x = torch.as_tensor(x)
            if dtype == torch.int64 and (x.dtype.is_floating_point or x.dtype == torch.bool):
                raise ValueError("DeviceCSR.from_edges: node ids and edge times must be integers, not %s" % x.dtype)
            return x.to(device=device, dtype=dtype).contiguous().view(-1)
        rowptr, col, max_deg, pay = ops.edges_to_csr(dev(src, torch.int64), dev(dst, torch.int64), n_nodes,
                                                     sel=dev(sel, torch.bool), weight=dev(weight, torch.float32),
                                                     time=dev(time, torch.int64), directed=directed, order=order,
                                                     duplicates=duplicates)
        csr = DeviceCSR(rowptr, col, int(n_nodes) + 1, max_deg)
        if weight is not None:
            return csr.with_weights(pay)
        return csr.with_times(pay) if time is not None else csr

    def transpose(self):
        """A^T over the same rows, on the stored ids as they are: row v lists u for every stored u -> v, ascending u,
        duplicates kept (ops.csr_transpose: one sort).  max_deg = the largest new row, at least 1.  A weighted or
        temporal adjacency is a ValueError."""
        from . import ops
        rowptr, col, max_deg = ops.csr_transpose(self)
        return DeviceCSR(rowptr, col, self.n_rows, max_deg)

    def symmetrized(self):
        """The union of the stored edges and their reverses, every (row, neighbour) once, ascending neighbour id
        (ops.csr_transpose(symmetric=True)).  A weighted or temporal adjacency is a ValueError."""
        from . import ops
        rowptr, col, max_deg = ops.csr_transpose(self, symmetric=True)
        return DeviceCSR(rowptr, col, self.n_rows, max_deg)

    def to_scipy(self):
        """The scipy csr_matrix of this adjacency in the reference's convention: shape (n_rows, max_deg), row v's
        neighbour ids as int64 data in columns 0..deg_v - 1.  One copy to the host."""
        from scipy import sparse
        indptr = self.rowptr.cpu().numpy()
        return sparse.csr_matrix((self.col.cpu().numpy().astype(np.int64), row_positions(indptr), indptr),
                                 shape=(self.n_rows, self.max_deg))

    def check(self):
        """Raise IndexError if a kernel saw an id outside the graph (synchronises)."""
        if int(self.err_flag.item()) != 0:
            self.err_flag.zero_()
            raise IndexError("sampler: node id out of range of the adjacency")

    @staticmethod
    def synthetic(n_rows, deg_lo, deg_hi, device, max_deg=None, seed=0, empty_every=0, chunk=1 << 29):
        """A random graph in the reference's sparse convention built ON THE DEVICE (benchmarks and the
        BASELINE-size tests: papers100M's 3.2e9 edges are 13 GB of int32 that no host round trip should carry):
        row 0 = the dummy (no neighbours), degrees uniform in [deg_lo, deg_hi], neighbour ids uniform in
        [1, n_rows); every `empty_every`-th row (if > 0) has no neighbours -> samples the dummy.  Row offsets are
        int64 (they pass 2^31), the edge array is filled in chunks (a single randint of > 2^31 elements is not
        something to rely on)."""
        gen = torch.Generator(device=device).manual_seed(int(seed))
        deg = torch.randint(int(deg_lo), int(deg_hi) + 1, (int(n_rows),), dtype=torch.int64, device=device, generator=gen)
        deg[0] = 0
        if empty_every:
            deg[3::int(empty_every)] = 0
        rowptr = torch.zeros(int(n_rows) + 1, dtype=torch.int64, device=device)
        torch.cumsum(deg, 0, out=rowptr[1:])
        del deg
        nnz = int(rowptr[-1])
        col = torch.empty(nnz, dtype=torch.int32, device=device)
        for o in range(0, nnz, chunk):
            n = min(chunk, nnz - o)
            col[o:o + n] = torch.randint(1, int(n_rows), (n,), dtype=torch.int32, device=device, generator=gen)
        return DeviceCSR(rowptr, col, n_rows, max_deg if max_deg is not None else int(deg_hi))


def importance_adj(adj, n_walks=50, walk_len=2, top=16, seed=0, device=None, p=1.0, q=1.0, restart=0.0):
    """Any sparse adjacency -> its importance-weighted one (DeviceCSR.importance), as the WeightedAdj a weighted problem
    would hand to the samplers.  adj: a scipy matrix in the reference's sparse convention, or a WeightedAdj (its walks
    then step in proportion to the edge weights).  -> WeightedAdj in the same convention: shape (n_rows, top), row v in
    columns 0..k_v - 1, data the neighbour ids most visited first, weight the visit counts.  Accepted as it is by
    sparse_weighted_neighbor_sampler, by full-neighbourhood inference (mean and mean-pool models, as for any weighted
    graph) and by DeviceCSR.from_scipy.  device: where the walks run -- default the GPU when there is one, else host
    mode (the same rows).  p, q, restart: as for DeviceCSR.importance (biased walks, restarts).  The defaults reach the
    toy results of the tests; nobody has tuned them on a real graph."""
    if device is None:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    if isinstance(adj, WeightedAdj):
        csr = DeviceCSR.from_scipy(adj.adj, device, weight=adj.weight)
    else:
        csr = DeviceCSR.from_scipy(adj, device)
    rowptr, col, counts = csr._importance_rows(n_walks, walk_len, top, seed, 1 << 20, p, q, restart)
    return WeightedAdj(DeviceCSR(rowptr, col, csr.n_rows, int(top)).to_scipy(), counts.cpu().numpy())


def graph_from_edges(edges, n_nodes, sel=None, weight=None, time=None, node_time=None, directed=False, order=None,
                     duplicates=None, device=None):
    """An edge list -> the adjacency the plugin surface trades in, in the reference's sparse convention: a scipy
    csr_matrix of shape (n_nodes + 1, max_deg), a WeightedAdj (weight: fp32 [E]) or a TemporalAdj (time: int64 [E];
    node_time: int64 [n_nodes + 1], the seeds' default query times).  edges: int array [E, 2] of node ids in
    0..n_nodes-1, or a pair (src, dst).  sel, directed, order, duplicates: as for DeviceCSR.from_edges, whose
    definition this is (include/gsage.h, "Graph construction"); under the defaults the matrix equals
    convert.make_sparse_adjacency(convert.graph_from_edgelist(edges, n_nodes), sel).  device: where it is built --
    default the GPU when there is one, else host mode (the same arrays); the result comes back in one copy."""
    from . import ops
    if device is None:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    device = torch.device(device)
    if isinstance(edges, (tuple, list)) and len(edges) == 2 and np.ndim(edges[0]) == 1:
        src, dst = np.asarray(edges[0]), np.asarray(edges[1])
    else:
        e = np.asarray(edges)
        if e.size == 0:
            e = e.reshape(0, 2)
        if e.ndim != 2 or e.shape[1] != 2:
            raise ValueError("graph_from_edges: edges must be an int array [E, 2] or a pair (src, dst)")
        src, dst = e[:, 0], e[:, 1]

    def dev(x, dtype, what):
        if x is None:
            return None
        x = np.asarray(x)
        if dtype == torch.int64 and x.dtype.kind not in "iu":
            raise ValueError("graph_from_edges: %s must be integers, not %s" % (what, x.dtype))
        return torch.from_numpy(np.ascontiguousarray(x)).to(device=device, dtype=dtype).contiguous().view(-1)
    rowptr, col, max_deg, pay = ops.edges_to_csr(
        dev(src, torch.int64, "node ids"), dev(dst, torch.int64, "node ids"), n_nodes, sel=dev(sel, torch.bool, "sel"),
        weight=dev(weight, torch.float32, "weight"), time=dev(time, torch.int64, "edge times"), directed=directed,
        order=order, duplicates=duplicates)
    csr = DeviceCSR(rowptr, col, int(n_nodes) + 1, max_deg)
    if weight is not None:
        csr.with_weights(pay)                               # (validates: finite and >= 0)
        return WeightedAdj(csr.to_scipy(), pay.cpu().numpy())
    if time is not None:
        csr.with_times(pay)                                 # (validates: below INT64_MAX, rows in time order)
        return TemporalAdj(csr.to_scipy(), pay.cpu().numpy(), node_time=node_time)
    return csr.to_scipy()


class DenseAdj(object):
    """The dense adjacency of the reference's default sampler (UniformNeighborSampler, nn_modules.py:19-49): an
    int64 [n_rows, K] table in HBM, every row pre-sampled to exactly K neighbours by the converter
    (utils/convert.py:71-98; ids 0-based, the dummy node is the LAST row).  Quacks like DeviceCSR where the fused
    engines need it (n_rows, max_deg = K, err_flag, check())."""

    def __init__(self, adj):
        assert torch.is_tensor(adj) and adj.dim() == 2 and adj.dtype == torch.int64, \
            "UniformNeighborSampler: adj must be a LongTensor [n_nodes + 1, K]"
        self.adj = adj.contiguous()
        self.n_rows, self.K = int(adj.shape[0]), int(adj.shape[1])
        self.max_deg = self.K
        self.err_flag = torch.zeros(1, dtype=torch.int32, device=adj.device)

    @property
    def device(self):
        return self.adj.device

    def check(self):
        """Raise IndexError if a kernel saw an id outside the table (synchronises)."""
        if self.adj.is_cuda and int(self.err_flag.item()) != 0:
            self.err_flag.zero_()
            raise IndexError("sampler: node id out of range of the adjacency")


class FeatureStore(object):
    """Device-resident node-feature table.  Quacks enough like the reference's `problem.feats`
    tensor for models.py / train.py: `.shape`, `.size()`, `feats[ids]`, `.is_cuda`."""

    def __init__(self, data, dim, scale=None):
        assert data.dim() == 2 and data.is_contiguous()
        assert (data.dtype == FP8) == (scale is not None), "an FP8 store, and only an FP8 store, carries column scales"
        if int(data.shape[0]) >= 2 ** 31:            # the gather kernels read the low 32-bit word of a node id
            raise ValueError("FeatureStore: %d rows; node ids must stay below 2^31 (include/gsage.h, gsage_gather_mean)"
                             % int(data.shape[0]))
        self.data = data               # [n_rows, ld]
        self.dim = int(dim)            # logical D (columns [D, ld) are zero)
        self.scale = scale             # FP8 only: fp32 [ld], powers of two (1.0 in the pad columns)

    @staticmethod
    def from_array(feats, device, dtype="bf16"):
        feats = torch.as_tensor(np.asarray(feats) if not torch.is_tensor(feats) else feats)
        n_rows, dim = feats.shape
        tdt = _DTYPES[dtype]
        if tdt == FP8:
            # (quantised where the result lives: the device's kernel, or the host mode for a CPU store)
            return FeatureStore.wrap(feats.to(device=device, dtype=torch.float32)).quantize()
        ld = _ld_for(dim, tdt)
        data = torch.zeros(n_rows, ld, dtype=tdt, device=device)
        data[:, :dim] = feats.to(device=device, dtype=torch.float32).to(tdt)
        return FeatureStore(data, dim)

    def quantize(self):
        """An FP8 store of this bf16 / fp32 store's values (gsage_quantize_fp8 on the GPU, quantize_fp8_host
        on the CPU: the same bytes and scales)."""
        if self.is_fp8:
            return self
        from . import ops
        q, scale = ops.quantize_fp8(self.data, self.dim, _ld_for(self.dim, FP8))
        return FeatureStore(q, self.dim, scale)

    @property
    def is_fp8(self):
        return self.data.dtype == FP8

    def nbytes(self):
        """Bytes of HBM (or host memory) the table occupies, scales included."""
        n = self.data.numel() * self.data.element_size()
        return n + (self.scale.numel() * 4 if self.scale is not None else 0)

    @staticmethod
    def synthetic(n_rows, dim, device, dtype="bf16", seed=0, chunk=1 << 23):
        """N(0, 1) rows generated on the device in chunks (a 111 M x 128 bf16 table is 28 GB; its fp32 staging copy
        would be twice that); row 0 (the dummy node) is zero."""
        assert dtype in ("bf16", "fp32"), "synthetic: bf16 or fp32 (then .quantize() for FP8)"
        tdt = _DTYPES[dtype]
        ld = _ld_for(dim, tdt)
        data = torch.zeros(int(n_rows), ld, dtype=tdt, device=device)
        gen = torch.Generator(device=device).manual_seed(int(seed))
        for o in range(0, int(n_rows), chunk):
            n = min(chunk, int(n_rows) - o)
            data[o:o + n, :dim] = torch.randn(n, int(dim), device=device, generator=gen).to(tdt)
        data[0].zero_()
        return FeatureStore(data, dim)

    @staticmethod
    def wrap(t):
        """Zero-copy view of an existing [n_rows, D] fp32 / bf16 tensor (ld == D)."""
        assert t.dtype in (torch.bfloat16, torch.float32), "wrap: fp32 / bf16 tensors (FP8 bytes need their scales)"
        return FeatureStore(t.detach().contiguous(), t.shape[1])

    @property
    def shape(self):
        return (self.data.shape[0], self.dim)

    def size(self, d=None):
        return self.shape if d is None else self.shape[d]

    @property
    def ld(self):
        return int(self.data.shape[1])

    @property
    def is_cuda(self):
        return self.data.is_cuda

    @property
    def device(self):
        return self.data.device

    @property
    def dtype(self):
        return self.data.dtype

    def cuda(self):
        return FeatureStore(self.data.cuda(), self.dim, None if self.scale is None else self.scale.cuda())

    def __getitem__(self, ids):
        return RowRef(self, ids)

    def dense(self):
        """fp32 [n_rows, D] copy (tests / CPU mode); an FP8 store decodes (the row gather over all rows)."""
        if self.is_fp8:
            from . import ops
            return ops.gather_rows(self, torch.arange(self.data.shape[0], device=self.device))
        return self.data[:, :self.dim].float()

    def decoded(self, dtype="bf16", n_rows=None):
        """The bf16 (or fp32) store that holds the decoded values of this FP8 store (of its first n_rows rows)
        exactly: every e4m3 value times a power of two is a bf16 number.  What full-neighbourhood inference reads
        as level 0, and what the FP8 paths are compared against."""
        assert self.is_fp8 and dtype in ("bf16", "fp32")
        from . import ops
        tdt = _DTYPES[dtype]
        ld = _ld_for(self.dim, tdt)
        rows = torch.arange(self.data.shape[0] if n_rows is None else int(n_rows), device=self.device)
        data = ops._gather_mean_fp8_raw(self.data, self.scale, self.dim, rows, int(rows.shape[0]), 1, tdt, ld)
        return FeatureStore(data, self.dim)


class RowRef(object):
    """`store[ids]`: rows of a FeatureStore selected by a LongTensor, not yet gathered."""

    def __init__(self, store, ids):
        self.store = store
        self.ids = ids.contiguous().view(-1)

    @property
    def shape(self):
        return (int(self.ids.shape[0]), self.store.dim)

    def size(self, d=None):
        return self.shape if d is None else self.shape[d]

    @property
    def is_cuda(self):
        return self.store.is_cuda

    @property
    def device(self):
        return self.store.device

    def materialize(self, dtype=torch.float32):
        """The reference's `feats[ids]` as a real [M, D] tensor (one gather kernel)."""
        from . import ops
        return ops.gather_rows(self.store, self.ids, out_dtype=dtype)
