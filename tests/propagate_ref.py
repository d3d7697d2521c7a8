"""Float64 numpy restatement of graph propagation (the definitions of include/gsage.h "Graph propagation" and
propagate.py), written from the definitions: an explicit edge list with the empty-row and out-of-range rules spelt out,
no sparse matmul.  Also the planted-partition toy the propagation tests share."""
import numpy as np

AUTOSCALE_MAX = 1000.0


def edges(indptr, col, n):
    """(dst, src, n_bad): the stored edges row by row in stored order, an id outside [0, n) DROPPED (it contributes 0)
    and counted.  A row without edges simply has none: it sums to 0, it does not read the dummy."""
    indptr = np.asarray(indptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    dst = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr[:n + 1]))
    ok = (col >= 0) & (col < n)
    return dst[ok], col[ok], int((~ok).sum())


def scales(indptr, n, norm):
    deg = np.diff(np.asarray(indptr, dtype=np.int64)[:n + 1]).astype(np.float64)
    one = np.ones(n)
    with np.errstate(divide="ignore"):
        inv = np.where(deg > 0, 1.0 / deg, 0.0)
        isq = np.where(deg > 0, 1.0 / np.sqrt(deg), 0.0)
    return {"sym": (isq, isq), "row": (inv, one), "col": (one, inv)}[norm]


def row_sums(dst, src, n, y):
    """acc[v] = the sum of y[u] over the kept edges (v, u) of edges(), which lists them row by row: one segment of
    y[src] per row that HAS kept edges; every other row stays 0."""
    acc = np.zeros((n, y.shape[1]))
    counts = np.bincount(dst, minlength=n)
    has = counts > 0
    if has.any():
        first = (np.cumsum(counts) - counts)[has]
        acc[has] = np.add.reduceat(y[src], first, axis=0)
    return acc


def step(dst, src, n, y, base, a, b, alpha, beta, lo, hi):
    """(out, yout) of one step: y [n, C] is the pre-scaled iterate."""
    acc = row_sums(dst, src, n, y)
    out = alpha * (a[:, None] * acc)
    if base is not None:
        out = beta * base + out
    out = np.minimum(np.maximum(out, lo), hi)
    return out, b[:, None] * out


def propagate(indptr, col, x, iters, alpha, base=None, norm="sym", clamp=None, fixed=None):
    x = np.array(x, dtype=np.float64)
    n = x.shape[0]
    base = x.copy() if base is None else np.array(base, dtype=np.float64)
    if fixed is not None:
        ids, vals = fixed
        x[ids] = vals
        base[ids] = vals
    lo, hi = (-np.inf, np.inf) if clamp is None else clamp
    dst, src, _ = edges(indptr, col, n)
    a, b = scales(indptr, n, norm)
    y = b[:, None] * x
    for _ in range(iters):
        x, y = step(dst, src, n, y, base, a, b, alpha, 1.0 - alpha, lo, hi)
    return x


def label_rows(targets, task, C):
    t = np.asarray(targets)
    if task == "classification":
        Y = np.zeros((t.size, C))
        Y[np.arange(t.size), t.reshape(-1)] = 1.0
        return Y
    return t[:, :C].astype(np.float64)


def label_propagation(indptr, col, n, targets, nodes, C, task="classification", iters=50, alpha=0.8, norm="sym"):
    base = np.zeros((n, C))
    base[nodes] = label_rows(targets, task, C)
    return propagate(indptr, col, base, iters, alpha, norm=norm, clamp=(0.0, 1.0))


def correct_and_smooth(indptr, col, logits, targets, nodes, task, iters=(50, 50), alpha=(0.8, 0.8), norm="sym",
                       autoscale=True, scale=1.0):
    """{"Z", "E0", "E", "s", "Zr", "G"} in float64."""
    z = np.asarray(logits, dtype=np.float64)
    n, C = z.shape
    if task == "classification":
        e = np.exp(z - z.max(1, keepdims=True))
        Z = e / e.sum(1, keepdims=True)
    else:
        Z = 1.0 / (1.0 + np.exp(-z))
    Y = label_rows(targets, task, C)
    E0 = np.zeros((n, C))
    E0[nodes] = Y - Z[nodes]
    s = None
    if autoscale:
        E = propagate(indptr, col, E0, iters[0], alpha[0], norm=norm, clamp=(-1.0, 1.0))
        sigma = np.abs(E0[nodes]).sum(1).mean()
        with np.errstate(divide="ignore", invalid="ignore"):
            s = sigma / np.abs(E).sum(1)
        s_raw = s.copy()
        s = np.where(np.isfinite(s) & (s <= AUTOSCALE_MAX), s, 1.0)
        Zr = Z + s[:, None] * E
    else:
        E = propagate(indptr, col, E0, iters[0], alpha[0], norm=norm, clamp=(-1.0, 1.0), fixed=(nodes, E0[nodes]))
        s_raw = None
        Zr = Z + scale * E
    G0 = Zr.copy()
    G0[nodes] = Y
    G = propagate(indptr, col, G0, iters[1], alpha[1], norm=norm, clamp=(0.0, 1.0))
    return {"Z": Z, "E0": E0, "E": E, "s": s, "s_raw": s_raw, "Zr": Zr, "G": G}


def symmetrise(indptr, col, n):
    """The structure A + A^T of a CSR (ids inside [0, n)): every stored edge and its reverse, duplicates removed,
    columns ascending -> (indptr int64 [n + 1], col int32)."""
    dst, src, _ = edges(indptr, col, n)
    keys = np.unique(np.concatenate([dst * n + src, src * n + dst]))
    rows, cols = keys // n, keys % n
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=ptr[1:])
    return ptr, cols.astype(np.int32)


# --------------------------------------------------------------------------------------------
# the planted-partition toy
# --------------------------------------------------------------------------------------------
TOY_N, TOY_C = 1200, 5


def toy(seed, n=TOY_N, C=TOY_C, p_in=0.03, p_out=0.003, labelled=0.3, signal=0.45):
    """A planted-partition graph over rows 1..n (row 0: the empty dummy), C classes, every 7th node isolated, both
    directions of every edge stored; `labelled` of the nodes are the train fold, the rest the test fold; the base
    logits are deliberately noisy (unit Gaussian noise plus `signal` on the true class).
    -> dict(indptr, col, n_rows, labels [n_rows], train, test, logits [n_rows, C])"""
    rng = np.random.RandomState(seed)
    N = n + 1
    labels = rng.randint(0, C, size=N)
    same = labels[:, None] == labels[None, :]
    A = np.triu(rng.rand(N, N) < np.where(same, p_in, p_out), 1)
    A = A | A.T
    iso = np.zeros(N, dtype=bool)
    iso[0] = True
    iso[7::7] = True
    A[iso, :] = False
    A[:, iso] = False
    rows, cols = np.nonzero(A)
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=N), out=indptr[1:])
    perm = rng.permutation(np.arange(1, N))
    k = int(labelled * n)
    train, test = np.sort(perm[:k]), np.sort(perm[k:])
    logits = rng.normal(size=(N, C)) + signal * np.eye(C)[labels]
    return {"indptr": indptr, "col": cols.astype(np.int32), "n_rows": N, "labels": labels, "train": train, "test": test,
            "logits": logits.astype(np.float32)}


def accuracy(scores, labels, nodes):
    return float((np.asarray(scores)[nodes].argmax(1) == labels[nodes]).mean())


def toy_accuracies(t, cs, lp):
    """(base, corrected, smoothed, label propagation) test accuracies from a correct_and_smooth dict and LP scores"""
    return tuple(accuracy(s, t["labels"], t["test"]) for s in (t["logits"], cs["Zr"], cs["G"], lp))
