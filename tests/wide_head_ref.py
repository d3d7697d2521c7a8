"""float64 numpy restatement of gsage_head_wide's contract (include/gsage.h), with n_valid:

    z = E / max(||E||_2, 1e-12);  logits = z W^T + b
    classification:  l_i = logsumexp(logits_i) - logits_i[y_i]
    multilabel:      l_i = (1/C) sum_c softplus(logits_ic) - y_ic logits_ic,  softplus(x) = max(x, 0) + log1p(exp(-|x|))
    loss = (1/bv) sum_{i < bv} l_i;  G = d loss / d logits (zero rows past bv);  dz = G W
    dE_i = (dz_i - z_i <z_i, dz_i>) / max(||E_i||, 1e-12);  dW = G^T z;  db = column sums of G

It is the reference's head (F.normalize -> fc -> F.cross_entropy / F.multilabel_soft_margin_loss) on the live rows alone;
tests/test_wide_head_host.py holds it against float64 autograd."""
import numpy as np

TASKS = ("classification", "multilabel_classification")
# the GPU test's shapes (B, C, D) and what each exercises
SHAPES = [
    (33, 121, 256),      # a partial last row tile, PPI's class count
    (5, 128, 600),       # fewer rows than one tile, every class lane full, D neither a slab multiple nor fitting the LDS
    (16, 65, 32),        # one class past two tiles, one k-slab
    (100, 3, 1024),      # the widest D, almost all class lanes masked
    (2, 2, 8),           # the smallest allowed shape
    (512, 121, 256),     # the shape of the workload
]


def make_case(B, C, D, task, seed=0):
    """E normal, W normal x 0.3, b normal (the scales of test_head_ce_forward_backward_vs_torch); class ids uniform,
    multilabel targets random bits."""
    rng = np.random.RandomState(1000 * seed + 7 * B + 3 * C + D)
    E = rng.normal(size=(B, D)).astype(np.float32)
    W = (rng.normal(size=(C, D)) * 0.3).astype(np.float32)
    b = rng.normal(size=(C,)).astype(np.float32)
    if task == "classification":
        y = rng.randint(0, C, size=(B,)).astype(np.int64)
    else:
        y = rng.randint(0, 2, size=(B, C)).astype(np.float32)
    return dict(E=E, W=W, b=b, y=y, task=task, B=B, C=C, D=D)


def reference(E, W, b, y, task, n_valid=None):
    """-> dict(preds [B, C], loss, dE [B, D], dW [C, D], db [C], rows [bv] = the l_i), all float64."""
    E, W, b = (np.asarray(t, dtype=np.float64) for t in (E, W, b))
    B, D = E.shape
    C = W.shape[0]
    bv = B if n_valid is None else int(n_valid)
    assert 1 <= bv <= B
    nrm = np.maximum(np.sqrt((E * E).sum(axis=1, keepdims=True)), 1e-12)
    z = E / nrm
    logits = z @ W.T + b
    G = np.zeros((B, C))
    x = logits[:bv]
    if task == "classification":
        y = np.asarray(y).reshape(-1)[:bv]
        m = x.max(axis=1, keepdims=True)
        lse = m[:, 0] + np.log(np.exp(x - m).sum(axis=1))
        rows = lse - x[np.arange(bv), y]
        P = np.exp(x - lse[:, None])
        P[np.arange(bv), y] -= 1.0
        G[:bv] = P / bv
    else:
        yy = np.asarray(y, dtype=np.float64)[:bv, :C]
        t = np.exp(-np.abs(x))
        rows = (np.maximum(x, 0.0) + np.log1p(t) - yy * x).sum(axis=1) / C
        sig = np.where(x >= 0, 1.0, t) / (1.0 + t)
        G[:bv] = (sig - yy) / C / bv
    dz = G @ W
    dE = (dz - z * (z * dz).sum(axis=1, keepdims=True)) / nrm
    return dict(preds=logits, loss=float(rows.sum() / bv), dE=dE, dW=G.T @ z, db=G.sum(axis=0), rows=rows)


_CACHE = {}


def case_reference(B, C, D, task, n_valid=None):
    """the float64 reference of make_case(B, C, D, task), computed once per session (read-only)"""
    key = (B, C, D, task, n_valid)
    if key not in _CACHE:
        c = make_case(B, C, D, task)
        ref = reference(c["E"], c["W"], c["b"], c["y"], task, n_valid)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = (c, ref)
    return _CACHE[key]
