"""The definition of one linear-probe pass (include/gsage.h, "Linear probe over embeddings") in numpy float64, the bound
a floating-point result is held to, and the inputs the GPU tests and the host tests share.

    z[i, c] = sum_d X[ids[i], d] W~[c, d] + b[c]
    classification:             l_i = logsumexp_c z[i, .] - z[i, y_i],        G[i, c] = softmax(z_i)[c] - [c == y_i]
    multilabel_classification:  l_i = (1/C) sum_c (softplus(z) - y z)[i, c],  G[i, c] = (sigmoid(z[i, c]) - y[i, c]) / C
    loss = (1/n) sum_i l_i,   dW = (1/n) G^T X[ids],   db = (1/n) sum_i G[i, .]

Operands are first rounded the way the mode under test sees them (retrieve_ref.round_operand): X and W RNE to bf16 for
"bf16", untouched fp32 for "fp32"; the bias stays fp32.
"""
import numpy as np

from retrieve_ref import round_operand

U = 2.0 ** -24                                    # unit round-off of fp32
TASKS = ("classification", "multilabel_classification")


def reference(table, ids, targets, W, b, task, mode):
    """-> dict: loss (float), dW [C, D], db [C] in float64, and the intermediates the bound needs (X, Wr, z, G)."""
    assert task in TASKS
    C, D = W.shape
    X = round_operand(np.asarray(table)[:, :D], mode).astype(np.float64)[np.asarray(ids, dtype=np.int64)]
    Wr = round_operand(W, mode).astype(np.float64)
    z = X @ Wr.T + np.asarray(b, dtype=np.float64)
    n = X.shape[0]
    if task == "classification":
        y = np.asarray(targets, dtype=np.int64).reshape(-1)
        m = z.max(axis=1, keepdims=True)
        lse = m[:, 0] + np.log(np.exp(z - m).sum(axis=1))
        rows = lse - z[np.arange(n), y]
        G = np.exp(z - lse[:, None])
        G[np.arange(n), y] -= 1.0
    else:
        y = np.asarray(targets, dtype=np.float64)[:, :C]
        sp = np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))
        rows = (sp - y * z).sum(axis=1) / C
        G = (1.0 / (1.0 + np.exp(-z)) - y) / C
    return {"loss": float(rows.mean()), "dW": G.T @ X / n, "db": G.sum(axis=0) / n, "X": X, "Wr": Wr, "z": z, "G": G,
            "rows": rows, "y": y, "task": task, "mode": mode, "b": np.asarray(b, dtype=np.float64)}


def grid(n, splits):
    """(S, depth): the partial rows the library writes for (n, splits) and the longest chain of fp32 additions one
    gradient element goes through -- the rows of a workgroup's range, then the S partial rows."""
    tiles = -(-n // 32)
    S = splits if splits > 0 else min(tiles, 256)
    return S, 32 * (-(-tiles // S)) + S


def bounds(ref, splits):
    """What |got - ref| may be, element by element, for a kernel that computes in fp32 (u = 2^-24) with operands rounded
    as `ref` has them.  No tuned constant: every term is a count of roundings times the magnitude it acts on.

    Logits.  Any order of fp32 accumulation of D products errs by at most D u sum_d |x_d w_d| <= D u |x_i| |w_c|; the
    factor 4 covers the rounded products of the fp32 mode, an accumulator that truncates (retrieve_ref's rule) and
    the rounding of the sum with the bias, which itself is exact to u |b_c|:
        eps_z(i, c) = 4 D u |x_i| |w~_c| + u |b_c|
    G.  Softmax: sum_j |dp_c / dz_j| = 2 p_c (1 - p_c) <= 1/2, so an error of at most e_i = max_c eps_z(i, c) in every
    logit moves p_c by at most e_i / 2.  Its own arithmetic: expf of a rounded argument z - m (|z - m| <= 2 max|z|, so
    u max|z| after the factor 1/2), expf itself (<= 2 ulp), a sum of C <= 128 terms as a 5-level tree plus 4 tiles
    plus the fold (<= 12 roundings), one division, one product, one subtraction: 32 roundings of a value <= 1.
        dG_cls(i, c) = max_c eps_z(i, c) / 2 + (32 + max_c |z_ic|) u
    Sigmoid: |s'| <= 1/4; expf, 1 + t, a division, the subtraction of y and the product with 1 / C: 8 roundings.
        dG_ml(i, c) = (eps_z(i, c) / 4 + 8 u) / C
    dW, db.  The error of G propagates through the sum, and the sum itself -- a chain of at most `depth` fp32
    additions (grid()), plus 4 for the product and the scaling by 1 / n -- errs by (depth + 4) u times the sum of the
    magnitudes.  In bf16 mode G enters as hi + lo, two bf16: the pair is G (1 + 2^-17) at worst.
        ddW(c, d) = (1/n) sum_i |x_id| dG(i, c) + ((depth + 4) u + [bf16] 2^-17) (1/n) sum_i |x_id| |G_ic|
        ddb(c)    = (1/n) sum_i dG(i, c) + (depth + 4) u (1/n) sum_i |G_ic|
    Loss.  classification: l_i = (m + log s) - z_y: logsumexp moves by at most e_i, z_y by eps_z, and logf, expf, the
    tree and the additions are 32 roundings of values <= max|z| + log C.  multilabel: d softplus / dz = sigmoid <= 1
    and |y| <= 1, so a term moves by at most 2 eps_z, plus 8 roundings of values <= |z| + 1.  The row terms are then
    added lane by lane, wave by wave and split by split: depth + 64 + 4 additions of magnitudes t_i.
        dloss = (1/n) sum_i dl_i + (depth + 68) u (1/n) sum_i t_i
    -> dict(loss, dW, db)."""
    X, Wr, z, G, b = ref["X"], ref["Wr"], ref["z"], ref["G"], ref["b"]
    n, D = X.shape
    C = Wr.shape[0]
    S, depth = grid(n, splits)
    eps_z = 4.0 * D * U * np.linalg.norm(X, axis=1)[:, None] * np.linalg.norm(Wr, axis=1)[None, :] \
        + U * np.abs(b)[None, :]
    zmax = np.abs(z).max(axis=1)
    if ref["task"] == "classification":
        e = eps_z.max(axis=1)
        dG = np.repeat((e / 2.0 + (32.0 + zmax) * U)[:, None], C, axis=1)
        dl = 2.0 * e + 32.0 * U * (zmax + np.log(C))
        lse = ref["rows"] + z[np.arange(n), ref["y"]]
        t = np.abs(lse) + np.abs(z[np.arange(n), ref["y"]])
    else:
        dG = (eps_z / 4.0 + 8.0 * U) / C
        dl = (2.0 * eps_z + 8.0 * U * (np.abs(z) + 1.0)).sum(axis=1) / C
        t = (np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z))) + np.abs(ref["y"] * z)).sum(axis=1) / C
    chain = (depth + 4.0) * U
    pair = 2.0 ** -17 if ref["mode"] == "bf16" else 0.0
    aX, aG = np.abs(X), np.abs(G)
    return {"dW": (dG.T @ aX + (chain + pair) * (aG.T @ aX)) / n,
            "db": (dG.sum(axis=0) + chain * aG.sum(axis=0)) / n,
            "loss": float((dl.sum() + (depth + 68.0) * U * t.sum()) / n)}


def excess(got, ref, splits, scale=1.0):
    """max over loss, dW and db of |got - ref| / (scale * bound): <= 1 means `got` is within the bound.  got: (loss,
    dW, db) as numbers / arrays."""
    bd = bounds(ref, splits)
    loss, dW, db = (np.asarray(v, dtype=np.float64) for v in got)
    assert dW.shape == ref["dW"].shape and db.shape == ref["db"].shape
    assert np.isfinite(loss) and np.isfinite(dW).all() and np.isfinite(db).all(), "non-finite result"
    r = {"loss": abs(float(loss) - ref["loss"]) / (scale * bd["loss"]),
         "dW": float((np.abs(dW - ref["dW"]) / (scale * bd["dW"])).max()),
         "db": float((np.abs(db - ref["db"]) / (scale * bd["db"])).max())}
    return r


def compare(got, ref, splits, scale=1.0, what=""):
    """Assert that (loss, dW, db) lie within `scale` times bounds(); the figures are printed first."""
    r = excess(got, ref, splits, scale)
    print("probe %s: |got - ref| / bound: loss %.3f  dW %.3f  db %.3f" % (what, r["loss"], r["dW"], r["db"]))
    assert r["loss"] <= 1.0 and r["dW"] <= 1.0 and r["db"] <= 1.0, (what, r)
    return r


# ---- shared data ------------------------------------------------------------------------------------------------------
# (n, D, C, splits): one row; odd sizes inside one tile; several tiles with a library-chosen and an odd split count; D
# and C that are no multiples of 32 with a D wider than one slab; the four-class-tile shape of a PPI-like problem; the
# widest D and C (D slabs, W~ read from global memory); more splits than tiles
CASES = [(1, 8, 2, 1), (33, 20, 5, 1), (1000, 72, 41, 0), (1000, 72, 41, 7), (257, 264, 65, 3), (300, 256, 121, 0),
         (64, 1024, 128, 2), (40, 16, 128, 64)]

_CASE = {}


def make_case(n, D, C, task, seed=0):
    """Inputs of one case (cached; nobody writes to them): a table of N = 2 n + 3 rows inside a wider buffer whose
    padding columns hold NaN, row norms spread over a factor of 100, ids a shuffled subset with duplicates, targets in
    which class C // 2 never occurs (multilabel: inside a wider buffer padded with NaN), W and b random.
    The scale of the rows (norms 0.01 .. 1) and of W (|w_c| ~ 0.3) is what lets the bound tell a G rounded to ONE bf16
    from the hi + lo pair at D = 1024: eps_z grows with D |x| |w|, the 2^-9 of a bf16 does not."""
    key = (n, D, C, task, seed)
    if key in _CASE:
        return _CASE[key]
    rng = np.random.RandomState(1000 * seed + 7 * n + 3 * D + C)
    N = 2 * n + 3
    buf = np.full((N, D + 3), np.nan, dtype=np.float32)
    rows = rng.normal(size=(N, D)) / np.sqrt(D)
    buf[:, :D] = rows * 10.0 ** rng.uniform(-2.0, 0.0, size=(N, 1))   # row norms 0.01 .. 1
    ids = rng.choice(N, size=n, replace=True).astype(np.int64)
    if n > 1:
        ids[-1] = ids[0]                                         # a duplicate for sure
    missing = C // 2
    if task == "classification":
        y = rng.randint(0, C - 1, size=n).astype(np.int64)
        y[y >= missing] += 1
        y[0] = 0                                                 # class 0 occurs for sure
        ybuf = y
    else:
        ybuf = np.full((n, C + 2), np.nan, dtype=np.float32)
        ybuf[:, :C] = (rng.uniform(size=(n, C)) < 0.3).astype(np.float32)
        ybuf[:, missing] = 0.0
        ybuf[0, 0] = 1.0                                         # class 0 occurs for sure
        y = ybuf[:, :C]
    W = (rng.normal(size=(C, D)) * 0.3 / np.sqrt(D)).astype(np.float32)  # |w_c| ~ 0.3: see below
    b = rng.normal(size=C).astype(np.float32)
    case = {"buf": buf, "table": buf[:, :D], "ids": ids, "ybuf": ybuf, "y": y, "W": W, "b": b, "missing": missing,
            "n": n, "D": D, "C": C, "task": task}
    _CASE[key] = case
    return case


_REFS = {}


def case_reference(n, D, C, task, mode, seed=0):
    key = (n, D, C, task, mode, seed)
    if key not in _REFS:
        c = make_case(n, D, C, task, seed)
        _REFS[key] = reference(c["table"], c["ids"], c["y"], c["W"], c["b"], task, mode)
    return _REFS[key]


def toy(seed, K, multilabel):
    """600 unit rows of width 20: one of K random unit centres plus 0.08 x normal noise, renormalised.  Labels: the
    centre (classification) or the three bits of its index (multilabel, K = 8).  Fit on the first 400, score the
    last 200.  -> (X fp32 [600, 20], y)"""
    r = np.random.RandomState(seed)
    cen = r.normal(size=(K, 20))
    cen /= np.linalg.norm(cen, axis=1, keepdims=True)
    k = r.randint(0, K, size=600)
    X = cen[k] + 0.08 * r.normal(size=(600, 20))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    y = ((k[:, None] >> np.arange(3)) & 1).astype(np.float32) if multilabel else k.astype(np.int64)
    return X.astype(np.float32), y
