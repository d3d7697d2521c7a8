"""The definition of one k-means assignment-and-accumulate pass and of the update (include/gsage.h, "K-means over
embeddings") in numpy float64, the bounds a floating-point result is held to, and the inputs the GPU tests and the host
tests share.

    s[i, c] = sum_d X[ids[i], d] C~[c, d] + bias[c]   for c < k_live
    a[i]    = the c < k_live with the largest s[i, c]; among equal scores the smallest c
    d2[i]   = max(0, |x_i|^2 - 2 s[i, a[i]])
    sums[c] = sum over {i : a[i] == c} of X[ids[i], :],   counts[c] = |{i : a[i] == c}|
    inertia = sum_i d2[i],   changed = |{i : labels_in[i] != a[i]}|

Operands are first rounded the way the mode under test sees them (retrieve_ref.round_operand): X and the centroids RNE to
bf16 for "bf16", untouched fp32 for "fp32"; the bias stays fp32.
"""
import numpy as np

from retrieve_ref import round_operand

U = 2.0 ** -24                                    # unit round-off of fp32
MAX_AMBIGUOUS = 0.01                              # of a case's rows


def bias_of(Cn, mode):
    """-1/2 |c~|^2 as fp32, from float64."""
    Cr = round_operand(Cn, mode).astype(np.float64)
    return (-0.5 * (Cr * Cr).sum(axis=1)).astype(np.float32)


def reference(table, ids, Cn, bias, mode, k_live=None):
    """-> dict: X [n, D], Cr [K, D], s [n, k_live] in float64, the float64 arg-max a, eps [n, k_live] and the mask of
    AMBIGUOUS rows.

    eps(i, c) = 4 D u sum_d |x_id c~_cd| + 2 u |bias_c|: any order of fp32 accumulation of D products errs by at most
    D u sum_d |x_d c_d|; the factor 4 covers the rounded products of the fp32 mode and an accumulator that truncates
    (retrieve_ref's rule); the bias is exact and the sum with it is one rounding of a value <= |z| + |bias|.
    A row is ambiguous if another centroid's score lies within eps(i, best) + max_c eps(i, c) of its best: only then can
    two computed scores change places.  A centroid that is a bit-for-bit copy of the best one (and so has the best's score
    in ANY arithmetic that gives a score one order) is not another centroid: the tie rule decides, not round-off."""
    K, D = Cn.shape
    k_live = K if k_live is None else k_live
    X = round_operand(np.asarray(table)[:, :D], mode).astype(np.float64)[np.asarray(ids, dtype=np.int64)]
    Cr = round_operand(Cn, mode).astype(np.float64)[:k_live]
    b = np.asarray(bias, dtype=np.float64)[:k_live]
    s = X @ Cr.T + b
    n = X.shape[0]
    a = np.argmax(s, axis=1)                                           # the first of equal scores
    eps = 4.0 * D * U * (np.abs(X) @ np.abs(Cr).T) + 2.0 * U * np.abs(b)[None, :]
    best = s[np.arange(n), a]
    gap = eps[np.arange(n), a] + eps.max(axis=1)
    same = np.all(Cr[a][:, None, :] == Cr[None, :, :], axis=2) & (b[a][:, None] == b[None, :])   # [n, k_live]: copies of the best
    rival = np.where(same, -np.inf, s)
    ambiguous = rival.max(axis=1) >= best - gap if k_live > 1 else np.zeros(n, dtype=bool)
    return {"X": X, "Cr": Cr, "b": b, "s": s, "a": a, "eps": eps, "ambiguous": ambiguous, "mode": mode, "k_live": k_live,
            "K": K, "D": D}


def grid(n, splits):
    """(S, depth): the partial rows the library writes for (n, splits) and the longest chain of fp32 additions one
    element of the sums goes through -- the rows of a workgroup's range, then the S partial rows (probe_ref.grid)."""
    tiles = -(-n // 32)
    S = splits if splits > 0 else min(tiles, 256)
    return S, 32 * (-(-tiles // S)) + S


def from_labels(ref, labels, labels_in=None):
    """sums, counts, inertia, changed and dist in float64 formed FROM THE GIVEN LABELS (the device's), so that a
    permitted flip of an ambiguous row does not move them."""
    X, s, K = ref["X"], ref["s"], ref["K"]
    n = X.shape[0]
    a = np.asarray(labels, dtype=np.int64)
    sums = np.zeros((K, X.shape[1]))
    np.add.at(sums, a, X)
    asum = np.zeros_like(sums)
    np.add.at(asum, a, np.abs(X))
    d2 = np.maximum(0.0, (X * X).sum(axis=1) - 2.0 * s[np.arange(n), a])
    return {"sums": sums, "abs_sums": asum, "counts": np.bincount(a, minlength=K), "dist": d2, "inertia": d2.sum(),
            "changed": int((np.asarray(labels_in) != a).sum()) if labels_in is not None else 0}


def bounds(ref, labels, splits):
    """What |got - from_labels()| may be for a kernel that computes in fp32.  Every term is a count of roundings times
    the magnitude it acts on.

    sums.  The one-hot is exact, the products x * 1 are exact: only the additions round -- a chain of at most `depth`
    (grid()) fp32 additions, plus 4 for whatever reduces the partial rows:
        dsums(c, d) = (depth + 4) u sum_{i in c} |x_id|
    dist.  |x_i|^2 is an fp32 sum of D squares in some order: (D + 4) u |x_i|^2 with the rounded squares; the score is
    off by eps(i, a_i) and doubled exactly; the subtraction rounds a value <= |x_i|^2 + 2 |s|; max(0, .) is 1-Lipschitz:
        ddist(i) = (D + 4) u |x_i|^2 + 2 eps(i, a_i) + u (|x_i|^2 + 2 |s_i,a_i|)
    inertia.  The rows' errors add up, and the sum itself is a chain of at most depth + 4 additions of the d2:
        dinertia = sum_i ddist(i) + (depth + 4) u sum_i d2(i)
    counts and changed are integers below 2^24 in fp32: exact."""
    X, s, eps = ref["X"], ref["s"], ref["eps"]
    n, D = X.shape
    a = np.asarray(labels, dtype=np.int64)
    _, depth = grid(n, splits)
    fl = from_labels(ref, labels)
    x2 = (X * X).sum(axis=1)
    ddist = (D + 4.0) * U * x2 + 2.0 * eps[np.arange(n), a] + U * (x2 + 2.0 * np.abs(s[np.arange(n), a]))
    return {"sums": (depth + 4.0) * U * fl["abs_sums"], "dist": ddist,
            "inertia": float(ddist.sum() + (depth + 4.0) * U * fl["dist"].sum())}


def check_pass(got, ref, splits, labels_in=None, scale=1.0, what=""):
    """got = (sums, counts, inertia, changed, labels[, dist]) as numbers / arrays.  Asserts: every unambiguous row has
    the float64 arg-max; every label is below k_live; counts and changed exactly, sums, inertia and dist within `scale`
    times bounds() of the float64 values formed from got's labels.  The figures are printed first.  -> the excesses."""
    sums, counts, inertia, changed, labels = (np.asarray(v) for v in got[:5])
    n = ref["X"].shape[0]
    assert labels.shape == (n,) and labels.min() >= 0 and labels.max() < ref["k_live"], (what, labels.min(), labels.max())
    amb = ref["ambiguous"]
    assert amb.mean() <= MAX_AMBIGUOUS, (what, "ambiguous rows", int(amb.sum()), n)
    wrong = (labels != ref["a"]) & ~amb
    fl = from_labels(ref, labels, labels_in)
    bd = bounds(ref, labels, splits)
    r = {"sums": float((np.abs(sums.astype(np.float64) - fl["sums"]) / np.maximum(scale * bd["sums"], 1e-300)).max()),
         "inertia": abs(float(inertia) - fl["inertia"]) / max(scale * bd["inertia"], 1e-300)}
    if len(got) > 5:
        r["dist"] = float((np.abs(np.asarray(got[5], dtype=np.float64) - fl["dist"]) / np.maximum(scale * bd["dist"], 1e-300)).max())
    print("kmeans %s: ambiguous %d / %d, wrong labels %d, |got - ref| / bound: %s"
          % (what, int(amb.sum()), n, int(wrong.sum()), "  ".join("%s %.3f" % kv for kv in sorted(r.items()))))
    assert not wrong.any(), (what, np.flatnonzero(wrong)[:8])
    assert np.isfinite(sums).all() and np.isfinite(float(inertia)), what
    assert np.array_equal(counts.astype(np.int64), fl["counts"]), what
    assert int(changed) == fl["changed"], (what, int(changed), fl["changed"])
    assert all(v <= 1.0 for v in r.values()), (what, r)
    return r


def update_reference(sums, counts, Cn, mode, spherical=False):
    """The update in float64 -> (centroids float64 [K, D], bias float64 [K], the number of empty clusters)."""
    C = np.array(Cn, dtype=np.float64)
    live = np.asarray(counts) > 0
    C[live] = np.asarray(sums, dtype=np.float64)[live] / np.asarray(counts, dtype=np.float64)[live][:, None]
    if spherical:
        C[live] /= np.linalg.norm(C[live], axis=1, keepdims=True)
    Cr = round_operand(C.astype(np.float32), mode).astype(np.float64)
    return C, (np.zeros(len(C)) if spherical else -0.5 * (Cr * Cr).sum(axis=1)), int((~live).sum())


def inertia_slack(n, D, splits=0):
    """How far the fp32 inertia of n rows with |x| <= 1 and centroids with |c| <= 1 may be from its exact value: the
    bound of bounds() with |x_i|^2 <= 1, sum_d |x_d c_d| <= 1, |bias| <= 1/2, |s| <= 3/2 and d2 <= 4."""
    _, depth = grid(n, splits)
    eps = 4.0 * D * U + U
    return n * ((D + 4.0) * U + 2.0 * eps + 4.0 * U) + (depth + 4.0) * U * 4.0 * n


# ---- shared data ------------------------------------------------------------------------------------------------------
# (n, D, K, splits): the smallest case; a tail tile and an odd D; an odd split count; two cluster tiles; the second slab
# and four cluster tiles; the widest D and K (D slabs, centroids read from global memory); more splits than tiles; a shape
# with a whole number of tiles per workgroup
CASES = [(1, 1, 1, 0), (33, 7, 2, 0), (257, 72, 31, 7), (1000, 72, 41, 0), (300, 264, 65, 0), (200, 1024, 128, 0),
         (500, 16, 128, 64), (4096, 256, 33, 0)]

_CASE = {}


def make_case(n, D, K, seed=0):
    """Inputs of one case (cached; nobody writes to them): K planted unit centres; N = 2 n + 3 table rows = a centre
    plus 0.5 x normal / sqrt(D) per coordinate, normalised, inside a wider buffer whose padding columns hold NaN
    (ldx = D + 3); ids a random choice with duplicates; the centroids under test = the centres + 0.1 x normal / sqrt(D),
    and for K > 2 the LAST centroid an exact copy of centroid 0: no row may ever get label K - 1, the cluster stays
    empty."""
    key = (n, D, K, seed)
    if key in _CASE:
        return _CASE[key]
    rng = np.random.RandomState(1000 * seed + 7 * n + 3 * D + K)
    N = 2 * n + 3
    cen = rng.normal(size=(K, D))
    cen /= np.linalg.norm(cen, axis=1, keepdims=True)
    planted = rng.randint(0, K, size=N)
    rows = cen[planted] + 0.5 * rng.normal(size=(N, D)) / np.sqrt(D)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    buf = np.full((N, D + 3), np.nan, dtype=np.float32)
    buf[:, :D] = rows
    ids = rng.choice(N, size=n, replace=True).astype(np.int64)
    if n > 1:
        ids[-1] = ids[0]                                         # a duplicate for sure
    Cn = (cen + 0.1 * rng.normal(size=(K, D)) / np.sqrt(D)).astype(np.float32)
    if K > 2:
        Cn[K - 1] = Cn[0]
    case = {"buf": buf, "table": buf[:, :D], "ids": ids, "Cn": Cn, "planted": planted[ids], "n": n, "D": D, "K": K,
            "duplicate": K - 1 if K > 2 else None}
    _CASE[key] = case
    return case


_REFS = {}


def case_reference(n, D, K, mode, seed=0, k_live=None):
    key = (n, D, K, mode, seed, k_live)
    if key not in _REFS:
        c = make_case(n, D, K, seed)
        _REFS[key] = reference(c["table"], c["ids"], c["Cn"], bias_of(c["Cn"], mode), mode, k_live)
    return _REFS[key]


def blobs(seed, K=5, n=600, D=32, radius=0.01):
    """n rows of width D around K centres that are more than 100 radii apart: centre k = 2 e_k (pairwise distance
    2 sqrt(2) = 283 radii), a row = its centre plus a step of length `radius` in a uniform direction.
    -> (X fp32 [n, D], planted int64 [n]); every blob holds at least one row."""
    r = np.random.RandomState(100 + seed)
    k = np.concatenate([np.arange(K), r.randint(0, K, size=n - K)])
    r.shuffle(k)
    off = r.normal(size=(n, D))
    off *= radius / np.linalg.norm(off, axis=1, keepdims=True)
    X = 2.0 * np.eye(K, D)[k] + off
    return X.astype(np.float32), k.astype(np.int64)
