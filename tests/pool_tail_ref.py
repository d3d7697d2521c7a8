"""Plain numpy restatements (int64 / float64) of what the pool engines' backward rests on: K3's outputs for backward
(gsage_pool_mlp / gsage_pool_mlp_packed: pooled, argmax, the ReLU sign words) and the five operations that consume
them (gsage_pool_route_bwd, gsage_pool_route_mean_bwd with its bias partials, gsage_pool_bias_partials,
gsage_pool_merge_bwd, gsage_attn_merge_bwd / _bwd2), written from include/gsage.h and the autograd they replace
(nn_modules.py:224-230, 240, 252).  Nothing here imports the product: the GPU tests (test_gpu_pool_tail.py) and the host
tests (test_pool_tail_host.py) both compare against this file.  bf16 bits come from update_tail_ref."""
import collections

import numpy as np

LIMIT = 2 ** 24              # |integer| below this: exact in float32 under any summation order


# ---- K3 on integer operands --------------------------------------------------------------------------------------
def first_argmax(hid):
    """[M, n, H] -> [M, H]: the row of the FIRST maximum of every (segment, channel), by a literal scan"""
    hid = np.asarray(hid)
    best = hid[:, 0].copy()
    arg = np.zeros(best.shape, dtype=np.int32)
    for r in range(1, hid.shape[1]):
        take = hid[:, r] > best
        best = np.where(take, hid[:, r], best)
        arg = np.where(take, np.int32(r), arg)
    return arg


def mask_words(pre):
    """[rows, H] pre-activations (H % 32 == 0) -> [rows, H / 32] uint32: bit c % 32 of word c / 32 of row r is set iff
    pre[r, c] > 0"""
    pre = np.asarray(pre)
    rows, H = pre.shape
    assert H % 32 == 0
    bits = (pre > 0).reshape(rows, H // 32, 32).astype(np.uint64)
    return (bits << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def mask_bits(words, H):
    """the inverse: [rows, H / 32] uint32 -> [rows, H] bool"""
    words = np.asarray(words, dtype=np.uint32)
    return ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(words.shape[0], -1)[:, :H]


def k3_exact(A_int, ids, W_int, b_int, M, n, mode):
    """pre = A[ids] @ W.T + b in int64; hid = max(pre, 0); pooled = max over the segment (int64) or sum / n (float64);
    argmax = the first maximum; mask = sign words (None unless H % 32 == 0).  mode: `max` | `mean`"""
    A = np.asarray(A_int, dtype=np.int64)[np.asarray(ids, dtype=np.int64)]
    W = np.asarray(W_int, dtype=np.int64)
    # (float64 products and sums of integers below 2^53 are exact, and BLAS is quicker than numpy's integer matmul)
    pre = np.rint(A.astype(np.float64) @ W.T.astype(np.float64)).astype(np.int64) + np.asarray(b_int, dtype=np.int64)
    assert pre.shape == (M * n, W.shape[0]) and int(np.abs(pre).max()) < LIMIT
    hid = np.maximum(pre, 0).reshape(M, n, -1)
    H = W.shape[0]
    out = dict(pre=pre, hid=hid, argmax=first_argmax(hid), mask=mask_words(pre) if H % 32 == 0 else None)
    assert mode in ("max", "mean")
    out["pooled"] = hid.max(axis=1) if mode == "max" else hid.sum(axis=1).astype(np.float64) / n
    return out


K3Case = collections.namedtuple("K3Case", "name M n K H a w b seed")   # a, w, b: entries in [-a, a], [-w, w], [-b, b]


def k3_inputs(case, table_rows=48):
    """-> (table [table_rows, K] int64, ids [M * n] int64, W [H, K] int64, bias [H] int64) of a case.  Row 0 of the
    table is zero (the project's padding row), and with n > 1 every segment holds one neighbour id twice (sampling
    with replacement): bit-identical hidden rows, so a tie wherever that neighbour wins."""
    rng = np.random.RandomState(case.seed)
    M, n, K, H = case.M, case.n, case.K, case.H
    table = rng.randint(-case.a, case.a + 1, size=(table_rows, K)).astype(np.int64)
    table[0] = 0
    W = rng.randint(-case.w, case.w + 1, size=(H, K)).astype(np.int64)
    b = rng.randint(-case.b, case.b + 1, size=H).astype(np.int64)
    ids = rng.randint(0, table_rows, size=(M, n)).astype(np.int64)
    if n > 1:
        for i in range(M):
            j1, j2 = sorted(rng.choice(n, size=2, replace=False))
            ids[i, j2] = ids[i, j1]
    ids = ids.reshape(-1)
    bound = case.a * case.w * K + case.b
    pre = table[ids] @ W.T + b
    assert bound < LIMIT and int(np.abs(pre).max()) < LIMIT, case.name
    return table, ids, W, b


def k3_census(ref, n):
    """fractions the fixtures are held to: (segment, channel) cells whose POSITIVE maximum is reached by two or more
    rows; pre-activations that are exactly 0; cells whose argmax is not row 0"""
    hid = ref["hid"]
    mx = hid.max(axis=1)
    tied = ((hid == mx[:, None, :]).sum(axis=1) >= 2) & (mx > 0)
    return dict(tied=float(tied.mean()), zero=float((ref["pre"] == 0).mean()), not_row0=float((ref["argmax"] != 0).mean()))


# ---- the backward operations (float64; selects, never products with a 0 / 1 gate) ------------------------------
def route_max_gate(pooled, argmax, n):
    """[M, n, H] bool: row j of segment i receives channel c iff argmax[i, c] == j and pooled[i, c] > 0 -- an argmax
    outside [0, n) routes nothing, a NaN pooled neither"""
    on = np.asarray(pooled)[:, None, :] > 0
    hit = np.asarray(argmax)[:, None, :] == np.arange(n)[None, :, None]
    return on & hit


def route_max(g, pooled, argmax, n):
    """out[i * n + j, c] = g[i, c] where route_max_gate, else 0"""
    g = np.asarray(g, dtype=np.float64)
    M, H = g.shape
    return np.where(route_max_gate(pooled, argmax, n), g[:, None, :], 0.0).reshape(M * n, H)


def route_mean(g, bits, n):
    """out[i * n + j, c] = g[i, c] / n where bit (i * n + j, c) is set, else 0"""
    g = np.asarray(g, dtype=np.float64)
    M, H = g.shape
    return np.where(np.asarray(bits).reshape(M, n, H), g[:, None, :] / n, 0.0).reshape(M * n, H)


def bias_max(g, pooled):
    """-> (column sums of g * (pooled > 0), column sums of |g| * (pooled > 0))"""
    t = np.where(np.asarray(pooled) > 0, np.asarray(g, dtype=np.float64), 0.0)
    return t.sum(axis=0), np.abs(t).sum(axis=0)


def bias_mean(g, bits, n):
    """-> (column sums of route_mean, column sums of |g| cnt / n)"""
    t = route_mean(g, bits, n)
    return t.sum(axis=0), np.abs(t).sum(axis=0)


def pool_merge(Hprev, DX, r_x, DN, r0, R):
    """dH[m, c] = (Hprev[m, c] > 0) ? (m < r_x ? DX[m, c] : +0) [+ DN[m - r0, c] when m >= r0] : +0, the one addition
    in IEEE float32 -- so a row with DX only keeps DX's bits (-0 included), and a row with DN only holds 0 + DN.
    -> float32 [R, D]"""
    DX = np.asarray(DX, dtype=np.float32)
    DN = np.asarray(DN, dtype=np.float32)
    D = np.asarray(Hprev).shape[1]
    v = np.zeros((R, D), dtype=np.float32)
    v[:r_x] = DX[:r_x]
    with np.errstate(invalid="ignore"):
        v[r0:] = v[r0:] + DN[:R - r0]
    return np.where(np.asarray(Hprev)[:R] > 0, v, np.float32(0.0)).astype(np.float32)


def hop_of(R, off):
    """[R] the hop of every row of a frontier whose hop k starts at off[k]"""
    hop = np.zeros(R, dtype=np.int64)
    for k in range(1, len(off)):
        hop[off[k]:] = k
    return hop


def attn_merge(DATT, DX, r_x, DAGG, ws, H, off, fan, R):
    """dIn[m] = mask(m) * (DATT[m] + (m < r_x ? DX[m] : 0) + (hop(m) >= 1 ? w[m] * DAGG[parent(m)] : 0)), w = ws[m -
    off[1]] or, with ws None, 1 / fan[hop]; parent(m) = off[k - 1] + (m - off[k]) // fan[k]; mask = H > 0 or, with H
    None, 1.  DATT and DX may be None.  -> (value, |DATT| + |DX| + |w DAGG|) as float64 [R, D], the second the scale
    of the rounding bound"""
    DAGG = np.asarray(DAGG, dtype=np.float64)
    D = DAGG.shape[1]
    val = np.zeros((R, D))
    mag = np.zeros((R, D))
    with np.errstate(invalid="ignore"):
        if DATT is not None:
            val += np.asarray(DATT, dtype=np.float64)[:R]
            mag += np.abs(np.asarray(DATT, dtype=np.float64)[:R])
        if DX is not None:
            val[:r_x] += np.asarray(DX, dtype=np.float64)[:r_x]
            mag[:r_x] += np.abs(np.asarray(DX, dtype=np.float64)[:r_x])
        hop = hop_of(R, off)
        for k in range(1, len(off)):
            m = np.nonzero(hop == k)[0]
            if m.shape[0] == 0:
                continue
            parent = off[k - 1] + (m - off[k]) // int(fan[k])
            w = np.asarray(ws, dtype=np.float64)[m - off[1]] if ws is not None else np.full(m.shape[0], 1.0 / int(fan[k]))
            t = w[:, None] * DAGG[parent]
            val[m] += t
            mag[m] += np.abs(t)
    if H is not None:
        on = np.asarray(H)[:R] > 0
        val, mag = np.where(on, val, 0.0), np.where(on, mag, 0.0)
    return val, mag


# The K3 cases of test_gpu_pool_tail.py (test_pool_tail_host.py holds their fixtures to the census conditions).
# BM = 64 rows per tile: 64 // n segments per workgroup.
K3_CASES = [
    K3Case("n5-M13-K16-H130", 13, 5, 16, 130, 1, 1, 1, 1),        # 12 segments per tile: a second, one-segment tile
    K3Case("n10-M7-K70-H96", 7, 10, 70, 96, 1, 1, 2, 2),          # 6 per tile
    K3Case("n15-M3-K602-H64", 3, 15, 602, 64, 2, 1, 2, 3),        # M < 64 // n = 4
    K3Case("n20-M4-K16-H288", 4, 20, 16, 288, 1, 1, 1, 4),        # 3 per tile; 288 = 256 + 32
    K3Case("n25-M5-K70-H640", 5, 25, 70, 640, 1, 1, 2, 5),        # 2 per tile; 640 % 256 = 128
    K3Case("n7-M10-K1433-H96", 10, 7, 1433, 96, 3, 2, 2, 6),      # 9 per tile
    K3Case("n3-M22-K16-H288", 22, 3, 16, 288, 1, 1, 1, 7),        # 21 per tile
    K3Case("n1-M70-K70-H130", 70, 1, 70, 130, 1, 1, 2, 8),        # 64 per tile
    K3Case("n64-M2-K16-H96", 2, 64, 16, 96, 1, 1, 1, 9),          # one segment per tile
    K3Case("n10-M13-K602-H288", 13, 10, 602, 288, 1, 1, 2, 10),   # three tiles x two column blocks
]
