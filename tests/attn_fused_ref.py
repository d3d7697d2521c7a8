"""A staged float64 restatement, in plain numpy, of the fused attention hop (csrc/gsage_attn_fused.hip:
k_attn_fused_fwd / k_attn_fused_bwd -- K4 / K4' with the attention MLP inside; the definition is nn_modules.py:293-296,
305-321 and its autograd).  STAGED: every stage is computed from the inputs the kernel itself had at that stage (its own
hid bits for a, its own a for ws, its own ws for agg_lp, its own da bits for dhid), never from exact upstream values, so
rounding differences do not accumulate and every bound below is a count of the operations of ONE stage.  Nothing here
imports the product: the GPU tests (test_gpu_attn_fused.py) and the host tests (test_attn_fused_host.py) both compare
against this file.  bf16 bits come from update_tail_ref.

Notation: u = 2^-24 (one float32 rounding), BF16_U = 2^-8 (one bf16 rounding, 8 significant bits), cols = 32 KS (the
columns the kernel reads of a row: KS = 1, 2, 4, 8, 19, 20 k-steps of 32), n the fan-out, |.| taken element by element.
A sum of K terms in ANY order puts at most K - 1 roundings on a term (K when the products are rounded float32 products
rather than exact bf16 x bf16 ones); (1 + u)^K - 1 <= (K + 1) u for K <= 640.  The constants c of the bounds:

  C_DOT = 2     K products summed: K + 2 covers K roundings per term and the second-order term (hid: cols exact products
                on the matrix cores; a, dhid: 32 exact products; the score: 32 rounded products; agg_lp: the n high-part
                products, the n low-part products -- 2^-8 of the sum, n 2^-8 <= 1/16 of a unit -- and the addition of the
                two partial sums; dxa and the softmax backward's dot: n rounded products)
  C_DWS = 6     the dot product with d agg: cols - 1 additions of the high parts, cols - 1 of the low parts at 2^-8 of the
                magnitude (<= 2.5 units at cols = 640), the addition of the two accumulators, the second-order term, and
                one unit that carries the second rounding of ds = w (dws - dot) (see ds_stage)
  T = 6 u       the absolute error of the kernel's tanh(v) = 1 - 2 / (exp(2 |v|) + 1) on v_exp_f32 / v_rcp_f32 at 1 ulp
                (= 2 u relative) each: with e = exp(2 |v|), r = 2 / (e + 1) <= 1 and t = 1 - r, the relative error of e is
                2 u (v_exp_f32) + 4 |v| u (the rounded product 2 |v| log2(e) in its argument), that of r is
                e / (e + 1) times as much + u (the addition) + 2 u (v_rcp_f32), and |dt| <= r d_r + u |t| (the
                subtraction) <= 2 e / (e + 1)^2 (2 u + 4 |v| u) + 3 u r + u <= (1/2) 2 u + 0.9 u + 3 u + u = 5.9 u, since
                2 e / (e + 1)^2 <= 1/2 and 8 |v| e / (e + 1)^2 = 2 |v| (1 - tanh^2 v) <= 0.9.  The form cancels for small
                |v|: the error is ABSOLUTE (relative error ~ 1 below |v| = 1e-5), a property of the kernel that is
                documented here and measured by the tiny-pre-activation case, not a defect
  softmax       expf within 2 ulp (4 u, part of the exponent's error), the sum of n <= 16 positive terms (n - 1 roundings),
                a division within 2.5 ulp (5 u), one unit of second order: w ((n - 1) + 5 + 1) u on top of the propagated
                score error; 2^-125 absolute for weights in the denormal range
  SPLIT = 2^-16 a float32 f as bf16 high and low parts: hi = bf16(f), lo = bf16(f - hi), |f - hi - lo| <= 2^-8 |f - hi| <=
                2^-16 |f| (the weights in agg_lp, d agg in dws)
"""
import collections
import zlib

import numpy as np

from update_tail_ref import bf16_rne, bf16_value

U = 2.0 ** -24
BF16_U = 2.0 ** -8
SPLIT = 2.0 ** -16
C_DOT = 2
C_DWS = 6
T_TANH = 6 * U
SOFTMAX_EXP = 4 * U                # expf within 2 ulp
SOFTMAX_DIV = 5 * U                # the division within 2.5 ulp
TINY = 2.0 ** -126                 # the smallest normal float32 / bf16
KSTEPS = (1, 2, 4, 8, 19, 20)
HA = 32                            # the attention MLP's width


def ksteps(D, ld=None):
    """k-steps of 32 columns the kernels run for rows of D columns (0: not covered), as af_ksteps / gsage_attn_fused_ok"""
    ks = -(-D // 32)
    for k in KSTEPS:
        if ks <= k:
            return k if ld is None or 32 * k <= ld else 0
    return 0


def cols_of(D):
    return 32 * ksteps(D)


def f64(bits):
    return bf16_value(bits).astype(np.float64)


# ---- the stages' values (float64; the host test holds them to autograd) --------------------------------------------
def hid_value(X, W0):
    return np.tanh(X @ W0.T)


def a_value(hid, W2):
    return hid @ W2.T


def ws_value(a, xa, M, n):
    s = np.einsum("mjh,mh->mj", a.reshape(M, n, HA), xa)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).reshape(M * n)


def agg_value(ws, X, M, n):
    return np.einsum("mj,mjc->mc", ws.reshape(M, n), X.reshape(M, n, -1))


def dws_value(X, g, M, n):
    return np.einsum("mjc,mc->mj", X.reshape(M, n, -1), g).reshape(M * n)


def ds_value(ws, dws, M, n):
    w, d = ws.reshape(M, n), dws.reshape(M, n)
    return (w * (d - (w * d).sum(axis=1, keepdims=True))).reshape(M * n)


def dxa_value(ds, na, M, n):
    return np.einsum("mj,mjh->mh", ds.reshape(M, n), na.reshape(M, n, HA))


def da_value(ds, xa, M, n):
    return (ds.reshape(M, n, 1) * xa[:, None, :]).reshape(M * n, HA)


def dhid_value(da, W2, hid):
    return (da @ W2) * (1.0 - hid * hid)


# ---- check ---------------------------------------------------------------------------------------------------------
def check(stage, got, want, bound, note=None):
    """EVERY element: |got - want| <= bound (a zero bound: equal).  -> the worst error / bound, asserted <= 1"""
    got, want, bound = (np.asarray(x, dtype=np.float64) for x in (got, want, bound))
    assert got.shape == want.shape == bound.shape, (stage, got.shape, want.shape, bound.shape)
    assert np.isfinite(want).all() and np.isfinite(bound).all() and (bound >= 0).all(), (stage, "the reference")
    assert np.isfinite(got).all(), (stage, "%d non-finite elements" % int((~np.isfinite(got)).sum()))
    err = np.abs(got - want)
    exact = bound == 0
    assert not err[exact].any(), (stage, "elements with a zero bound must be exact")
    ratio = float((err[~exact] / bound[~exact]).max()) if (~exact).any() else 0.0
    print(stage, "worst error / bound = %.4f" % ratio)
    if note is not None:
        note(stage, ratio=ratio)
    if ratio > 1.0:
        i = np.unravel_index(int(np.argmax(np.where(exact, 0.0, err / np.where(exact, 1.0, bound)))), err.shape)
        raise AssertionError((stage, "error / bound = %.4f at %s: got %.9g, want %.9g, bound %.3g"
                              % (ratio, i, got[i], want[i], bound[i])))
    return ratio


def _bf16_out(want, err32):
    """the bound of a bf16 output: the float32 result's error and the rounding of that result"""
    return err32 + BF16_U * (np.abs(want) + err32)


# ---- the stages' references and bounds -----------------------------------------------------------------------------
def hid_stage(x_bits, w0_bits):
    """-> (tanh(pre64), bound, pre64): bf16 rounding of the result + (1 - tanh^2) (cols + c) u sum |w x| + T; the slope
    1 - tanh^2 is taken at the end of the pre-activation's error interval nearest 0, where it is largest"""
    X, W0 = f64(x_bits), f64(w0_bits)
    cols = X.shape[1]
    pre = X @ W0.T
    e_pre = (cols + C_DOT) * U * (np.abs(X) @ np.abs(W0).T)
    slope = 1.0 - np.tanh(np.maximum(np.abs(pre) - e_pre, 0.0)) ** 2
    want = np.tanh(pre)
    return want, _bf16_out(want, slope * e_pre + T_TANH), pre


def a_stage(hid_bits, w2_bits):
    hid, W2 = f64(hid_bits), f64(w2_bits)
    return a_value(hid, W2), (HA + C_DOT) * U * (np.abs(hid) @ np.abs(W2).T)


def ws_stage(a32, xa32, M, n):
    """from the kernel's own a.  The score's error e_k = (32 + c) u sum |a xa| + u |s_k - max| (the subtraction) + the
    exponential's 4 u moves the exponent; an exact softmax of scores off by at most e_k is 1 / (1 + R') with
    R' = sum_{k != j} (w_k / w_j) exp(d_k - d_j), so |w' - w| <= w q / (1 - q), q = sum_{k != j} w_k expm1(e_k + e_j)
    (first order: w (2 e + ...) for uniform e); then the sum and the division.  -> (w, bound, s - max)"""
    a, xa = np.asarray(a32, dtype=np.float64).reshape(M, n, HA), np.asarray(xa32, dtype=np.float64)
    s = np.einsum("mjh,mh->mj", a, xa)
    sm = s - s.max(axis=1, keepdims=True)
    ex = np.exp(sm)
    w = ex / ex.sum(axis=1, keepdims=True)
    e = (HA + C_DOT) * U * np.einsum("mjh,mh->mj", np.abs(a), np.abs(xa)) + U * np.abs(sm) + SOFTMAX_EXP
    # q_j = sum_{k != j} w_k expm1(e_k + e_j)
    pair = np.expm1(np.minimum(e[:, :, None] + e[:, None, :], 50.0))             # [m, j, k]
    pair[:, np.arange(n), np.arange(n)] = 0.0
    q = np.minimum(np.einsum("mjk,mk->mj", pair, w), 0.5)
    bound = w * q / (1.0 - q) + w * ((n - 1) * U + SOFTMAX_DIV + U) + 2 * TINY
    return w.reshape(M * n), bound.reshape(M * n), sm.reshape(M * n)


def agg_stage(ws32, x_bits, M, n):
    """from the kernel's own ws: bf16 rounding of the result + (2^-16 + (n + c) u) sum_j |w_j x_j| (+ the weights'
    denormal range)"""
    w, X = np.asarray(ws32, dtype=np.float64).reshape(M, n), f64(x_bits).reshape(M, n, -1)
    want = np.matmul(w[:, None, :], X)[:, 0]
    mag = np.matmul(np.abs(w)[:, None, :], np.abs(X))[:, 0]
    err32 = (SPLIT + (n + C_DOT) * U) * mag + n * TINY * np.abs(X).max(axis=1)
    return want, _bf16_out(want, err32)


def dws_stage(x_bits, g32, M, n):
    """-> (dws, dws_err): (2^-16 + (cols + c) u) sum |x g|.  (Finite junk in g's columns [D, cols) meets the rows' zero
    pads: 0 * junk = 0 exactly, here as in the kernel.)"""
    X, g = f64(x_bits).reshape(M, n, -1), np.asarray(g32, dtype=np.float64)
    cols = X.shape[2]
    want = np.matmul(X, g[:, :, None])[:, :, 0]
    mag = np.matmul(np.abs(X), np.abs(g)[:, :, None])[:, :, 0]
    return want.reshape(M * n), ((SPLIT + (cols + C_DWS) * U) * mag).reshape(M * n)


def ds_stage(ws32, dws, dws_err, M, n):
    """ds_err = w (dws_err + sum_j w_j dws_err_j + (n + c) u sum |w dws|) + u |ds|.  (ds takes two roundings, the
    subtraction's and the product's: the second, u |ds| <= u w |dws| + u w sum |w dws|, is the unit C_DWS and the
    n + c below already carry.)  A weight in the denormal range may be flushed or lose bits: 2^-126 (2 + |dws - dot|)."""
    w, d, de = (np.asarray(x, dtype=np.float64).reshape(M, n) for x in (ws32, dws, dws_err))
    dot = (w * d).sum(axis=1, keepdims=True)
    ds = w * (d - dot)
    err = w * (de + (w * de).sum(axis=1, keepdims=True) + (n + C_DOT + 1) * U * np.abs(w * d).sum(axis=1, keepdims=True)) + \
        U * np.abs(ds) + TINY * (2 + np.abs(d - dot))
    return ds.reshape(M * n), err.reshape(M * n)


def dxa_stage(ds, ds_err, na32, M, n):
    na = np.asarray(na32, dtype=np.float64).reshape(M, n, HA)
    ds, ds_err = ds.reshape(M, n), ds_err.reshape(M, n)
    want = np.einsum("mj,mjh->mh", ds, na)
    bound = np.einsum("mj,mjh->mh", ds_err, np.abs(na)) + (n + C_DOT) * U * np.einsum("mj,mjh->mh", np.abs(ds), np.abs(na))
    return want, bound + n * TINY                                                 # (products in the denormal range)


def da_stage(ds, ds_err, xa32, M, n):
    """bf16 rounding of the result + |xa| ds_err (+ the float32 product's own rounding)"""
    xa = np.asarray(xa32, dtype=np.float64)
    want = da_value(ds, xa, M, n)
    err32 = da_value(ds_err, np.abs(xa), M, n) + U * np.abs(want) + TINY            # (+ a result in the denormal range)
    return want, _bf16_out(want, err32)


def dhid_stage(da_bits, w2_bits, hid_bits):
    """from the kernel's own da bits and the given hid: bf16 rounding of the result + (32 + c) u sum |w2 da| (1 - hid^2)
    + the roundings of 1 - hid^2 (hid^2 is exact: 16 significant bits) and of the product"""
    da, W2, hid = f64(da_bits), f64(w2_bits), f64(hid_bits)
    fac = 1.0 - hid * hid
    dhg = da @ W2
    want = dhg * fac
    err32 = (HA + C_DOT) * U * (np.abs(da) @ np.abs(W2)) * fac + 2 * U * np.abs(want)
    return want, _bf16_out(want, err32 + TINY * (1 + np.abs(W2).sum(axis=0)))       # (+ da in the denormal range)


def _blocks(M, n, cols):
    step = max(1, (1 << 22) // max(1, n * cols))                                  # ~32 MiB of float64 rows per block
    return [(lo, min(M, lo + step)) for lo in range(0, M, step)]


def verify_forward(inp, out, what="", note=None, stages=("hid", "a", "ws", "agg_lp")):
    """every forward stage of `out` (hid bits [M n, 32], a [M n, 32], ws [M n], agg_lp bits [M, cols]) against the
    staged reference -> {stage: worst error / bound}; raises at the first stage beyond its bound.  Also: the columns
    [D, cols) of agg_lp are zeros."""
    M, n, D = inp["M"], inp["n"], inp["D"]
    cols = inp["x"].shape[1]
    res = {}
    parts = {k: [] for k in stages}
    for lo, hi in _blocks(M, n, cols):
        r = slice(lo * n, hi * n)
        m = hi - lo
        if "hid" in stages:
            want, bound, _ = hid_stage(inp["x"][r], inp["W0"])
            parts["hid"].append((f64(out["hid"][r]), want, bound))
        if "a" in stages:
            want, bound = a_stage(out["hid"][r], inp["W2"])
            parts["a"].append((out["a"][r], want, bound))
        if "ws" in stages:
            want, bound, _ = ws_stage(out["a"][r], inp["xa"][lo:hi], m, n)
            parts["ws"].append((out["ws"][r], want, bound))
        if "agg_lp" in stages:
            want, bound = agg_stage(out["ws"][r], inp["x"][r], m, n)
            parts["agg_lp"].append((f64(out["agg_lp"][lo:hi]), want, bound))
    for k in stages:
        got, want, bound = (np.concatenate([p[i] for p in parts[k]]) for i in range(3))
        res[k] = check(what + k, got, want, bound, note)
    if "agg_lp" in stages:
        assert not (np.asarray(out["agg_lp"])[:, D:] & 0x7fff).any(), (what, "columns [D, cols) of agg_lp must be zeros")
    return res


def verify_backward(binp, out, what="", note=None, stages=("dxa", "da", "dhid")):
    """the backward stages of `out` (da bits, dhid bits [M n, 32], dxa [M, 32]; an emulation's dws and ds too when
    `stages` names them) -> {stage: worst error / bound}"""
    M, n = binp["M"], binp["n"]
    cols = binp["x"].shape[1]
    res = {}
    parts = {k: [] for k in stages}
    for lo, hi in _blocks(M, n, cols):
        r = slice(lo * n, hi * n)
        m = hi - lo
        dws, dws_err = dws_stage(binp["x"][r], binp["g"][lo:hi], m, n)
        ds, ds_err = ds_stage(binp["ws"][r], dws, dws_err, m, n)
        if "dws" in stages:
            parts["dws"].append((out["dws"][r], dws, dws_err))
        if "ds" in stages:
            parts["ds"].append((out["ds"][r], ds, ds_err))
        if "dxa" in stages:
            parts["dxa"].append((out["dxa"][lo:hi],) + dxa_stage(ds, ds_err, binp["na"][r], m, n))
        if "da" in stages:
            parts["da"].append((f64(out["da"][r]),) + da_stage(ds, ds_err, binp["xa"][lo:hi], m, n))
        if "dhid" in stages:
            parts["dhid"].append((f64(out["dhid"][r]),) + dhid_stage(out["da"][r], binp["W2"], binp["hid"][r]))
    for k in stages:
        got, want, bound = (np.concatenate([p[i] for p in parts[k]]) for i in range(3))
        res[k] = check(what + k, got, want, bound, note)
    return res


# ---- a float32 emulation of the kernels' rounding points, with the mutants --------------------------------------------
# mutant -> the stages it may push beyond their bounds (every other stage still passes: the stages are fed the
# emulation's own intermediate results)
_DWS_ON = ("dws", "ds", "dxa", "da")        # dws and ds are no outputs: dxa and da are held to the INPUTS' ds
MUTANTS = collections.OrderedDict([
    ("a", ("agg_lp",)),                      # the weights without their low parts
    ("b", ("hid", "agg_lp") + _DWS_ON),      # child n - 2 reads child n - 1's row
    ("c", ("hid", "agg_lp") + _DWS_ON),      # every parent on an even trip computes on the previous parent's tile
    ("d", _DWS_ON),                          # d agg without its low parts
    ("e", _DWS_ON[1:]),                      # the last child's ds without the `- dot` term
    ("f", ("hid",)),                         # hid truncated instead of rounded to nearest
    ("g", ("hid", "agg_lp") + _DWS_ON),      # chunk c and c ^ 1 of rows 4..7 swapped
])
F32 = np.float32


def rows_seen(x_bits, M, n, mutant, stride):
    """the child rows a (mutated) kernel computes on"""
    x = np.array(x_bits).reshape(M, n, -1)
    if mutant == "b":
        x[:, n - 2] = x[:, n - 1]
    elif mutant == "c":                      # trips are counted from 1: parents [stride, 2 stride), [3 stride, 4 stride) ...
        p = np.arange(M)
        stale = (p // stride) % 2 == 1
        x[stale] = x[p[stale] - stride]
    elif mutant == "g":
        ch = x[:, 4:8].reshape(M, min(n, 8) - 4, -1, 2, 8) if n > 4 else None
        if ch is not None:
            x[:, 4:8] = ch[:, :, :, ::-1, :].reshape(M, min(n, 8) - 4, -1)
    return x.reshape(M * n, -1)


def _tanh32(v):
    """1 - 2 / (exp(2 |v|) + 1) in float32, every operation rounded once"""
    with np.errstate(over="ignore"):
        e = np.exp(F32(2) * np.abs(v))
        t = F32(1) - F32(2) * (F32(1) / (e + F32(1)))
    return np.copysign(t, v).astype(F32)


def _split(f):
    hi = bf16_value(bf16_rne(f))
    return hi, bf16_value(bf16_rne((f - hi).astype(F32)))


def emulate_forward(inp, mutant=None, stride=None):
    """the forward kernel's rounding points in float32 (sums in numpy's order) -> hid bits, a, ws, agg_lp bits"""
    M, n = inp["M"], inp["n"]
    xf = bf16_value(rows_seen(inp["x"], M, n, mutant, stride))
    pre = xf @ bf16_value(inp["W0"]).T
    t = _tanh32(pre)
    hid = (t.view(np.uint32) >> 16).astype(np.uint16) if mutant == "f" else bf16_rne(t)
    a = bf16_value(hid) @ bf16_value(inp["W2"]).T
    s = (a.reshape(M, n, HA) * inp["xa"][:, None, :]).sum(axis=2, dtype=F32)
    with np.errstate(under="ignore"):
        ex = np.exp(s - s.max(axis=1, keepdims=True))
    w = (ex / ex.sum(axis=1, keepdims=True, dtype=F32)).astype(F32)
    hi, lo = _split(w)
    x3 = xf.reshape(M, n, -1)
    acc = np.einsum("mj,mjc->mc", hi, x3)
    if mutant != "a":
        acc = acc + np.einsum("mj,mjc->mc", lo, x3)
    assert pre.dtype == a.dtype == s.dtype == w.dtype == acc.dtype == F32
    return dict(hid=hid, a=a, ws=w.reshape(M * n), agg_lp=bf16_rne(acc))


def emulate_backward(binp, mutant=None, stride=None):
    """the backward kernel's rounding points in float32 -> dws, ds (internal), da bits, dhid bits, dxa"""
    M, n = binp["M"], binp["n"]
    x3 = bf16_value(rows_seen(binp["x"], M, n, mutant, stride)).reshape(M, n, -1)
    ghi, glo = _split(binp["g"])
    dws = np.einsum("mjc,mc->mj", x3, ghi)
    if mutant != "d":
        dws = dws + np.einsum("mjc,mc->mj", x3, glo)
    w = binp["ws"].reshape(M, n)
    dot = (w * dws).sum(axis=1, keepdims=True, dtype=F32)
    ds = w * (dws - dot)
    if mutant == "e":
        ds[:, n - 1] = w[:, n - 1] * dws[:, n - 1]
    dxa = np.einsum("mj,mjh->mh", ds, binp["na"].reshape(M, n, HA))
    da = bf16_rne((ds[:, :, None] * binp["xa"][:, None, :]).reshape(M * n, HA))
    hid = bf16_value(binp["hid"])
    dhg = bf16_value(da) @ bf16_value(binp["W2"])
    dhid = bf16_rne(dhg * (F32(1) - hid * hid))
    assert dws.dtype == ds.dtype == dxa.dtype == dhg.dtype == F32
    return dict(dws=dws.reshape(M * n), ds=ds.reshape(M * n), da=da, dhid=dhid, dxa=dxa)


# ---- the cases of test_gpu_attn_fused.py (the host test runs them with a stand-in for the device's CU count) -----------
# trips: 0 = M as given; k > 0: M = 3 k CUs + 5 (k = 1 under GSAGE_AF_WAVES = GSAGE_AF_PER_CU = 1: every wave makes three
# trips and five make four; k = 16 at the default geometry, at most 16 waves per CU)
# layout: "plain" | "strides" (every leading dimension off the engine's) | "row0" (ids = NULL, row0 = 123) | "far" (rows
# behind byte offset 2^32).  special: see inputs()
Case = collections.namedtuple("Case", "name D n M ld trips layout special")


def _r64(v):
    return -(-v // 64) * 64


def _cases():
    out = []
    for D, n in ((32, 2), (64, 15), (128, 16), (256, 5), (602, 10), (640, 16)):
        out.append(Case("trips-D%d-n%d" % (D, n), D, n, None, _r64(D), 1, "plain", None))
    for D, n in ((32, 2), (602, 10)):
        out.append(Case("trips16-D%d-n%d" % (D, n), D, n, None, _r64(D), 16, "plain", None))
    for n in (2, 3, 4, 5, 8, 15, 16):
        out.append(Case("fan-n%d" % n, 64, n, 37, 64, 0, "plain", "repeats"))
    for D in (1, 8, 31, 32, 33, 65, 129, 257, 300, 608, 609, 640):
        # ld: the 64-round-up; 640 for D = 257 and 300 (KS = 19 needs ld >= 608) and 256 for D = 129 (five k-steps run as
        # KS = 8: 256 columns; at ld = 192 the shape is refused, which test_gpu_attn_fused.py asserts)
        out.append(Case("width-D%d" % D, D, 5, 21, {257: 640, 300: 640, 129: 256}.get(D, _r64(D)), 0, "plain", None))
    out.append(Case("width-D64-ld1024", 64, 5, 21, 1024, 0, "plain", None))
    out.append(Case("strides", 602, 10, 19, 640, 0, "strides", None))
    out.append(Case("row0", 70, 5, 21, 128, 0, "row0", None))
    out.append(Case("far", 620, 5, 21, 640, 0, "far", None))
    out.append(Case("small-M1", 602, 5, 1, 640, 0, "plain", None))
    out.append(Case("small-M3", 64, 5, 3, 64, 0, "plain", None))
    for sp in ("zero_rows", "saturated", "peaked", "same_rows", "tiny"):
        out.append(Case("special-" + sp, 100, 10, 21, 128, 0, "plain", sp))
    return out


CASES = _cases()
POOL_ROWS = 5000
FAR_ROWS = 64


def case_M(case, cus):
    return case.M if case.trips == 0 else 3 * case.trips * cus + 5


def inputs(case, cus):
    """-> (forward inputs, backward inputs), seeded by the case's name.  pool: bf16 bits [P, cols] of the distinct rows
    (columns [D, cols) zero), ids [M n] into it, x = pool[ids]; W0 [32, cols] (zero pads), W2 [32, 32] bits; xa float32.
    The backward's inputs are independent of the forward: ws a random softmax, na / xa / g normals (g's columns [D, cols)
    hold +-1e30: never to reach dws), hid random bf16 in (-1, 1).  special:
      repeats    ids repeated inside a parent (every third parent its first two, one parent all of them)
      zero_rows  pool row 0 is the padding row (all zeros); every fourth child and one whole parent read it
      saturated  rows >= 0, unit h of W0 of one sign, W0 * 64: every |pre-activation| > 20
      peaked     xa * 30
      same_rows  all children of a parent read one row
      tiny       W0 * 2^-20
    For the special cases the backward runs on the forward's own outputs (chain())."""
    rng = np.random.RandomState(zlib.crc32(case.name.encode()) & 0x7fffffff)
    D, n, M = case.D, case.n, case_M(case, cus)
    cols = cols_of(D)
    P = FAR_ROWS if case.layout == "far" else POOL_ROWS
    pool = np.zeros((P, cols), dtype=np.float32)
    pool[:, :D] = 0.7 * rng.standard_normal(size=(P, D))
    w0 = np.zeros((32, cols), dtype=np.float32)
    w0[:, :D] = rng.standard_normal(size=(32, D)) / np.sqrt(D)
    ids = rng.randint(1 if case.layout == "far" else 0, P, size=(M, n)).astype(np.int64)   # (far: row 0 starts below 2^32)
    xa = rng.standard_normal(size=(M, HA)).astype(np.float32)
    sp = case.special
    if sp == "repeats":
        ids[::3, 1] = ids[::3, 0]
        ids[M // 2, :] = ids[M // 2, 0]
    elif sp == "zero_rows":
        pool[0] = 0.0
        ids[ids == 0] = 1
        flat = ids.reshape(-1)
        flat[::4] = 0
        ids[M // 2, :] = 0
    elif sp == "saturated":
        pool = np.abs(pool)
        w0 = 64.0 * np.abs(w0) * np.where(np.arange(32) % 2 == 0, 1.0, -1.0)[:, None]
    elif sp == "peaked":
        xa = (30.0 * xa).astype(np.float32)
    elif sp == "same_rows":
        ids[:, :] = ids[:, :1]
    elif sp == "tiny":
        w0 = w0 * 2.0 ** -20
    pool_bits, w0_bits = bf16_rne(pool), bf16_rne(w0.astype(np.float32))
    w2_bits = bf16_rne((rng.standard_normal(size=(HA, HA)) / np.sqrt(HA)).astype(np.float32))
    ids = ids.reshape(-1)
    fwd = dict(M=M, n=n, D=D, pool=pool_bits, ids=ids, x=pool_bits[ids], W0=w0_bits, W2=w2_bits, xa=xa)
    s = 2.0 * rng.standard_normal(size=(M, n))
    e = np.exp(s - s.max(axis=1, keepdims=True))
    g = np.zeros((M, cols), dtype=np.float32)
    g[:, :D] = rng.standard_normal(size=(M, D))
    g[:, D:] = np.where(rng.randint(0, 2, size=(M, cols - D)) == 1, 1e30, -1e30)
    bwd = dict(M=M, n=n, D=D, x=fwd["x"], W2=w2_bits, g=g, ws=(e / e.sum(axis=1, keepdims=True)).astype(np.float32).reshape(M * n),
               na=rng.standard_normal(size=(M * n, HA)).astype(np.float32),
               xa=rng.standard_normal(size=(M, HA)).astype(np.float32),
               hid=bf16_rne(rng.uniform(-0.99, 0.99, size=(M * n, HA)).astype(np.float32)))
    return fwd, bwd


def chain(fwd, bwd, out):
    """the backward's inputs taken from a forward's outputs (the special cases): ws, na = a, hid and the parents' xa"""
    return dict(bwd, ws=np.array(out["ws"]), na=np.array(out["a"]), hid=np.array(out["hid"]), xa=fwd["xa"])
