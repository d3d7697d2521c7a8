"""Plain numpy restatement (float64) of the K5 projection GEMM gsage_linear_nt (csrc/gsage_linear.hip),

    C[m, g * c_gstride + j] = act(sum_k A_g[m, k] * W_g[j, k] + bias[g * N + j]),        act: none | relu | tanh

of the entry point's choice of kernel and of store_tile's choice of store path, written from include/gsage.h and the
conditions in the entry point.  Nothing here imports the product: the GPU tests (test_gpu_linear.py) and the host tests
(test_linear_host.py) both compare against this file.  bf16 bits come from update_tail_ref."""
import numpy as np

from update_tail_ref import bf16_rne, bf16_value            # noqa: F401  (the one copy of the bf16 helpers)

BM, BN = 64, 128              # rows and columns of one workgroup's output tile
EPC = {"bf16": 8, "f32": 4}   # elements per 16-byte chunk
LINE = {"bf16": 64, "f32": 32}            # elements per 128-byte line = one k-tile of a row
ESZ = {"bf16": 2, "f32": 4}
ACTS = ("none", "relu", "tanh")
U32 = 2.0 ** -24              # unit roundoff of float32
U16 = 2.0 ** -8               # unit roundoff of bfloat16 (8 significant bits)
# expf's accuracy.  ROCm's documentation is not shipped with the toolchain, so the figure is ASSUMED: 3 ulp, what the
# OpenCL 3.0 specification (section 7.4, "Relative error as ULPs", exp, full profile) requires of the device library's
# exp, which HIP's expf calls; HIP's own "HIP math API" page lists expf at 1 ulp, which is inside it.
EXPF_ULP = 3.0


def round_up(x, m):
    return -(-int(x) // int(m)) * int(m)


def operand_values(x, dtype):
    """the values the kernel multiplies: float32 as they are, bf16 after round-to-nearest-even -> float64"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == "bf16":
        x = bf16_value(bf16_rne(x))
    return x.astype(np.float64)


def activate(pre, act):
    assert act in ACTS
    pre = np.asarray(pre, dtype=np.float64)
    return np.maximum(pre, 0.0) if act == "relu" else np.tanh(pre) if act == "tanh" else pre


def linear_pre(A, W, bias, dtype="f32"):
    """A [M, K], W [N, K], bias [N] or None -> the pre-activations [M, N] in float64"""
    pre = operand_values(A, dtype) @ operand_values(W, dtype).T
    return pre if bias is None else pre + np.asarray(bias, dtype=np.float32).astype(np.float64)[None, :]


def linear_ref(A, W, bias, act, dtype="f32"):
    """act(A W^T + bias) in float64, from the operands exactly as the kernel sees them"""
    return activate(linear_pre(A, W, bias, dtype), act)


# ---- the dispatch, restated ----------------------------------------------------------------------------------------
def k5_path(dtype, lda, ldw, K):
    """the kernel gsage_linear_nt launches: ("dma", NBUF, nk) -- k_linear_nt_dma<T, ACT, NBUF> over nk k-tiles -- when
    both leading dimensions are whole 128-byte lines that hold K rounded up to a line, else ("staged", nk) --
    k_linear_nt<T, false, ACT>"""
    line = LINE[dtype]
    kpad = round_up(K, line)
    nk = kpad // line
    kchunks = -(-int(K) // EPC[dtype])
    assert nk == -(-kchunks // 8)                                    # the kernels' own count: ceil(ceil(K / epc) / 8)
    if lda % line == 0 and ldw % line == 0 and kpad <= lda and kpad <= ldw:
        return ("dma", min(nk, 3), nk)
    return ("staged", nk)


def half_w(N, n0):
    """the DMA kernel's column tile at n0 fetches only the lower 64 rows of its W tile"""
    return N - n0 <= 64


def store_path(c_dtype, C_ptr, ldc, g, c_gstride, N, n0):
    """store_tile's path for group g's column tile at n0: 16-byte chunks through LDS (`wide`) or per element"""
    epc = EPC[c_dtype]
    ncols = min(N - n0, BN)
    cbase = g * c_gstride + n0
    wide = ncols % epc == 0 and ldc % epc == 0 and cbase % epc == 0 and C_ptr % 16 == 0
    return "wide" if wide else "element"


def column_tiles(N):
    return list(range(0, N, BN))


# ---- bounds --------------------------------------------------------------------------------------------------------
def abs_bound(A, W, bias, K, dtype="f32"):
    """per cell, for the pre-activation: (K + 2) 2^-24 (sum_k |a_k w_k| + |bias|) -- the worst case of a float32 fused
    multiply-add chain of length K (one rounding per product) plus the bias addition.  For bf16 operands (exact
    products, float32 accumulation inside the matrix instruction in an order the ISA does not state) the same bound is
    an ASSUMPTION."""
    mag = np.abs(operand_values(A, dtype)) @ np.abs(operand_values(W, dtype)).T
    if bias is not None:
        mag = mag + np.abs(np.asarray(bias, dtype=np.float64))[None, :]
    return (K + 2) * U32 * mag


def tanh_term(pre, pre_bound):
    """what the float32 evaluation of t = 1 - 2 / (expf(2 |v|) + 1) adds to |tanh(v) - t|, from its operations:
      x = 2 |v|            exact
      e = expf(x)          relative error <= EXPF_ULP 2^-23
      s = e + 1            one rounding; e's relative error shrinks by e / (e + 1) < 1
      q = 2 / s            one rounding (the build keeps HIP's correctly rounded float32 division)
      t = 1 - q            one rounding, relative to t <= 1
    so q = q0 (1 + eta), |eta| <= (EXPF_ULP 2^-23 + 2 2^-24) (1 + 2^-20), and |t - t0| <= q0 |eta| + 2^-24 (t0 + q0
    |eta|) with q0 = 2 / (exp(2 |v|) + 1) <= 1, taken at the smallest |v| the pre-activation's own bound allows (q0
    falls with |v|).  expf overflows to +inf past |v| = 44.4: q = 0 and t = 1, inside the same bound."""
    v = np.maximum(np.abs(np.asarray(pre, dtype=np.float64)) - pre_bound, 0.0)
    with np.errstate(over="ignore"):
        q0 = 2.0 / (np.exp(2.0 * v) + 1.0)
    eta = (EXPF_ULP * 2.0 ** -23 + 2 * U32) * (1 + 2.0 ** -20)
    return q0 * eta + U32 * (1.0 + q0 * eta)


def out_bound(pre, pre_bound, act, c_dtype):
    """the bound of the stored value: relu and tanh are 1-Lipschitz, tanh adds tanh_term, a bf16 output adds its
    rounding 2^-8 |ref|"""
    b = np.asarray(pre_bound, dtype=np.float64)
    if act == "tanh":
        b = b + tanh_term(pre, pre_bound)
    if c_dtype == "bf16":
        b = b + U16 * np.abs(activate(pre, act))
    return b
