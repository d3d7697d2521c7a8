"""Plain numpy restatement of the gather kernels (csrc/gsage_gather.hip): K2 gather+mean in its single, multi-segment
and FP8 forms, its backward and the K6 scatter-add,

    out[i, c]            = (sum_{j < n} table[ids[i * n + j], c]) / n          (ids == NULL: row i * n + j itself)
    dneibs[i * n + j, c] = dagg[i, c] / n
    grad[ids[r], c]     += scale * rows[r / n, c]

and of the entry points' dispatch: dispatch_vec, fill_multi, fp8_out_vec_ok, the `wide` predicate of
gsage_gather_mean_multi_adam and the grid.  Written from include/gsage.h and the conditions in the entry points.
Nothing here imports the product: the GPU tests (test_gpu_gather.py) and the host tests (test_gather_host.py) both
compare against this file.  bf16 bits come from update_tail_ref (the same arithmetic as f32_to_bf16 of gsage_common.h).

The arithmetic contract, as gather_mean_chunk documents it: a float32 accumulator that starts at +0 and takes the n rows
in neighbour order j = 0 .. n-1, ONE float32 division by float(n), then round-to-nearest-even where the output is bf16.
mean_in_order is exactly that; mean64 is the same operations in float64."""
import numpy as np

from update_tail_ref import bf16_rne, bf16_value            # noqa: F401  (the one copy of the bf16 helpers)

ESZ = {"bf16": 2, "f32": 4, "fp8": 1}
U32 = 2.0 ** -24              # unit roundoff of float32
U16 = 2.0 ** -8               # unit roundoff of bfloat16
GRID_CAP = 16384              # grid_for: at most this many workgroups of 256 work items; the rest by a stride loop
WIDE_ITEMS = 256 * 1024       # the wide kernel only for a gather role of at most this many work items


def ceil_div(a, b):
    return -(-int(a) // int(b))


def round_up(x, m):
    return ceil_div(x, m) * int(m)


# ---- the arithmetic --------------------------------------------------------------------------------------------------
def mean_in_order(rows, scale=None):
    """rows [M, n, D] float32 (the values the kernel accumulates: bf16 / e4m3 operands already decoded) -> [M, D] float32:
    a float32 add chain from +0 in the order j = 0 .. n-1, times the column's scale for an FP8 table, one float32
    division by float32(n)"""
    rows = np.asarray(rows)
    assert rows.dtype == np.float32 and rows.ndim == 3
    M, n, D = rows.shape
    acc = np.zeros((M, D), dtype=np.float32)
    for j in range(n):
        acc = acc + rows[:, j, :]
        assert acc.dtype == np.float32
    if scale is not None:
        acc = acc * np.asarray(scale, dtype=np.float32)[None, :D]
    out = acc / np.float32(n)
    assert out.dtype == np.float32
    return out


def mean64(rows, scale=None):
    """the same mean in float64"""
    rows = np.asarray(rows, dtype=np.float64)
    s = rows.sum(axis=1)
    if scale is not None:
        s = s * np.asarray(scale, dtype=np.float64)[None, :rows.shape[2]]
    return s / rows.shape[1]


def mean_bound(rows, out_dtype="f32"):
    """per cell: (n + 1) 2^-24 sum_j |x_j| / n -- n - 1 roundings of the running sum plus a division taken at 2 units --
    plus 2^-8 |ref| for a bf16 output"""
    rows = np.asarray(rows, dtype=np.float64)
    n = rows.shape[1]
    b = (n + 1) * U32 * np.abs(rows).sum(axis=1) / n
    if out_dtype == "bf16":
        b = b + U16 * np.abs(mean64(rows))
    return b


def out_bits(values, out_dtype):
    """float32 results -> the bits the kernel stores"""
    values = np.ascontiguousarray(values, dtype=np.float32)
    return bf16_rne(values) if out_dtype == "bf16" else values.view(np.uint32)


def decode_e4m3(codes):
    """OCP e4m3fn bytes -> float32 (through torch's CPU conversion)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(codes, dtype=np.uint8)).view(torch.float8_e4m3fn)
    return t.float().numpy()


def mean_bwd(dagg, n):
    """[M, D] float32 -> [M * n, D] float32: float32(g) / float32(n), each row n times"""
    g = np.asarray(dagg)
    assert g.dtype == np.float32
    return np.repeat(g / np.float32(n), n, axis=0)


def scatter_add64(init, rows, ids, n, scale):
    """-> (grad float64, magnitude |init| + sum |scale * row|, count of rows landing per cell [T, D]); scale is the
    float32 the kernel is handed"""
    init = np.asarray(init, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.float64)
    s = float(np.float32(scale))
    src = rows[np.arange(len(ids)) // n] * s
    grad, mag = init.copy(), np.abs(init)
    cnt = np.zeros(init.shape, dtype=np.int64)
    np.add.at(grad, ids, src)
    np.add.at(mag, ids, np.abs(src))
    np.add.at(cnt, ids, 1)
    return grad, mag, cnt


def scatter_bound(mag, cnt):
    """(c + 1) 2^-24 (|init| + sum |scale * row|): c float32 adds in any order and one multiply"""
    return (cnt + 1) * U32 * mag


# ---- the dispatch, restated ------------------------------------------------------------------------------------------
def vec(dtype, out_dtype, ld, out_ld, table_addr, out_addr, D):
    """dispatch_vec: the widest chunk of 8 (bf16 -> bf16 only) / 4 / 2 / 1 elements that is an aligned unit in the table
    and in the output and whose round_up(D, VEC) fits both leading dimensions.  Addresses in bytes."""
    assert dtype in ("bf16", "f32") and out_dtype in ("bf16", "f32")
    kmax = 8 if dtype == "bf16" and out_dtype == "bf16" else 4

    def ok(v):
        return (ld % v == 0 and out_ld % v == 0 and table_addr % (v * ESZ[dtype]) == 0 and
                out_addr % (v * ESZ[out_dtype]) == 0 and round_up(D, v) <= ld and round_up(D, v) <= out_ld)

    for v in (8, 4, 2):
        if v <= kmax and ok(v):
            return v
    return 1


def chunks(D, v):
    return ceil_div(D, v)


def written_cols(D, v):
    """a bf16 / fp32 launch writes columns [0, round_up(D, VEC)) of rows < M: [D, ..) as +0"""
    return round_up(D, v)


def fp8_out_vec_ok(out_addr, out_dtype, D, out_ld):
    """can an FP8 launch write the output in 16-byte pieces?"""
    e = 8 if out_dtype == "bf16" else 4
    return out_ld % e == 0 and round_up(D, e) <= out_ld and out_addr % 16 == 0


def fp8_written_cols(out_addr, out_dtype, D, out_ld):
    """16-byte pieces whose first column is below D (VS), or element stores below D"""
    e = 8 if out_dtype == "bf16" else 4
    return round_up(D, e) if fp8_out_vec_ok(out_addr, out_dtype, D, out_ld) else int(D)


def check_single(dtype, out_dtype, ld, out_ld, M, n, D):
    """what gsage_gather_mean requires before it launches"""
    if not (n > 0 and M >= 0 and D > 0):
        raise ValueError("bad sizes")
    if not (ld >= D and out_ld >= D):
        raise ValueError("leading dimension smaller than D")
    if M and (dtype not in ("bf16", "f32") or out_dtype not in ("bf16", "f32")):
        raise ValueError("unsupported dtype pair")


def check_fp8(ld, out_ld, M, n, D, out_dtype, out_addr=0):
    """what gsage_gather_mean_fp8 requires"""
    check_single("bf16", out_dtype, ld, out_ld, M, n, D)
    if not (ld % 16 == 0 and round_up(D, 16) <= ld):
        raise ValueError("rows are whole 16-byte chunks")
    if out_addr % ESZ[out_dtype]:
        raise ValueError("misaligned output")


def fill_multi(M, n, dtype, out_dtype, ld, D, out_ld, table_addrs=None, out_addrs=None):
    """fill_multi of a multi-segment launch -> dict(vec, chunks, all_single, rpi [n_seg], first [n_seg + 1]); ValueError
    where the entry point refuses"""
    n_seg = len(M)
    if not 1 <= n_seg <= 8:
        raise ValueError("1..8 segments")
    v = {"fp8": 16, "bf16": 8, "f32": 4}[dtype]
    if dtype == "fp8":
        if out_dtype not in ("bf16", "f32"):
            raise ValueError("bf16 or fp32 output")
        if not (D > 0 and ld % 16 == 0 and round_up(D, 16) <= ld and fp8_out_vec_ok(0, out_dtype, D, out_ld)):
            raise ValueError("needs 16-byte row chunks")
    else:
        if not (out_dtype == dtype or out_dtype == "bf16"):
            raise ValueError("bf16 -> bf16, fp32 -> fp32 or fp32 -> bf16")
        if not (D > 0 and ld % v == 0 and out_ld % v == 0 and round_up(D, v) <= ld and round_up(D, v) <= out_ld):
            raise ValueError("needs 16-byte row chunks")
    for s in range(n_seg):
        if not (M[s] >= 0 and n[s] > 0):
            raise ValueError("bad segment %d" % s)
        for addrs in (table_addrs, out_addrs):
            if addrs is not None and (not addrs[s] or addrs[s] % 16):
                raise ValueError("bad segment %d" % s)
    ch = ceil_div(D, v)
    all_single = all(k == 1 for k in n)
    rpi = [4 if dtype == "bf16" and not all_single and k == 1 else 1 for k in n]
    first = [0]
    for s in range(n_seg):
        first.append(first[-1] + ceil_div(M[s], rpi[s]) * ch)
    return dict(vec=v, chunks=ch, all_single=all_single, rpi=rpi, first=first)


def multi_path(dtype, out_dtype, all_single, rpi):
    """per segment: "copy4" (the all-single loop: four work items per lane), "rows4" (four rows per work item) or
    "mean" (gather_mean_chunk).  The two row-copy paths exist for bf16 -> bf16 only."""
    lowp = dtype == "bf16" and out_dtype == "bf16"
    return ["copy4" if lowp and all_single else "rows4" if lowp and r == 4 else "mean" for r in rpi]


def wide(dtype, has_ids, n, total, in_launch_norm=False):
    """the `wide` predicate of gsage_gather_mean_multi_adam (GSAGE_GATHER_WIDE unset): a bf16 launch without the
    in-launch norm whose largest fan-out among the segments WITH a row list is above 8 and whose gather role has at
    most 256 Ki work items runs k_gather_multi_adam_wide (16 rows in flight per lane)"""
    max_n = max([k for k, h in zip(n, has_ids) if h] + [0])
    return dtype == "bf16" and not in_launch_norm and max_n > 8 and total <= WIDE_ITEMS


def grid_for(items):
    return min(max(ceil_div(items, 256), 1), GRID_CAP)


def workgroups(items, n_side=0):
    """workgroups of a launch over `items` work items, plus the side roles' own"""
    return grid_for(items) + n_side


def bwd_vec(D, ld, out_ld, dagg_addr, out_addr):
    """gsage_segment_mean_bwd: the 16-byte kernel k_segment_mean_bwd<4> or the scalar one"""
    return 4 if D % 4 == 0 and ld % 4 == 0 and out_ld % 4 == 0 and dagg_addr % 16 == 0 and out_addr % 16 == 0 else 1


def bwd_items(M, n, D, v):
    return M * n * (D // 4 if v == 4 else D)


def scatter_items(M, n, D):
    return M * n * D
