"""Float64 restatements, in plain numpy, of the tail of a training step (csrc/gsage_optim.hip, gsage_optim_dev.h):
the sum of the weight-gradient partial buffers into the flat bucket (gsage_finalize_grads), clip_grad_norm_ + Adam
(gsage_clip_adam_step / gsage_clip_adam_meet) and the bf16 / fp32 / fragment-ordered operand copies
(gsage_prep_weights and the same stores made by the update).  Nothing here imports the product: the GPU tests
(test_gpu_update_tail.py) and the host tests (test_update_tail_host.py) both compare against this file."""
import collections

import numpy as np

EPS24 = 2.0 ** -24            # half an ulp of a float32 of magnitude 1: one rounding of a float32 operation
RTOL, ATOL = 2e-6, 2e-7       # test_flat_adam_equals_torch_clip_plus_adam's tolerance, applied per element

# One gsage_reduce_desc as the reference sees it: partial buffer s, row r, column c is bufs[buf][off + s * stride +
# r * ld + c]; the sum over s lands at flat[out_off + r * cols + c].
Red = collections.namedtuple("Red", "buf off stride out_off S rows cols ld")


# ---- bf16 -------------------------------------------------------------------------------------------------------
def bf16_rne(x):
    """float32 -> the bits (uint16) of the nearest bfloat16, ties to even; NaN stays a (quiet) NaN"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7fffffff) > 0x7f800000
    r = (u + 0x7fff + ((u >> 16) & 1)) >> 16
    r = np.where(nan, (u >> 16) | 0x40, r)
    return r.astype(np.uint16)


def bf16_value(bits):
    """the float32 value of bfloat16 bits"""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def special_values():
    """+-0, denormals, halfway cases (ties to even, both directions), the largest float (rounds to inf), +-inf"""
    f = np.float32
    tiny = np.array([1, 0x7fff, 0x8000, 0x18000, 0x7fffff], dtype=np.uint32).view(np.float32)      # denormals
    return np.concatenate([np.array([0.0, -0.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8),
                                     1 + 2.0 ** -8 + 2.0 ** -23, np.finfo(f).max, -np.finfo(f).max, np.inf, -np.inf,
                                     np.finfo(f).tiny], dtype=f), tiny, -tiny])


# ---- gradient finalisation -----------------------------------------------------------------------------------------
def _terms(d, bufs):
    """[S, rows, cols] float64: the values descriptor d adds up (pad columns and gaps between buffers left out)"""
    b = np.asarray(bufs[d.buf], dtype=np.float32)
    out = np.empty((d.S, d.rows, d.cols), dtype=np.float64)
    for s in range(d.S):
        lo = d.off + s * d.stride
        out[s] = b[lo:lo + d.rows * d.ld].reshape(d.rows, d.ld)[:, :d.cols]
    return out


def finalize(descs, bufs, n, drop=None):
    """-> (flat [n] float64, NaN where no descriptor writes; per-descriptor sum of squares of the sums).
    drop = (descriptor index, buffer index): that one partial buffer is left out (a deliberately wrong reference)."""
    flat = np.full(n, np.nan, dtype=np.float64)
    sq = np.zeros(len(descs), dtype=np.float64)
    for k, d in enumerate(descs):
        t = _terms(d, bufs)
        if drop is not None and drop[0] == k:
            t = np.delete(t, drop[1], axis=0)
        s = t.sum(axis=0).reshape(-1)
        assert d.out_off >= 0 and d.out_off + s.shape[0] <= n
        flat[d.out_off:d.out_off + s.shape[0]] = s
        sq[k] = float((s * s).sum())
    return flat, sq


def finalize_magnitude(descs, bufs, n):
    """[n] float64: sum_s |x_s| of every destination element (0 where no descriptor writes): the scale of the bound
    S * 2^-24 * sum_s |x_s| on a float32 sum of S terms in any order and grouping"""
    mag = np.zeros(n, dtype=np.float64)
    for d in descs:
        a = np.abs(_terms(d, bufs)).sum(axis=0).reshape(-1)
        mag[d.out_off:d.out_off + a.shape[0]] = a
    return mag


def finalize_bound(descs, bufs, n):
    """[n] float64: S * 2^-24 * sum_s |x_s| per destination element.  Every partial sum of a float32 summation of S
    terms is at most sum |x_s| (1 + S 2^-24) in magnitude and each of the at most S - 1 additions rounds once (half an
    ulp = 2^-24 relative), whatever the order or the grouping -- S = 1 is a copy and must be exact."""
    bound = np.zeros(n, dtype=np.float64)
    mag = finalize_magnitude(descs, bufs, n)
    for d in descs:
        sl = slice(d.out_off, d.out_off + d.rows * d.cols)
        bound[sl] = (d.S if d.S > 1 else 0) * EPS24 * mag[sl]
    return bound


# ---- clip + Adam ---------------------------------------------------------------------------------------------------
def clip_adam(p, g, m, v, lr, t, betas, eps, wd, max_norm):
    """One update, number t >= 1, in float64: torch.nn.utils.clip_grad_norm_(params, max_norm) followed by
    torch.optim.Adam's step (L2 weight decay added to the clipped gradient, bias corrections 1 - beta^t).
    -> dict(p, g (the clipped gradient), m, v, norm (before clipping), coef)"""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2 = float(betas[0]), float(betas[1])
    norm = float(np.sqrt((g * g).sum()))
    coef = min(1.0, float(max_norm) / (norm + 1e-6))
    gc = g * coef
    ge = gc + float(wd) * p if wd != 0 else gc
    m1 = b1 * m + (1.0 - b1) * ge
    v1 = b2 * v + (1.0 - b2) * ge * ge
    bc1 = 1.0 - b1 ** int(t)
    bc2 = 1.0 - b2 ** int(t)
    step_size = float(lr) / bc1
    denom = np.sqrt(v1) / np.sqrt(bc2) + float(eps)
    return dict(p=p - step_size * (m1 / denom), g=gc, m=m1, v=v1, norm=norm, coef=coef)


def adam_state(n, seed, norm):
    """p, g, m, v (float32) with |g| = norm, and a state Adam can be in: v >= m^2 + 1e-3, so |m| / sqrt(v) < 1 and the
    update stays below lr / (1 - beta1^t).  (With v independent of m, single elements had |m| / sqrt(v) ~ 1 000: the new
    p is then the small difference of two large numbers, and a tolerance relative to it measures the conditioning of
    the input, not the kernel.)"""
    rng = np.random.RandomState(seed)
    p = rng.normal(size=n).astype(np.float32)
    g = rng.normal(size=n)
    g = (g * (norm / np.sqrt((g * g).sum()))).astype(np.float32)
    m = (rng.normal(size=n) * 0.1).astype(np.float32)
    v = (m.astype(np.float64) ** 2 + 1e-3 * (1 + rng.uniform(size=n))).astype(np.float32)
    return dict(p=p, g=g, m=m, v=v)


def clip_adam_float32(p, g, m, v, lr, t, betas, eps, wd, max_norm):
    """clip_adam once more, in numpy float32 with the roundings of adam_workgroup / adam_update (gsage_optim_dev.h): the
    squared norm rounded once, coef = max_norm / (norm + 1e-6), 1 - beta formed in float32, sqrt(v) * (1 / sqrt(bc2))
    + eps, p - step_size * (m / denom), nothing contracted.  Not a reference: a measure of what float32 alone costs
    against clip_adam in this formulation, without a GPU."""
    F = np.float32
    p, g, m, v = (np.asarray(a, dtype=F) for a in (p, g, m, v))
    b1, b2, eps, wd, lr, mx = F(betas[0]), F(betas[1]), F(eps), F(wd), F(lr), F(max_norm)
    total = np.sqrt(F((g.astype(np.float64) ** 2).sum()))
    coef = min(F(1), mx / (total + F(1e-6)))
    bc1, bc2 = F(1) - F(float(b1) ** int(t)), F(1) - F(float(b2) ** int(t))
    step_size, rsqrt_bc2 = lr / bc1, F(1) / np.sqrt(bc2)
    gc = g * coef
    ge = gc + wd * p if wd != 0 else gc
    m1 = b1 * m + (F(1) - b1) * ge
    v1 = b2 * v + ((F(1) - b2) * ge) * ge
    denom = np.sqrt(v1) * rsqrt_bc2 + eps
    return dict(p=p - step_size * (m1 / denom), g=gc, m=m1, v=v1, norm=float(total), coef=float(coef))


def excess(a, b):
    """max over the elements of |a - b| / (ATOL + RTOL |b|): <= 1 means within the project's tolerance"""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((np.abs(a - b) / (ATOL + RTOL * np.abs(b))).max())


def torch_step(p, g, m, v, lr, t, betas, eps, wd, max_norm, dtype):
    """The same update by torch itself on CPU tensors of `dtype`: clip_grad_norm_ + torch.optim.Adam.step() with the
    optimizer's state set to (step t - 1, m, v).  -> dict(p, g, m, v, norm) as float64 numpy arrays."""
    import torch
    prm = torch.nn.Parameter(torch.tensor(np.asarray(p), dtype=dtype))
    opt = torch.optim.Adam([prm], lr=float(lr), betas=tuple(betas), eps=float(eps), weight_decay=float(wd))
    opt.state[prm] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.tensor(np.asarray(m), dtype=dtype),
                      "exp_avg_sq": torch.tensor(np.asarray(v), dtype=dtype)}
    prm.grad = torch.tensor(np.asarray(g), dtype=dtype)
    norm = torch.nn.utils.clip_grad_norm_([prm], float(max_norm))
    opt.step()
    st = opt.state[prm]
    assert int(st["step"]) == t
    return dict(p=prm.detach().double().numpy(), g=prm.grad.double().numpy(), m=st["exp_avg"].double().numpy(),
                v=st["exp_avg_sq"].double().numpy(), norm=float(norm))


def float32_torch_excess(p, g, m, v, lr, t, betas, eps, wd, max_norm):
    """What float32 arithmetic costs on these inputs: `excess` of torch's float32 update against clip_adam, per
    tensor.  Inputs must be float32 values (both sides start from the same numbers)."""
    import torch
    ref = clip_adam(p, g, m, v, lr, t, betas, eps, wd, max_norm)
    got = torch_step(p, g, m, v, lr, t, betas, eps, wd, max_norm, torch.float32)
    return {k: excess(got[k], ref[k]) for k in ("p", "g", "m", "v")}


# ---- the fragment-ordered weight copy ---------------------------------------------------------------------------------
def packed_index(r, c, kc):
    """Offset of W[r][c] inside Wp[jb][kc][lane][e] (include/gsage.h, gsage_linear_nt_packed; one group):
    W[jb*32 + (lane & 31)][k*16 + (lane >> 5)*8 + e] sits at ((jb * kc + k) * 64 + lane) * 8 + e, kc = 4 ceil(K / 64).
    r, c: ints or integer arrays."""
    r = np.asarray(r, dtype=np.int64)
    c = np.asarray(c, dtype=np.int64)
    jb, row = r // 32, r % 32
    k, within = c // 16, c % 16
    lane = row + 32 * (within // 8)
    e = within % 8
    return ((jb * int(kc) + k) * 64 + lane) * 8 + e


def packed_kc(K):
    return 4 * ((int(K) + 63) // 64)


def packed_elems(N, K):
    return ((int(N) + 31) // 32) * packed_kc(K) * 64 * 8
