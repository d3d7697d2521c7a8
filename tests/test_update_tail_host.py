"""update_tail_ref (the float64 restatement the GPU tests of the step tail compare against) checked without a GPU:
clip_adam against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam, packed_index against the header's five-index
layout, bf16_rne against torch's conversion, finalize against a literal loop.

Measured here (torch 2.x on the CPU, the 6-step schedule below): float32 torch against float64 clip_adam, as
`excess` = max |a - b| / (2e-7 + 2e-6 |b|), is at most 0.03 (p), 0.03 (m), 0.0004 (v), 0.08 (clipped g) in a single
step -- float32 rounding alone stays well inside the project's tolerance, so the GPU tests start from it."""
import numpy as np
import pytest
import torch

import update_tail_ref as ut
from util import note_parity

SHAPES = [(37, 19), (128,), (5, 64, 3), (1,)]          # test_flat_adam_equals_torch_clip_plus_adam's bucket
SCALES = [0.01, 3.0, 0.2, 10.0, 0.001, 1.0]           # norm = scale * sqrt(1792): not clipped at 0.01 and 0.001
N = sum(int(np.prod(s)) for s in SHAPES)


def _schedule(wd, dtype):
    """the six steps by torch in `dtype` -> per step (inputs as float64 arrays, lr, t, torch's outputs)"""
    torch.manual_seed(0)
    prm = [torch.nn.Parameter(torch.randn(*s).to(dtype)) for s in SHAPES]
    opt = torch.optim.Adam(prm, lr=0.01, weight_decay=wd)
    flat = lambda ts: np.concatenate([t.detach().double().numpy().reshape(-1) for t in ts])
    out, lr = [], 0.01
    for step in range(6):
        grads = [(torch.randn(*s) * SCALES[step]).to(dtype) for s in SHAPES]
        for p, g in zip(prm, grads):
            p.grad = g.clone()
        if step == 3:
            lr = 0.003
            for grp in opt.param_groups:
                grp["lr"] = lr
        if step == 0:
            m0, v0 = np.zeros(N), np.zeros(N)
        else:
            m0, v0 = flat([opt.state[p]["exp_avg"] for p in prm]), flat([opt.state[p]["exp_avg_sq"] for p in prm])
        p0, g0 = flat(prm), flat(grads)
        norm = float(torch.nn.utils.clip_grad_norm_(prm, 5))
        opt.step()
        got = dict(p=flat(prm), g=flat([p.grad for p in prm]), m=flat([opt.state[p]["exp_avg"] for p in prm]),
                   v=flat([opt.state[p]["exp_avg_sq"] for p in prm]), norm=norm)
        out.append((p0, g0, m0, v0, lr, step + 1, got))
    return out


@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_clip_adam_is_torch_in_float64(wd):
    """6 steps, float64 on both sides: every step's p, clipped g, m, v and norm agree to 1e-12"""
    clipped = []
    for p0, g0, m0, v0, lr, t, got in _schedule(wd, torch.float64):
        ref = ut.clip_adam(p0, g0, m0, v0, lr, t, (0.9, 0.999), 1e-8, wd, 5.0)
        clipped.append(ref["coef"] < 1.0)
        assert abs(ref["norm"] - got["norm"]) <= 1e-12 * got["norm"]
        for k in ("p", "g", "m", "v"):
            err = float(np.abs(ref[k] - got[k]).max())
            assert err <= 1e-12 * max(1.0, float(np.abs(got[k]).max())), (k, t, err)
    assert clipped == [False, True, True, True, False, True]


@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_float32_torch_error_is_recorded(wd):
    """the same schedule in float32: each step from torch's own float32 state against clip_adam in float64 -- the
    excess over (rtol 2e-6, atol 2e-7) that float32 arithmetic alone costs; recorded, and inside the tolerance"""
    worst = {}                                         # tensor -> the largest single-step float32 excess
    for p0, g0, m0, v0, lr, t, got in _schedule(wd, torch.float32):
        ref = ut.clip_adam(p0, g0, m0, v0, lr, t, (0.9, 0.999), 1e-8, wd, 5.0)
        assert abs(ref["norm"] - got["norm"]) <= 1e-6 * got["norm"]
        for k in ("p", "g", "m", "v"):
            e = ut.excess(got[k], ref[k])
            worst[k] = max(worst.get(k, 0.0), e)
        # torch_step (state injected into a fresh one-tensor optimizer) is the same update as the running optimizer's,
        # up to the roundings in which torch's one-tensor and many-tensor code paths differ
        again = ut.torch_step(p0, g0, m0, v0, lr, t, (0.9, 0.999), 1e-8, wd, 5.0, torch.float32)
        for k in ("p", "g", "m", "v"):
            assert ut.excess(again[k], got[k]) <= 0.5, (k, t)
            worst[k] = max(worst[k], ut.excess(again[k], ref[k]))
    print("float32 torch vs float64 clip_adam, excess over (2e-6, 2e-7):", worst)
    note_parity("host/float32_torch/wd%g" % wd, **worst)
    assert all(e <= 1.0 for e in worst.values()), worst


def test_float32_restatement_of_the_kernel_arithmetic_is_inside_the_tolerance():
    """clip_adam_float32 (adam_update's roundings in numpy) against clip_adam on the states and sizes of the GPU tests
    (adam_state; t = 3 from a running state, t = 1 from m = v = 0), float32-rounded hyperparameters on both sides:
    recorded, and well inside (2e-6, 2e-7) -- while the same restatement against DOUBLE betas is not (v at n = 1)"""
    f32 = lambda x: float(np.float32(x))
    betas, worst, zero = (f32(0.9), f32(0.999)), {}, {}
    for n in (1, 3, 4, 1023, 1024, 1025, 4100, 2048 * 1024 + 1028):
        for norm, wd in ((12.0, 0.0), (12.0, 1e-3), (2.0, 0.0), (2.0, 1e-3)):
            st = ut.adam_state(n, n % 1000 + int(norm), norm)
            for t, acc in ((3, worst), (1, zero)):
                if t == 1 and n not in (1024, 1025):       # (the zero-state GPU cases; at 2 M elements single gradients
                    continue                               # are small enough for g^2 to underflow in float32)
                if t == 1:
                    st = dict(st, m=np.zeros(n, dtype=np.float32), v=np.zeros(n, dtype=np.float32))
                args = (st["p"], st["g"], st["m"], st["v"], f32(0.01), t, betas, f32(1e-8), f32(wd), 5.0)
                got, ref = ut.clip_adam_float32(*args), ut.clip_adam(*args)
                for k in "pgmv":
                    acc[k] = max(acc.get(k, 0.0), ut.excess(got[k], ref[k]))
    note_parity("host/float32_restatement/running_state", **worst)
    note_parity("host/float32_restatement/zero_state", **zero)
    print("float32 restatement, running state:", worst, "zero state:", zero)
    assert all(e <= 0.25 for e in list(worst.values()) + list(zero.values()))
    st = ut.adam_state(1, 1 + 12, 12.0)
    args = [st["p"], st["g"], st["m"], st["v"], f32(0.01), 3, betas, f32(1e-8), 0.0, 5.0]
    got = ut.clip_adam_float32(*args)
    args[6] = (0.9, 0.999)
    dv = ut.excess(got["v"], ut.clip_adam(*args)["v"])
    note_parity("host/float32_restatement/n1_against_double_betas", v=dv)
    assert dv > 1.0


def test_float32_torch_excess_helper():
    rng = np.random.RandomState(3)
    p, g, m = (rng.normal(size=1025).astype(np.float32) for _ in range(3))
    v = (rng.uniform(size=1025) * 0.01).astype(np.float32)
    e = ut.float32_torch_excess(p, g, m * 0.1, v, 0.01, 3, (0.9, 0.999), 1e-8, 1e-3, 5.0)
    assert set(e) == {"p", "g", "m", "v"} and all(0.0 <= x <= 1.0 for x in e.values()), e


@pytest.mark.parametrize("N_,K", [(1, 1), (33, 65), (37, 19)])
def test_packed_index_is_the_header_layout(N_, K):
    """Wp[jb][kc][lane][e] = W[jb*32 + (lane & 31)][kc*16 + (lane >> 5)*8 + e], 0 outside N x K: a literal loop"""
    kc_total, jb_total = 4 * ((K + 63) // 64), (N_ + 31) // 32
    assert kc_total == ut.packed_kc(K) and jb_total * kc_total * 64 * 8 == ut.packed_elems(N_, K)
    W = np.arange(1, N_ * K + 1, dtype=np.int64).reshape(N_, K)
    Wp = np.zeros((jb_total, kc_total, 64, 8), dtype=np.int64)
    for jb in range(jb_total):
        for kc in range(kc_total):
            for lane in range(64):
                for e in range(8):
                    r, c = jb * 32 + (lane & 31), kc * 16 + (lane >> 5) * 8 + e
                    if r < N_ and c < K:
                        Wp[jb, kc, lane, e] = W[r, c]
    flat = Wp.reshape(-1)
    rr, cc = np.meshgrid(np.arange(N_), np.arange(K), indexing="ij")
    idx = ut.packed_index(rr, cc, kc_total)
    assert np.array_equal(flat[idx], W)
    assert len(np.unique(idx)) == N_ * K                         # one slot per element
    rest = np.ones(flat.shape[0], dtype=bool)
    rest[idx.reshape(-1)] = False
    assert not flat[rest].any()                                  # and every other slot is padding
    assert int(ut.packed_index(N_ - 1, K - 1, kc_total)) == int(idx[-1, -1])


def test_bf16_rne_is_torchs_conversion():
    rng = np.random.RandomState(0)
    x = np.concatenate([rng.normal(size=4096).astype(np.float32) * np.float32(10.0) ** rng.randint(-42, 38, size=4096),
                        ut.special_values()])
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = ut.bf16_rne(x)
    assert np.array_equal(got, want)
    assert np.array_equal(ut.bf16_value(got), torch.from_numpy(x).to(torch.bfloat16).float().numpy())
    # ties to even, by hand: 1 + 2^-8 is halfway between 1 and 1 + 2^-7 (even: 1); 1 + 3 2^-8 goes up to 1 + 2^-6
    assert list(ut.bf16_rne(np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8], dtype=np.float32))) == [0x3f80, 0x3f82]


def test_finalize_is_the_literal_sum():
    rng = np.random.RandomState(1)
    d = [ut.Red(0, 1, 37, 2, 3, 4, 5, 7), ut.Red(1, 0, 8, 30, 2, 1, 3, 4)]
    bufs = [rng.normal(size=1 + 3 * 37).astype(np.float32), rng.normal(size=16).astype(np.float32)]
    flat, sq = ut.finalize(d, bufs, 40)
    want = np.full(40, np.nan)
    for k in d:
        for r in range(k.rows):
            for c in range(k.cols):
                want[k.out_off + r * k.cols + c] = sum(float(bufs[k.buf][k.off + s * k.stride + r * k.ld + c])
                                                      for s in range(k.S))
    assert np.allclose(flat, want, rtol=1e-15, atol=0, equal_nan=True)
    assert np.allclose(sq, [np.nansum(want[2:22] ** 2), np.nansum(want[30:33] ** 2)], rtol=1e-14)
    less, _ = ut.finalize(d, bufs, 40, drop=(0, 2))
    assert not np.allclose(less[2:22], flat[2:22]) and np.array_equal(less[30:33], flat[30:33])
    b = ut.finalize_bound(d, bufs, 40)
    assert b[0] == 0 and (b[2:22] > 0).all()
