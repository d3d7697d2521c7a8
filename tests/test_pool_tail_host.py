"""pool_tail_ref (the restatement the GPU tests of K3's backward outputs and of the pool backward kernels compare
against) checked without a GPU: its routes, bias gradients and merges against torch autograd in float64 of the literal
formulation (relu(linear) -> view(M, n, H) -> max(1) / mean(1), the level's cat) on inputs without ties, its
first-maximum rule against np.argmax on inputs with ties, its mask words against a literal loop -- and the conditions
the K3 fixtures of test_gpu_pool_tail.py are held to (ties, zero pre-activations, argmax spread), for every case.

Measured here for pool_tail_ref.K3_CASES: 17 - 77 % of the cells with n > 1 have a tied positive maximum, 1 - 15 % of
the pre-activations are exactly 0, and with n >= 5 the argmax is not row 0 in 63 - 94 % of the cells."""
import numpy as np
import pytest
import torch

import pool_tail_ref as pr


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float(np.abs(a - b).max())
    assert err <= 1e-12 * max(1.0, float(np.abs(b).max())), (what, err)


@pytest.mark.parametrize("mode", ["max", "mean"])
@pytest.mark.parametrize("M,n,K,H", [(7, 5, 11, 64), (3, 1, 4, 32), (4, 25, 9, 96)])
def test_routes_and_bias_gradients_are_autograd(mode, M, n, K, H):
    """d loss / d pre-activation and d loss / d bias of relu(linear(x)).view(M, n, H).max(1) / .mean(1), loss = <pooled,
    g>, against route_max / route_mean and bias_max / bias_mean fed with what K3 leaves behind (argmax, pooled; the
    sign words)"""
    torch.manual_seed(M * 100 + n)
    x = torch.randn(M * n, K, dtype=torch.float64)
    lin = torch.nn.Linear(K, H).double()
    g = torch.randn(M, H, dtype=torch.float64)
    pre = lin(x)
    pre.retain_grad()
    hid = torch.relu(pre).view(M, n, H)
    pooled = hid.max(1)[0] if mode == "max" else hid.mean(1)
    (pooled * g).sum().backward()
    hid_np = hid.detach().numpy()
    pos = np.sort(hid_np, axis=1)[:, ::-1]
    if n > 1:                                                    # no tied positive maxima: autograd is unambiguous
        assert ((pos[:, 0] > pos[:, 1]) | (pos[:, 0] == 0)).all()
    if mode == "max":
        arg = pr.first_argmax(hid_np)
        route = pr.route_max(g.numpy(), pooled.detach().numpy(), arg, n)
        bias, _ = pr.bias_max(g.numpy(), pooled.detach().numpy())
    else:
        words = pr.mask_words(pre.detach().numpy())
        bits = pr.mask_bits(words, H)
        assert np.array_equal(bits, pre.detach().numpy() > 0)
        route = pr.route_mean(g.numpy(), bits, n)
        bias, _ = pr.bias_mean(g.numpy(), bits, n)
    _close(route, pre.grad.numpy(), ("route", mode))
    _close(bias, lin.bias.grad.numpy(), ("bias", mode))
    _close(route.sum(axis=0), bias, "the bias gradient is the column sum of the route")


def _dyadic(rng, *shape):
    """float32 values k / 1024, |k| <= 4096: sums of two are exact in float32"""
    return (rng.randint(-4096, 4097, size=shape) / 1024.0).astype(np.float32)


@pytest.mark.parametrize("r_x,r0", [(9, 4), (6, 6), (3, 8), (0, 0), (14, 14), (14, 0)])
def test_pool_merge_is_autograd_of_the_level(r_x, r0):
    """x = relu(z) [R, D] feeds fc_x with its first r_x rows and the pooling MLP with its rows from r0 on (the level's
    cat): d loss / d z for loss = <x[:r_x], DX> + <x[r0:], DN>"""
    R, D = 14, 8
    rng = np.random.RandomState(r_x * 20 + r0)
    z = torch.tensor(rng.normal(size=(R, D)), dtype=torch.float64, requires_grad=True)
    DX, DN = _dyadic(rng, max(r_x, 1), D), _dyadic(rng, max(R - r0, 1), D)
    x = torch.relu(z)
    loss = (x[:r_x] * torch.from_numpy(DX[:r_x]).double()).sum() + (x[r0:] * torch.from_numpy(DN[:R - r0]).double()).sum()
    loss.backward()
    got = pr.pool_merge(x.detach().numpy(), DX, r_x, DN, r0, R)
    assert got.dtype == np.float32
    _close(got, z.grad.numpy(), (r_x, r0))


def test_pool_merge_keeps_the_signed_zero_of_a_lone_source():
    """the float32 definition the GPU test pins bit for bit: DX alone keeps its bits, 0 + DN makes -0 a +0"""
    Hp = np.ones((3, 4), dtype=np.float32)
    DX = np.full((1, 4), -0.0, dtype=np.float32)
    DN = np.full((2, 4), -0.0, dtype=np.float32)
    out = pr.pool_merge(Hp, DX, 1, DN, 1, 3).view(np.uint32)
    assert (out[0] == 0x80000000).all() and (out[1:] == 0).all()
    both = pr.pool_merge(Hp, np.full((3, 4), -0.0, dtype=np.float32), 3, np.full((3, 4), -0.0, dtype=np.float32), 0, 3)
    assert (both.view(np.uint32) == 0x80000000).all()


@pytest.mark.parametrize("form", ["pool_level0", "mean_over_prep", "attention"])
def test_attn_merge_is_autograd_of_the_level(form):
    """a 3-hop frontier (5 seeds, fan-outs 3 and 4): every row feeds att(.) (DATT), the first r_x rows feed fc_x (DX)
    and every child feeds its parent's aggregate with weight ws or 1 / fan -- d loss / d z against attn_merge in the
    engines' three call shapes"""
    rng = np.random.RandomState(len(form))
    D, off, fan = 6, [0, 5, 20], [1, 3, 4]
    R, r_x = 80, 20
    gated = form != "pool_level0"
    z = torch.tensor(rng.normal(size=(R, D)), dtype=torch.float64, requires_grad=True)
    x = torch.relu(z) if gated else z
    DATT = None if form == "mean_over_prep" else rng.normal(size=(R, D))
    DX = rng.normal(size=(r_x, D))
    DAGG = rng.normal(size=(off[2], D))
    ws = rng.uniform(size=R - off[1]) if form == "attention" else None
    loss = (x[:r_x] * torch.from_numpy(DX)).sum()
    if DATT is not None:
        loss = loss + (x * torch.from_numpy(DATT)).sum()
    for k in (1, 2):
        lo, hi = off[k], off[k + 1] if k + 1 < len(off) else R
        kids = x[lo:hi].view(-1, fan[k], D)
        w = torch.from_numpy(ws[lo - off[1]:hi - off[1]]).view(-1, fan[k], 1) if ws is not None else 1.0 / fan[k]
        agg = (kids * w).sum(1)                                    # [parents of hop k, D]
        loss = loss + (agg * torch.from_numpy(DAGG[off[k - 1]:off[k - 1] + agg.shape[0]])).sum()
    loss.backward()
    val, mag = pr.attn_merge(DATT, DX, r_x, DAGG, ws, x.detach().numpy() if gated else None, off, fan, R)
    _close(val, z.grad.numpy(), form)
    assert (mag >= np.abs(val) - 1e-12).all()


def test_first_maximum_rule_is_np_argmax_on_ties():
    rng = np.random.RandomState(3)
    hid = rng.randint(0, 3, size=(40, 9, 32))                      # three values over nine rows: ties everywhere
    hid[0] = 0                                                     # all-zero cells: row 0
    arg = pr.first_argmax(hid)
    assert np.array_equal(arg, np.argmax(hid, axis=1))
    assert (np.sort(hid, axis=1)[:, -1] == np.sort(hid, axis=1)[:, -2]).mean() > 0.8 and (arg[0] == 0).all()


def test_mask_words_bit_order():
    """bit c % 32 of word c / 32, by a literal loop; and the round trip through mask_bits"""
    rng = np.random.RandomState(4)
    pre = rng.randint(-2, 3, size=(5, 96))
    words = pr.mask_words(pre)
    want = np.zeros((5, 3), dtype=np.uint32)
    for r in range(5):
        for c in range(96):
            if pre[r, c] > 0:
                want[r, c // 32] |= np.uint32(1 << (c % 32))
    assert words.dtype == np.uint32 and np.array_equal(words, want)
    assert np.array_equal(pr.mask_bits(words, 96), pre > 0)


@pytest.mark.parametrize("case", pr.K3_CASES, ids=[c.name for c in pr.K3_CASES])
def test_k3_fixture_conditions(case):
    """every K3 case of the GPU test, generated with its seed: exact in float32, one duplicated neighbour per segment,
    enough tied positive maxima, enough pre-activations that are exactly 0, the argmax spread over the rows"""
    table, ids, W, b = pr.k3_inputs(case)
    ref = pr.k3_exact(table, ids, W, b, case.M, case.n, "max")
    assert int(np.abs(ref["pre"]).max()) < 2 ** 24
    census = pr.k3_census(ref, case.n)
    print(case.name, census)
    if case.n > 1:
        seg = ids.reshape(case.M, case.n)
        assert all(np.unique(row).shape[0] < case.n for row in seg)
        assert census["tied"] >= 0.05
    assert census["zero"] >= 0.001
    if case.n >= 5:
        assert census["not_row0"] >= 0.5
    mean = pr.k3_exact(table, ids, W, b, case.M, case.n, "mean")
    assert np.array_equal(mean["pooled"], ref["hid"].sum(axis=1) / float(case.n)) and mean["pooled"].dtype == np.float64
    if case.H % 32 == 0:
        assert np.array_equal(pr.mask_bits(ref["mask"], case.H), ref["pre"] > 0)
    else:
        assert ref["mask"] is None
