"""linear_ref (the restatement the GPU tests of the K5 projection GEMM compare against) checked without a GPU: its
product and activations against torch.nn.functional.linear in float64, the bf16 helpers it reuses against torch's
conversion on specials, ties and subnormals -- and the case table of test_gpu_linear.py held to the dispatch restated in
linear_ref: every case runs the kernel, the half_w tiles and the store paths it claims, stays inside its buffers, and
together the cases claim every instantiation of both kernels, every phase of the three-buffer ring, both half_w values,
both store paths for both output types and all three a_rows variants on both kernels."""
import numpy as np
import pytest
import torch

import linear_ref as lr
import test_gpu_linear as tgl

CASES = tgl.CASES


# ---- the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", lr.ACTS)
@pytest.mark.parametrize("M,N,K,bias", [(7, 5, 11, True), (1, 1, 1, False), (33, 70, 130, True)])
def test_linear_ref_is_torch_linear(M, N, K, bias, act):
    rng = np.random.RandomState(M + N + K)
    A = rng.standard_normal(size=(M, K)).astype(np.float32)
    W = rng.standard_normal(size=(N, K)).astype(np.float32)
    b = rng.standard_normal(size=N).astype(np.float32) if bias else None
    fn = {"none": lambda x: x, "relu": torch.relu, "tanh": torch.tanh}[act]
    for dtype in ("f32", "bf16"):
        tA, tW = torch.from_numpy(A), torch.from_numpy(W)
        if dtype == "bf16":
            tA, tW = tA.bfloat16().float(), tW.bfloat16().float()
        want = fn(torch.nn.functional.linear(tA.double(), tW.double(), torch.from_numpy(b).double() if bias else None))
        got = lr.linear_ref(A, W, b, act, dtype)
        assert got.dtype == np.float64 and got.shape == (M, N)
        err = float(np.abs(got - want.numpy()).max())
        assert err <= 1e-13 * K, (dtype, act, err)
    if K > 1:
        assert not np.array_equal(lr.linear_pre(A, W, b, "f32"), lr.linear_pre(A, W, b, "bf16"))


def test_bf16_helpers_are_torchs_conversion():
    """specials, ties in both directions, subnormals, NaN (quiet, signalling, negative: a quiet NaN comes out)"""
    f = np.float32
    ties = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -23,
                     1 + 2.0 ** -8 - 2.0 ** -24], dtype=f)
    sub = np.array([1, 0x7fff, 0x8000, 0x8001, 0x18000, 0x7fffff, 0x800000], dtype=np.uint32)
    sub = np.concatenate([sub, sub | np.uint32(0x80000000)]).view(f)
    spec = np.array([0.0, -0.0, np.inf, -np.inf, np.finfo(f).max, -np.finfo(f).max, np.finfo(f).tiny], dtype=f)
    rng = np.random.RandomState(1)
    x = np.concatenate([ties, sub, spec, rng.standard_normal(size=2048).astype(f)])
    want = torch.from_numpy(x).bfloat16().view(torch.int16).numpy().view(np.uint16)
    got = lr.bf16_rne(x)
    assert np.array_equal(got, want)
    assert np.array_equal(lr.bf16_value(got).view(np.uint32), torch.from_numpy(x).bfloat16().float().numpy().view(np.uint32))
    assert list(lr.bf16_rne(ties[:2])) == [0x3f80, 0x3f82]
    nans = np.array([0x7fc00000, 0x7f800001, 0xffc00000, 0x7fffffff], dtype=np.uint32).view(f)
    nb = lr.bf16_rne(nans)
    assert ((nb & 0x7fff) > 0x7f80).all() and ((nb & 0x0040) != 0).all()                 # NaN, quiet
    # (torch's conversion gives a NaN too, but its payload depends on the build: compared by class)
    assert nb[0] == 0x7fc0 and torch.isnan(torch.from_numpy(nans).bfloat16().float()).all()
    assert np.isnan(lr.bf16_value(nb)).all()


def test_dispatch_restatement():
    """k5_path, half_w and store_path at hand-worked points"""
    assert lr.k5_path("bf16", 64, 64, 8) == ("dma", 1, 1) and lr.k5_path("bf16", 128, 128, 65) == ("dma", 2, 2)
    assert lr.k5_path("bf16", 64, 128, 65) == ("staged", 2)           # K rounded up to a line does not fit lda
    assert lr.k5_path("bf16", 192, 192, 129) == ("dma", 3, 3) and lr.k5_path("bf16", 1472, 1472, 1433) == ("dma", 3, 23)
    assert lr.k5_path("bf16", 200, 192, 192) == ("staged", 3) and lr.k5_path("bf16", 192, 200, 192) == ("staged", 3)
    assert lr.k5_path("f32", 32, 32, 32) == ("dma", 1, 1) and lr.k5_path("f32", 64, 64, 33) == ("dma", 2, 2)
    assert lr.k5_path("f32", 1440, 1440, 1433) == ("dma", 3, 45) and lr.k5_path("f32", 36, 32, 32) == ("staged", 1)
    assert lr.half_w(64, 0) and not lr.half_w(65, 0) and lr.half_w(136, 128) and not lr.half_w(200, 128)
    sp = lr.store_path
    assert sp("bf16", 0, 144, 0, 0, 136, 0) == "wide" and sp("bf16", 0, 144, 0, 0, 136, 128) == "wide"
    assert sp("bf16", 0, 144, 0, 0, 130, 0) == "wide" and sp("bf16", 0, 144, 0, 0, 130, 128) == "element"
    assert sp("bf16", 0, 148, 0, 0, 136, 0) == "element" and sp("f32", 0, 148, 0, 0, 136, 0) == "wide"
    assert sp("bf16", 0, 288, 1, 132, 136, 0) == "element" and sp("f32", 0, 288, 1, 132, 136, 0) == "wide"
    assert sp("f32", 4, 144, 0, 0, 136, 0) == "element" and sp("f32", 16, 144, 0, 0, 136, 0) == "wide"


# ---- the case table --------------------------------------------------------------------------------------------------
def _tiles(case):
    return lr.column_tiles(case.N)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_runs_what_it_claims(case):
    """the claimed kernel, half_w per column tile and store path per (group, column tile) against the restated dispatch
    (C's alignment from the case's element offset into a 16-byte aligned allocation); and the call is legal and stays
    inside its buffers"""
    epc, line = lr.EPC[case.dtype], lr.LINE[case.dtype]
    assert lr.k5_path(case.dtype, case.lda, case.ldw, case.K) == case.kernel
    if case.kernel[0] == "dma":
        assert case.halfw == "".join("T" if lr.half_w(case.N, n0) else "F" for n0 in _tiles(case))
        assert case.kernel[1] == min(case.kernel[2], 3)
    else:
        assert case.halfw is None
    c_ptr = case.c_off * lr.ESZ[case.c_dtype]
    stores = "|".join("".join(lr.store_path(case.c_dtype, c_ptr, case.ldc, g, case.c_gstride, case.N, n0)[0].upper()
                              for n0 in _tiles(case)) for g in range(case.groups))
    assert stores == case.stores
    # what the entry point requires
    assert case.lda % epc == 0 and case.ldw % epc == 0 and lr.round_up(case.K, epc) <= min(case.lda, case.ldw)
    assert case.M >= 1 and case.N >= 1 and 1 <= case.K <= 1433 and 1 <= case.groups <= (3 if not case.a_shared else 65535)
    # reads: whole lines (DMA) / whole chunks (staged) of rows inside each group's region, on 16-byte boundaries
    reach = lr.round_up(case.K, line if case.kernel[0] == "dma" else epc)
    assert reach <= case.lda and reach <= case.ldw
    a_gs, w_gs = tgl.strides(case)
    assert a_gs % epc == 0 and w_gs % epc == 0 and a_gs != w_gs != case.c_gstride
    assert (a_gs == 0 if case.a_shared else a_gs > tgl.table_rows(case) * case.lda)                  # slack between groups
    assert w_gs > (case.N + tgl.GUARD) * case.ldw
    assert tgl.table_rows(case) > case.M
    # writes: every cell inside its row, the rows disjoint between groups, the allocation holds them and the guard rows
    assert case.ldc > case.groups * case.N
    assert (case.groups - 1) * case.c_gstride + case.N <= case.ldc
    assert case.groups == 1 or case.c_gstride >= case.N
    idx = tgl.cell_index(case)
    assert 0 <= idx.min() and idx.max() < case.c_off + case.M * case.ldc == tgl.out_elems(case) - tgl.GUARD * case.ldc
    assert np.unique(idx).size == idx.size
    assert case.data in ("int", "real") and (case.data == "real" or case.act in ("none", "relu"))


def test_cases_cover_every_kernel_and_path():
    claimed = {}
    for c in CASES:
        claimed.setdefault((c.dtype,) + c.kernel[:2] if c.kernel[0] == "dma" else (c.dtype, "staged"), set()).add(c.act)
    # every instantiation k_linear_nt_dma<{bf16, fp32}, {none, relu, tanh}, {1, 2, 3}> and k_linear_nt<.., false, ..>
    for dt in ("bf16", "f32"):
        for key in [(dt, "dma", 1), (dt, "dma", 2), (dt, "dma", 3), (dt, "staged")]:
            assert claimed.get(key) == set(lr.ACTS), (key, claimed.get(key))
    exact = [c for c in CASES if c.data == "int"]
    for dt in ("bf16", "f32"):
        mine = [c for c in exact if c.dtype == dt]
        dma = [c for c in mine if c.kernel[0] == "dma"]
        # the ring: NBUF = 1 and 2, every phase of NBUF = 3 and a long chain; the staged kernel at the same counts
        nks = {c.kernel[2] for c in dma}
        assert {1, 2, 3, 4, 5, 6, 7} <= nks and max(nks) >= 23
        assert {1, 2, 3, 4, 5, 6, 7} <= {c.kernel[1] for c in mine if c.kernel[0] == "staged"}
        # ragged K: a partial last chunk and a partial last line, on both kernels
        for kind in ("dma", "staged"):
            assert {1, 70, 602} <= {c.K for c in mine if c.kernel[0] == kind}
            assert any(c.K % lr.EPC[dt] for c in mine if c.kernel[0] == kind)
        # half_w: both values, both in one launch, per ring depth 3; a 72-column second tile
        for nbuf in (1, 2, 3):
            hw = "".join(c.halfw for c in dma if c.kernel[1] == nbuf)
            assert "T" in hw and "F" in hw, (dt, nbuf)
        assert any(c.halfw == "FT" for c in dma) and any(c.halfw == "FF" and c.N == 200 for c in dma)
        assert {1, 32, 41, 64, 65, 72, 128, 129, 136, 200} <= {c.N for c in dma if c.kernel == ("dma", 3, 4)}
        # rows: one real row in the second row tile (M = 65) on every ring case, and the edges
        assert all(c.M == 65 and c.N == 136 for c in mine if c.family == "ring")
        assert {1, 63, 64, 65, 129} <= {c.M for c in mine}
        assert any(not c.bias for c in dma) and any(not c.bias for c in mine if c.kernel[0] == "staged")
        # many workgroups of half_w tiles that share A and stream W: the deepest ring's drains and the two-buffer kernel
        busy = {c.kernel for c in dma if c.a_shared and c.groups >= 512 and c.halfw == "T" and c.M == 64}
        assert {("dma", 3, 7), ("dma", 2, 2)} <= busy
        # groups and the three a_rows variants, on both kernels
        for kind in ("dma", "staged"):
            for G in (2, 3):
                assert {"none", "all", "g0"} == {c.a_rows for c in mine if c.kernel[0] == kind and c.groups == G}
        # the staged layouts: both operands off a line multiple, and only W
        line = lr.LINE[dt]
        assert any(c.lda % line and c.ldw % line for c in mine) and any(c.lda % line == 0 and c.ldw % line for c in mine)
        # NaN columns past round_up(K, line) on the DMA path
        assert any(c.lda > lr.round_up(c.K, line) and c.ldw > lr.round_up(c.K, line) for c in dma)
    # both store paths for both output types, from either input type; one launch with a wide and an element tile; each
    # of the four conditions of the wide path turned off on its own
    for cd in ("bf16", "f32"):
        for dt in ("bf16", "f32"):
            st = [c for c in exact if c.c_dtype == cd and c.dtype == dt]
            assert any("W" in c.stores for c in st) and any("E" in c.stores for c in st)
            assert any(c.stores == "WE" for c in st) and any(c.stores == "WW|EE" for c in st)
            epc = lr.EPC[cd]
            ok = [c for c in st if c.family == "store"]
            assert any(c.N % epc and c.ldc % epc == 0 and c.c_off == 0 for c in ok)                       # ragged N
            assert any(c.N % epc == 0 and c.ldc % epc and c.c_off == 0 for c in ok)                       # ldc
            assert any(c.N % epc == 0 and c.ldc % epc == 0 and c.c_gstride % epc and c.groups > 1 for c in ok)
            assert any(c.N % epc == 0 and c.ldc % epc == 0 and (c.c_off * lr.ESZ[cd]) % 16 == 4 for c in ok)
            assert any(c.c_off == 602 and c.ldc == 704 and (602 * lr.ESZ[cd]) % 16 for c in ok)            # the engines'
    # the bounded cases: one shape per kernel and ring depth, every act, both output types, both store paths
    real = [c for c in CASES if c.data == "real"]
    for dt in ("bf16", "f32"):
        for cd in ("bf16", "f32"):
            for act in lr.ACTS:
                kinds = {c.kernel[:2] if c.kernel[0] == "dma" else ("staged",) for c in real
                         if (c.dtype, c.c_dtype, c.act) == (dt, cd, act) and c.stores == "WE"}
                assert kinds == {("dma", 1), ("dma", 2), ("dma", 3), ("staged",)}, (dt, cd, act, kinds)


def test_exact_cases_are_exact():
    """integer operands: every pre-activation an integer below 2^24 (checked where the operands are drawn), a fair
    share of negative ones for relu, the operands exactly representable in bf16, the a_rows permutation with a repeat
    and unnamed table rows"""
    seen = set()
    for case in CASES:
        if case.data != "int" or case.K not in (1, 192, 1433) or (case.K, case.dtype, case.a_rows) in seen:
            continue
        seen.add((case.K, case.dtype, case.a_rows))
        L = tgl.logical(case)
        assert 64 * case.K + 100 < 2 ** 24
        for g in range(case.groups):
            assert np.array_equal(lr.bf16_value(lr.bf16_rne(L["A"][g])), L["A"][g])
            assert float(np.abs(L["pre"][g]).max()) < 2 ** 24 and 0.2 < float((L["pre"][g] < 0).mean()) < 0.8
        if case.a_rows != "none":
            assert np.unique(L["ids"]).size < case.M and np.unique(L["ids"]).size < tgl.table_rows(case)
            assert not np.array_equal(L["ids"], np.arange(case.M))


def test_host_buffers_hold_nan_where_nothing_may_be_read():
    """the layout the GPU test builds: zeros exactly in [K, round_up(K, line or chunk)), NaN past it, in the rows no
    index names, in W rows >= N and in the slack between groups; feeding the buffers back through the reference with
    the padding included gives the same product"""
    for name in ("ring-bf16-K70-dma", "ring-f32-K70-staged", "groups-bf16-G3-g0-dma", "groups-f32-G2-all-staged",
                 "cols-f32-N41"):
        case = next(c for c in CASES if c.name == name)
        L = tgl.logical(case)
        A, W = tgl.host_buffers(case)
        a_gs, w_gs = tgl.strides(case)
        T = tgl.table_rows(case)
        reach = lr.round_up(case.K, (lr.LINE if case.kernel[0] == "dma" else lr.EPC)[case.dtype])
        for g in range(case.groups):
            ra = A[g * a_gs:g * a_gs + T * case.lda + 3 * lr.EPC[case.dtype]]
            rows = ra[:T * case.lda].reshape(T, case.lda)
            used = np.zeros(T, dtype=bool)
            used[L["used"][g]] = True
            assert np.isnan(rows[~used]).all() and (~used).any() and np.isnan(ra[T * case.lda:]).all()
            assert not np.isnan(rows[used, :reach]).any() and not rows[used, case.K:reach].any()
            assert np.isnan(rows[used, reach:]).all()
            rw = W[g * w_gs:(g + 1) * w_gs]
            wr = rw[:case.N * case.ldw].reshape(case.N, case.ldw)
            assert np.isnan(rw[case.N * case.ldw:]).all() and rw[case.N * case.ldw:].size > tgl.GUARD * case.ldw
            assert not np.isnan(wr[:, :reach]).any() and not wr[:, case.K:reach].any() and np.isnan(wr[:, reach:]).all()
            src = rows[L["ids"]] if tgl.indirect(case, g) else rows[:case.M]
            bias = None if L["bias"] is None else L["bias"][g]
            assert np.array_equal(lr.linear_pre(src[:, :reach], wr[:, :reach], bias, case.dtype), L["pre"][g])


def test_bounds():
    """abs_bound against its formula on a hand-worked cell; tanh_term between one and six float32 roundings; the bf16
    output term"""
    A = np.array([[1.0, -2.0, 0.5]], dtype=np.float32)
    W = np.array([[3.0, 1.0, -4.0]], dtype=np.float32)
    b = np.array([-0.25], dtype=np.float32)
    assert np.array_equal(lr.abs_bound(A, W, b, 3), np.array([[5 * 2.0 ** -24 * (3 + 2 + 2 + 0.25)]]))
    assert np.array_equal(lr.abs_bound(A, W, None, 3), np.array([[5 * 2.0 ** -24 * 7]]))
    v = np.array([0.0, 0.1, 1.0, 5.0, 50.0, -1.0])
    t = lr.tanh_term(v, np.zeros(6))
    assert (t >= 2.0 ** -24).all() and (t <= 10 * 2.0 ** -24).all() and t[0] > t[2] > t[3] > t[4] and t[2] == t[5]
    assert (lr.tanh_term(v, np.full(6, 0.01)) >= t).all()
    pre, pb = np.array([[2.0]]), np.array([[1e-6]])
    assert lr.out_bound(pre, pb, "none", "f32")[0, 0] == 1e-6 == lr.out_bound(pre, pb, "relu", "f32")[0, 0]
    assert lr.out_bound(pre, pb, "none", "bf16")[0, 0] == 1e-6 + 2.0 ** -8 * 2.0
    assert lr.out_bound(pre, pb, "tanh", "bf16")[0, 0] == 1e-6 + lr.tanh_term(pre, pb)[0, 0] + 2.0 ** -8 * np.tanh(2.0)
