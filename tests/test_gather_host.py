"""gather_ref (the restatement the GPU tests of the gather kernels compare against) checked without a GPU: its in-order
float32 mean against its float64 mean within the bound the scatter test uses, its dispatch restatement at hand-worked
points -- and the case table of test_gpu_gather.py held to that restatement: every case runs the chunk width, the store
path, the row-copy path and the kernel it claims, stays inside its buffers, and together the cases claim every
instantiation, path, fan-out and item count listed in test_cases_cover_every_kernel_and_path."""
import numpy as np
import pytest
import torch

import gather_ref as gr
import test_gpu_gather as tgg

SINGLES, MULTIS = tgg.SINGLES, tgg.MULTIS


# ---- the reference ---------------------------------------------------------------------------------------------------
def test_mean_in_order_is_a_float32_chain():
    """hand-worked: 2^24 + 1 + 1 in float32 stays 2^24 from the left and reaches 2^24 + 2 from the right; the sum starts
    at +0 (a lone -0 row gives +0); one division"""
    f = np.float32
    rows = np.array([[[2.0 ** 24], [1.0], [1.0]]], dtype=f)
    assert gr.mean_in_order(rows)[0, 0] == f(2.0 ** 24) / f(3)
    assert gr.mean_in_order(rows[:, ::-1])[0, 0] == f(2.0 ** 24 + 2) / f(3)
    assert gr.mean64(rows)[0, 0] == (2.0 ** 24 + 2) / 3
    z = gr.mean_in_order(np.array([[[-0.0]]], dtype=f))
    assert z.view(np.uint32)[0, 0] == 0
    sc = np.array([0.25], dtype=f)
    assert gr.mean_in_order(np.array([[[3.0], [2.0]]], dtype=f), sc)[0, 0] == f(1.25) / f(2)
    assert gr.mean64(np.array([[[3.0], [2.0]]]), sc)[0, 0] == 0.625


def test_bf16_bits_and_e4m3_decode():
    x = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -1.5, 0.0], dtype=np.float32)
    want = torch.from_numpy(x).bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(gr.out_bits(x, "bf16"), want) and list(want[:2]) == [0x3f80, 0x3f82]
    assert np.array_equal(gr.out_bits(x, "f32"), x.view(np.uint32))
    v = gr.decode_e4m3(np.arange(256, dtype=np.uint8))
    assert v[0x38] == 1.0 and v[0x7e] == 448.0 and v[0x01] == 2.0 ** -9 and v[0xb8] == -1.0
    assert np.isnan(v[0x7f]) and np.isnan(v[0xff]) and np.isfinite(np.delete(v, [0x7f, 0xff])).all()


def test_dispatch_restatement():
    """vec, fp8_out_vec_ok, fill_multi, wide, grid_for and bwd_vec at hand-worked points"""
    v = gr.vec
    assert v("bf16", "bf16", 64, 56, 0, 0, 40) == 8 and v("bf16", "f32", 64, 56, 0, 0, 40) == 4
    assert v("bf16", "bf16", 132, 136, 0, 0, 130) == 4 and v("bf16", "bf16", 16, 20, 0, 0, 9) == 4
    assert v("bf16", "bf16", 602, 12, 0, 0, 9) == 2 and v("f32", "f32", 131, 136, 0, 0, 130) == 1
    assert v("bf16", "bf16", 7, 16, 0, 0, 7) == 1 and v("bf16", "bf16", 8, 16, 0, 0, 7) == 8
    assert v("bf16", "bf16", 16, 24, 2, 0, 9) == 1 and v("bf16", "bf16", 16, 24, 4, 0, 9) == 2
    assert v("bf16", "bf16", 16, 24, 8, 0, 9) == 4 and v("f32", "f32", 16, 24, 0, 4, 9) == 1
    assert v("f32", "bf16", 16, 24, 0, 8, 9) == 4 and v("f32", "bf16", 16, 24, 0, 4, 9) == 2
    ok = gr.fp8_out_vec_ok
    assert ok(0, "bf16", 17, 24) and not ok(0, "bf16", 17, 25) and not ok(2, "bf16", 17, 24) and not ok(0, "bf16", 17, 16)
    assert ok(0, "f32", 17, 20) and not ok(4, "f32", 17, 20)
    assert gr.fp8_written_cols(0, "bf16", 17, 24) == 24 and gr.fp8_written_cols(0, "f32", 17, 24) == 20
    assert gr.fp8_written_cols(2, "bf16", 17, 24) == 17
    p = gr.fill_multi([5, 0, 301, 7], [1, 8, 1, 3], "bf16", "bf16", 64, 42, 56)
    assert p == dict(vec=8, chunks=6, all_single=False, rpi=[4, 1, 4, 1], first=[0, 12, 12, 468, 510])
    p = gr.fill_multi([5, 301], [1, 1], "bf16", "bf16", 64, 42, 56)
    assert p["all_single"] and p["rpi"] == [1, 1] and p["first"] == [0, 30, 1836]
    p = gr.fill_multi([5, 7], [1, 3], "f32", "bf16", 64, 42, 56)
    assert p["vec"] == 4 and p["chunks"] == 11 and p["rpi"] == [1, 1]
    assert gr.multi_path("bf16", "bf16", False, [4, 1]) == ["rows4", "mean"]
    assert gr.multi_path("bf16", "bf16", True, [1, 1]) == ["copy4", "copy4"]
    assert gr.multi_path("f32", "bf16", True, [1]) == ["mean"] and gr.multi_path("fp8", "bf16", True, [1]) == ["mean"]
    for bad in (dict(M=[], n=[]), dict(M=[1] * 9, n=[1] * 9), dict(M=[1], n=[0]), dict(M=[1], n=[1], ld=36),
                dict(M=[1], n=[1], out_dtype="f32"), dict(M=[1], n=[1], out_addrs=[2]), dict(M=[1], n=[1], D=60, out_ld=56)):
        kw = dict(dtype="bf16", out_dtype="bf16", ld=64, D=42, out_ld=56)
        kw.update(bad)
        with pytest.raises(ValueError):
            gr.fill_multi(**kw)
    assert gr.wide("bf16", [True, False], [9, 12], 100) and not gr.wide("bf16", [True, False], [8, 12], 100)
    assert not gr.wide("f32", [True], [9], 100) and not gr.wide("bf16", [True], [9], 256 * 1024 + 1)
    assert gr.wide("bf16", [True], [9], 256 * 1024) and not gr.wide("bf16", [True], [9], 100, in_launch_norm=True)
    assert gr.grid_for(0) == 1 and gr.grid_for(257) == 2 and gr.grid_for(16384 * 256 + 1) == 16384
    assert gr.workgroups(275, 19) == 2 + 19
    assert gr.bwd_vec(48, 52, 56, 0, 0) == 4 and gr.bwd_vec(50, 52, 56, 0, 0) == 1 and gr.bwd_vec(48, 52, 57, 0, 0) == 1
    assert gr.bwd_vec(48, 52, 56, 4, 0) == 1 and gr.bwd_vec(48, 52, 56, 0, 4) == 1
    assert gr.bwd_items(37, 3, 48, 4) == 37 * 3 * 12 and gr.bwd_items(37, 3, 48, 1) == gr.scatter_items(37, 3, 48)
    for bad in (dict(n=0), dict(ld=30), dict(out_ld=30), dict(dtype="fp8")):
        kw = dict(dtype="bf16", out_dtype="bf16", ld=64, out_ld=56, M=3, n=2, D=40)
        kw.update(bad)
        with pytest.raises(ValueError):
            gr.check_single(**kw)


# ---- the case table --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SINGLES, ids=[c.name for c in SINGLES])
def test_single_case_runs_what_it_claims(case):
    """the claimed chunk width and written columns (store path for FP8) from the case's element offsets into 16-byte
    aligned allocations; the call is legal and stays inside its buffers, and the sentinel shows on every side"""
    taddr, oaddr = case.tab_off * gr.ESZ[case.dtype], case.out_off * gr.ESZ[case.out_dtype]
    if case.dtype == "fp8":
        gr.check_fp8(case.ld, case.out_ld, case.M, case.n, case.D, case.out_dtype, oaddr)
        assert case.vec == 16 and case.tab_off == 0 and case.fn in ("fp8", "rows_fp8")
        assert (case.store == "VS") == gr.fp8_out_vec_ok(oaddr, case.out_dtype, case.D, case.out_ld)
        assert case.cols == gr.fp8_written_cols(oaddr, case.out_dtype, case.D, case.out_ld)
        reach = gr.round_up(case.D, 16)
        assert case.fn == "fp8" or (case.n == 1 and case.ids)
    else:
        gr.check_single(case.dtype, case.out_dtype, case.ld, case.out_ld, case.M, case.n, case.D)
        assert case.fn == "mean" and case.store is None
        assert case.vec == gr.vec(case.dtype, case.out_dtype, case.ld, case.out_ld, taddr, oaddr, case.D)
        assert case.cols == gr.written_cols(case.D, case.vec)
        reach = case.cols
    assert case.D <= case.cols <= case.out_ld and reach <= case.ld
    assert case.cols < case.out_ld                                     # a sentinel column behind the written ones
    assert case.data in ("int", "real")
    if case.M < 100000:
        inp = tgg.case_inputs(case)
        assert inp["R"] > int(inp["named"].sum()) >= (1 if case.M else 0)          # rows no id names: NaN
        tab = tgg.host_table(inp, case.dtype, case.ld, case.tab_off)
        assert tab.size >= case.tab_off + (inp["R"] - 1) * case.ld + reach


@pytest.mark.parametrize("case", MULTIS, ids=[c.name for c in MULTIS])
def test_multi_case_runs_what_it_claims(case):
    """rpi, first and the per-segment path against fill_multi; the kernel of the side-role launch against `wide`; the
    segment outputs 16-byte aligned, adjacent and disjoint"""
    Ms, ns, has = [s[0] for s in case.segs], [s[1] for s in case.segs], [s[2] for s in case.segs]
    rows = tgg.seg_rows(case)
    esz = gr.ESZ[case.out_dtype]
    oaddrs = [4096 + r * case.out_ld * esz for r in rows[:-1]]
    plan = gr.fill_multi(Ms, ns, case.dtype, case.out_dtype, case.ld, case.D, case.out_ld, [4096] * len(Ms), oaddrs)
    assert tuple(plan["rpi"]) == case.rpi and tuple(plan["first"]) == case.first
    assert tuple(gr.multi_path(case.dtype, case.out_dtype, plan["all_single"], plan["rpi"])) == case.path
    assert tgg.multi_cols(case) < case.out_ld and tgg.multi_cols(case) == gr.round_up(case.D, 16 // esz if case.dtype == "fp8"
                                                                                      else plan["vec"])
    total = case.first[-1]
    assert total > 0
    if case.entry == "multi_adam":
        assert case.dtype == case.out_dtype == "bf16"
        assert case.kernel == ("wide" if gr.wide(case.dtype, has, ns, total) else "narrow")
    else:
        assert case.kernel == case.entry
    assert rows[0] == 1 and all(b - a == M for a, b, M in zip(rows, rows[1:], Ms))


def test_cases_cover_every_kernel_and_path():
    fam = lambda f, cs=SINGLES: [c for c in cs if c.family == f]
    # 1. the fan-out sweep: every n, with and without ids, all four type pairs, both tiers, at M = 33, D = 40, ld = 64
    for dt, od in tgg.PAIRS:
        for data in ("int", "real"):
            mine = [c for c in fam("sweep") if (c.dtype, c.out_dtype, c.data) == (dt, od, data)]
            assert all((c.M, c.D, c.ld) == (33, 40, 64) for c in mine)
            assert {c.n for c in mine if c.ids} == {1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 23, 24, 25, 31, 32, 33}
            assert {c.n for c in mine if not c.ids} == {1, 3, 4, 5, 7, 8, 9, 11, 12, 13, 16, 21}
    # the ladder: every combination of (eights, fours, ones > 0)
    assert {(n // 8 > 0, n % 8 // 4 > 0, n % 4 > 0) for n in tgg.SWEEP_NULL} == \
        {(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)} - {(False, False, False)}
    # 2. dispatch_vec: every reachable VEC per pair, each way of selecting it, the D and M sets
    for dt, od in tgg.PAIRS:
        mine = [c for c in fam("vec") if (c.dtype, c.out_dtype) == (dt, od)]
        assert {c.vec for c in mine} == ({8, 4, 2, 1} if (dt, od) == ("bf16", "bf16") else {4, 2, 1})
        assert any(c.vec == 4 and c.ld % 8 == 4 and c.out_ld % 8 == 0 for c in mine)
        assert any(c.vec == 4 and c.ld % 8 == 0 and c.out_ld % 8 == 4 for c in mine)
        assert any(c.vec == 2 and c.ld == 602 for c in mine) and any(c.vec == 1 and c.ld % 2 for c in mine)
        assert any(c.vec == 1 and c.D == c.ld == 7 for c in mine)
        assert any(c.vec == 1 and c.tab_off == 1 and c.ld % 8 == 0 and c.out_ld % 8 == 0 for c in mine)
        assert any(c.vec == 1 and c.out_off == 1 and c.ld % 8 == 0 and c.out_ld % 8 == 0 for c in mine)
        assert {c.D for c in mine} == {1, 7, 9, 130, 602} and {c.M for c in mine} == {1, 33, 257}
        for v in {c.vec for c in mine} - {1}:
            assert any(c.vec == v and c.cols > c.D for c in mine), v                  # a zero tail at every width
        assert {c.data for c in mine} == {"int", "real"} and any(not c.ids for c in mine)
    # 3. the grid cap: the smallest item count past it, and M = 0
    cap = next(c for c in fam("cap") if c.M)
    assert (cap.dtype, cap.n) == ("bf16", 2) and tgg.POOL == 64
    items = cap.M * gr.chunks(cap.D, cap.vec)
    assert items == gr.GRID_CAP * 256 + 1 and gr.workgroups(items) == gr.GRID_CAP
    assert any(c.M == 0 for c in fam("cap"))
    assert all(gr.workgroups(c.M * gr.chunks(c.D, c.vec)) < gr.GRID_CAP for c in SINGLES if c.family != "cap")
    # 4. all-single
    one = fam("single", MULTIS)
    assert all(set(c.path) == {"copy4"} and (c.dtype, c.out_dtype) == ("bf16", "bf16") for c in one)
    totals = sorted(c.first[-1] for c in one)
    assert totals[:4] == [1, 1023, 1024, 1025] and 4900 <= totals[4] <= 5100
    assert {len(c.segs) for c in one} >= {1, 3, 8} and {c.D for c in one} == {8, 9, 602}
    assert all(c.ld == gr.round_up(c.D, 8) + 8 for c in one)
    kinds = {frozenset(s[2] for s in c.segs if s[0]) for c in one}
    assert kinds >= {frozenset([True]), frozenset([False]), frozenset([True, False])}
    assert any(c.segs[i][0] == 0 and 0 < i < len(c.segs) - 1 for c in one for i in range(len(c.segs)))
    assert any(c.D % 8 for c in one)
    # 5. mixed
    mix = fam("mixed", MULTIS)
    lowp = [c for c in mix if c.dtype == "bf16"]
    for data in ("int", "real"):
        r4 = {(s[0], s[2]) for c in lowp if c.data == data for s, p in zip(c.segs, c.path) if p == "rows4"}
        assert r4 >= {(M, i) for M in (1, 2, 3, 4, 5, 301) for i in (True, False)}
        assert {s[1] for c in lowp if c.data == data for s in c.segs} >= {1, 3, 8, 9, 25}
        for od in ("f32", "bf16"):
            assert any((c.dtype, c.out_dtype, c.data) == ("f32", od, data) and set(c.path) == {"mean"} and
                       1 in {s[1] for s in c.segs} for c in mix)
    assert all("rows4" in c.path and "mean" in c.path for c in lowp) and all(c.D % 8 for c in lowp)
    assert any(len(c.segs) == 8 for c in lowp) and any(s[0] == 0 for c in mix for s in c.segs)
    # 6. FP8
    for od in ("bf16", "f32"):
        f8 = [c for c in fam("fp8") if c.out_dtype == od]
        for st, why in (("VS", lambda c: True), ("ES", lambda c: c.out_ld % 2 == 1), ("ES", lambda c: c.out_off == 1)):
            assert {(c.n, c.D) for c in f8 if c.store == st and why(c)} == \
                {(n, D) for n in (1, 8, 9, 25) for D in (16, 17, 40, 602)}
        assert {c.fn for c in f8} == {"fp8", "rows_fp8"} and any(not c.ids for c in f8)
        m8 = [c for c in fam("fp8", MULTIS) if c.out_dtype == od]
        assert m8 and all(c.entry == "multi_fp8" for c in m8) and any(all(s[1] == 1 for s in c.segs) for c in m8)
        assert any(not s[2] for c in m8 for s in c.segs) and any(s[0] == 0 for c in m8 for s in c.segs)
    # 7. the side role: the wide kernel over the listed fan-outs (n = 12 without a row list does not count), and the
    # narrow kernel by the item count alone
    role = fam("role", MULTIS)
    w = [c for c in role if c.kernel == "wide"]
    assert {c.data for c in w} == {"int", "real"}
    for c in w:
        assert {s[1] for s in c.segs if s[2]} == {1, 9, 16, 17, 25, 33, 40} and [s[1] for s in c.segs if not s[2]] == [12]
        assert c.first[-1] <= gr.WIDE_ITEMS
    nar = [c for c in role if c.kernel == "narrow"]
    assert nar and all(max(s[1] for s in c.segs if s[2]) > 8 and c.first[-1] > gr.WIDE_ITEMS for c in nar)
    assert all(gr.workgroups(c.first[-1]) < gr.GRID_CAP for c in MULTIS)
    # 8. backward, 9. scatter
    assert {(D, v) for _n, D, _l, _o, _i, _f, v in tgg.BWD} >= {(4, 4), (48, 4), (50, 1)}
    assert any(v == 1 and o % 2 for _n, D, _l, o, _i, _f, v in tgg.BWD)
    assert any(v == 1 and f == 1 for *_x, f, v in tgg.BWD) and any(v == 1 and i == 1 for *_x, i, _f, v in tgg.BWD)
    for name, D, ld, old, ioff, ooff, v in tgg.BWD:
        assert gr.bwd_vec(D, ld, old, 4 * ioff, 4 * ooff) == v and ld >= D < old, name
    assert tgg.BWD_N == (1, 3, 10) and tgg.BWD_M == (1, 37)
    sc = tgg.SCATTER
    assert {(n, D) for n, D, _s, _d, _e in sc} == {(n, D) for n in (1, 3) for D in (1, 16, 50)}
    assert {np.float32(s) for _n, _D, s, _d, _e in sc} == {np.float32(1), np.float32(0.25), np.float32(1.0 / 3.0)}
    assert all((d == "int") == (np.log2(s) == int(np.log2(s))) for _n, _D, s, d, _e in sc) and any(e for *_x, e in sc)
    assert tgg.SC_NAMED * 4 < tgg.SC_M and tgg.SC_NAMED < tgg.SC_ROWS


# ---- the inputs ------------------------------------------------------------------------------------------------------
def _all_inputs():
    """(case name, segment inputs, out dtype) of every case but the 838 861-row one (same construction, same range)"""
    for c in SINGLES:
        if c.M < 100000:
            yield c.name, tgg.case_inputs(c), c.out_dtype, c.data
    for c in MULTIS:
        for s, inp in enumerate(tgg.case_inputs(c)):
            yield "%s/%d" % (c.name, s), inp, c.out_dtype, c.data


def test_integer_inputs_keep_every_partial_sum_exact():
    """int tier: integers in [-64, 64], so every partial sum in ANY order is an integer of magnitude <= 64 n < 2^24; FP8:
    multiples of 2^-9 of magnitude <= 448, so 2^9 times any partial sum is an integer <= 2^9 448 n < 2^24; the scales
    are powers of two in [2^-8, 2^8]"""
    seen = 0
    for name, inp, _od, data in _all_inputs():
        if data != "int":
            continue
        v = inp["values"][inp["named"]].astype(np.float64)
        unit = 2.0 ** 9 if inp["codes"] is not None else 1.0
        assert np.array_equal(v * unit, np.rint(v * unit)), name
        assert float(np.abs(v * unit).max(initial=0.0)) * inp["n"] < 2 ** 24, name
        if inp["scale"] is not None:
            e = np.log2(inp["scale"])
            assert np.array_equal(e, np.rint(e)) and e.min() >= -8 and e.max() <= 8, name
        seen += 1
    assert seen > 300
    assert 64 * 2 < 2 ** 24                                           # the grid-cap case: n = 2


def test_in_order_reference_is_within_its_bound_of_float64():
    """both tiers: |mean_in_order - mean64| <= (n + 1) 2^-24 sum |x| / n per cell (exactly 0 on the int tier up to the
    division's rounding); real inputs hold no denormals and no zeros, ids repeat inside a mean"""
    worst = 0.0
    for name, inp, od, data in _all_inputs():
        if inp["M"] == 0:
            continue
        M = min(inp["M"], 400)
        rows = tgg.gathered(inp, 0, M)
        got = gr.mean_in_order(rows, inp["scale"]).astype(np.float64)
        ref = gr.mean64(rows, inp["scale"])
        sc = 1.0 if inp["scale"] is None else inp["scale"].astype(np.float64)[None, :]
        bound = gr.mean_bound(rows) * sc
        assert (np.abs(got - ref) <= bound).all(), name
        ok = bound > 0
        worst = max(worst, float((np.abs(got - ref)[ok] / bound[ok]).max(initial=0.0)))
        if data == "real":
            v = np.abs(inp["values"][inp["named"]])
            assert v.min() >= 2.0 ** -40 and v.max() < 2.0 ** 12, name
        if inp["ids"] is not None and inp["n"] > 1:
            assert np.unique(inp["ids"][:inp["n"]]).size == 1, name
            assert inp["M"] < 2 or inp["ids"][inp["n"]] == inp["ids"][inp["n"] + 1], name
            assert int(inp["named"].sum()) < inp["R"]
    assert 0 < worst <= 1.0
    # and the reference is order-sensitive on the real tier: the reversed chain differs somewhere
    c = next(c for c in SINGLES if c.name == "sweep-f32-f32-ids-n25-real")
    rows = tgg.gathered(tgg.case_inputs(c), 0, c.M)
    assert not np.array_equal(gr.mean_in_order(rows), gr.mean_in_order(rows[:, ::-1]))


def test_host_tables_hold_nan_where_nothing_may_be_read():
    for name in ("vec-bf16-bf16-max-D602-int", "vec-f32-f32-v1-table-off-real", "fp8-bf16-D17-n9-vs",
                 "sweep-bf16-f32-null-n5-int"):
        c = next(c for c in SINGLES if c.name == name)
        inp = tgg.case_inputs(c)
        tab = tgg.host_table(inp, c.dtype, c.ld, c.tab_off)
        if c.dtype == "fp8":
            nan = (tab & 0x7f) == 0x7f
        elif c.dtype == "bf16":
            nan = np.isnan(gr.bf16_value(tab))
        else:
            nan = np.isnan(tab)
        R = inp["R"]
        assert nan[:c.tab_off].all() and nan[c.tab_off + R * c.ld:].all()
        rows = nan[c.tab_off:c.tab_off + R * c.ld].reshape(R, c.ld)
        assert rows[~inp["named"]].all() and (~inp["named"]).any()
        assert not rows[inp["named"], :c.D].any() and rows[inp["named"], c.D:].all()
        assert c.ld > c.D
        if c.dtype == "fp8":
            s = tgg.host_scale(inp)
            assert s.size >= gr.round_up(c.D, 16) and np.isnan(s[c.D:]).all() and not np.isnan(s[:c.D]).any()


def test_scatter_reference():
    init = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
    rows = np.array([[1.0, 10.0], [2.0, 20.0]])
    ids = np.array([2, 2, 0, 2])
    g, mag, cnt = gr.scatter_add64(init, rows, ids, 2, 0.5)
    assert np.array_equal(g, [[2.0, 12.0], [3.0, 4.0], [5.0 + 0.5 + 0.5 + 1.0, 6.0 + 5 + 5 + 10]])
    assert np.array_equal(cnt, [[1, 1], [0, 0], [3, 3]]) and np.array_equal(mag, np.abs(g))
    assert np.array_equal(gr.scatter_bound(mag, cnt)[2], 4 * 2.0 ** -24 * mag[2])
    assert np.array_equal(gr.mean_bwd(np.array([[3.0], [1.0]], dtype=np.float32), 2),
                          np.array([[1.5], [1.5], [0.5], [0.5]], dtype=np.float32))
