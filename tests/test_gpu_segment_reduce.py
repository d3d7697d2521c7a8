"""gsage_segment_reduce (csrc/gsage_fullgraph.hip) called directly, against the float64 restatement of
segment_reduce_ref: every mode, table type, output type and activation at the widths where the team size, the number of
passes over a row and the last chunk change, on a graph whose degrees sit on the slice and batch boundaries; softmax
scores that overflow an unstabilised exponential; out-of-range ids; degenerate plans; and the proof that the comparison
fails when the reference loses one edge.

Tolerances (segment_reduce_ref.compare) are derived, not tuned: max and rows of effective degree 1 are exact; a mean is
within (deg + 2) 2^-24 of its magnitude sum; the softmax mode is within 8 times the error a plain float32 restatement
makes on the same inputs; a bf16 output adds one bf16 store."""
import numpy as np
import pytest
import torch

import segment_reduce_ref as sr
from conftest import pkg
from util import note_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# each team size (8, 16, 32, 64 lanes of one 16-byte chunk) at its upper edge and one chunk above it; a partial last
# chunk; two and three passes of a 64-lane team over the row
WIDTHS = {"bf16": [1, 7, 8, 9, 64, 65, 100, 128, 136, 256, 264, 512, 520, 1032],
          "fp32": [1, 3, 4, 5, 32, 33, 36, 128, 130, 256, 260, 516]}
# on the shipped slice length: a partial chunk at the smallest team, a team edge, one chunk above one, two passes
WIDTHS_256 = {"bf16": [7, 64, 136, 520], "fp32": [3, 33, 130, 260]}
GRID = [(8, t, D) for t in ("bf16", "fp32") for D in WIDTHS[t]] + \
       [(256, t, D) for t in ("bf16", "fp32") for D in WIDTHS_256[t]]

_DEVICE = {}


def _adj(L, slice_len=None):
    """(graph, its DeviceCSR, its plan for slice_len): L = 8 through plan(adj, slice_len=8), L = 256 through the
    default plan"""
    gs = pkg()
    slice_len = slice_len or L
    key = (L, slice_len)
    if key not in _DEVICE:
        g = sr.graph(L)
        adj = g.csr(DEV)
        plan = gs.infer.plan(adj) if slice_len == gs.infer.SLICE_LEN else gs.infer.plan(adj, slice_len=slice_len)
        assert plan["slice_len"] == slice_len
        _DEVICE[key] = (g, adj, plan)
    return _DEVICE[key]


def _run(g, adj, plan, r, D, tdt, odt, mode, act, wide, use_infer=False):
    """one launch -> (the [n, D] result on the CPU, the untouched-columns check done)"""
    gs = pkg()
    table = sr.device_table(r["table"], tdt, wide, DEV)
    keys = sr.device_keys(r["keys"], wide, DEV) if mode == "softmax" else None
    buf, out = sr.out_buffer(g.n, D, odt, DEV)
    if use_infer:
        nat = gs._native
        code = {"mean": nat.SEG_MEAN, "max": nat.SEG_MAX, "softmax": nat.SEG_SOFTMAX_WEIGHTED}[mode]
        gs.infer.segment_reduce(adj, table[:, :D], code, out, nat.ACT_RELU if act == "relu" else nat.ACT_NONE, keys=keys)
    else:
        sr.launch(adj, plan, table, D, mode, out, act, keys)
    host = buf.cpu()
    pad = sr.bits(host[:, D:])
    assert bool((pad == sr.bits(torch.full_like(host[:, D:], sr.OUT_PAD))).all()), \
        ("columns at and beyond D were written", mode, tdt, odt, D, act, wide)
    return host[:, :D].contiguous()


@pytest.mark.parametrize("mode", sr.MODES)
@pytest.mark.parametrize("L,tdt,D", GRID)
def test_parity_grid(L, tdt, D, mode):
    """modes x table type x output type x activation x width, ld == Dp and ld > Dp, strided output"""
    g, adj, plan = _adj(L)
    if L == 8:
        assert plan["n_long"] >= 70 and plan["n_short"] >= 70       # both launches: more than one workgroup
    else:
        assert 3 <= plan["n_long"] <= 16 and g.col.shape[0] < 40000
    r = sr.cached(g, D, tdt, "L%d" % L)
    ref, S = r[mode]
    for odt in ("fp32", "bf16"):
        for act in ("none", "relu"):
            for wide in (False, True):
                what = (mode, "table " + tdt, "out " + odt, "D %d" % D, act, "ld > Dp" if wide else "ld == Dp", "L %d" % L)
                got = _run(g, adj, plan, r, D, tdt, odt, mode, act, wide, use_infer=(L == 256))
                if mode == "softmax":
                    # measured before anything is asserted: the kernel's error next to the float32 restatement's
                    kerr = sr.float32_error(got.double().numpy(), np.maximum(ref, 0) if act == "relu" else ref, S)
                    note_parity("segreduce/L%d/%s-%s/D%d/%s/%s" % (L, tdt, odt, D, act, "wide" if wide else "tight"),
                                float32_restatement=r["e32"], kernel=kerr, bound=8 * r["e32"])
                sr.compare(got, ref, S, g.deg, mode, odt, what, act, e32=r["e32"])
    assert int(adj.err_flag.item()) == 0


@pytest.mark.parametrize("L", [8, 256])
@pytest.mark.parametrize("tdt,D", [("bf16", 136), ("fp32", 33)])
def test_max_is_bit_equal_across_slice_lengths(L, tdt, D):
    """a maximum does not depend on how the row was cut: slice_len 8 and 256 plans of the same graph, same bits"""
    g, adj, _ = _adj(L)
    gs = pkg()
    r = sr.cached(g, D, tdt, "L%d" % L)
    p8 = dict(gs.infer.plan(adj, slice_len=8))
    p256 = dict(gs.infer.plan(adj, slice_len=256))
    assert p8["n_slices"] > p256["n_slices"] and p8["n_long"] > p256["n_long"]
    a = _run(g, adj, p8, r, D, tdt, "fp32", "max", "none", False)
    b = _run(g, adj, p256, r, D, tdt, "fp32", "max", "none", False)
    assert torch.equal(sr.bits(a), sr.bits(b))


# ---- softmax at scores that overflow an unstabilised exponential ----------------------------------------------
def _extreme_graph(L):
    """96 rows of random degree, keys scaled so that the scores of a row span about +-200, and four arranged rows:
    a long row (3L + 5 edges) and a short one (L - 1 = 23 edges: three batches of 8) whose largest score sits at the
    very end (every earlier partial / batch is rescaled), and the same two with it at the very start (every later
    weight underflows to 0)."""
    n, long_deg, short_deg = 96, 3 * L + 5, L - 1
    rng = np.random.RandomState(5)
    deg = rng.randint(1, 40, size=n)
    deg[0] = 0
    rows = {"long_last": 1, "long_first": 2, "short_last": 3, "short_first": 4}
    deg[1] = deg[2] = long_deg
    deg[3] = deg[4] = short_deg
    g = sr.from_degrees(deg, rng, L)
    keys = (rng.normal(size=(n, 32)) * 3.5).astype(np.float32)
    col = g.col.copy()
    for name, v in rows.items():
        b, e = int(g.rowptr[v]), int(g.rowptr[v + 1])
        nb = rng.permutation(n)[:e - b]                 # distinct ids: one largest score
        s = keys[nb].astype(np.float64) @ keys[v].astype(np.float64)
        top = int(np.argmax(s))
        assert s.max() - np.sort(s)[-2] > 0 and s.max() - s.min() > 200
        nb = np.concatenate([np.delete(nb, top), nb[top:top + 1]] if name.endswith("last")
                            else [nb[top:top + 1], np.delete(nb, top)])
        col[b:e] = nb
    return sr.Graph(g.rowptr, col, L, rows), keys


@pytest.mark.parametrize("tdt,D", [("fp32", 130), ("bf16", 65)])
def test_softmax_at_extreme_scores(tdt, D):
    L = 24                                              # a short row can then span three batches of 8 edges
    g, keys = _extreme_graph(L)
    gs = pkg()
    adj = g.csr(DEV)
    plan = gs.infer.plan(adj, slice_len=L)
    assert {int(v) for v in plan["long_rows"][:, 0].cpu()} >= {g.at["long_last"], g.at["long_first"]}
    table = sr.stored(np.random.RandomState(6).normal(size=(g.n, D)), tdt)
    ref, S = sr.reference(g.rowptr, g.col, table, keys, "softmax")
    s_row = keys[g.col[g.rowptr[1]:g.rowptr[2]]].astype(np.float64) @ keys[1].astype(np.float64)
    assert s_row.max() > 89 and s_row.max() - s_row.min() > 200          # expf overflows fp32 above 88.7
    e32 = sr.float32_error(sr.softmax_float32(g.rowptr, g.col, table, keys), ref, S)
    r = {"table": table, "keys": keys}
    for odt in ("fp32", "bf16"):
        got = _run(g, adj, plan, r, D, tdt, odt, "softmax", "none", False)
        assert bool(torch.isfinite(got).all())
        kerr = sr.float32_error(got.double().numpy(), ref, S)
        note_parity("segreduce/extreme/%s-%s/D%d" % (tdt, odt, D), float32_restatement=e32, kernel=kerr, bound=8 * e32)
        sr.compare(got, ref, S, g.deg, "softmax", odt, ("softmax, extreme scores", tdt, odt, D), e32=e32)
    assert int(adj.err_flag.item()) == 0


# ---- the comparison fails when the reference loses one edge ------------------------------------------------------
def _dropped(L, case):
    g = sr.graph(L)
    if case == "last edge of a long row's last slice":
        v = g.at[3 * L + 5]
        return v, int(g.deg[v]) - 1
    if case == "9th edge of a degree-9 row":
        return g.at[9], 8
    v = g.at[L + 1]                                     # the single edge of the second slice
    return v, L


@pytest.mark.parametrize("case", ["last edge of a long row's last slice", "9th edge of a degree-9 row",
                                  "single edge of the second slice of a degree L + 1 row"])
@pytest.mark.parametrize("L", [8, 256])
def test_comparison_sees_a_dropped_edge(L, case):
    """mean, fp32 in and out: the kernel is right (the comparison passes), and the same comparison fails against a
    reference that lost one edge"""
    g, adj, plan = _adj(L)
    D = 33
    r = sr.cached(g, D, "fp32", "L%d" % L)
    got = _run(g, adj, plan, r, D, "fp32", "fp32", "mean", "none", False)
    sr.compare(got, *r["mean"], g.deg, "mean", "fp32", "intact reference")
    v, k = _dropped(L, case)
    assert 0 <= k < g.deg[v]
    ref, S = sr.reference(g.rowptr, g.col, r["table"], None, "mean", drop=(v, k))
    with pytest.raises(AssertionError, match="row %d " % v):
        sr.compare(got, ref, S, g.deg, "mean", "fp32", case)


# ---- ids outside the graph -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sr.MODES)
def test_out_of_range_ids_read_row_zero_and_raise_the_flag(mode):
    """one id == n_rows in a short row, one == -1 in the last slice of a long row: the kernel clamps before it loads"""
    L, D, tdt = 8, 36, "fp32"
    base = sr.graph(L)
    v_short, v_long = base.at[7], base.at[3 * L + 5]
    g = base.with_ids([(int(base.rowptr[v_short]) + 3, base.n), (int(base.rowptr[v_long + 1]) - 2, -1)])
    gs = pkg()
    adj = g.csr(DEV)
    plan = gs.infer.plan(adj, slice_len=L)
    table, keys = sr.inputs(g.n, D, tdt, seed=77)
    ref, S = sr.reference(g.rowptr, g.col, table, keys, mode)
    clean, _ = sr.reference(base.rowptr, base.col, table, keys, mode)
    assert not np.array_equal(ref[v_short], clean[v_short]) or mode == "max"
    e32 = sr.float32_error(sr.softmax_float32(g.rowptr, g.col, table, keys), ref, S) if mode == "softmax" else None
    got = _run(g, adj, plan, {"table": table, "keys": keys}, D, tdt, "fp32", mode, "none", False)
    assert int(adj.err_flag.item()) == 1
    sr.compare(got, ref, S, g.deg, mode, "fp32", ("out-of-range ids", mode), e32=e32)
    with pytest.raises(IndexError):
        adj.check()
    assert int(adj.err_flag.item()) == 0
    adj.check()


# ---- determinism -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sr.MODES)
@pytest.mark.parametrize("tdt,D", [("bf16", 264), ("fp32", 33)])
def test_two_calls_are_bit_equal(tdt, D, mode):
    g, adj, plan = _adj(8)
    r = sr.cached(g, D, tdt, "L8")
    for odt in ("fp32", "bf16"):
        a = _run(g, adj, plan, r, D, tdt, odt, mode, "none", False)
        b = _run(g, adj, plan, r, D, tdt, odt, mode, "none", False)
        assert torch.equal(sr.bits(a), sr.bits(b)), (mode, tdt, odt, D)


# ---- degenerate plans ----------------------------------------------------------------------------------------------
def _degenerate(kind):
    rng = np.random.RandomState(9)
    n, L = 150, 8
    if kind == "no long row":
        deg = rng.randint(0, L + 1, size=n)
        deg[7] = L
    else:
        deg = rng.randint(L + 1, 4 * L, size=n)
        deg[0] = 0
        deg[11::13] = 0
    return sr.from_degrees(deg, rng, L)


@pytest.mark.parametrize("tdt,D", [("bf16", 65), ("fp32", 5)])
@pytest.mark.parametrize("kind", ["no long row", "every non-empty row long"])
def test_degenerate_plans(kind, tdt, D):
    g = _degenerate(kind)
    gs = pkg()
    adj = g.csr(DEV)
    plan = gs.infer.plan(adj, slice_len=g.L)
    if kind == "no long row":
        assert plan["n_slices"] == 0 and plan["n_long"] == 0 and plan["n_short"] == g.n
    else:
        assert plan["n_short"] == int((g.deg == 0).sum()) > 0 and plan["n_long"] == g.n - plan["n_short"]
    r = sr.cached(g, D, tdt, kind)
    for mode in sr.MODES:
        for odt in ("fp32", "bf16"):
            got = _run(g, adj, plan, r, D, tdt, odt, mode, "none", False)
            sr.compare(got, *r[mode], g.deg, mode, odt, (kind, mode, tdt, odt, D), e32=r["e32"])
    assert int(adj.err_flag.item()) == 0
