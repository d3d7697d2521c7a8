"""-m gpu: the LSTM recurrence kernels (csrc/gsage_lstm.hip) at the tiles, widths and lengths they ship with.
tests/test_gpu_lstm.py stops at M = 257, H = 512 per direction and n = 25; every launch it makes takes the 16-row
sequence tile.  Here: the 32-row tile (M = 32 CUs + 17: every tile full but the last, which has 17 live rows), the mixed
32-row forward / 16-row backward, the widest and the longest admitted shapes, saturated gates, and what the guards of a
partial tile must not write -- through the C entry points with caller-chosen leading dimensions where ops.lstm_last
would hide them.  Every case asserts the tile it claims to reach through gsage_lstm_tile before it trusts its result."""
import numpy as np
import pytest
import torch

import lstm_harness
import lstm_ref
from conftest import pkg
from lstm_harness import GRAD_BOUND_BF16, TOL_BF16, TOL_FP32
from util import close, close_fro, note_parity

pytestmark = pytest.mark.gpu
gs = pkg()
ops = gs.ops
nat = gs._native
DEV = "cuda"

M0 = 49                 # base problem: three full 16-row tiles and one live row of a fourth
GUARD = 32              # guard sequences behind every array: a whole tile's worth of rows a bad guard could reach
# sentinel bit patterns (quiet NaNs with a payload: a guard that READS padding poisons its result as well)
SENT = {torch.bfloat16: (torch.int16, 0x7FC5), torch.float32: (torch.int32, 0x7FC00005)}


@pytest.fixture(autouse=True)
def _warm():
    ops.warmup(torch.device(DEV))
    yield
    ops.set_compute_dtype("bf16")


def _m32():
    """sequences that fill a 32-row tile on every CU and leave 17 live rows in one more: the last tile straddles the
    row groups of 4 a lane half owns (rows 16 of 17 and up: q = 8, lane half 0 only)"""
    return 32 * nat.device_info()["cu_count"] + 17


def _tiles(mode, M, H):
    code = ops._code(ops.torch_dtype(mode))
    return nat.lib().gsage_lstm_tile(code, M, H, 0), nat.lib().gsage_lstm_tile(code, M, H, 1)


def _filled(rows, cols, dtype):
    t = torch.empty(rows, cols, dtype=dtype, device=DEV)
    it, pat = SENT[dtype]
    t.view(it).fill_(pat)
    return t


def _untouched(t, what):
    it, pat = SENT[t.dtype]
    assert bool((t.view(it) == pat).all()), "%s: a guard element was overwritten" % (what,)


def _all_written(t, what):
    it, pat = SENT[t.dtype]
    assert not bool((t.view(it) == pat).any()), "%s: a live element was never written" % (what,)


def _abi(mode, GX, w_hh, dh, pad=(0, 0, 0, 0, 0)):
    """gsage_lstm_pack_whh / _fwd / _bwd through the C ABI.  GX [M, n, 4H] in the compute type, w_hh fp32 [4H, H] (None
    with n = 1: null Wp, hprev and carry), dh fp32 [M, H]; pad = elements added to (ldg, ldh, ldo, lddh, lddg).  Every
    array is pre-filled with the sentinel and has GUARD sequences behind its last row; on return the padding columns,
    the guard rows and row (m, 0) of hprev still hold it and every live element was written.
    -> dict of the live parts: gates [M, n, 4H], cseq [M, n, H], hprev [M, n - 1, H] (rows t >= 1), out [M, H],
    dG [M, n, 4H]"""
    cdt = ops.torch_dtype(mode)
    code = ops._code(cdt)
    L = nat.lib()
    M, n, H4 = GX.shape
    H = H4 // 4
    assert GX.dtype == cdt and dh.dtype == torch.float32 and (w_hh is not None or n == 1)
    ldg, ldh, ldo, lddh, lddg = 4 * H + pad[0], H + pad[1], H + pad[2], H + pad[3], 4 * H + pad[4]
    R = (M + GUARD) * n
    gates, dG = _filled(R, ldg, cdt), _filled(R, lddg, cdt)
    gates[:M * n, :4 * H] = GX.reshape(M * n, 4 * H)
    cseq = _filled(R, H, torch.float32)
    out = _filled(M + GUARD, ldo, cdt)
    dhb = _filled(M + GUARD, lddh, torch.float32)
    dhb[:M, :H] = dh
    hprev = carry = wp = wpb = None
    if n > 1:
        hprev, carry = _filled(R, ldh, cdt), _filled(M + GUARD, 2 * H, torch.float32)
        w = w_hh.to(DEV).float().contiguous()
        Hp = (H + 31) // 32 * 32
        wp = torch.empty(int(L.gsage_lstm_packed_elems(H)), dtype=cdt, device=DEV)
        nat.check(L.gsage_lstm_pack_whh(ops._ptr(w), w.stride(0), H, code, ops._ptr(wp), ops._stream()), "pack")
        wpb = ops._off(wp, 4 * Hp * Hp)
    nat.check(L.gsage_lstm_fwd(ops._ptr(gates), code, ldg, ops._ptr(wp), M, n, H, ops._ptr(cseq), ops._ptr(hprev), ldh,
                               ops._ptr(out), ldo, ops._stream()), "lstm_fwd")
    nat.check(L.gsage_lstm_bwd(ops._ptr(gates), code, ldg, wpb, M, n, H, ops._ptr(cseq), ops._ptr(dhb), lddh,
                               ops._ptr(dG), lddg, ops._ptr(carry), ops._stream()), "lstm_bwd")
    torch.cuda.synchronize()
    what = (mode, M, n, H, pad)
    for name, t, rows, cols in (("gates", gates, M * n, 4 * H), ("dG", dG, M * n, 4 * H), ("cseq", cseq, M * n, H),
                                ("out", out, M, H), ("dh", dhb, M, H), ("carry", carry, M, 2 * H)):
        if t is None:
            continue
        _untouched(t[rows:], what + (name, "guard rows"))
        _untouched(t[:rows, cols:], what + (name, "padding columns"))
        _all_written(t[:rows, :cols], what + (name,))
    res = {"gates": gates[:M * n, :4 * H].reshape(M, n, 4 * H), "dG": dG[:M * n, :4 * H].reshape(M, n, 4 * H),
           "cseq": cseq[:M * n].reshape(M, n, H), "out": out[:M, :H]}
    if n > 1:
        _untouched(hprev[M * n:], what + ("hprev", "guard rows"))
        hp = hprev[:M * n].view(M, n, ldh)
        _untouched(hp[:, 0], what + ("hprev", "row (m, 0) is the caller's"))
        _untouched(hp[:, :, H:], what + ("hprev", "padding columns"))
        _all_written(hp[:, 1:, :H], what + ("hprev",))
        res["hprev"] = hp[:, 1:, :H]
    return {k: v.clone() for k, v in res.items()}


_BASE = {}


def _base(mode, n, H):
    """the 49-sequence base problem of (mode, n, H), run alone on 16-row tiles with tight leading dimensions and checked
    against the float64 recurrence of tests/lstm_ref.py: computed once, shared, never changed.
    -> (GX, w_hh, dh, result of _abi)"""
    key = (mode, n, H)
    if key not in _BASE:
        cdt = ops.torch_dtype(mode)
        rng = np.random.RandomState(7 * H + n)
        GX = torch.from_numpy(rng.normal(size=(M0, n, 4 * H)).astype(np.float32)).to(cdt).to(DEV)
        dh = torch.from_numpy(rng.normal(size=(M0, H)).astype(np.float32)).to(DEV)
        w_hh = None
        if n > 1:       # nn.LSTM's initialisation: U(-1 / sqrt(H), 1 / sqrt(H))
            w_hh = torch.from_numpy(rng.uniform(-1, 1, size=(4 * H, H)).astype(np.float32) / np.float32(np.sqrt(H)))
        assert _tiles(mode, M0, H) == (16, 16)
        got = _abi(mode, GX, w_hh, dh)
        rounding = "bf16" if mode == "bf16" else None
        gates, c, hprev, out, dG = lstm_ref.recurrence(GX.float().cpu().numpy(), None if w_hh is None else w_hh.numpy(),
                                                       dh.cpu().numpy(), rounding)
        want = {"gates": gates, "cseq": c, "out": out, "dG": dG}
        if n > 1:
            want["hprev"] = hprev[:, 1:]
        errs = {}
        for k, b in want.items():
            a = got[k].float().cpu().numpy().astype(np.float64)
            errs[k + "_maxabs"] = float(np.abs(a - b).max())
            errs[k + "_fro"] = float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-12))
        print("lstm abi base n %d H %d %s: %s" % (n, H, mode, {k: "%.3g" % v for k, v in sorted(errs.items())}))
        note_parity("lstm_abi_base_n%d_H%d_%s" % (n, H, mode), **errs)
        for k, b in want.items():
            a = got[k].float().cpu().numpy()
            if mode == "fp32":
                close(a, b, (key, k), *TOL_FP32)
            elif k == "dG":
                close_fro(a, b, (key, k), GRAD_BOUND_BF16)
            else:
                close(a, b, (key, k), *TOL_BF16)
        _BASE[key] = (GX, w_hh, dh, got)
    return _BASE[key]


def _replicated(mode, n, H, M, tiles, pad=(0, 0, 0, 0, 0)):
    """M sequences, sequence m = base sequence m % 49: every tensor of every sequence bit-equal to its base sequence's"""
    GX, w_hh, dh, base = _base(mode, n, H)
    assert _tiles(mode, M, H) == tiles, (_tiles(mode, M, H), tiles)
    idx = torch.arange(M, device=DEV) % M0
    got = _abi(mode, GX[idx].contiguous(), w_hh, dh[idx].contiguous(), pad)
    assert set(got) == set(base)
    for k, v in got.items():
        assert torch.equal(v, base[k][idx]), (mode, n, H, M, k, "differs from the base sequence")


# (n, H per mode, tiles (forward, backward) at M32)
INDEPENDENCE = {"t32_32": (3, {"bf16": 40, "fp32": 40}, (32, 32)),
                "t32_16": (2, {"bf16": 640, "fp32": 320}, (32, 16)),     # backward: the LDS image of 32 rows does not fit
                "one_step": (1, {"bf16": 40, "fp32": 40}, (32, 32))}    # no W_hh: null Wp / hprev / carry


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("case", sorted(INDEPENDENCE))
def test_a_sequence_does_not_depend_on_its_tile(case, mode):
    """An MFMA output row depends on its own A row only, so a sequence's out, activated gates, c, h and dG are the SAME
    BITS alone on 16-row tiles (M = 49; 16/16) and replicated into M32 sequences on 32-row tiles, or on a 32-row forward
    and a 16-row backward over the same reserve.  The base is anchored to the float64 recurrence."""
    n, H, tiles = INDEPENDENCE[case]
    _replicated(mode, n, H[mode], _m32(), tiles)


PADS = (16, 24, 16, 24, 24)         # ldg, ldh, ldo, lddh, lddg


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("M", ["M32", 37])
def test_guards_leave_padding_and_guard_rows_alone(M, mode):
    """Padded leading dimensions and a partial last tile: 17 live rows of 32 (M32; sized for 16-row tiles the batch ends
    one row into a tile) and 5 live rows of 16 (M = 16 * 2 + 5).  _abi checks every padding column, the guard rows behind
    gates, cseq, hprev, out, dG and carry, and row (m, 0) of hprev; the live values stay the base sequences' bits."""
    if M == "M32":
        _replicated(mode, 3, 40, _m32(), (32, 32), PADS)
    else:
        _replicated(mode, 3, 40, M, (16, 16), PADS)


# ---- contract edges through ops.lstm_last -----------------------------------------------------------------------------
# name: ((M, n, D, hidden_dim, bidirectional), modes, tile to assert or None); M = None stands for M32
EDGES = {
    "m32_uni": ((None, 3, 24, 40, False), ("fp32", "bf16"), 32),       # the production tile end to end
    "m32_bidir": ((None, 2, 16, 48, True), ("fp32", "bf16"), 32),      # + the reverse direction's single step
    "h1024": ((33, 4, 32, 1024, False), ("bf16",), None),              # the widest direction: forward LDS > 64 KiB
    "h800_bidir": ((33, 3, 32, 1600, True), ("bf16",), None),          # 25 unit blocks over 8 waves: uneven
    "h300_bidir": ((33, 3, 32, 600, True), ("fp32", "bf16"), None),    # Hp = 320: 10 blocks, the last one padded
    "n128": ((33, 128, 16, 40, False), ("fp32", "bf16"), None),        # the longest sequence
    "n127_bidir": ((17, 127, 16, 66, True), ("fp32", "bf16"), None),
}
EDGE_RUNS = [(k, m) for k in sorted(EDGES) for m in EDGES[k][1]]


def _edge(name, mode, **kw):
    (M, n, D, hid, bidir), _, tile = EDGES[name]
    M = _m32() if M is None else M
    if tile is not None:
        assert _tiles(mode, M, hid // (1 + bidir)) == (tile, tile)
    return lstm_harness.run((M, n, D, hid, bidir), mode, 40 + sorted(EDGES).index(name),
                            "lstm_edge_%s_%s%s" % (name, mode, kw.pop("tag", "")), **kw)


@pytest.mark.parametrize("name,mode", EDGE_RUNS)
def test_contract_edges_against_the_float64_oracle(name, mode):
    """ops.lstm_last (K5 projection, recurrence, K5b / K5 gradients) at the edges of gsage_lstm_ok and on the 32-row tile,
    at the tolerances of test_shape_sweep_against_the_float64_oracle."""
    lstm_harness.compare(_edge(name, mode), mode, name)


# ---- sensitivity ------------------------------------------------------------------------------------------------------
def _zero_last_sequences(k):
    def edit(weights, kw):
        def gx(GX):
            GX = GX.copy()
            GX[-k:] = 0
            return GX
        kw["gx_edit"] = gx
    return edit


def _zero_last_unit_whh(weights, kw):
    H = weights[1].shape[1]
    weights[1][H - 1::H] = 0            # rows g H + (H - 1): the four gates of the last unit


@pytest.mark.parametrize("edit", ["last_15_sequences", "last_unit"])
def test_comparison_sees_the_partial_tile_and_the_padded_unit_block(edit):
    """the fp32 comparison of the M32 case fails when the oracle's input alone changes in the 15 last sequences (rows 2
    to 16 of the partial last tile) or in W_hh's rows of unit 39 (the padded second unit block)"""
    e = _zero_last_sequences(15) if edit == "last_15_sequences" else _zero_last_unit_whh
    r = _edge("m32_uni", "fp32", oracle_edit=e, tag="_edit_" + edit)
    with pytest.raises(AssertionError):
        lstm_harness.compare(r, "fp32", edit)


# ---- saturated gates --------------------------------------------------------------------------------------------------
SAT_SHAPE = (40, 6, 16, 96, False)
SAT_SCALE = 300.0       # rows of the first 20 sequences: pre-activations of std ~ 70 (W_ih ~ U(+-0.1), 16 features)


def _saturating_rows(nb):
    M, n = SAT_SHAPE[:2]
    nb = nb.copy()
    nb[:M // 2 * n] *= SAT_SCALE
    return nb


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_saturated_gates_stay_finite_and_within_tolerance(mode):
    """bf16 mode computes sigmoid and tanh from the hardware exp and reciprocal and relies on exp overflowing to
    infinity and rcp(inf) = 0.  Half of the sequences are scaled so that at least 1 % of ALL pre-activations of the oracle
    exceed |90| (exp(90) overflows fp32) and none exceeds |700| (float64 exp's limit); the other half stays N(0, 1) so
    that the gradients are not all zero."""
    r = lstm_harness.run(SAT_SHAPE, mode, 60, "lstm_saturated_%s" % mode, rows=_saturating_rows)
    d = r["ref"]["dirs"][0]
    pre = np.abs(d.GX + d.hprev @ d.Wh.T)
    assert pre.max() < 700 and (pre > 90).mean() >= 0.01, (pre.max(), (pre > 90).mean())
    for k, v in r["got"].items():
        assert np.isfinite(v).all(), (mode, k)
    assert any(np.linalg.norm(r["want"][k]) > 0 for k in r["want"] if k != "out")
    lstm_harness.compare(r, mode, "saturated")
