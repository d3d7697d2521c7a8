"""No GPU needed: the float64 restatement of the LSTM aggregator (tests/lstm_ref.py) reproduces the vectors recorded
from the reference, and the recurrence kernels' entry points exist, are bound and validate their arguments on the
host."""
import ctypes

import numpy as np

import lstm_ref
from conftest import load_golden, pkg
from util import close

gs = pkg()


def test_lstm_ref_reproduces_the_golden_vectors():
    """Anchors the oracle of tests/test_gpu_lstm.py to the reference: outputs, dx, dneibs and every parameter gradient
    of all recorded cases, the exact zeros of weight_hh_l0_reverse included."""
    g = load_golden("lstm_kat.npz")
    assert int(g["n_cases"]) == 4
    bidir_seen = 0
    for c in range(int(g["n_cases"])):
        p = "c%d_" % c
        M, n, D, h, hid, bidir = [int(v) for v in g[p + "dims"]]
        w = {k[len(p + "w_"):]: g[k] for k in g.files if k.startswith(p + "w_")}
        out, dx, dn, grads = lstm_ref.aggregator(g[p + "x"], g[p + "neibs"], w, str(g[p + "act"]) == "relu", g[p + "G"])
        close(out, g[p + "out"], (c, "out"), 1e-5, 1e-6)
        close(dx, g[p + "dx"], (c, "dx"), 1e-5, 1e-6)
        close(dn, g[p + "dneibs"], (c, "dneibs"), 1e-5, 1e-6)
        assert set(grads) == set(w)
        for k, v in grads.items():
            close(v, g[p + "g_" + k], (c, k), 1e-5, 1e-6)
        if bidir:
            bidir_seen += 1
            assert not grads["lstm.weight_hh_l0_reverse"].any() and not g[p + "g_lstm.weight_hh_l0_reverse"].any()
    assert bidir_seen == 2


def test_bf16_rounding_helper_is_round_to_nearest_even():
    import torch
    v = np.random.RandomState(0).normal(size=4096) * np.logspace(-6, 6, 4096)
    v = np.concatenate([v, [1.00390625, 1.01171875, 0.0, -1.00390625]])        # ties: to even
    want = torch.from_numpy(v.astype(np.float32)).to(torch.bfloat16).double().numpy()
    assert np.array_equal(lstm_ref.bf16(v), want)


def test_lstm_entry_points_exported_and_bound():
    nat = gs._native
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in ("gsage_lstm_fwd", "gsage_lstm_bwd", "gsage_lstm_ok", "gsage_lstm_pack_whh", "gsage_lstm_packed_elems",
                 "gsage_lstm_tile"):
        assert hasattr(lib, name), name
        assert name in nat.SIGNATURES, name
    assert hasattr(gs.ops, "lstm_last")
    assert nat.lib().gsage_abi_version() == 6


def test_lstm_ok_says_which_shapes_the_kernels_take():
    L = gs._native.lib()
    nat = gs._native
    assert L.gsage_lstm_ok(nat.BF16, 512, 25) == 1 and L.gsage_lstm_ok(nat.F32, 512, 10) == 1
    assert L.gsage_lstm_ok(nat.BF16, 1, 1) == 1 and L.gsage_lstm_ok(nat.F32, 20, 128) == 1
    assert L.gsage_lstm_ok(nat.BF16, 256, 129) == 0 and L.gsage_lstm_ok(nat.BF16, 256, 0) == 0
    assert L.gsage_lstm_ok(nat.BF16, 0, 4) == 0 and L.gsage_lstm_ok(7, 16, 4) == 0
    assert L.gsage_lstm_ok(nat.BF16, 1024, 4) == 1 and L.gsage_lstm_ok(nat.BF16, 1025, 4) == 0
    assert L.gsage_lstm_ok(nat.F32, 513, 4) == 0
    assert L.gsage_lstm_packed_elems(20) == 8 * 32 * 32 and L.gsage_lstm_packed_elems(512) == 8 * 512 * 512
    # gsage_lstm_tile: where the LDS image of 32 rows does not fit, 16 whatever M (elsewhere it depends on the CU count)
    assert L.gsage_lstm_tile(nat.BF16, 1 << 20, 640, 1) == 16 and L.gsage_lstm_tile(nat.F32, 1 << 20, 320, 1) == 16
    assert L.gsage_lstm_tile(nat.BF16, 49, 40, 0) == 16 and L.gsage_lstm_tile(nat.F32, 49, 513, 0) == 0


def test_lstm_bad_arguments_return_einval_without_gpu():
    L = gs._native.lib()
    p = ctypes.c_void_p(16)
    assert L.gsage_lstm_fwd(p, 1, 32, p, 4, 200, 8, p, p, 8, p, 8, None) == -1 and b"n = 200" in L.gsage_last_error()
    assert L.gsage_lstm_fwd(p, 1, 31, p, 4, 3, 8, p, p, 8, p, 8, None) == -1 and b"ldg" in L.gsage_last_error()
    assert L.gsage_lstm_fwd(p, 5, 32, p, 4, 3, 8, p, p, 8, p, 8, None) == -1 and b"dtype" in L.gsage_last_error()
    assert L.gsage_lstm_fwd(p, 0, 4096, p, 4, 3, 600, p, p, 600, p, 600, None) == -1 and b"H = 600" in L.gsage_last_error()
    assert L.gsage_lstm_fwd(p, 1, 32, p, 4, 3, 8, p, p, 8, p, 7, None) == -1 and b"ldo" in L.gsage_last_error()
    assert L.gsage_lstm_fwd(p, 1, 32, p, 4, 3, 8, None, p, 8, p, 8, None) == -1 and b"null" in L.gsage_last_error()
    assert L.gsage_lstm_bwd(p, 1, 32, p, 4, 0, 8, p, p, 8, p, 32, p, None) == -1 and b"n = 0" in L.gsage_last_error()
    assert L.gsage_lstm_bwd(p, 1, 32, p, 4, 3, 8, p, p, 7, p, 32, p, None) == -1 and b"lddh" in L.gsage_last_error()
    assert L.gsage_lstm_bwd(p, 1, 32, p, 4, 3, 8, p, p, 8, p, 16, p, None) == -1 and b"lddg" in L.gsage_last_error()
    assert L.gsage_lstm_bwd(p, 1, 32, None, 4, 3, 8, p, p, 8, p, 32, p, None) == -1 and b"null" in L.gsage_last_error()
    assert L.gsage_lstm_pack_whh(p, 4, 8, 1, p, None) == -1 and b"ldw" in L.gsage_last_error()
    assert L.gsage_lstm_pack_whh(None, 8, 8, 1, p, None) == -1 and b"null" in L.gsage_last_error()
    # an empty batch is not an error and launches nothing
    before = gs._native.launch_count()
    assert L.gsage_lstm_fwd(None, 1, 32, None, 0, 3, 8, None, None, 8, None, 8, None) == 0
    assert gs._native.launch_count() == before


def test_host_mode_keeps_the_stock_lstm_and_its_state_dict():
    import torch
    agg = gs.aggregator_lookup["lstm"](input_dim=6, output_dim=4, activation=None, hidden_dim=8, bidirectional=True)
    assert isinstance(agg.lstm, torch.nn.LSTM)
    assert set(agg.state_dict()) == {"lstm." + k + s for k in lstm_ref.PARAMS for s in ("", "_reverse")} | \
        {"fc_x.weight", "fc_neib.weight"}
