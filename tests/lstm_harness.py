"""Shared by tests/test_gpu_lstm.py and tests/test_gpu_lstm_tiles.py (test infrastructure): one ops.lstm_last call, output
and every gradient, next to the float64 oracle of tests/lstm_ref.py on the same rows and weights, and the comparison
both files assert."""
import numpy as np
import torch

import lstm_ref
from conftest import pkg
from util import close, close_fro, note_parity

gs = pkg()
ops = gs.ops
DEV = "cuda"

TOL_FP32 = (2e-4, 2e-5)         # fp32 mode: close(rtol, atol), every tensor
TOL_BF16 = (4e-2, 4e-2)         # TOL["bf16"] of test_gpu_model.py
GRAD_BOUND_BF16 = 3e-2          # GRAD_BOUND["bf16"] of test_gpu_engine_shapes.py (relative Frobenius)


def param_names(bidir):
    return list(lstm_ref.PARAMS) + ([k + "_reverse" for k in lstm_ref.PARAMS] if bidir else [])


def run(shape, mode, seed, key, rows=None, oracle_edit=None):
    """shape = (M, n, D, hidden_dim, bidirectional).  Rows N(0, 1) from RandomState(seed), an nn.LSTM initialised under
    torch.manual_seed(100 + seed), G bf16-representable (both modes see the same G).  rows(nb [M n, D]) -> nb changes the
    input of BOTH sides; oracle_edit(weights, kw) changes the oracle's input only (weights: the list of parameter
    arrays, kw: keyword arguments of lstm_ref.lstm_last).  -> dict(got, want, errs, ref, names); the measured errors are
    printed and go to note_parity under `key`."""
    M, n, D, hid, bidir = shape
    ops.set_compute_dtype(mode)
    torch.manual_seed(100 + seed)
    lstm = torch.nn.LSTM(D, hid // (1 + bidir), bidirectional=bidir, batch_first=True)
    rng = np.random.RandomState(seed)
    nb_np = rng.normal(size=(M * n, D)).astype(np.float32)
    G = lstm_ref.bf16(rng.normal(size=(M, hid))).astype(np.float32)     # bf16-representable: both modes see the same G
    if rows is not None:
        nb_np = np.ascontiguousarray(rows(nb_np), dtype=np.float32)
    names = param_names(bidir)
    w_np = [getattr(lstm, k).detach().numpy().copy() for k in names]
    w_ref, kw = [w.copy() for w in w_np], {}
    if oracle_edit is not None:
        oracle_edit(w_ref, kw)
    ref = lstm_ref.lstm_last(nb_np, M, w_ref[:4], w_ref[4:] if bidir else None, G=G,
                             rounding="bf16" if mode == "bf16" else None, **kw)
    lstm = lstm.to(DEV)
    params = [getattr(lstm, k) for k in names]
    nb = torch.from_numpy(nb_np).to(DEV).requires_grad_(True)
    out = ops.lstm_last(nb, M, *params[:4], reverse=params[4:] if bidir else None)
    assert out.shape == (M, hid) and out.dtype == ops.torch_dtype()
    (out.float() * torch.from_numpy(G).to(DEV)).sum().backward()
    got = {"out": out.detach().float().cpu().numpy(), "dneibs": nb.grad.cpu().numpy()}
    want = {"out": ref["out"], "dneibs": ref["dneibs"]}
    for k, p, r in zip(names, params, ref["grads"]):
        assert p.grad is not None, k
        got[k], want[k] = p.grad.cpu().numpy(), r
    errs = {}
    for k in got:
        a, b = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        errs[k + "_maxabs"] = float(np.abs(a - b).max())
        errs[k + "_fro"] = float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-12))
    print("%s: %s" % (key.replace("_", " "), {k: "%.3g" % v for k, v in sorted(errs.items())}))
    note_parity(key, **errs)
    return {"got": got, "want": want, "errs": errs, "ref": ref, "names": names, "bidir": bidir}


def compare(r, mode, what):
    """fp32 mode: close(2e-4, 2e-5).  bf16 mode against the rounding-aware oracle: output at TOL["bf16"], gradients at
    3e-2 relative Frobenius (no ReLU in the recurrence: no mask flips)."""
    got, want = r["got"], r["want"]
    if r["bidir"]:
        assert not got["weight_hh_l0_reverse"].any()
    for k in got:
        if mode == "fp32":
            close(got[k], want[k], (what, mode, k), *TOL_FP32)
        elif k == "out":
            close(got[k], want[k], (what, mode, k), *TOL_BF16)
        elif np.linalg.norm(want[k]) > 0:
            close_fro(got[k], want[k], (what, mode, k), GRAD_BOUND_BF16)
