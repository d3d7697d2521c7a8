"""attn_fused_ref (the staged restatement the GPU test of the fused attention hop compares against) checked without a
GPU: fed exact upstream values its stages are torch autograd in float64 of the definition (nn_modules.py:293-296,
305-321); a float32 emulation of the kernels' rounding points passes every stage's bound on every case of
test_gpu_attn_fused.py (the device's CU count replaced by CUS below, which only sets M of the trip cases); and each of
seven mutants of that emulation -- what a subtly wrong kernel would compute -- is pushed beyond the bound of a stage it
corrupts, and of no other stage, on every case it can show on.  The mutants are the evidence that the bounds are tight
enough: one that passed would mean tame inputs or a wrong bound.

A mutant cannot show on (`_shows`): (c) a case of one trip; (g) fewer than five children; (b) and (a) all children
reading one row (equal rows; equal weights 1 / n whose dropped low parts, 2^-10 of the sum, stay below the bf16 rounding
of the result); (f) hid = +-1 or a few float32 ulps (saturated, tiny: truncation and rounding agree)."""
import numpy as np
import pytest
import torch

import attn_fused_ref as af

CUS = 4                                                              # stand-in for the device's CU count


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float(np.abs(a - b).max())
    assert err <= 1e-12 * max(1.0, float(np.abs(b).max())), (what, err)


@pytest.mark.parametrize("M,n,D", [(7, 5, 11), (3, 2, 40), (4, 16, 9)])
def test_stages_fed_exact_values_are_autograd(M, n, D):
    """loss = <agg, g>: hid, a, ws, agg and d loss / d ws (dws), d s (ds), d xa (dxa), d a (da), d pre-activation (dhid,
    before its rounding points)"""
    torch.manual_seed(M * 100 + n)
    dt = torch.float64
    X, W0, W2 = torch.randn(M * n, D, dtype=dt), torch.randn(32, D, dtype=dt) / D ** 0.5, torch.randn(32, 32, dtype=dt) / 32 ** 0.5
    xa, g = torch.randn(M, 32, dtype=dt, requires_grad=True), torch.randn(M, D, dtype=dt)
    pre = X @ W0.t()
    pre.requires_grad_(True).retain_grad()
    hid = torch.tanh(pre)
    a = hid @ W2.t()
    a.retain_grad()
    s = torch.bmm(a.view(M, n, 32), xa.unsqueeze(2)).squeeze(2)
    s.retain_grad()
    ws = torch.softmax(s, dim=1)
    ws.retain_grad()
    agg = (X.view(M, n, D) * ws.unsqueeze(2)).sum(1)
    (agg * g).sum().backward()
    Xn, W0n, W2n, xan, gn = (t.detach().numpy() for t in (X, W0, W2, xa, g))
    r_hid = af.hid_value(Xn, W0n)
    r_a = af.a_value(r_hid, W2n)
    r_ws = af.ws_value(r_a, xan, M, n)
    _close(r_hid, hid.detach().numpy(), "hid")
    _close(r_a, a.detach().numpy(), "a")
    _close(r_ws, ws.detach().numpy().reshape(-1), "ws")
    _close(af.agg_value(r_ws, Xn, M, n), agg.detach().numpy(), "agg")
    r_dws = af.dws_value(Xn, gn, M, n)
    r_ds = af.ds_value(r_ws, r_dws, M, n)
    r_da = af.da_value(r_ds, xan, M, n)
    _close(r_dws, ws.grad.numpy().reshape(-1), "dws")
    _close(r_ds, s.grad.numpy().reshape(-1), "ds")
    _close(af.dxa_value(r_ds, r_a, M, n), xa.grad.numpy(), "dxa")
    _close(r_da, a.grad.numpy(), "da")
    _close(af.dhid_value(r_da, W2n, r_hid), pre.grad.numpy(), "dhid")


def test_stage_functions_agree_with_the_stage_values():
    """the references inside the bound functions are the value functions above on the same inputs"""
    fwd, bwd = af.inputs(af.CASES[8], CUS)
    M, n = fwd["M"], fwd["n"]
    out = af.emulate_forward(fwd)
    X = af.f64(fwd["x"])
    _close(af.hid_stage(fwd["x"], fwd["W0"])[0], af.hid_value(X, af.f64(fwd["W0"])), "hid")
    _close(af.a_stage(out["hid"], fwd["W2"])[0], af.a_value(af.f64(out["hid"]), af.f64(fwd["W2"])), "a")
    _close(af.ws_stage(out["a"], fwd["xa"], M, n)[0], af.ws_value(out["a"].astype(np.float64), fwd["xa"].astype(np.float64), M, n), "ws")
    _close(af.agg_stage(out["ws"], fwd["x"], M, n)[0], af.agg_value(out["ws"].astype(np.float64), X, M, n), "agg")
    bo = af.emulate_backward(bwd)
    dws, de = af.dws_stage(bwd["x"], bwd["g"], M, n)
    D = bwd["D"]
    _close(dws, af.dws_value(X[:, :D], bwd["g"][:, :D].astype(np.float64), M, n), "dws (the junk in g's pads excluded)")
    ds, dse = af.ds_stage(bwd["ws"], dws, de, M, n)
    _close(ds, af.ds_value(bwd["ws"].astype(np.float64), dws, M, n), "ds")
    _close(af.dxa_stage(ds, dse, bwd["na"], M, n)[0], af.dxa_value(ds, bwd["na"].astype(np.float64), M, n), "dxa")
    _close(af.da_stage(ds, dse, bwd["xa"], M, n)[0], af.da_value(ds, bwd["xa"].astype(np.float64), M, n), "da")
    _close(af.dhid_stage(bo["da"], bwd["W2"], bwd["hid"])[0],
           af.dhid_value(af.f64(bo["da"]), af.f64(bwd["W2"]), af.f64(bwd["hid"])), "dhid")


def test_kstep_rule():
    assert [af.ksteps(D) for D in (1, 32, 33, 64, 65, 128, 129, 256, 257, 608, 609, 640, 641)] == \
        [1, 1, 2, 2, 4, 4, 8, 8, 19, 19, 20, 20, 0]
    assert af.ksteps(129, 192) == 0 and af.ksteps(129, 256) == 8 and af.ksteps(300, 320) == 0 and af.ksteps(300, 640) == 19
    for c in af.CASES:
        assert af.ksteps(c.D, c.ld) > 0, c.name


_RUNS = {}


def _run(case):
    """inputs and the unmutated emulation of a case, once for the module"""
    if case.name not in _RUNS:
        fwd, bwd = af.inputs(case, CUS)
        out = af.emulate_forward(fwd)
        if case.special not in (None, "repeats"):
            bwd = af.chain(fwd, bwd, out)
        _RUNS[case.name] = (fwd, bwd, out, af.emulate_backward(bwd))
    return _RUNS[case.name]


FWD_STAGES, BWD_STAGES = ("hid", "a", "ws", "agg_lp"), ("dws", "ds", "dxa", "da", "dhid")


@pytest.mark.parametrize("case", af.CASES, ids=[c.name for c in af.CASES])
def test_emulation_within_every_bound(case):
    fwd, bwd, out, bout = _run(case)
    af.verify_forward(fwd, out, case.name + "/")
    af.verify_backward(bwd, bout, case.name + "/", stages=BWD_STAGES)
    if case.special == "saturated":
        assert np.abs(af.hid_stage(fwd["x"], fwd["W0"])[2]).min() > 20 and ((out["hid"] & 0x7fff) == 0x3f80).all()
        assert not (bout["dhid"] & 0x7fff).any()
    if case.special == "zero_rows":
        zero = ~fwd["x"].any(axis=1)
        assert zero.sum() >= fwd["M"] * fwd["n"] // 4 and not out["hid"][zero].any() and not out["a"][zero].any()
    if case.special == "peaked":
        sm = af.ws_stage(out["a"], fwd["xa"], fwd["M"], fwd["n"])[2].reshape(fwd["M"], fwd["n"])
        one_hot = (np.sort(sm, axis=1)[:, -2] < -110)
        assert one_hot.sum() >= 1 and (sm < -110).sum() >= 50, "too few weights that underflow"
        assert not out["ws"].reshape(sm.shape)[sm < -110].any()


def _shows(mutant, case):
    if mutant == "c":
        return case.trips > 0
    if mutant == "g":
        return case.n >= 5
    if mutant in ("a", "b"):
        return case.special != "same_rows"
    if mutant == "f":
        return case.special not in ("saturated", "tiny")
    return True


def _failing(verify, inp, out, stages):
    bad = set()
    for k in stages:
        try:
            verify(inp, out, stages=(k,))
        except AssertionError:
            bad.add(k)
    return bad


@pytest.mark.parametrize("mutant", list(af.MUTANTS))
def test_mutant_is_rejected_in_a_stage_it_corrupts(mutant, capsys):
    shown = 0
    for case in af.CASES:
        if not _shows(mutant, case):
            continue
        fwd, bwd, out, bout = _run(case)
        stride = CUS * max(case.trips, 1)
        mf = af.emulate_forward(fwd, mutant, stride)
        mb = af.emulate_backward(bwd, mutant, stride)
        bad = _failing(af.verify_forward, fwd, mf, FWD_STAGES) | _failing(af.verify_backward, bwd, mb, BWD_STAGES)
        assert bad and bad <= set(af.MUTANTS[mutant]), (mutant, case.name, sorted(bad))
        shown += 1
    capsys.readouterr()
    assert shown >= 8, (mutant, shown)
