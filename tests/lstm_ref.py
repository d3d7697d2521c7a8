"""NumPy float64 restatement of the LSTM aggregator (test infrastructure): forward and full backward, written from the
equations, both directions, with the last-position quirk -- the aggregator keeps `seq[:, -1, :]` of a batch_first LSTM,
i.e. the forward direction's final h and the reverse direction's FIRST step (one cell evaluation on the last
neighbour from a zero state; its weight_hh therefore gets an exactly zero gradient).

    gates_t = x_t W_ih^T + b_ih + b_hh + h_{t-1} W_hh^T         (order i, f, g, o)
    i, f, o = sigmoid(.), g = tanh(.);  c_t = f c_{t-1} + i g;  h_t = o tanh(c_t)

rounding="bf16" rounds (to nearest even) exactly where the kernels store bf16 and sums everything in float64: the
neighbour rows, the weights, GX = x W_ih^T + b, the h operand of the next step (and the result), the saved gates the
backward reads, and dG.  c, the biases and every accumulation stay unrounded."""
import numpy as np


def bf16(a):
    """float64 -> nearest bf16 (ties to even) -> float64"""
    u = np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32)).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def _rounder(rounding):
    return bf16 if rounding == "bf16" else (lambda a: np.asarray(a, dtype=np.float64))


def recurrence(GX, w_hh, dh=None, rounding=None):
    """The sequential part alone, as gsage_lstm_fwd / _bwd see it: GX [M, steps, 4H] = the projected rows plus both
    biases (taken as given: the caller rounds it), w_hh [4H, H] (None for one step: no recurrent term), dh [M, H] =
    gradient of the last h or None.  -> (gates [M, steps, 4H] activated, as saved; c [M, steps, H]; hprev [M, steps, H],
    row t = the step's INPUT state; out [M, H]; dG [M, steps, 4H] or None)."""
    r = _rounder(rounding)
    GX = np.asarray(GX, dtype=np.float64)
    M, steps, H4 = GX.shape
    H = H4 // 4
    Wh = r(w_hh) if w_hh is not None else np.zeros((4 * H, H))
    assert w_hh is not None or steps == 1
    h, c = np.zeros((M, H)), np.zeros((M, H))
    gates, cs, hprev = np.zeros((M, steps, 4 * H)), np.zeros((M, steps, H)), np.zeros((M, steps, H))
    for t in range(steps):
        pre = GX[:, t] + h @ Wh.T
        i, f, g, o = _sigmoid(pre[:, :H]), _sigmoid(pre[:, H:2 * H]), np.tanh(pre[:, 2 * H:3 * H]), _sigmoid(pre[:, 3 * H:])
        c = f * c + i * g
        hprev[:, t] = h
        h = r(o * np.tanh(c))
        gates[:, t] = r(np.concatenate([i, f, g, o], axis=1))
        cs[:, t] = c
    if dh is None:
        return gates, cs, hprev, h, None
    dh = np.asarray(dh, dtype=np.float64)
    dc = np.zeros((M, H))
    dG = np.zeros((M, steps, 4 * H))
    for t in range(steps - 1, -1, -1):
        i, f, g, o = (gates[:, t, k * H:(k + 1) * H] for k in range(4))
        tc = np.tanh(cs[:, t])
        cprev = cs[:, t - 1] if t > 0 else np.zeros((M, H))
        dc = dc + dh * o * (1 - tc * tc)
        dG[:, t] = r(np.concatenate([dc * g * i * (1 - i), dc * cprev * f * (1 - f), dc * i * (1 - g * g),
                                     dh * tc * o * (1 - o)], axis=1))
        dh = dG[:, t] @ Wh
        dc = dc * f
    return gates, cs, hprev, h, dG


class Direction(object):
    """One LSTM direction over X [M, steps, D]; .out = h after the last step; .backward(dh) fills the gradients."""

    def __init__(self, X, w_ih, w_hh, b_ih, b_hh, rounding=None, gx_edit=None):
        r = _rounder(rounding)
        self.rounding = rounding
        self.X = r(X)
        self.Wi, self.Wh = r(w_ih), r(w_hh)
        M, steps, _ = self.X.shape
        self.GX = r(self.X @ self.Wi.T + (np.asarray(b_ih, dtype=np.float64) + np.asarray(b_hh, dtype=np.float64)))
        if gx_edit is not None:           # (a sensitivity test's change to the projected rows)
            self.GX = gx_edit(self.GX)
        self.gates, self.c, self.hprev, self.out, _ = recurrence(self.GX, self.Wh, None, rounding)
        self.H, self.steps = self.Wh.shape[1], steps

    def backward(self, dh):
        H, M = self.H, self.X.shape[0]
        dG = recurrence(self.GX, self.Wh, dh, self.rounding)[4]
        self.dG = dG
        flat = dG.reshape(M * self.steps, 4 * H)
        self.d_w_ih = flat.T @ self.X.reshape(M * self.steps, -1)
        self.d_w_hh = flat.T @ self.hprev.reshape(M * self.steps, H)
        self.d_b = flat.sum(axis=0)
        self.d_X = dG @ self.Wi
        return self


def lstm_last(neibs, M, fwd, rev=None, G=None, rounding=None, gx_edit=None):
    """neibs [M n, D]; fwd / rev: (w_ih, w_hh, b_ih, b_hh) of a direction (rev None: unidirectional); G: gradient of
    the result or None; gx_edit(GX [M, n, 4H]) -> GX: a change to the forward direction's projected rows.
    -> dict(out [M, hidden], dirs = the Direction objects, and with G: dneibs, grads = [d w_ih, d w_hh, d b_ih, d b_hh]
    per direction, forward first)."""
    neibs = np.asarray(neibs, dtype=np.float64)
    X = neibs.reshape(M, -1, neibs.shape[1])
    n = X.shape[1]
    dirs = [Direction(X, *fwd, rounding=rounding, gx_edit=gx_edit)]
    if rev is not None:
        dirs.append(Direction(X[:, n - 1:n], *rev, rounding=rounding))
    res = {"out": np.concatenate([d.out for d in dirs], axis=1), "dirs": dirs}
    if G is None:
        return res
    G = np.asarray(G, dtype=np.float64)
    H = dirs[0].H
    dirs[0].backward(G[:, :H])
    dn = dirs[0].d_X.copy()
    if rev is not None:
        dirs[1].backward(G[:, H:])
        dn[:, n - 1] += dirs[1].d_X[:, 0]
    res["dneibs"] = dn.reshape(M * n, -1)
    res["grads"] = [v for d in dirs for v in (d.d_w_ih, d.d_w_hh, d.d_b, d.d_b)]
    return res


PARAMS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def aggregator(x, neibs, w, relu, G):
    """LSTMAggregator.forward and its backward (no rounding): w = the module's state_dict as arrays.
    -> (out, dx, dneibs, {parameter name: gradient})"""
    x = np.asarray(x, dtype=np.float64)
    w = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    M = x.shape[0]
    fwd = tuple(w["lstm." + k] for k in PARAMS)
    rev = tuple(w["lstm." + k + "_reverse"] for k in PARAMS) if "lstm.weight_ih_l0_reverse" in w else None
    agg = lstm_last(neibs, M, fwd, rev)["out"]
    Wx, Wn = w["fc_x.weight"], w["fc_neib.weight"]
    h = Wx.shape[0]
    out = np.concatenate([x @ Wx.T, agg @ Wn.T], axis=1)
    dO = np.asarray(G, dtype=np.float64)
    if relu:
        dO = dO * (out > 0)
        out = np.maximum(out, 0)
    grads = {"fc_x.weight": dO[:, :h].T @ x, "fc_neib.weight": dO[:, h:].T @ agg}
    back = lstm_last(neibs, M, fwd, rev, G=dO[:, h:] @ Wn)
    names = ["lstm." + k for k in PARAMS] + (["lstm." + k + "_reverse" for k in PARAMS] if rev is not None else [])
    grads.update(dict(zip(names, back["grads"])))
    return out, dO[:, :h] @ Wx, back["dneibs"], grads
