"""qt_lstm_stream_forward (csrc/lstm_stream.hip) on the GPU, through the C ABI, every buffer between guard bands
(tests/_guard.py); the workspace and the carry rows in front of a stream's start are handed over NaN-filled.

Accuracy is measured, not fixed in advance.  The reference is the float64 loops of tests/_lstm_stream_ref.py on exactly the
f32 inputs the kernel reads.  The same windows are computed with the existing, float64-verified route -- qt_lstm_forward for
layer 0 on the materialised windows, a torch f32 product for layer 1's input, qt_lstm_forward again, short windows at their
own length -- and e_old / e_new are the two routes' max absolute errors against float64.  The bound is
e_new <= 4 e_old + 2^-20: both routes are the same recurrence in the same precision and differ only in summation order, so
their errors are of one size; 4x covers the spread of a maximum over a small sample, the floor a saturated case where e_old is
exactly 0; a wrong gate, row or weight index shows at 1e-2 or more.  One stream of 3 x 35 frames per (H, T, regime) is
computed once by both references; a case (S, n, seen) is a slice of it.
"""
import functools

import numpy as np
import pytest
import torch

import _lstm_stream_ref as R
from _guard import Guard
from _util import pkg

pytestmark = pytest.mark.gpu
TILE = R.TILE
FLOOR = 2.0 ** -20
FRAMES = 16 + 2 * TILE + 3      # the longest stream a case reads: seen = T = 16, n = 2 TILE + 3


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _lib():
    L = pkg("_lib")
    return L, L.lib()


def _n_values(T):
    return sorted({n for n in (1, T - 1, T, T + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3) if n >= 1})


def _seen_values(T):
    return sorted({0, 1, T - 1, T})


class _Weights:
    """the six weight operands on the device, transposed as the kernel reads them, between guard bands"""

    def __init__(self, w, dev):
        self.guard = Guard(dev)
        self.t = {}
        for name in R.NAMES:
            a = torch.from_numpy(w[name])
            self.t[name] = self.guard.input(name, a.t().contiguous() if a.dim() == 2 else a)

    def ptrs(self, L):
        return [L.ptr(self.t[k]) for k in R.NAMES]


def _run(L, lib, W, buf, seen, n, T, H, carry=True, written=True):
    """one guarded call on xproj0 `buf` [S][T-1+n][4H] (numpy f32): (hlast, carry_out or None) as CPU tensors"""
    dev = W.guard.dev
    S = buf.shape[0]
    g = Guard(dev)
    x = g.input("xproj0", torch.from_numpy(buf))
    hlast = g.output("hlast", (S, n, H), torch.float32, written=written)
    cout = g.output("carry_out", (S, T - 1, 4 * H), torch.float32, written=written) if carry and T > 1 else None
    ws_bytes = lib.qt_lstm_stream_workspace_bytes(S, n, T, H)
    ws = g.workspace("workspace", ws_bytes)
    L.check(lib.qt_lstm_stream_forward(L.ptr(x), *W.ptrs(L), L.ptr(hlast), L.ptr(cout), L.ptr(ws), ws_bytes, seen, S, n, T, H,
                                       L.stream_ptr()), "qt_lstm_stream_forward")
    g.check()
    return hlast.cpu(), None if cout is None else cout.cpu()


def _old_route(L, lib, W, w_dev, rows, T, H):
    """h1 of the last step of every window of `rows` [S][FRAMES][4H] by qt_lstm_forward x 2 (+ a torch f32 product), windows
    of one length per launch: [S][FRAMES][H] on the CPU"""
    dev = W.guard.dev
    S, frames, _ = rows.shape
    xr = torch.from_numpy(rows).to(dev)
    out = torch.empty(S, frames, H)
    f32 = dict(dtype=torch.float32, device=dev)
    for length in range(1, T + 1):
        ends = [g for g in range(frames) if min(T, g + 1) == length]
        if not ends:
            continue
        idx = torch.tensor([[g - length + 1 + t for t in range(length)] for g in ends], device=dev)
        xw = xr[:, idx].reshape(S * len(ends), length, 4 * H).contiguous()
        B = xw.shape[0]
        hout = None
        for layer in (0, 1):
            if layer == 1:
                xw = (hout.view(B * length, H) @ w_dev["wih1"].t() + w_dev["bih1"]).view(B, length, 4 * H).contiguous()
            gates, cell = torch.empty(B, length, 4 * H, **f32), torch.empty(B, length, H, **f32)
            hprev, hout = torch.empty(B, length, H, **f32), torch.empty(B, length, H, **f32)
            L.check(lib.qt_lstm_forward(L.ptr(xw), L.ptr(W.t["whh%d" % layer]), L.ptr(W.t["bhh%d" % layer]), L.ptr(gates),
                                        L.ptr(cell), L.ptr(hprev), L.ptr(hout), B, length, H, L.stream_ptr()),
                    "qt_lstm_forward")
        out[:, ends] = hout[:, -1].view(S, len(ends), H).cpu()
    return out


@functools.lru_cache(maxsize=None)
def _world(H, T, regime):
    """inputs, weights on the device and both references of one (H, T, regime), computed once"""
    dev = torch.device("cuda:0")
    L, lib = _lib()
    w = R.weights(H)
    rows = R.stream_rows(H, 3, FRAMES, regime)
    W = _Weights(w, dev)
    w_dev = {k: torch.from_numpy(v).to(dev) for k, v in w.items()}
    ref64, _ = R.stream_forward(R.call_buffer(rows, 0, FRAMES, T, fill=0.0), w, 0, FRAMES, T, np.float64)
    old = _old_route(L, lib, W, w_dev, rows, T, H)
    err_old = np.abs(old.double().numpy() - ref64).max(axis=2)          # [3][FRAMES]
    assert float(err_old.max()) <= 1e-4                                 # the yardstick itself is sound
    return rows, W, ref64, err_old


@pytest.mark.parametrize("regime", ["normal", "saturated"])
@pytest.mark.parametrize("T", [1, 2, 4, 16])
@pytest.mark.parametrize("H", [64, 256])
def test_stream_matches_float64_as_closely_as_the_window_route(H, T, regime):
    _dev()
    L, lib = _lib()
    rows, W, ref64, err_old = _world(H, T, regime)
    worst = (0.0, 0.0)
    for S in (1, 3):
        sl = slice(1, 2) if S == 1 else slice(0, 3)
        for n in _n_values(T):
            for seen in _seen_values(T):
                buf = R.call_buffer(rows[sl], seen, n, T)               # NaN in front of the stream's start
                hlast, cout = _run(L, lib, W, buf, seen, n, T, H)
                e_new = float(np.abs(hlast.double().numpy() - ref64[sl, seen:seen + n]).max())
                e_old = float(err_old[sl, seen:seen + n].max())
                print(f"H={H} T={T} {regime} S={S} n={n} seen={seen}: e_old={e_old:.3e} e_new={e_new:.3e}")
                assert e_new <= 4 * e_old + FLOOR, (S, n, seen, e_old, e_new)
                if e_new >= worst[1]:
                    worst = (e_old, e_new)
                if cout is not None:
                    want = np.zeros((S, T - 1, 4 * H), np.float32)
                    for k in range(T - 1):
                        if seen + n - (T - 1) + k >= 0:
                            want[:, k] = buf[:, n + k]
                    assert np.array_equal(cout.numpy(), want), (S, n, seen)
    W.guard.check()
    print(f"H={H} T={T} {regime}: largest e_new={worst[1]:.3e} (e_old={worst[0]:.3e})")


@pytest.mark.parametrize("H,T", [(64, 4), (256, 4), (64, 16), (256, 2)])
def test_a_nan_row_reaches_exactly_the_windows_that_hold_it(H, T):
    """row r of xproj0 is read by frames r-T+1 .. r of the call (frame f reads rows f .. f+T-1) and by nothing else"""
    _dev()
    L, lib = _lib()
    rows, W, _, _ = _world(H, T, "normal")
    n, seen = 2 * TILE + 3, T
    clean = R.call_buffer(rows[:3], seen, n, T)
    last = T - 1 + n - 1
    for s, r in ((0, 0), (1, T - 2), (2, T - 1 + TILE - 1), (1, T - 1 + TILE), (0, last)):
        buf = clean.copy()
        buf[s, r] = np.nan
        hlast, _ = _run(L, lib, W, buf, seen, n, T, H, written=False)
        nan = torch.isnan(hlast)
        want = torch.zeros(3, n, dtype=torch.bool)
        want[s, max(0, r - T + 1):min(n, r + 1)] = True
        assert torch.equal(nan.all(dim=2), want), (s, r)
        assert torch.equal(nan.any(dim=2), want), (s, r)
    W.guard.check()


@pytest.mark.parametrize("T", [1, 2, 4, 16])
@pytest.mark.parametrize("H", [64, 256])
def test_every_split_and_a_stream_alone_give_the_bits_of_one_call(H, T):
    _dev()
    L, lib = _lib()
    rows, W, _, _ = _world(H, T, "normal")
    frames = 2 * TILE + 3
    rows = rows[:, :frames]
    whole_h, whole_c = _run(L, lib, W, R.call_buffer(rows, 0, frames, T), 0, frames, T, H)
    for cut in sorted({c for c in (1, T - 1, T, TILE, TILE + 1) if 0 < c < frames}):
        h_a, c_a = _run(L, lib, W, R.call_buffer(rows, 0, cut, T), 0, cut, T, H)
        carry = c_a.numpy() if c_a is not None else np.zeros((3, 0, 4 * H), np.float32)
        buf = np.concatenate([carry, rows[:, cut:]], axis=1)
        h_b, c_b = _run(L, lib, W, buf, cut, frames - cut, T, H)
        assert torch.equal(torch.cat([h_a, h_b], dim=1), whole_h), cut
        if T > 1:
            assert torch.equal(c_b, whole_c), cut
    alone_h, alone_c = _run(L, lib, W, R.call_buffer(rows[1:2], 0, frames, T), 0, frames, T, H)
    assert torch.equal(alone_h, whole_h[1:2])
    if T > 1:
        assert torch.equal(alone_c, whole_c[1:2])
    W.guard.check()


def test_stage_puts_the_new_rows_behind_the_carry():
    dev = _dev()
    L, lib = _lib()
    S, n, T, H = 3, 5, 4, 64
    g = Guard(dev)
    gen = torch.Generator().manual_seed(5)
    carry = g.input("carry_in", torch.randn(S, T - 1, 4 * H, generator=gen))
    xnew = g.input("xnew", torch.randn(S, n, 4 * H, generator=gen))
    out = g.output("xproj0", (S, T - 1 + n, 4 * H), torch.float32)
    L.check(lib.qt_lstm_stream_stage(L.ptr(carry), L.ptr(xnew), L.ptr(out), S, n, T, H, L.stream_ptr()), "qt_lstm_stream_stage")
    g.check()
    assert torch.equal(out, torch.cat([carry, xnew], dim=1))
