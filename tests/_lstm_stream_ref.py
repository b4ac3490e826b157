"""The stream rule of the 2-layer LSTM (include/qtcnn.h, qt_lstm_stream_forward) as plain loops, in float64 and in f32,
shared by tests/test_lstm_stream_cpu.py and tests/test_lstm_stream_gpu.py.

S streams advance together by n frames per call, `seen` frames came before.  Frame f of the call (global index
g = seen + f) gets h1 at the last step of the LSTM run from a zero state over the len = min(T, g + 1) frames ending at g.
xproj0 [S][T-1+n][4H] holds layer 0's input products, b_ih included: the T - 1 carry rows first, then the call's rows, so the
window of frame f is rows f + T - len .. f + T - 1, and rows of frames in front of the stream's start are never read.
torch gate order i, f, g, o.
"""
import numpy as np
import torch

TILE = 8   # QT_LSTM_STREAM_TILE
NAMES = ("whh0", "bhh0", "wih1", "bih1", "whh1", "bhh1")


def weights(H, seed=0):
    """W_hh0 [4H][H], b_hh0 [4H], W_ih1 [4H][H], b_ih1, W_hh1, b_hh1 (f32 numpy), scaled as _head_bounds.lstm_inputs does"""
    g = torch.Generator().manual_seed(7000 + 10 * H + seed)
    out = {}
    for name in NAMES:
        out[name] = (torch.randn(4 * H, H, generator=g) / H ** 0.5 if name[0] == "w" else
                     torch.randn(4 * H, generator=g) * 0.1).numpy()
    return out


def stream_rows(H, S, frames, regime, seed=0):
    """layer 0's input products of S streams of `frames` frames, [S][frames][4H] f32 numpy.  "saturated": x 30 and every 16th
    column at +-120, so that gates reach exactly 0 and 1 and __expf(-x) overflows (the regime of _head_bounds.lstm_inputs)"""
    g = torch.Generator().manual_seed(1000 * H + 10 * frames + S + seed)
    x = torch.randn(S, frames, 4 * H, generator=g)
    if regime == "saturated":
        x = x * 30.0
        x[:, :, 1::16] = torch.sign(x[:, :, 1::16]) * 120.0
    else:
        assert regime == "normal"
    return x.numpy()


def call_buffer(rows, seen, n, T, fill=np.nan):
    """xproj0 [S][T-1+n][4H] of the call that handles frames seen .. seen+n-1 of `rows` [S][frames][4H]: the carry rows in
    front of the stream's start hold `fill`"""
    S, _, C = rows.shape
    buf = np.full((S, T - 1 + n, C), fill, rows.dtype)
    for r in range(T - 1 + n):
        g = seen - (T - 1) + r
        if g >= 0:
            buf[:, r] = rows[:, g]
    return buf


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def _cell(pre, c, H):
    i, f, g, o = _sigmoid(pre[:H]), _sigmoid(pre[H:2 * H]), np.tanh(pre[2 * H:3 * H]), _sigmoid(pre[3 * H:])
    c = f * c + i * g
    return c, o * np.tanh(c)


def stream_forward(xproj0, w, seen, n, T, dtype=np.float64):
    """(hlast [S][n][H], carry [S][T-1][4H]) of one call, window by window and step by step in `dtype`; the carry is the
    last T - 1 rows of xproj0, rows in front of the stream's start as zeros"""
    x = xproj0.astype(dtype)
    W = {k: v.astype(dtype) for k, v in w.items()}
    S, rows, C = x.shape
    H = C // 4
    assert rows == T - 1 + n
    hlast = np.zeros((S, n, H), dtype)
    for s in range(S):
        for f in range(n):
            length = min(T, seen + f + 1)
            h0, c0, h1, c1 = (np.zeros(H, dtype) for _ in range(4))
            for r in range(f + T - length, f + T):
                c0, h0 = _cell(x[s, r] + W["bhh0"] + W["whh0"] @ h0, c0, H)
                c1, h1 = _cell(W["bih1"] + W["bhh1"] + W["wih1"] @ h0 + W["whh1"] @ h1, c1, H)
            hlast[s, f] = h1
    carry = np.zeros((S, T - 1, C), dtype)
    for k in range(T - 1):
        if seen + n - (T - 1) + k >= 0:
            carry[:, k] = x[:, n + k]
    return hlast, carry


def run_calls(rows, w, cuts, T, dtype=np.float32, fill=np.nan):
    """a stream handed over in consecutive calls cut at `cuts` (frame indices): (hlast [S][frames][H], final carry); the
    carry of a call is the next call's, the first call's holds `fill`"""
    S, frames, C = rows.shape
    carry = np.full((S, T - 1, C), fill, dtype)
    parts = []
    for a, b in zip([0] + list(cuts), list(cuts) + [frames]):
        buf = np.concatenate([carry, rows[:, a:b].astype(dtype)], axis=1)
        h, carry = stream_forward(buf, w, a, b - a, T, dtype)
        parts.append(h)
    return np.concatenate(parts, axis=1), carry


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64).tolist()
