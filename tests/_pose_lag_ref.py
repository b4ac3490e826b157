"""Fixed-lag pose-order posteriors and revised paths (include/qtcnn.h, qt_pose_lag_smooth and qt_pose_lag_decode) as plain
loops, built on tests/_pose_posterior_ref.py (float64 and numpy f32) and tests/_pose_order_ref.py (integers).  A stream's frames
carry global indices g; a call covers [seen, seen + n) and emits [g0, g1) (`span`); the answer for frame g is conditioned on the
frames up to w = min(g + lag, the call's last frame).  Between calls the history travels in a `state` dict that holds what
the kernels' carries hold (`unpack_*_carry` / `pack_*_carry` turn a kernel's carry into the same fields and back).  `split`
drives consecutive calls.  The reference project has no such step."""
import numpy as np

import _pose_order_ref as O
import _pose_posterior_ref as R

F32, F64 = np.float32, np.float64
LAG_MAX = 63


def span(seen, n, lag, flush):
    """(g0, g1): the frames a call emits"""
    return max(0, seen - lag), (seen + n if flush else max(0, seen + n - lag))


def live(which, n, lag):
    """the route the library picks by itself: one new frame, or n (lag + 1) <= 16 (smooth) / 4096 (decode), a flush alone
    counting its pending frames"""
    return n == 1 or (n or lag) * (lag + 1) <= (16 if which == "smooth" else 4096)


def _tail(history, new, lag):
    """the last `lag` rows of history + new along axis 1, zeros in front of the stream's start"""
    both = np.concatenate([np.zeros_like(history), history, new], axis=1)
    return both[:, both.shape[1] - lag:]


def smooth(probs, state_class, trans, init=None, lag=0, flush=False, state=None, F=F64):
    """probs f32 [B, n, C] (n may be 0 with flush).  Returns (g0, (lagged [B,count,S], lagged_class [B,count,C], filtered
    [B,n,S], evidence float64 [B]), state): state = dict(seen, total float64 [B], a_last [B,S], a [B,lag,S], q int64
    [B,lag,S]), slot k of the history being frame seen - lag + k."""
    probs = np.asarray(probs, F32)
    B, n, C = probs.shape
    S = len(state_class)
    T = (O.clamp_trans(trans).reshape(S, S) / 256.0).astype(F)
    start = np.zeros(S, F) if init is None else (O.clamp_trans(init) / 256.0).astype(F)
    if state is None:
        state = dict(seen=0, total=np.zeros(B, F64), a_last=np.zeros((B, S), F), a=np.zeros((B, lag, S), F),
                     q=np.zeros((B, lag, S), np.int64))
    seen = state["seen"]
    assert n >= 1 or flush
    g0, g1 = span(seen, n, lag, flush)
    q_new = np.stack([O.emissions(probs[b], state_class) for b in range(B)]) if n else np.zeros((B, 0, S), np.int64)
    E_new = (q_new / 256.0).astype(F)
    first = np.broadcast_to(start, (B, S)).astype(F) if seen == 0 else state["a_last"].astype(F)
    if n:
        rows_new, c = R.forward(E_new, T, first, F)
    else:
        rows_new, c = np.zeros((B, 0, S), F), np.zeros((B, 0), F64)
    h = min(lag, seen)                                          # the history frames that exist: g0 .. seen - 1
    A = np.concatenate([state["a"][:, lag - h:].astype(F), rows_new], axis=1)
    E = np.concatenate([(state["q"][:, lag - h:] / 256.0).astype(F), E_new], axis=1)
    last = seen + n - 1
    lagged = np.empty((B, g1 - g0, S), F)
    for g in range(g0, g1):
        w = min(g + lag, last)
        if w == g:
            lagged[:, g - g0] = np.exp2(A[:, g - g0])
            continue
        b = np.zeros((B, S), F)
        for f in range(w - 1, g - 1, -1):
            b = R.b_step(E[:, f + 1 - g0], T, b, F)
        u = A[:, g - g0] + b
        m, lg = R.L(u, -1, F)
        lagged[:, g - g0] = np.exp2((u - m[..., None]) - lg[..., None])
    total, evidence = state["total"].copy(), np.zeros(B, F64)
    for f in range(n):                                          # one addition per frame, onto the running total
        total += c[:, f]
        evidence += c[:, f]
    new = dict(seen=seen + n, total=total, a_last=rows_new[:, -1].copy() if n else first.copy(),
               a=_tail(state["a"].astype(F), rows_new, lag), q=_tail(state["q"], q_new, lag))
    return g0, (lagged, R.by_class(lagged, state_class, C, F), np.exp2(rows_new), evidence), new


def decode(probs, state_class, trans, init=None, lag=0, flush=False, state=None):
    """Returns (g0, (lag_path int64 [B,count], filtered int64 [B,n]), state): state = dict(seen, offset int64 [B], delta int64
    [B,S] (maximum 0), psi int64 [B,lag,S])."""
    probs = np.asarray(probs, F32)
    B, n, C = probs.shape
    S = len(state_class)
    trans = O.clamp_trans(trans).reshape(S, S)
    init = np.zeros(S, np.int64) if init is None else O.clamp_trans(init)
    if state is None:
        state = dict(seen=0, offset=np.zeros(B, np.int64), delta=np.zeros((B, S), np.int64), psi=np.zeros((B, lag, S), np.int64))
    seen = state["seen"]
    assert n >= 1 or flush
    g0, g1 = span(seen, n, lag, flush)
    last, h = seen + n - 1, min(lag, seen)
    path, filtered = np.empty((B, g1 - g0), np.int64), np.empty((B, n), np.int64)
    psi_new = np.empty((B, n, S), np.int64)
    offset, delta = state["offset"].copy(), np.empty((B, S), np.int64)
    for b in range(B):
        e = O.emissions(probs[b], state_class)
        d = init.copy() if seen == 0 else state["delta"][b].copy()
        for f in range(n):
            cand = d[:, None] + trans                           # [i, j]
            psi_new[b, f] = np.argmax(cand, axis=0)             # the lowest i that attains the maximum
            d = cand[psi_new[b, f], np.arange(S)] + e[f]
            filtered[b, f] = int(np.argmax(d))                  # the lowest j
        psi = np.concatenate([state["psi"][b, lag - h:], psi_new[b]], axis=0)      # frames g0 ..
        for g in range(g0, g1):
            w = min(g + lag, last)
            s = int(filtered[b, w - seen]) if w >= seen else int(np.argmax(state["delta"][b]))
            for f in range(w, g, -1):
                s = int(psi[f - g0, s])
            path[b, g - g0] = s
        m = int(d.max())
        offset[b] += m
        delta[b] = d - m
    new = dict(seen=seen + n, offset=offset, delta=delta, psi=_tail(state["psi"], psi_new, lag))
    return g0, (path, filtered), new


def split(fn, probs, cuts, *args, flush_last=True, **kw):
    """consecutive calls of `fn` (smooth or decode) cut at `cuts`: (the first emitted frame, the outputs joined along the frame
    axis (the evidence summed), the last state, the calls' own returns)"""
    n = probs.shape[1]
    edges = [0] + list(cuts) + [n]
    state, calls = None, []
    for k, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        g0, outs, state = fn(probs[:, a:b], *args, flush=flush_last and k == len(edges) - 2, state=state, **kw)
        calls.append((g0, outs))
    joined = tuple(sum(o[i] for _, o in calls) if calls[0][1][i].ndim == 1 and calls[0][1][i].dtype == F64
                   else np.concatenate([o[i] for _, o in calls], axis=1) for i in range(len(calls[0][1])))
    return calls[0][0], joined, state, calls


def smooth_carry_stride(S, lag):
    return (8 + 4 * S * (1 + lag) + 2 * S * lag + 7) // 8 * 8


def decode_carry_stride(S, lag):
    return (8 + 4 * S + lag * S + 7) // 8 * 8


def unpack_smooth_carry(raw, B, S, lag, seen):
    """a kernel's carry (bytes) as the f32 loops' state; the padding behind each stream is not looked at"""
    raw = np.frombuffer(bytes(raw), np.uint8).reshape(B, smooth_carry_stride(S, lag))
    at = lambda lo, n, dt: np.stack([np.frombuffer(raw[b, lo:lo + n].tobytes(), dt) for b in range(B)])
    return dict(seen=seen, total=at(0, 8, F64)[:, 0], a_last=at(8, 4 * S, F32),
                a=at(8 + 4 * S, 4 * S * lag, F32).reshape(B, lag, S),
                q=at(8 + 4 * S * (1 + lag), 2 * S * lag, np.int16).reshape(B, lag, S).astype(np.int64))


def pack_smooth_carry(state, S, lag):
    """the f32 loops' state as a kernel's carry, zeros in the padding"""
    B = state["a_last"].shape[0]
    out = np.zeros((B, smooth_carry_stride(S, lag)), np.uint8)
    for b in range(B):
        body = np.array([state["total"][b]], F64).tobytes() + state["a_last"][b].astype(F32).tobytes() + \
            state["a"][b].astype(F32).tobytes() + state["q"][b].astype(np.int16).tobytes()
        out[b, :len(body)] = np.frombuffer(body, np.uint8)
    return out


def unpack_decode_carry(raw, B, S, lag, seen):
    raw = np.frombuffer(bytes(raw), np.uint8).reshape(B, decode_carry_stride(S, lag))
    at = lambda lo, n, dt: np.stack([np.frombuffer(raw[b, lo:lo + n].tobytes(), dt) for b in range(B)])
    return dict(seen=seen, offset=at(0, 8, np.int64)[:, 0], delta=at(8, 4 * S, np.int32).astype(np.int64),
                psi=at(8 + 4 * S, S * lag, np.uint8).reshape(B, lag, S).astype(np.int64))


def pack_decode_carry(state, S, lag):
    B = state["delta"].shape[0]
    out = np.zeros((B, decode_carry_stride(S, lag)), np.uint8)
    for b in range(B):
        body = np.array([state["offset"][b]], np.int64).tobytes() + state["delta"][b].astype(np.int32).tobytes() + \
            state["psi"][b].astype(np.uint8).tobytes()
        out[b, :len(body)] = np.frombuffer(body, np.uint8)
    return out


def same_state(got, want):
    """the fields of two states, bit for bit (integers by value)"""
    assert got.keys() == want.keys()
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if w.dtype.kind == "f":
            assert g.dtype == w.dtype and O.bits(g) == O.bits(w), k
        else:
            assert g.shape == w.shape and (g.astype(np.int64) == w.astype(np.int64)).all(), k
