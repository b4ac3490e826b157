"""Fixed-lag pose-order decoding with hold durations (include/qtcnn.h, qt_pose_duration_lag_decode) as plain loops: Python and
np.int64 integers, one frame after the other (inside a frame the D x S and S x S candidates are one integer array each).  The
rule is restated as the header writes it; every beta, dlen, from and end of a call's frames is kept, and what lies before the
call comes out of a `state` dict that holds what the kernel's carry holds (`unpack_carry` / `pack_carry` turn a kernel's carry
into the same fields and back): cum of the last frame, g[f] = beta[f] - cum[f] of the last D values of f at row f mod D, the
words (dlen - 1) | from << 7 of the last `lag` values of f, and the tail word of the newest f.  Everything is an integer, so the
kernel is compared with these for equality.  The emission rule and the clamps are tests/_pose_order_ref.py's, the emitted span
and `split` tests/_pose_lag_ref.py's; nothing of them is restated.  The reference project has no such step."""
import numpy as np

from _pose_lag_ref import span, split  # noqa: F401
from _pose_order_ref import F32, clamp_trans, emissions


def _word(d, j):
    return (int(d) - 1) | int(j) << 7


def decode(probs, state_class, trans, dur, init=None, dur_open=None, lag=0, flush=False, state=None):
    """probs f32 [B, n, C] (n may be 0 with flush).  Returns (g0, (lag_path [B,count], lag_start [B,count], filtered [B,n],
    score [B,n]), state), all int64: state = dict(seen, cum [B,S], g [B,D,S], hist [B,lag,S], tail [B]), slot k of hist being
    f = seen - lag + 1 + k (zeros for f <= 0)."""
    probs = np.asarray(probs, F32)
    B, n, C = probs.shape
    S = len(state_class)
    trans = clamp_trans(trans).reshape(S, S)
    dur = clamp_trans(dur).reshape(S, -1)
    D = dur.shape[1]
    dur_open = dur if dur_open is None else clamp_trans(dur_open).reshape(S, D)
    init = np.zeros(S, np.int64) if init is None else clamp_trans(init)
    if state is None:
        state = dict(seen=0, cum=np.zeros((B, S), np.int64), g=np.zeros((B, D, S), np.int64),
                     hist=np.zeros((B, lag, S), np.int64), tail=np.zeros(B, np.int64))
    seen = state["seen"]
    assert n >= 1 or flush
    g0, g1 = span(seen, n, lag, flush)
    end_f, last = seen + n, seen + n - 1
    path, start = np.empty((B, g1 - g0), np.int64), np.empty((B, g1 - g0), np.int64)
    filtered, score = np.empty((B, n), np.int64), np.empty((B, n), np.int64)
    new = dict(seen=end_f, cum=np.empty((B, S), np.int64), g=state["g"].copy(), hist=np.zeros((B, lag, S), np.int64),
               tail=state["tail"].copy())
    cols = np.arange(S)
    for b in range(B):
        e = emissions(probs[b], state_class) if n else np.zeros((0, S), np.int64)
        cum = {seen: state["cum"][b].copy()}                    # cum[f], f >= seen
        G = {}                                                  # beta[f] - cum[f]
        beta, dlen, frm, dlen_open, end, best = {}, {}, {}, {}, {}, {}
        if seen == 0:
            beta[0] = (init[:, None] + trans).max(axis=0)
            G[0] = beta[0].copy()                               # cum[0] = 0
            new["g"][b, 0] = G[0]
        else:
            for f in range(max(0, seen - D + 1), seen + 1):
                G[f] = state["g"][b, f % D]
            for k in range(lag):                                # the words of f = seen - lag + 1 + k
                f = seen - lag + 1 + k
                if f > 0:
                    dlen[f], frm[f] = (state["hist"][b, k] & 127) + 1, state["hist"][b, k] >> 7
            t = int(state["tail"][b])
            end[seen] = t >> 7
            dlen_open[seen] = {end[seen]: (t & 127) + 1}        # known at the end state only
        for f in range(seen + 1, end_f + 1):
            cum[f] = cum[f - 1] + e[f - 1 - seen]
            m = min(D, f)
            d = np.arange(1, m + 1)
            back = np.stack([G[f - k] for k in d])              # [d - 1][j]: beta[f - d] - cum[f - d]
            table = np.array(dur.T[:m])
            if f <= D:
                table[f - 1] = dur_open[:, f - 1]               # f - d == 0: the segment touches the stream's start
            cand = back + table + cum[f]
            k = np.argmax(cand, axis=0)                         # the lowest d
            alpha, dlen[f] = cand[k, cols], k + 1
            cand = back + dur_open.T[:m] + cum[f]               # as if the stream were cut after frame f
            k = np.argmax(cand, axis=0)
            alpha_open, dlen_open[f] = cand[k, cols], k + 1
            step = alpha[:, None] + trans                       # [i][j]: from the closed alpha
            frm[f] = np.argmax(step, axis=0)                    # the lowest i
            beta[f] = step[frm[f], cols]
            G[f] = beta[f] - cum[f]
            new["g"][b, f % D] = G[f]
            end[f] = int(np.argmax(alpha_open))                 # the lowest j
            best[f] = int(alpha_open[end[f]])
            filtered[b, f - 1 - seen], score[b, f - 1 - seen] = end[f], best[f]
        for g in range(g0, g1):
            F = min(g + lag, last) + 1
            j, f = end[F], F
            d = int(dlen_open[F][j])
            while f - d > g:
                f -= d
                j = int(frm[f][j])
                d = int(dlen[f][j])
            path[b, g - g0], start[b, g - g0] = j, f - d
        new["cum"][b] = cum[end_f]
        for k in range(lag):
            f = end_f - lag + 1 + k
            if f > 0:
                new["hist"][b, k] = [_word(dlen[f][j], frm[f][j]) for j in range(S)]
        if n:
            new["tail"][b] = _word(dlen_open[end_f][end[end_f]], end[end_f])
    return g0, (path, start, filtered, score), new


def carry_stride(S, D, lag):
    return (8 * S + 8 * D * S + 2 * lag * S + 2 + 7) // 8 * 8


def workspace_bytes(B, n, S):
    return (B * n * S * 2 + 7) // 8 * 8 + (B * n * 2 + 7) // 8 * 8


def unpack_carry(raw, B, S, D, lag, seen):
    """a kernel's carry (bytes) as the loops' state; the padding behind each stream must be zeros"""
    raw = np.frombuffer(bytes(raw), np.uint8).reshape(B, carry_stride(S, D, lag))
    at = lambda lo, n, dt: np.stack([np.frombuffer(raw[b, lo:lo + n].tobytes(), dt) for b in range(B)]).astype(np.int64)
    lo_g, lo_h = 8 * S, 8 * S + 8 * D * S
    lo_t = lo_h + 2 * lag * S
    assert not raw[:, lo_t + 2:].any()
    return dict(seen=seen, cum=at(0, 8 * S, np.int64), g=at(lo_g, 8 * D * S, np.int64).reshape(B, D, S),
                hist=at(lo_h, 2 * lag * S, np.uint16).reshape(B, lag, S), tail=at(lo_t, 2, np.uint16)[:, 0])


def pack_carry(state, S, D, lag):
    """the loops' state as a kernel's carry, zeros in the padding"""
    B = state["cum"].shape[0]
    out = np.zeros((B, carry_stride(S, D, lag)), np.uint8)
    for b in range(B):
        body = state["cum"][b].astype(np.int64).tobytes() + state["g"][b].astype(np.int64).tobytes() + \
            state["hist"][b].astype(np.uint16).tobytes() + np.array([state["tail"][b]], np.uint16).tobytes()
        out[b, :len(body)] = np.frombuffer(body, np.uint8)
    return out


def same_state(got, want):
    assert got.keys() == want.keys()
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and (g.astype(np.int64) == w.astype(np.int64)).all(), k
