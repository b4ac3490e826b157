"""The pose-order decode with hold durations (include/qtcnn.h, qt_pose_duration_decode) as plain loops: Python and np.int64
integers, one frame after the other, nothing vectorised across frames (inside a frame the D x S and S x S candidates are one
integer array each).  The rule is restated as the header writes it, with the prefix sums cum and every beta kept, not with the
kernel's ring.  Everything is an integer from the emission score on, so every output of the kernel is compared with these for
equality.  Also here: the run-length count (qt_pose_duration_count) by a walk, the three host helpers restated, and the seeded
tracks of the box-prior test with the labels they were drawn from.  The emission rule, its table and the clamp are
tests/_pose_order_ref.py's; nothing of them is restated.  The reference project has no such step, so there is no fixture."""
import numpy as np

from _pose_order_ref import F32, SCORE_FLOOR, TRANS_FLOOR, bits, clamp_trans, emissions, q_array  # noqa: F401

DUR_MAX = 128                                    # QT_POSE_DUR_MAX


def stream_length(lengths, b, frames):
    return frames if lengths is None else min(max(int(lengths[b]), 1), frames)


def decode(probs, state_class, trans, dur, init=None, dur_open=None, lengths=None):
    """probs f32 [B,T,C]; state_class [S]; trans [S,S]; dur [S,D]; init [S] or None; dur_open [S,D] or None (dur); lengths [B]
    or None.  Returns (path int64 [B,T], start int64 [B,T], score int64 [B]); -1 at and beyond a stream's length."""
    probs = np.asarray(probs, F32)
    B, frames, C = probs.shape
    S = len(state_class)
    trans = clamp_trans(trans).reshape(S, S)
    dur = clamp_trans(dur).reshape(S, -1)
    D = dur.shape[1]
    dur_open = dur if dur_open is None else clamp_trans(dur_open).reshape(S, D)
    init = np.zeros(S, np.int64) if init is None else clamp_trans(init)
    path, start = np.full((B, frames), -1, np.int64), np.full((B, frames), -1, np.int64)
    score = np.empty(B, np.int64)
    cols = np.arange(S)
    for b in range(B):
        T = stream_length(lengths, b, frames)
        e = emissions(probs[b, :T], state_class)
        cum = np.zeros((T + 1, S), np.int64)
        for f in range(T):
            cum[f + 1] = cum[f] + e[f]
        beta = np.empty((T, S), np.int64)
        alpha = np.empty((T + 1, S), np.int64)
        dlen, frm = np.zeros((T + 1, S), np.int64), np.zeros((T + 1, S), np.int64)
        beta[0] = (init[:, None] + trans).max(axis=0)
        for f in range(1, T + 1):
            n = min(D, f)
            d = np.arange(1, n + 1)
            table = np.array(dur_open.T[:n] if f == T else dur.T[:n])          # [d - 1][j]
            if f <= D:
                table[f - 1] = dur_open[:, f - 1]                             # f - d == 0: the stream's first segment
            cand = beta[f - d] + table + (cum[f] - cum[f - d])                 # [d - 1][j]
            k = np.argmax(cand, axis=0)                                       # the lowest d that attains the maximum
            alpha[f], dlen[f] = cand[k, cols], k + 1
            if f < T:
                step = alpha[f][:, None] + trans                              # [i][j]
                frm[f] = np.argmax(step, axis=0)                              # the lowest i
                beta[f] = step[frm[f], cols]
        j = int(np.argmax(alpha[T]))                                          # the lowest j
        score[b] = alpha[T, j]
        f = T
        while True:
            d = int(dlen[f, j])
            path[b, f - d:f], start[b, f - d:f] = j, f - d
            f -= d
            if f == 0:
                break
            j = int(frm[f, j])
    return path, start, score


def count_durations(path, S, D, lengths=None, counts=None):
    """counts int64 [S, D] (added to a copy of `counts`): the run lengths of path int64 [B, T], by a walk"""
    path = np.asarray(path, np.int64)
    B, frames = path.shape
    counts = np.zeros((S, D), np.int64) if counts is None else np.array(counts, np.int64)
    for b in range(B):
        T = stream_length(lengths, b, frames)
        f = 0
        while f < T:
            v, s = int(path[b, f]), f
            while f < T and int(path[b, f]) == v:
                f += 1
            if 0 <= v < S and s > 0 and f < T:
                counts[v, min(f - s, D) - 1] += 1
    return counts


def runs_of(values):
    """[(start, length, value)] of one stream's frames, every value"""
    out, s = [], 0
    for f in range(1, len(values) + 1):
        if f == len(values) or values[f] != values[s]:
            out.append((s, f - s, int(values[s])))
            s = f
    return out


# ---- the host helpers, restated ---------------------------------------------------------------------------------------------------
def duration_prior(counts, pseudo_count=1.0):
    counts = np.asarray(counts, np.int64)
    out = np.empty(counts.shape, np.int32)
    for j, row in enumerate(counts):
        r = [float(c) + float(pseudo_count) for c in row]
        R = sum(r)
        for k, v in enumerate(r):
            out[j, k] = SCORE_FLOOR if R == 0 else int(q_array(np.array([v / R], np.float64).astype(F32))[0])
    return out


def hold_prior(S, D, shortest, longest, inside=0, outside=TRANS_FLOOR):
    return np.array([[inside if shortest <= d <= longest else outside for d in range(1, D + 1)] for _ in range(S)], np.int32)


def geometric_durations(stay, S, D):
    return np.array([[(d - 1) * stay for d in range(1, D + 1)] for _ in range(S)], np.int32)


def suffix_max(dur):
    dur = np.asarray(dur)
    out = np.array(dur)
    for d in range(dur.shape[1] - 2, -1, -1):
        out[:, d] = np.maximum(out[:, d], out[:, d + 1])
    return out


# ---- data -------------------------------------------------------------------------------------------------------------------------
def make_tracks(seed, batch, frames, C, run=9):
    """(probs, lead): _pose_order_ref.make_probs(seed, batch, frames, C, run) draw for draw, and the labels it was built around
    (the dominant class before some frames were sent off), int64 [batch, frames]"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((batch, frames, C)).astype(F32)
    lead = (np.arange(frames)[None, :] // run + rng.integers(0, C, (batch, 1))) % C
    off = rng.random((batch, frames)) < 0.1
    noisy = np.where(off, rng.integers(0, C, (batch, frames)), lead)
    np.put_along_axis(z, noisy[..., None], z.max(axis=2, keepdims=True) + F32(1.0), axis=2)
    ex = np.exp(z - z.max(axis=2, keepdims=True))
    return (ex / ex.sum(axis=2, keepdims=True)).astype(F32), lead.astype(np.int64)
