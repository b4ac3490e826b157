"""The pose-order posteriors with hold durations (include/qtcnn.h, qt_pose_duration_posterior) on the host: the explicit-duration
forward-backward in log2 over the duration decoder's integer emissions, one frame after the other.  `loops64` is the rule in
float64.  `loops_mixed` is the same loops with the rule's precision: a level (Bt, Al, Be, Bs, Z) is a double, inside an L the
maximum is taken out in double and the terms 2^(x - m), their sum and its log2 are f32, the exponent of begin, endp and of a
count's term is formed in double, rounded to f32 and 2^ taken in f32; occ and dur_counts are sums in double.  It is the yardstick
that a kernel's own f32 rounding is held against.  Both vectorise over the streams of one length and over the states; inside an L
the terms are added one after the other in ascending d (or i, j): np.add.accumulate, which keeps its dtype.  `brute` weighs every
segmentation of a tiny video.  The emission rule, the clamp and the stream lengths are tests/_pose_order_ref.py's and
tests/_pose_duration_ref.py's; nothing of them is restated.  The reference project has no such step, so there is no fixture."""
import itertools

import numpy as np

from _pose_duration_ref import stream_length
from _pose_order_ref import clamp_trans, emissions

F32, F64 = np.float32, np.float64
NAMES = ("posterior", "class_posterior", "begin", "evidence", "dur_counts", "endp")


def L(x, F):
    """L over axis 0 of x (float64): the maximum out in float64, the terms 2^(x - m) and their sum in ascending index in F, log2
    of the sum in F, added to the maximum in float64"""
    m = x.max(axis=0)
    terms = np.exp2((x - m).astype(F))
    s = np.add.accumulate(terms, axis=0, dtype=F)[-1]
    return m + np.log2(s).astype(F64)


def pow2(x, F):
    return np.exp2(x.astype(F))


def tables(S, trans, dur, init, dur_open):
    """(T [S,S], Dur [S,D], DurOpen [S,D], start [S]) in bits, float64 (exact)"""
    T = clamp_trans(trans).reshape(S, S) / 256.0
    Dur = clamp_trans(dur).reshape(S, -1) / 256.0
    DurOpen = Dur if dur_open is None else clamp_trans(dur_open).reshape(Dur.shape) / 256.0
    start = np.zeros(S) if init is None else clamp_trans(init) / 256.0
    return T, Dur, DurOpen, start


def sweep(e, T, Dur, DurOpen, start, F):
    """e int64 [nb, n, S]: the emissions of nb streams of n frames each.  Returns (begin [nb,n,S] in F, endp [nb,n,S] in F with
    row f - 1 for f = 1 .. n, occ float64 [nb,n,S], Z float64 [nb], counts float64 [nb,S,D])"""
    nb, n, S = e.shape
    D = Dur.shape[1]
    cum = np.zeros((nb, n + 1, S), np.int64)
    for f in range(n):
        cum[:, f + 1] = cum[:, f] + e[:, f]
    cum = cum / 256.0                                                      # exact; a difference of two of them is seg
    Bt, Al = np.empty((nb, n, S)), np.empty((nb, n + 1, S))
    Be, Bs = np.zeros((nb, n + 1, S)), np.empty((nb, n, S))
    Bt[:, 0] = L(np.broadcast_to((start[:, None] + T)[:, None, :], (S, nb, S)), F)
    for f in range(1, n + 1):
        k = min(D, f)
        d = np.arange(1, k + 1)
        table = np.array(DurOpen.T[:k] if f == n else Dur.T[:k])           # [d - 1][j]
        if f <= D:
            table[f - 1] = DurOpen[:, f - 1]                               # f - d == 0: the stream's first segment
        x = Bt[:, f - d] + table[None] + (cum[:, f][:, None] - cum[:, f - d])          # [nb][d - 1][j]
        Al[:, f] = L(np.moveaxis(x, 1, 0), F)
        if f < n:
            Bt[:, f] = L(np.moveaxis(Al[:, f][:, :, None] + T[None], 1, 0), F)        # x[i][b][j]
    Z = L(np.moveaxis(Al[:, n], 1, 0), F)
    for f in range(n - 1, -1, -1):
        k = min(D, n - f)
        d = np.arange(1, k + 1)
        table = np.array(DurOpen.T[:k] if f == 0 else Dur.T[:k])
        if n - f <= D:
            table[n - f - 1] = DurOpen[:, n - f - 1]                       # f + d == n: the stream's last segment
        x = table[None] + (cum[:, f + d] - cum[:, f][:, None]) + Be[:, f + d]
        Bs[:, f] = L(np.moveaxis(x, 1, 0), F)
        if f >= 1:
            Be[:, f] = L(np.moveaxis(T[None] + Bs[:, f][:, None, :], 2, 0), F)         # x[j][b][i]
    z = Z[:, None, None]
    begin = pow2(Bt + Bs - z, F)
    endp = pow2(Al[:, 1:] + Be[:, 1:] - z, F)
    occ = np.empty((nb, n, S))
    occ[:, n - 1] = endp[:, n - 1]
    for t in range(n - 2, -1, -1):
        occ[:, t] = occ[:, t + 1] + endp[:, t].astype(F64) - begin[:, t + 1].astype(F64)    # endp[t + 1] is row t
    counts = np.zeros((nb, S, D))
    for f in range(n - 1, 1, -1):                                          # descending f; the uncut segments [f - d, f)
        k = min(D, f - 1)
        d = np.arange(1, k + 1)
        x = Bt[:, f - d] + Dur.T[:k][None] + (cum[:, f][:, None] - cum[:, f - d]) + Be[:, f][:, None, :] - z
        counts[:, :, :k] += np.moveaxis(pow2(x, F), 1, 2).astype(F64)
    return begin, endp, occ, Z, counts


def by_class(post, state_class, C, F):
    out = np.zeros(post.shape[:-1] + (C,), F)
    for j, k in enumerate(state_class):                                    # ascending j
        if 0 <= int(k) < C:
            out[..., int(k)] = (out[..., int(k)] + post[..., j]).astype(F)
    return out


def loops(probs, state_class, trans, dur, init=None, dur_open=None, lengths=None, F=F64):
    """probs f32 [B,T,C]; state_class [S]; trans [S,S]; dur [S,D]; init [S] or None; dur_open [S,D] or None (dur); lengths [B] or
    None.  Returns (posterior [B,T,S], class_posterior [B,T,C], begin [B,T,S], log2_evidence float64 [B], dur_counts float64
    [S,D] from zero, endp [B,T,S] with row f - 1 for f = 1 .. T_b), the probabilities in float64 for F = float64 and in f32
    otherwise; rows at and beyond a stream's length are zeros."""
    probs = np.asarray(probs, F32)
    B, frames, C = probs.shape
    S = len(state_class)
    T, Dur, DurOpen, start = tables(S, trans, dur, init, dur_open)
    out = F64 if F is F64 else F32
    post, begin, endp = (np.zeros((B, frames, S), out) for _ in range(3))
    cls = np.zeros((B, frames, C), out)
    evidence, per_stream = np.zeros(B), np.zeros((B,) + Dur.shape)
    n_of = [stream_length(lengths, b, frames) for b in range(B)]
    for n in sorted(set(n_of)):
        bs = [b for b in range(B) if n_of[b] == n]
        e = np.stack([emissions(probs[b, :n], state_class) for b in bs]).astype(np.int64)
        bg, ep, occ, Z, counts = sweep(e, T, Dur, DurOpen, start, F)
        r = np.maximum(occ, 0.0)
        R = np.zeros(r.shape[:-1])
        for j in range(S):                                                 # ascending j, float64
            R = R + r[..., j]
        with np.errstate(divide="ignore", invalid="ignore"):
            p = np.where(R[..., None] > 0, r / R[..., None], 1.0 / S).astype(out)
        post[bs, :n], begin[bs, :n], endp[bs, :n] = p, bg, ep
        cls[bs, :n] = by_class(p, state_class, C, out)
        evidence[bs], per_stream[bs] = Z, counts
    dur_counts = np.zeros(Dur.shape)
    for b in range(B):                                                     # ascending stream, from zero
        dur_counts += per_stream[b]
    return post, cls, begin, evidence, dur_counts, endp


def loops64(*a, **k):
    return loops(*a, **k, F=F64)


def loops_mixed(*a, **k):
    return loops(*a, **k, F=F32)


def brute(probs, state_class, trans, dur, init=None, dur_open=None):
    """one stream [n, C]: every segmentation into (state, length <= D) pairs weighed in float64.  Returns (posterior [n,S],
    begin [n,S], endp [n,S] with row f - 1, log2_evidence, dur_counts [S,D])"""
    probs = np.asarray(probs, F32)
    n, S = probs.shape[0], len(state_class)
    T, Dur, DurOpen, start = tables(S, trans, dur, init, dur_open)
    D = Dur.shape[1]
    E = emissions(probs, state_class) / 256.0
    first = np.log2(np.exp2(start[:, None] + T).sum(axis=0))              # Bt[0]

    def compositions(left):
        if left == 0:
            yield ()
        for d in range(1, min(D, left) + 1):
            for rest in compositions(left - d):
                yield (d,) + rest

    post, begin, endp, counts, total = np.zeros((n, S)), np.zeros((n, S)), np.zeros((n, S)), np.zeros((S, D)), 0.0
    for lens in compositions(n):
        bounds = np.concatenate([[0], np.cumsum(lens)])
        for states in itertools.product(range(S), repeat=len(lens)):
            w = first[states[0]]
            for k, (j, d) in enumerate(zip(states, lens)):
                a, z = bounds[k], bounds[k + 1]
                w += (DurOpen if a == 0 or z == n else Dur)[j, d - 1] + E[a:z, j].sum()
                if k:
                    w += T[states[k - 1], j]
            w = np.exp2(w)
            total += w
            for k, (j, d) in enumerate(zip(states, lens)):
                a, z = bounds[k], bounds[k + 1]
                post[a:z, j] += w
                begin[a, j] += w
                endp[z - 1, j] += w
                if a > 0 and z < n:
                    counts[j, d - 1] += w
    return post / total, begin / total, endp / total, float(np.log2(total)), counts / total
