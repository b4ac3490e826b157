"""The learner of the chain with hold durations (include/qtcnn.h, qt_pose_duration_prior_expect / _count_paths / _update) on
the host.  `loops64` is the E-step's rule in float64: the levels Bt, Al, Be, Bs, Z of tests/_pose_duration_posterior_ref.py (its
recurrences with its L, frame by frame; that file returns no levels, so they are walked here and its dur_counts and evidence
are what the tests hold these against), the pairwise terms xi_f[i][j] of every frame from them, a stream's terms added in
descending f and the streams in ascending order from zero, in float64.  `loops_mixed` is the same loops with the rule's
precision: double levels, the exponent of a term formed in double, rounded to f32 and 2^ taken in f32, double sums.  It is the
yardstick that a kernel's own f32 rounding is held against.  `brute` weighs every segmentation of a tiny video, `count_paths`
walks given segmentations, `m_step` is the M-step in numpy and `fit` the EM loop.  Every E-step function returns what ONE call
adds: (trans_counts float64 [S, S], start_counts float64 [S], dur_counts float64 [S, D], totals float64 [2] = (evidence in
bits, frames)).  The reference project has no such step, so there is no fixture."""
import itertools

import numpy as np

import _pose_duration_posterior_ref as P
import _pose_prior_ref as PR
from _pose_duration_ref import stream_length
from _pose_order_ref import TRANS_FLOOR, emissions, q_array

F32, F64 = np.float32, np.float64
L, pow2, tables = P.L, P.pow2, P.tables


def levels(e, T, Dur, DurOpen, start, F):
    """e int64 [nb, n, S] -> (Bt [nb,n,S], Al [nb,n+1,S] (row 0 unused), Be [nb,n+1,S], Bs [nb,n,S], Z [nb], cum [nb,n+1,S]),
    float64: _pose_duration_posterior_ref.sweep's recurrences, line for line"""
    nb, n, S = e.shape
    D = Dur.shape[1]
    cum = np.zeros((nb, n + 1, S), np.int64)
    for f in range(n):
        cum[:, f + 1] = cum[:, f] + e[:, f]
    cum = cum / 256.0
    Bt, Al = np.empty((nb, n, S)), np.zeros((nb, n + 1, S))
    Be, Bs = np.zeros((nb, n + 1, S)), np.empty((nb, n, S))
    Bt[:, 0] = L(np.broadcast_to((start[:, None] + T)[:, None, :], (S, nb, S)), F)
    for f in range(1, n + 1):
        k = min(D, f)
        d = np.arange(1, k + 1)
        table = np.array(DurOpen.T[:k] if f == n else Dur.T[:k])
        if f <= D:
            table[f - 1] = DurOpen[:, f - 1]
        x = Bt[:, f - d] + table[None] + (cum[:, f][:, None] - cum[:, f - d])
        Al[:, f] = L(np.moveaxis(x, 1, 0), F)
        if f < n:
            Bt[:, f] = L(np.moveaxis(Al[:, f][:, :, None] + T[None], 1, 0), F)
    Z = L(np.moveaxis(Al[:, n], 1, 0), F)
    for f in range(n - 1, -1, -1):
        k = min(D, n - f)
        d = np.arange(1, k + 1)
        table = np.array(DurOpen.T[:k] if f == 0 else Dur.T[:k])
        if n - f <= D:
            table[n - f - 1] = DurOpen[:, n - f - 1]
        x = table[None] + (cum[:, f + d] - cum[:, f][:, None]) + Be[:, f + d]
        Bs[:, f] = L(np.moveaxis(x, 1, 0), F)
        if f >= 1:
            Be[:, f] = L(np.moveaxis(T[None] + Bs[:, f][:, None, :], 2, 0), F)
    return Bt, Al, Be, Bs, Z, cum


def sweep(e, T, Dur, DurOpen, start, F):
    """per stream: (trans [nb,S,S], start_counts [nb,S], dur [nb,S,D], Z [nb]), float64; a stream's terms in descending f"""
    nb, n, S = e.shape
    D = Dur.shape[1]
    Bt, Al, Be, Bs, Z, cum = levels(e, T, Dur, DurOpen, start, F)
    z = Z[:, None, None]
    trans = np.zeros((nb, S, S))
    for f in range(n - 1, 0, -1):
        x = Al[:, f][:, :, None] + T[None] + Bs[:, f][:, None, :] - z                 # [b][i][j]
        trans += pow2(x, F).astype(F64)
    x0 = pow2(start[None, :, None] + T[None] + Bs[:, 0][:, None, :] - z, F).astype(F64)
    first = np.zeros((nb, S))
    for j in range(S):                                                               # ascending j
        first = first + x0[:, :, j]
    dur = np.zeros((nb, S, D))
    for f in range(n - 1, 1, -1):                                                    # the uncut segments [f - d, f)
        k = min(D, f - 1)
        d = np.arange(1, k + 1)
        x = Bt[:, f - d] + Dur.T[:k][None] + (cum[:, f][:, None] - cum[:, f - d]) + Be[:, f][:, None, :] - z
        dur[:, :, :k] += np.moveaxis(pow2(x, F), 1, 2).astype(F64)
    return trans, first, dur, Z


def per_stream(probs, state_class, trans, dur, init=None, dur_open=None, lengths=None, F=F64):
    """(trans [B,S,S], start_counts [B,S], dur [B,S,D], Z [B], frames [B]) of every stream"""
    probs = np.asarray(probs, F32)
    B, frames, C = probs.shape
    S = len(state_class)
    T, Dur, DurOpen, start = tables(S, trans, dur, init, dur_open)
    tc, st, dc, ev = np.zeros((B, S, S)), np.zeros((B, S)), np.zeros((B,) + Dur.shape), np.zeros(B)
    n_of = np.array([stream_length(lengths, b, frames) for b in range(B)])
    for n in sorted(set(n_of.tolist())):
        bs = [b for b in range(B) if n_of[b] == n]
        e = np.stack([emissions(probs[b, :n], state_class) for b in bs]).astype(np.int64)
        tc[bs], st[bs], dc[bs], ev[bs] = sweep(e, T, Dur, DurOpen, start, F)
    return tc, st, dc, ev, n_of


def loops(probs, state_class, trans, dur, init=None, dur_open=None, lengths=None, F=F64):
    tc, st, dc, ev, n_of = per_stream(probs, state_class, trans, dur, init, dur_open, lengths, F)
    out = [np.zeros(a.shape[1:]) for a in (tc, st, dc)]
    bits, frames = F64(0), 0
    for b in range(len(ev)):                                                         # ascending stream, from zero
        for acc, a in zip(out, (tc, st, dc)):
            acc += a[b]
        bits, frames = bits + ev[b], frames + int(n_of[b])
    return out[0], out[1], out[2], np.array([bits, float(frames)], F64)


def loops64(*a, **k):
    return loops(*a, **k, F=F64)


def loops_mixed(*a, **k):
    return loops(*a, **k, F=F32)


def brute(probs, state_class, trans, dur, init=None, dur_open=None):
    """one stream [n, C]: _pose_duration_posterior_ref.brute's loop over every segmentation, with the transitions between
    its segments and the start state weighed too.  Returns (trans_counts [S,S], start_counts [S], dur_counts [S,D], evidence in
    bits)"""
    probs = np.asarray(probs, F32)
    n, S = probs.shape[0], len(state_class)
    T, Dur, DurOpen, start = tables(S, trans, dur, init, dur_open)
    D = Dur.shape[1]
    E = emissions(probs, state_class) / 256.0

    def compositions(left):
        if left == 0:
            yield ()
        for d in range(1, min(D, left) + 1):
            for rest in compositions(left - d):
                yield (d,) + rest

    tc, st, dc, total = np.zeros((S, S)), np.zeros(S), np.zeros((S, D)), 0.0
    for lens in compositions(n):
        bounds = np.concatenate([[0], np.cumsum(lens)])
        for states in itertools.product(range(S), repeat=len(lens)):
            w = 0.0
            for k, (j, d) in enumerate(zip(states, lens)):
                a, z = bounds[k], bounds[k + 1]
                w += (DurOpen if a == 0 or z == n else Dur)[j, d - 1] + E[a:z, j].sum()
                if k:
                    w += T[states[k - 1], j]
            for i in range(S):                                                       # the virtual step out of `start`
                wi = np.exp2(w + start[i] + T[i, states[0]])
                total += wi
                st[i] += wi
                for k, (j, d) in enumerate(zip(states, lens)):
                    if k:
                        tc[states[k - 1], j] += wi
                    if bounds[k] > 0 and bounds[k + 1] < n:
                        dc[j, d - 1] += wi
    return tc / total, st / total, dc / total, float(np.log2(total))


def boundaries(path, start, n):
    """the frames 1 .. n - 1 at which a segment begins"""
    if start is None:
        return [f for f in range(1, n) if path[f] != path[f - 1]]
    return [f for f in range(1, n) if start[f] == f]


def count_paths(path, S, D, start=None, lengths=None):
    """path int64 [B, n], start int64 [B, n] or None: the header's hard counts by a walk, integers in float64"""
    path = np.asarray(path, np.int64)
    B, frames = path.shape
    tc, st, dc, total = np.zeros((S, S)), np.zeros(S), np.zeros((S, D)), 0
    for b in range(B):
        n = stream_length(lengths, b, frames)
        p = path[b]
        cuts = boundaries(p, None if start is None else np.asarray(start)[b], n)
        for f in cuts:
            if 0 <= p[f - 1] < S and 0 <= p[f] < S:
                tc[p[f - 1], p[f]] += 1
        for s, e in zip(cuts[:-1], cuts[1:]):                                        # s > 0 and e < n
            if 0 <= p[s] < S:
                dc[p[s], min(e - s, D) - 1] += 1
        if 0 <= p[0] < S:
            st[p[0]] += 1
        total += n
    return tc, st, dc, np.array([0.0, float(total)], F64)


def dur_rows(dur_counts, dur, dur_allowed=None, dur_pseudo_count=1.0):
    """the M-step of dur: int64 [S, D]"""
    dur = np.asarray(dur, np.int64)
    allowed = dur > TRANS_FLOOR if dur_allowed is None else np.asarray(dur_allowed, bool)
    out = np.array(dur)
    for j in range(dur.shape[0]):
        r = np.where(allowed[j], np.asarray(dur_counts, F64)[j] + dur_pseudo_count, 0.0)
        R = F64(0)
        for v in r:                                                                  # ascending
            R = R + v
        if R > 0:
            out[j] = np.where(allowed[j], q_array((r / R).astype(F32)), TRANS_FLOOR)
    return out


def suffix_max(dur):
    dur = np.asarray(dur)
    return np.maximum.accumulate(dur[:, ::-1], axis=1)[:, ::-1].copy()


def m_step(trans_counts, start_counts, dur_counts, trans, init, dur, allowed=None, dur_allowed=None, pseudo_count=0.0,
           dur_pseudo_count=1.0, learn_init=False):
    """(trans int64 [S,S], init int64 [S] or None, dur int64 [S,D], near [S,S] bool, near_init [S] bool): trans and init by
    _pose_prior_ref.m_step (the entries within 1e-6 of a rounding boundary marked), dur by dur_rows"""
    new, new_init, near, near_init = PR.m_step(trans_counts, start_counts, trans, init, allowed, pseudo_count, learn_init)
    return new, new_init, dur_rows(dur_counts, dur, dur_allowed, dur_pseudo_count), near, near_init


def fit(videos, state_class, trans, dur, init=None, dur_open="suffix_max", iterations=1, pseudo_count=0.0, dur_pseudo_count=1.0,
        learn_init=False, F=F64, final=True):
    """EM on the host.  videos: a list of (probs, lengths or None).  dur_open: "suffix_max" (rewritten after every M-step), a
    table or None (kept).  Returns (trans, init, dur, dur_open, [(evidence, frames) of every E-step]); with `final` one more
    E-step after the last update, so that the history has iterations + 1 entries."""
    trans, dur = np.asarray(trans, np.int64), np.asarray(dur, np.int64)
    allowed, dur_allowed = trans > TRANS_FLOOR, dur > TRANS_FLOOR
    learn_open = isinstance(dur_open, str)
    open_ = suffix_max(dur) if learn_open else dur_open
    history = []
    for it in range(iterations + bool(final)):
        S, D = dur.shape
        acc = [np.zeros((S, S)), np.zeros(S), np.zeros((S, D)), np.zeros(2)]
        for probs, lengths in videos:
            for a, c in zip(acc, loops(probs, state_class, trans, dur, init, open_, lengths, F=F)):
                a += c
        history.append((float(acc[3][0]), int(acc[3][1])))
        if it == iterations:
            break
        trans, init, dur, _, _ = m_step(acc[0], acc[1], acc[2], trans, init, dur, allowed, dur_allowed, pseudo_count,
                                        dur_pseudo_count, learn_init)
        if learn_open:
            open_ = suffix_max(dur)
    return trans, init, dur, open_, history
