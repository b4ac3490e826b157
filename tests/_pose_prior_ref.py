"""The pose-order learner (include/qtcnn.h, qt_pose_prior_expect / _count_paths / _update) on the host.  `loops64` is the
E-step's rule in float64: the forward rows and the b rows of tests/_pose_posterior_ref.py, the pairwise posteriors xi of every
frame from them, summed into an f32-or-F partial per (sequence, tile of TILE frames) in the backward sweep's order, the tiles
then the sequences added in ascending order in float64.  `loops32` is the same loops in numpy f32 with the same float64
accumulators: the yardstick that the kernel's own f32 rounding is held against.  `tiled` restates the parallel form (the
posterior's tile products and scan, a sweep per tile from the tile's start a and end b) with the tile size as a parameter,
`brute_force` weighs every path, `m_step` and `count_paths` are the other two entry points.  Every function returns what ONE
call adds: (counts float64 [S, S], start_counts float64 [S], totals float64 [2] = (evidence in bits, frames))."""
import itertools

import numpy as np

import _pose_posterior_ref as P
from _pose_order_ref import TRANS_FLOOR, clamp_trans

F32, F64 = np.float32, np.float64
TILE = P.TILE


def xi_of(x, F):
    """x [..., S, S] -> 2^(x - Z) with Z = L over (i, j): the maximum out, the sum over i ascending and inside it j ascending (a
    cumulative sum of the flattened array adds in exactly that order, in F)"""
    S = x.shape[-1]
    m = x.max(axis=(-2, -1))
    p = np.exp2(x - m[..., None, None]).astype(F)
    s = np.cumsum(p.reshape(p.shape[:-2] + (S * S,)), axis=-1, dtype=F)[..., -1]
    Z = (m + np.log2(s).astype(F)).astype(F)
    return np.exp2(x - Z[..., None, None]).astype(F)


def sweep(E, T, rows, a0, b_last, f0, tile, partials, F):
    """the backward sweep over the frames f0 .. f0 + n - 1 whose emissions are E [..., n, S] and whose a_f are `rows`; a0
    [..., S]: a in front of the first of them, b_last: b at the last.  xi of every frame but a video's frame 0 goes onto
    partials[frame // tile] ([..., S, S] in F, made on demand); returns the start counts [..., S] in F where f0 == 0."""
    n, S = E.shape[-2], E.shape[-1]
    b, start = b_last, None
    for f in range(n - 1, -1, -1):
        if f < n - 1:
            b = P.b_step(E[..., f + 1, :], T, b, F)
        g = E[..., f, :] + b
        ap = rows[..., f - 1, :] if f > 0 else a0
        x = ((ap[..., :, None] + T) + g[..., None, :]).astype(F)
        xi = xi_of(x, F)
        if f0 + f == 0:
            start = np.zeros(xi.shape[:-1], F)
            for j in range(S):                                  # ascending j
                start = (start + xi[..., j]).astype(F)
        else:
            t = (f0 + f) // tile
            partials[t] = (partials.get(t, np.zeros(xi.shape, F)) + xi).astype(F)
    return start


def _finish(per_stream, start, evidence, n):
    """per_stream: a list over the sequences of {tile: partial}; tiles ascending, then sequences ascending, in float64"""
    S = start.shape[-1]
    counts, start_counts, bits = np.zeros((S, S), F64), np.zeros(S, F64), F64(0)
    for b, partials in enumerate(per_stream):
        sb = np.zeros((S, S), F64)
        for t in sorted(partials):
            sb += partials[t].astype(F64)
        counts += sb
        start_counts += start[b].astype(F64)
        bits += evidence[b]
    return counts, start_counts, np.array([bits, float(len(per_stream) * n)], F64)


def loops(probs, state_class, trans, init=None, F=F64, tile=TILE):
    probs, B, n, C, S, T, start, _ = P._setup(probs, state_class, trans, init, None, F)
    E = np.stack([P.scores(probs[b], state_class, F) for b in range(B)])
    first = np.broadcast_to(start, (B, S)).astype(F)
    rows, c = P.forward(E, T, first, F)
    evidence = np.zeros(B, F64)
    for f in range(n):
        evidence += c[:, f]
    partials = {}
    begin = sweep(E, T, rows, first, np.zeros((B, S), F), 0, tile, partials, F)
    return _finish([{t: p[b] for t, p in partials.items()} for b in range(B)], begin, evidence, n)


def loops64(*a, **k):
    return loops(*a, **k, F=F64)


def loops32(*a, **k):
    return loops(*a, **k, F=F32)


def tiled(probs, state_class, trans, init=None, tile=TILE, F=F64):
    """the tiled route: steps (a) and (b) of _pose_posterior_ref.tiled (row-normalised tile products, the start vector forward
    and the end vector backward through them), then every tile forward from its start and swept backward from its end"""
    probs, B, n, C, S, T, start, _ = P._setup(probs, state_class, trans, init, None, F)
    tiles = [(a, min(a + tile, n)) for a in range(0, n, tile)]
    per_stream, begin, evidence = [], np.zeros((B, S), F), np.zeros(B, F64)
    for b in range(B):
        E = P.scores(probs[b], state_class, F)
        products, offsets = [], []
        for a, z in tiles:                                      # (a)
            Q, off = T + E[a][None, :], np.zeros(S, F64)
            for f in range(a + 1, z):
                r = Q.max(axis=1)
                off += r
                m, lg = P.L((Q - r[:, None])[:, :, None] + T[None, :, :], 1, F)
                Q = E[f][None, :] + (m + lg)
            r = Q.max(axis=1)
            products.append(Q - r[:, None])
            offsets.append(off + r)
        v = start
        starts, before, ev = [v], [F64(0)], F64(0)              # (b), forward
        for t in range(len(tiles) - 1):
            w = v.astype(F64) + offsets[t]
            W = w.max()
            m, lg = P.L((w - W).astype(F)[:, None] + products[t], 0, F)
            mA, lgA = P.L(m + lg, 0, F)
            v = ((m + lg) - mA) - lgA
            ev = ev + (W + (F64(mA) + F64(lgA)))
            starts.append(v)
            before.append(ev)
        ends, bv = [None] * len(tiles), np.zeros(S, F)          # (b), backward
        ends[-1] = bv
        for t in range(len(tiles) - 1, 0, -1):
            m, lg = P.L(products[t] + bv[None, :], 1, F)
            Bd = offsets[t] + (m + lg).astype(F64)
            bv = (Bd - Bd.max()).astype(F)
            ends[t - 1] = bv
        partials = {}
        for t, (a, z) in enumerate(tiles):
            rows, c = P.forward(E[a:z], T, starts[t], F)
            got = sweep(E[a:z], T, rows, starts[t], ends[t], a, tile, partials, F)
            if a == 0:
                begin[b] = got
        call = before[-1]
        for v_c in c:
            call += v_c
        evidence[b] = call
        per_stream.append(partials)
    return _finish(per_stream, begin, evidence, n)


def brute_force(probs, state_class, trans, init=None):
    """one sequence [n, C]: every start state and every one of the S^n paths weighed in float64: (counts, start_counts,
    evidence in bits)"""
    probs = np.asarray(probs, F32)
    n, S = probs.shape[0], len(state_class)
    T = clamp_trans(trans).reshape(S, S) / 256.0
    start = np.zeros(S) if init is None else clamp_trans(init) / 256.0
    E = P.scores(probs, state_class, F64)
    counts, start_counts, mass = np.zeros((S, S)), np.zeros(S), 0.0
    for i in range(S):
        for path in itertools.product(range(S), repeat=n):
            w = start[i] + T[i, path[0]] + E[0, path[0]]
            for f in range(1, n):
                w += T[path[f - 1], path[f]] + E[f, path[f]]
            w = np.exp2(w)
            mass += w
            start_counts[i] += w
            for f in range(1, n):
                counts[path[f - 1], path[f]] += w
    return counts / mass, start_counts / mass, np.log2(mass)


def m_row(r, old):
    """(the new row, which entries lie within 1e-6 of a rounding boundary)"""
    r = np.asarray(r, F64)
    R = F64(0)
    for v in r:                                                 # ascending
        R = R + v
    if not R > 0:
        return np.array(old, np.int64), np.zeros(len(r), bool)
    out, near = np.full(len(r), TRANS_FLOOR, np.int64), np.zeros(len(r), bool)
    for j, v in enumerate(r):
        if v > 0:
            y = 256.0 * np.log2(v / R)
            out[j] = int(min(max(np.rint(y), TRANS_FLOOR), 0))
            near[j] = abs((y - np.floor(y)) - 0.5) <= 1e-6 and TRANS_FLOOR < y < 0
    return out, near


def m_step(counts, start_counts, trans, init=None, allowed=None, pseudo_count=0.0, learn_init=False):
    """(trans int64 [S, S], init int64 [S] or None, near [S, S] bool, near_init [S] bool).  allowed: None for `trans > -65536`."""
    trans = np.asarray(trans, np.int64)
    S = trans.shape[0]
    allowed = trans > TRANS_FLOOR if allowed is None else np.asarray(allowed, bool)
    new, near = np.empty((S, S), np.int64), np.zeros((S, S), bool)
    for i in range(S):
        r = np.where(allowed[i], np.asarray(counts, F64)[i] + pseudo_count, 0.0)
        new[i], near[i] = m_row(r, trans[i])
    if not learn_init:
        return new, (None if init is None else np.asarray(init, np.int64)), near, np.zeros(S, bool)
    old = np.zeros(S, np.int64) if init is None else np.asarray(init, np.int64)
    new_init, near_init = m_row(np.asarray(start_counts, F64) + pseudo_count, old)
    return new, new_init, near, near_init


def count_paths(path, S):
    """path int64 [B, n]: a transition with an end outside [0, S) is left out, and so is a start outside it"""
    path = np.asarray(path, np.int64)
    B, n = path.shape
    counts, start_counts = np.zeros((S, S), F64), np.zeros(S, F64)
    for b in range(B):
        if 0 <= path[b, 0] < S:
            start_counts[path[b, 0]] += 1
        for f in range(1, n):
            i, j = path[b, f - 1], path[b, f]
            if 0 <= i < S and 0 <= j < S:
                counts[i, j] += 1
    return counts, start_counts, np.array([0.0, float(B * n)], F64)


def fit(videos, state_class, trans, init=None, iterations=1, pseudo_count=0.0, learn_init=False, F=F64):
    """EM on the host: (trans, init, [(evidence, frames) of every E-step])"""
    allowed = np.asarray(trans, np.int64) > TRANS_FLOOR
    trans, history = np.asarray(trans, np.int64), []
    for _ in range(iterations):
        S = trans.shape[0]
        counts, start_counts, totals = np.zeros((S, S)), np.zeros(S), np.zeros(2)
        for probs in videos:
            c, s, t = loops(probs, state_class, trans, init, F=F)
            counts, start_counts, totals = counts + c, start_counts + s, totals + t
        history.append((float(totals[0]), int(totals[1])))
        trans, init, _, _ = m_step(counts, start_counts, trans, init, allowed, pseudo_count, learn_init)
    return trans, init, history
