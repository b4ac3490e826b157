"""The pose-order posteriors (include/qtcnn.h, qt_pose_posterior) on the host: forward-backward in log2 over the decoder's
integer emissions, one frame after the other.  `loops64` is the rule in float64, `loops32` the same loops in numpy f32 (np.exp2,
np.log2, every maximum taken out, every sum in ascending order): the yardstick that a kernel's own f32 rounding is held
against.  Inside a frame the S x S candidates of every stream are one array, but every sum over states is a loop in ascending
state, so an element sees the additions of the rule in the rule's order.  `tiled` restates the parallel form of
csrc/pose_posterior.hip (row-normalised tile products in the (L, +) semiring, the scan in both directions, the replay) with the
tile size as a parameter; tests/test_pose_posterior_cpu.py holds it against the loops.  The reference project has no such
step."""
import numpy as np

from _pose_order_ref import clamp_trans, q_array

F32, F64 = np.float32, np.float64
TILE = 64


def scores(probs, state_class, F):
    """probs f32 [T, C] -> E [T, S] = q / 256 (exact in f32); a state whose class is outside [0, C) gets the floor"""
    T, C = probs.shape
    e = np.full((T, len(state_class)), -8192, np.int64)
    for s, k in enumerate(state_class):
        if 0 <= int(k) < C:
            e[:, s] = q_array(probs[:, int(k)])
    return (e / 256.0).astype(F)


def L(x, axis, F):
    """L over one axis: (m, lg) with m the maximum and lg = log2 of the sum, in ascending index, of 2^(x - m)"""
    x = np.moveaxis(x, axis, 0)
    m = x.max(axis=0)
    s = np.zeros_like(m)
    for k in range(x.shape[0]):
        s = (s + np.exp2(x[k] - m)).astype(F)
    return m, np.log2(s).astype(F)


def forward(E, T, a_prev, F):
    """frames of E [..., n, S] from a_prev [..., S] (leading axes: streams, which never meet): (the a_f rows [..., n, S], c_f as
    float64 [..., n])"""
    n = E.shape[-2]
    rows, c = np.empty(E.shape, F), np.empty(E.shape[:-1], np.float64)
    for f in range(n):
        m, lg = L(a_prev[..., :, None] + T, -2, F)              # x[i][j] = a_prev[i] + T[i][j], L over i
        A = E[..., f, :] + (m + lg)
        mA, lgA = L(A, -1, F)
        a_prev = (A - mA[..., None]) - lgA[..., None]
        rows[..., f, :], c[..., f] = a_prev, mA.astype(np.float64) + lgA.astype(np.float64)
    return rows, c


def b_step(E_next, T, b_next, F):
    """b of a frame from the next frame's: L_j (T[i][j] + (E[f + 1][j] + b[f + 1][j])), less its maximum"""
    g = E_next + b_next
    m, lg = L(T + g[..., None, :], -1, F)
    B = m + lg
    return B - B.max(axis=-1, keepdims=True)


def backward(E, T, rows, b_last, call_end, F):
    """posterior rows [..., n, S] of the frames whose a_f are `rows`; b_last [..., S]: b at the last of them; call_end: that frame
    is the call's last, where the posterior is the filtered row itself"""
    n = E.shape[-2]
    post, b = np.empty(E.shape, F), b_last
    for f in range(n - 1, -1, -1):
        if f < n - 1:
            b = b_step(E[..., f + 1, :], T, b, F)
        if call_end and f == n - 1:
            post[..., f, :] = np.exp2(rows[..., f, :])
        else:
            u = rows[..., f, :] + b
            m, lg = L(u, -1, F)
            post[..., f, :] = np.exp2((u - m[..., None]) - lg[..., None])
    return post


def by_class(post, state_class, C, F):
    out = np.zeros(post.shape[:-1] + (C,), F)
    for j, k in enumerate(state_class):                         # ascending j
        if 0 <= int(k) < C:
            out[..., int(k)] = (out[..., int(k)] + post[..., j]).astype(F)
    return out


def _setup(probs, state_class, trans, init, carry, F):
    probs = np.asarray(probs, F32)
    B, n, C = probs.shape
    S = len(state_class)
    T = (clamp_trans(trans).reshape(S, S) / 256.0).astype(F)
    start = np.zeros(S, F) if init is None else (clamp_trans(init) / 256.0).astype(F)
    carry = np.zeros((B, S + 2), F64) if carry is None else np.array(carry, F64)
    return probs, B, n, C, S, T, start, carry


def loops(probs, state_class, trans, init=None, carry=None, F=F64):
    """probs f32 [B,n,C]; carry float64 [B,S+2] as before the call (None: zeros; not written).  Returns (posterior [B,n,S],
    filtered [B,n,S], class_posterior [B,n,C], log2_evidence float64 [B], carry float64 [B,S+2]), the first three in F."""
    probs, B, n, C, S, T, start, carry = _setup(probs, state_class, trans, init, carry, F)
    E = np.stack([scores(probs[b], state_class, F) for b in range(B)])
    first = np.where(carry[:, :1] == 0, start[None, :], carry[:, 2:].astype(F)).astype(F)
    rows, c = forward(E, T, first, F)
    filt = np.exp2(rows)
    post = backward(E, T, rows, np.zeros((B, S), F), True, F)
    evidence = np.zeros(B, F64)
    for f in range(n):                                          # one addition per frame, onto the running total
        carry[:, 1] += c[:, f]
        evidence += c[:, f]
    carry[:, 0] += n
    carry[:, 2:] = rows[:, -1]
    return post, filt, by_class(post, state_class, C, F), evidence, carry


def loops64(*a, **k):
    return loops(*a, **k, F=F64)


def loops32(*a, **k):
    return loops(*a, **k, F=F32)


def tiled(probs, state_class, trans, init=None, carry=None, tile=TILE, F=F64):
    """the tiled route: (a) every tile's product of M_f[i][j] = T[i][j] + E[f][j] in the (L, +) semiring, row-normalised (row
    maximum 0 after every frame, the shifts summed per row in float64), (b) the start vector forward through the products of
    tiles 0 .. tiles - 2 and the end vector backward through those of tiles tiles - 1 .. 1, offsets added in float64 and the
    maximum out before going back to F, (c) every tile replayed from its start and swept backward from its end.  Same returns as
    loops."""
    probs, B, n, C, S, T, start, carry = _setup(probs, state_class, trans, init, carry, F)
    post, filt = np.empty((B, n, S), F), np.empty((B, n, S), F)
    evidence = np.zeros(B, F64)
    tiles = [(a, min(a + tile, n)) for a in range(0, n, tile)]
    for b in range(B):
        E = scores(probs[b], state_class, F)
        products, offsets = [], []
        for a, z in tiles:                                      # (a)
            Q, off = T + E[a][None, :], np.zeros(S, F64)
            for f in range(a + 1, z):
                r = Q.max(axis=1)
                off += r
                P = Q - r[:, None]
                m, lg = L(P[:, :, None] + T[None, :, :], 1, F)           # L over k of P[i][k] + T[k][j]
                Q = E[f][None, :] + (m + lg)
            r = Q.max(axis=1)
            products.append(Q - r[:, None])
            offsets.append(off + r)
        v = start if carry[b, 0] == 0 else carry[b, 2:].astype(F)
        starts, before, ev = [v], [F64(0)], F64(0)              # (b), forward
        for t in range(len(tiles) - 1):
            w = v.astype(F64) + offsets[t]
            W = w.max()
            wf = (w - W).astype(F)
            m, lg = L(wf[:, None] + products[t], 0, F)
            A = m + lg
            mA, lgA = L(A, 0, F)
            v = (A - mA) - lgA
            ev = ev + (W + (F64(mA) + F64(lgA)))
            starts.append(v)
            before.append(ev)
        ends, bv = [None] * len(tiles), np.zeros(S, F)          # (b), backward
        ends[-1] = bv
        for t in range(len(tiles) - 1, 0, -1):
            m, lg = L(products[t] + bv[None, :], 1, F)
            Bd = offsets[t] + (m + lg).astype(F64)
            bv = (Bd - Bd.max()).astype(F)
            ends[t - 1] = bv
        for t, (a, z) in enumerate(tiles):                      # (c)
            rows, c = forward(E[a:z], T, starts[t], F)
            filt[b, a:z] = np.exp2(rows)
            post[b, a:z] = backward(E[a:z], T, rows, ends[t], t == len(tiles) - 1, F)
        call = before[-1]
        for v_c in c:
            call += v_c
        evidence[b] = call
        carry[b, 0] += n
        carry[b, 1] += call
        carry[b, 2:] = rows[-1]
    return post, filt, by_class(post, state_class, C, F), evidence, carry


def brute_force(probs, state_class, trans, init=None):
    """one stream [n, C] from its first frame, every one of the S^n paths weighed in float64: (posterior [n,S], filtered [n,S],
    log2_evidence)"""
    import itertools
    probs = np.asarray(probs, F32)
    n, S = probs.shape[0], len(state_class)
    T = clamp_trans(trans).reshape(S, S) / 256.0
    start = np.zeros(S) if init is None else clamp_trans(init) / 256.0
    E = scores(probs, state_class, F64)
    post, filt, evidence = np.zeros((n, S)), np.zeros((n, S)), 0.0
    for upto in range(1, n + 1):                                # the paths over the first `upto` frames give filtered[upto - 1]
        mass = np.zeros(S)
        for path in itertools.product(range(S), repeat=upto):
            # a path's weight: every start state i with weight 2^start[i], then the transitions and emissions along it
            w = np.log2(np.sum(np.exp2(start + T[:, path[0]]))) + E[0, path[0]]
            for f in range(1, upto):
                w += T[path[f - 1], path[f]] + E[f, path[f]]
            mass[path[-1]] += np.exp2(w)
            if upto == n:
                for f in range(n):
                    post[f, path[f]] += np.exp2(w)
        filt[upto - 1] = mass / mass.sum()
        if upto == n:
            evidence = np.log2(mass.sum())
    return post / post.sum(axis=1, keepdims=True), filt, evidence
