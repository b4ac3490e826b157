"""The pose-order decode (include/qtcnn.h, qt_pose_order_decode) as plain loops: Python and np.int64 integers, one frame after
the other, nothing vectorised across frames (inside a frame the S x S candidates are one integer array).  Everything is an
integer from the emission score on, so every output of the kernels is compared with these for equality.  `tiled` restates
the parallel form of csrc/pose_order.hip (tile products, scan, replay, back-maps) in the same integers; tests/
test_pose_order_cpu.py holds it equal to the loops.  The reference project has no such step, so there is no fixture of it."""
import numpy as np

TILE, MAX_STATES, MAX_CLASSES = 64, 64, 64       # csrc/pose_order.hip, include/qtcnn.h
GROUP = 32                                       # tiles per group of the scan's two levels
MAX_FRAMES = 1 << 20
SCORE_FLOOR, TRANS_FLOOR = -8192, -65536
F32 = np.float32

LOG2_TABLE = (
      1,   2,   4,   5,   6,   8,   9,  11,  12,  13,  15,  16,  18,  19,  20,  22,
     23,  24,  26,  27,  28,  30,  31,  32,  34,  35,  36,  38,  39,  40,  42,  43,
     44,  45,  47,  48,  49,  50,  52,  53,  54,  55,  57,  58,  59,  60,  62,  63,
     64,  65,  66,  68,  69,  70,  71,  72,  74,  75,  76,  77,  78,  80,  81,  82,
     83,  84,  85,  86,  88,  89,  90,  91,  92,  93,  94,  95,  97,  98,  99, 100,
    101, 102, 103, 104, 105, 106, 108, 109, 110, 111, 112, 113, 114, 115, 116, 117,
    118, 119, 120, 121, 122, 123, 124, 125, 126, 127, 128, 129, 131, 132, 133, 134,
    135, 136, 137, 138, 139, 140, 140, 141, 142, 143, 144, 145, 146, 147, 148, 149,
    150, 151, 152, 153, 154, 155, 156, 157, 158, 159, 160, 161, 162, 163, 163, 164,
    165, 166, 167, 168, 169, 170, 171, 172, 173, 173, 174, 175, 176, 177, 178, 179,
    180, 181, 182, 182, 183, 184, 185, 186, 187, 188, 189, 189, 190, 191, 192, 193,
    194, 195, 195, 196, 197, 198, 199, 200, 200, 201, 202, 203, 204, 205, 205, 206,
    207, 208, 209, 210, 210, 211, 212, 213, 214, 214, 215, 216, 217, 218, 218, 219,
    220, 221, 222, 222, 223, 224, 225, 226, 226, 227, 228, 229, 229, 230, 231, 232,
    233, 233, 234, 235, 236, 236, 237, 238, 239, 239, 240, 241, 242, 242, 243, 244,
    245, 245, 246, 247, 248, 248, 249, 250, 251, 251, 252, 253, 253, 254, 255, 256)
_TABLE = np.array(LOG2_TABLE, np.int64)
_P_MIN_BITS = (127 - 32) << 23        # 2^-32
_ONE_BITS = 127 << 23


def bits(a):
    """the bytes of an array: the only comparison used"""
    return np.ascontiguousarray(a).tobytes()


def q(p):
    """the emission score of one f32, from its bit pattern"""
    b = int(np.array([p], F32).view(np.uint32)[0])
    if b >> 31:                                   # negative numbers, -0.0, -inf, NaNs with the sign set
        return SCORE_FLOOR
    if b > 0x7F800000 or b < _P_MIN_BITS:         # NaN; zero, denormals and everything below 2^-32
        return SCORE_FLOOR
    if b >= _ONE_BITS:                            # 1.0 and above, +inf
        return 0
    return 256 * ((b >> 23) - 127) + LOG2_TABLE[(b >> 15) & 255]


def q_array(p):
    """q over an array (the same case distinction on the bit patterns; elementwise, so no frame sees another)"""
    b = np.ascontiguousarray(p, F32).view(np.uint32).astype(np.int64)
    out = 256 * ((b >> 23) - 127) + _TABLE[(b >> 15) & 255]
    out = np.where(b >= _ONE_BITS, 0, out)
    out = np.where((b >> 31 != 0) | (b > 0x7F800000) | (b < _P_MIN_BITS), SCORE_FLOOR, out)
    return out.astype(np.int64)


def clamp_trans(a):
    return np.clip(np.asarray(a, np.int64), TRANS_FLOOR, 0)


def emissions(probs, state_class):
    """probs f32 [T, C] -> int64 [T, S]; a state whose class is outside [0, C) gets the floor"""
    T, C = probs.shape
    e = np.full((T, len(state_class)), SCORE_FLOOR, np.int64)
    for s, k in enumerate(state_class):
        if 0 <= int(k) < C:
            e[:, s] = q_array(probs[:, int(k)])
    return e


def decode(probs, state_class, trans, init=None, carry=None):
    """probs f32 [B,T,C]; state_class [S]; trans [S,S]; init [S] or None; carry int64 [B,S+2] as before the call (None: zeros;
    not written).  Returns (path int64 [B,T], filtered int64 [B,T], emissions int32 [B,T,S], carry int64 [B,S+2])."""
    probs = np.asarray(probs, F32)
    B, T, C = probs.shape
    S = len(state_class)
    trans = clamp_trans(trans).reshape(S, S)
    init = np.zeros(S, np.int64) if init is None else clamp_trans(init)
    carry = np.zeros((B, S + 2), np.int64) if carry is None else np.array(carry, np.int64)
    path, filtered = np.empty((B, T), np.int64), np.empty((B, T), np.int64)
    em = np.empty((B, T, S), np.int32)
    for b in range(B):
        e = emissions(probs[b], state_class)
        em[b] = e
        d = init.copy() if carry[b, 0] == 0 else carry[b, 2:].copy()
        psi = np.empty((T, S), np.int64)
        for f in range(T):
            cand = d[:, None] + trans                      # [i, j]
            psi[f] = np.argmax(cand, axis=0)               # the lowest i that attains the maximum
            d = cand[psi[f], np.arange(S)] + e[f]
            filtered[b, f] = int(np.argmax(d))             # the lowest j
        s = int(filtered[b, T - 1])
        for f in range(T - 1, -1, -1):
            path[b, f] = s
            s = int(psi[f, s])
        m = int(d.max())
        carry[b, 0] += T
        carry[b, 1] += m
        carry[b, 2:] = d - m
    return path, filtered, em, carry


def decode_split(probs, state_class, trans, init, cuts, carry=None):
    """consecutive calls cut at `cuts`: (paths of the calls joined, filtered, emissions, last carry, the last call's path)"""
    T = probs.shape[1]
    parts = []
    for a, b in zip([0] + list(cuts), list(cuts) + [T]):
        p, f, e, carry = decode(probs[:, a:b], state_class, trans, init, carry)
        parts.append((p, f, e))
    joined = [np.concatenate([x[i] for x in parts], axis=1) for i in range(3)]
    return joined[0], joined[1], joined[2], carry, parts[-1][0]


def scan_trip_tiles(S):
    """products that step (b) of the tiled route stages at a time: 16 KB of LDS, at most 16"""
    return max(1, min(16, 4096 // (S * S)))


def _times(P, Q):
    """(max, +) product of two S x S matrices"""
    return (P[:, :, None] + Q[None, :, :]).max(axis=1)


def tiled(probs, state_class, trans, init=None, carry=None, tile=TILE, group=GROUP):
    """the tiled route in integers: (a) a tile's product of the matrices M_f[i][j] = trans[i][j] + e[f][j] in the (max, +)
    semiring, (b) the start vector carried through the products, on two levels: through the products of whole groups of `group`
    tiles first, then inside every group from the group's start, (c) a replay of every tile from its start vector with the
    vector step (psi, filtered) and the tile's back-map, (d) end states from the last tile backwards, then every tile's own
    backtrace.  One stream per call of the inner loop; same returns as decode."""
    probs = np.asarray(probs, F32)
    B, T, C = probs.shape
    S = len(state_class)
    trans = clamp_trans(trans).reshape(S, S)
    init = np.zeros(S, np.int64) if init is None else clamp_trans(init)
    carry = np.zeros((B, S + 2), np.int64) if carry is None else np.array(carry, np.int64)
    path, filtered = np.empty((B, T), np.int64), np.empty((B, T), np.int64)
    em = np.empty((B, T, S), np.int32)
    tiles = [(a, min(a + tile, T)) for a in range(0, T, tile)]
    for b in range(B):
        e = emissions(probs[b], state_class)
        em[b] = e
        products = []
        for a, z in tiles[:-1]:                                            # (a): the last tile's product is never needed
            P = trans + e[a][None, :]
            for f in range(a + 1, z):
                P = (P[:, :, None] + trans[None, :, :]).max(axis=1) + e[f][None, :]
            products.append(P)
        groups = -(-len(tiles) // group)                                   # (b)
        gstarts = [init.copy() if carry[b, 0] == 0 else carry[b, 2:].copy()]
        for g in range(groups - 1):                                        # the last group's product is never needed
            Q = products[g * group]
            for P in products[g * group + 1:(g + 1) * group]:
                Q = _times(Q, P)
            gstarts.append((gstarts[-1][:, None] + Q).max(axis=0))
        starts = []
        for g in range(groups):
            starts.append(gstarts[g])
            for u in range(min(group, len(tiles) - g * group) - 1):
                starts.append((starts[-1][:, None] + products[g * group + u]).max(axis=0))
        psis, back, d = [], [], None
        for (a, z), d0 in zip(tiles, starts):                              # (c)
            mx = int(d0.max())
            d = d0 - mx                                                    # the kernel's range: a constant changes no argmax
            psi = np.empty((z - a, S), np.int64)
            for f in range(a, z):
                cand = d[:, None] + trans
                psi[f - a] = np.argmax(cand, axis=0)
                d = cand[psi[f - a], np.arange(S)] + e[f]
                filtered[b, f] = int(np.argmax(d))
            bm = np.arange(S)
            for f in range(z - a - 1, -1, -1):
                bm = psi[f][bm]
            psis.append(psi)
            back.append(bm)
            d = d + mx
        ends = [0] * len(tiles)                                            # (d)
        ends[-1] = int(filtered[b, T - 1])
        for t in range(len(tiles) - 1, 0, -1):
            ends[t - 1] = int(back[t][ends[t]])
        for (a, z), psi, s in zip(tiles, psis, ends):
            for f in range(z - 1, a - 1, -1):
                path[b, f] = s
                s = int(psi[f - a][s])
        m = int(d.max())
        carry[b, 0] += T
        carry[b, 1] += m
        carry[b, 2:] = d - m
    return path, filtered, em, carry


def decode_float64(probs, state_class, trans, init=None):
    """Viterbi in float64 with 256 log2 p in place of q: one stream [T, C] from its first frame; returns the path"""
    probs = np.asarray(probs, np.float64)
    T = probs.shape[0]
    S = len(state_class)
    trans = np.asarray(trans, np.float64).reshape(S, S)
    with np.errstate(divide="ignore"):
        e = 256.0 * np.log2(probs[:, np.asarray(state_class)])
    d = np.zeros(S) if init is None else np.asarray(init, np.float64)
    psi = np.empty((T, S), np.int64)
    for f in range(T):
        cand = d[:, None] + trans
        psi[f] = np.argmax(cand, axis=0)
        d = cand[psi[f], np.arange(S)] + e[f]
    path = np.empty(T, np.int64)
    s = int(np.argmax(d))
    for f in range(T - 1, -1, -1):
        path[f] = s
        s = int(psi[f, s])
    return path


def cycles(path, wrap_from, wrap_to, last=None):
    """path int64 [B,T]; last: the previous call's last state per stream, or None (-1: none).  Returns (counts int64 [B], the
    new last states)."""
    B, T = path.shape
    counts = np.zeros(B, np.int64)
    last = np.full(B, -1, np.int64) if last is None else np.array(last, np.int64)
    for b in range(B):
        prev = int(last[b])
        for f in range(T):
            s = int(path[b, f])
            if prev == wrap_from and s == wrap_to:
                counts[b] += 1
            prev = s
        last[b] = prev
    return counts, last


def cyclic_prior(step_classes, stay, advance, skip=None, other=TRANS_FLOOR, wrap=True):
    """(state_class int32 [S], trans int32 [S,S]) of a left-to-right cycle; later assignments win where S is small"""
    S = len(step_classes)
    trans = [[other] * S for _ in range(S)]
    for s in range(S):
        for step, value in ((2, skip), (1, advance), (0, stay)):
            if value is None:
                continue
            j = s + step
            if j >= S:
                if not wrap:
                    continue
                j %= S
            trans[s][j] = value
    return np.array(step_classes, np.int32), np.array(trans, np.int32)


def make_probs(seed, batch, frames, C, run=9):
    """f32 rows that sum to about one; the dominant class walks 0, 1, 2, ... every `run` frames or so, with some frames off"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((batch, frames, C)).astype(F32)
    lead = (np.arange(frames)[None, :] // run + rng.integers(0, C, (batch, 1))) % C
    off = rng.random((batch, frames)) < 0.1
    lead = np.where(off, rng.integers(0, C, (batch, frames)), lead)
    np.put_along_axis(z, lead[..., None], z.max(axis=2, keepdims=True) + F32(1.0), axis=2)
    ex = np.exp(z - z.max(axis=2, keepdims=True))
    return (ex / ex.sum(axis=2, keepdims=True)).astype(F32)
