"""The pose timeline's two rules (include/qtcnn.h, qt_timeline_smooth / qt_timeline_decode) as plain Python loops: np.float32
adds in ascending frame order and one np.float32 division for the mean, integers for everything else.  Sums in a stated order,
one IEEE division and integers leave nothing to a tolerance: every output of the kernels is compared with these for equality
of bits.  `smooth_vectorised` is the same arithmetic in array form (held equal to the loop by tests/test_timeline_cpu.py) for
the GPU tests' larger sizes; the decode loop is cheap enough at every size used.  The reference project has no such step, so
there is no fixture of it."""
import numpy as np

TILE, TRIP, MAX_WINDOW, MAX_CLASSES, STATE = 64, 64, 64, 64, 8      # csrc/timeline.hip, include/qtcnn.h
AHEAD = 4                          # trips the decode kernel loads ahead: its loop's period is AHEAD * TRIP frames per call
MAX_FRAMES = 1 << 22
CONF_ONE = 65536
RUN_MAX = (1 << 31) - 1
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]        # what a NaN mean is stored as
SEEN, STABLE, CAND, RUN, SEG_START, SEG_LEN, SEG_CONF, TOTAL = range(8)
F32 = np.float32


def bits(a):
    """the bytes of an array: the only comparison used"""
    return np.ascontiguousarray(a).tobytes()


def arg_beats(av, ai, bv, bi):
    """loss.hip's total order: a NaN beats every number, then the larger value, then the lower index"""
    an, bn = av != av, bv != bv
    if an != bn:
        return an
    if not an and av != bv:
        return av > bv
    return ai < bi


def argmax(row):
    best = 0
    for k in range(1, len(row)):
        if arg_beats(row[k], k, row[best], best):
            best = k
    return best


def _seen(hist_count, batch, W):
    if hist_count is None:
        return np.zeros(batch, np.int64)
    return np.clip(np.asarray(hist_count, np.int64), 0, W - 1)


def smooth(probs, W, hist=None, hist_count=None):
    """probs f32 [B,T,C]; hist f32 [B,W-1,C] (slot 0 the most recent) with hist_count [B], or None.  Returns smoothed f32
    [B,T,C], pred int64 [B,T], confidence f32 [B,T], hist_out f32 [B,W-1,C], hist_count_out int32 [B]."""
    probs = np.asarray(probs, F32)
    B, T, C = probs.shape
    back = W - 1
    seen = _seen(hist_count, B, W)
    out = np.empty((B, T, C), F32)
    pred = np.empty((B, T), np.int64)
    conf = np.empty((B, T), F32)
    hist_out = np.zeros((B, back, C), F32)
    with np.errstate(all="ignore"):
        for b in range(B):
            row = lambda g: probs[b, g] if g >= 0 else hist[b, -1 - g]
            for f in range(T):
                n = min(W, int(seen[b]) + f + 1)
                for k in range(C):
                    s = F32(row(f - n + 1)[k])
                    for g in range(f - n + 2, f + 1):
                        s = F32(s + F32(row(g)[k]))
                    m = F32(s / F32(n))
                    out[b, f, k] = QNAN if m != m else m
                pred[b, f] = argmax(out[b, f])
                conf[b, f] = out[b, f, pred[b, f]]
            for s in range(min(back, int(seen[b]) + T)):
                hist_out[b, s] = row(T - 1 - s)
    return out, pred, conf, hist_out, np.minimum(back, seen + T).astype(np.int32)


def smooth_vectorised(probs, W, hist=None, hist_count=None):
    """`smooth` with the frames of all streams side by side: the same adds in the same order per element"""
    probs = np.asarray(probs, F32)
    B, T, C = probs.shape
    back = W - 1
    seen = _seen(hist_count, B, W)
    ext = np.zeros((B, back + T, C), F32)                     # row g of a stream at index back + g
    ext[:, back:] = probs
    for b in range(B):
        for s in range(int(seen[b])):
            ext[b, back - 1 - s] = hist[b, s]
    n = np.minimum(W, seen[:, None] + np.arange(T)[None, :] + 1)      # [B,T]
    s = np.zeros((B, T, C), F32)
    with np.errstate(all="ignore"):
        for off in range(back, -1, -1):                       # the oldest row first
            rows = ext[:, back - off:back - off + T]          # row f - off of every frame f
            first, later = (n - 1 == off)[..., None], (n - 1 > off)[..., None]
            s = np.where(first, rows, np.where(later, s + rows, s))
        out = s / n[..., None].astype(F32)
    assert out.dtype == F32
    out[np.isnan(out)] = QNAN
    nan = np.isnan(out)
    pred = np.where(nan.any(axis=2), nan.argmax(axis=2), np.where(nan, -np.inf, out).argmax(axis=2)).astype(np.int64)
    conf = np.take_along_axis(out, pred[..., None], axis=2)[..., 0]
    hist_out = ext[:, ::-1][:, :back].copy()                  # slot s = row T - 1 - s; rows nobody gave are zeros
    return out, pred, conf, hist_out, np.minimum(back, seen + T).astype(np.int32)


def q(x):
    """a confidence in units of 1 / 65536: rint(clamp(x, 0, 1) * 65536), 0 for a NaN"""
    x = F32(x)
    if x != x:
        return 0
    return int(np.rint(F32(min(max(x, F32(0)), F32(1))) * F32(CONF_ONE)))


def _close(segments, capacity, b, state):
    total = int(state[b, TOTAL])
    if 0 <= total < capacity:
        segments[b, total] = (state[b, SEG_START], state[b, SEG_LEN], state[b, STABLE] - 1, state[b, SEG_CONF])
    state[b, TOTAL] = total + 1


def decode(pred, conf, C, min_run, min_conf, state, segments=None, flush=False):
    """pred int64 [B,T], conf f32 [B,T] (T may be 0 with flush); state int64 [B,8] and segments int64 [B,capacity,4] as they
    are before the call (neither is written).  Returns (stable int64 [B,T], state, segments) after it."""
    pred, conf = np.asarray(pred, np.int64), np.asarray(conf, F32)
    B, T = pred.shape
    state = np.array(state, np.int64)
    segments = np.zeros((B, 0, 4), np.int64) if segments is None else np.array(segments, np.int64)
    capacity = segments.shape[1]
    min_conf = F32(min_conf)
    stable_out = np.empty((B, T), np.int64)
    for b in range(B):
        st = state[b]
        for f in range(T):
            t = int(st[SEEN]) + f
            c = int(pred[b, f]) if (conf[b, f] >= min_conf and 0 <= pred[b, f] < C) else -1
            if c == st[CAND] - 1:
                st[RUN] = min(int(st[RUN]) + 1, RUN_MAX)
            else:
                st[CAND], st[RUN] = c + 1, 1
            stable = int(st[CAND]) - 1 if st[RUN] >= min_run else int(st[STABLE]) - 1
            if stable != st[STABLE] - 1:
                if st[STABLE] > 0 and st[SEG_LEN] > 0:
                    _close(segments, capacity, b, state)
                st[STABLE] = stable + 1
                st[SEG_START], st[SEG_LEN], st[SEG_CONF] = (t, 0, 0) if stable >= 0 else (0, 0, 0)
            if stable >= 0:
                st[SEG_LEN] += 1
                st[SEG_CONF] += q(conf[b, f])
            stable_out[b, f] = stable
        st[SEEN] += T
        if flush:
            if st[STABLE] > 0 and st[SEG_LEN] > 0:
                _close(segments, capacity, b, state)
            st[SEG_START], st[SEG_LEN], st[SEG_CONF] = (st[SEEN] if st[STABLE] > 0 else 0), 0, 0
    return stable_out, state, segments


def segment_list(state, segments, b=0):
    """[(start, length, label, mean_confidence)] of stream b, as PoseTimeline.segments() gives it"""
    n = int(state[b, TOTAL])
    assert n <= segments.shape[1]
    return [(int(a), int(m), int(k), float(np.float64(s) / (np.float64(CONF_ONE) * np.float64(m)))) for a, m, k, s in segments[b, :n]]


def transitions(state, segments, C):
    """(counts [C,C], dwell [C]) of the closed segments of all streams, a Python count"""
    counts, dwell = np.zeros((C, C), np.int64), np.zeros(C, np.int64)
    for b in range(state.shape[0]):
        rec = segments[b, :min(int(state[b, TOTAL]), segments.shape[1])]
        for i, (_, m, k, _) in enumerate(rec):
            dwell[k] += m
            if i:
                counts[rec[i - 1][2], k] += 1
    return counts, dwell


# ---- seeded inputs ------------------------------------------------------------------------------------------------------
def make_probs(seed, batch, frames, C, run=9):
    """f32 rows that sum to about one, the dominant class changing every `run` frames or so"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((batch, frames, C)).astype(F32)
    lead = np.repeat(rng.integers(0, C, (batch, frames // run + 2)), run, axis=1)[:, rng.integers(0, run):][:, :frames]
    np.put_along_axis(z, lead[..., None], z.max(axis=2, keepdims=True) + F32(1.5), axis=2)
    e = np.exp(z - z.max(axis=2, keepdims=True))
    return (e / e.sum(axis=2, keepdims=True)).astype(F32)


def make_labels(seed, batch, frames, C, run=9, flicker=0.05, low=0.1, min_conf=0.5):
    """(pred int64, confidence f32) [batch, frames]: label runs of about `run` frames, `flicker` of the frames another class
    (or one outside [0, C)), `low` of the confidences below min_conf, a few NaN or outside [0, 1]"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(max(run - 4, 1), run + 5, (batch, frames // max(run - 4, 1) + 2))
    pred = np.stack([np.repeat(rng.integers(0, C, lengths.shape[1]), lengths[b])[:frames] for b in range(batch)]).astype(np.int64)
    pred = pred.reshape(batch, frames)
    flick = rng.random((batch, frames)) < flicker
    pred[flick] = rng.integers(-1, C + 1, int(flick.sum()))
    conf = (min_conf + (1 - min_conf) * rng.random((batch, frames))).astype(F32)
    weak = rng.random((batch, frames)) < low
    conf[weak] = (min_conf * rng.random(int(weak.sum()))).astype(F32)
    odd = rng.random((batch, frames)) < 0.02
    conf[odd] = rng.choice(np.array([np.nan, 1.5, -0.25, 1.0, 0.0], F32), int(odd.sum()))
    return pred, conf
