"""The rule of qt_segments_update / qt_segments_encode (include/qtcnn.h) as plain Python and np.int64 loops: runs by a
frame-by-frame walk, the full Levenshtein table, matching in Python integers with cross-multiplied comparisons.

A second, independent statement of the two hard parts checks the first (tests/test_segments_cpu.py): the Levenshtein distance
by anti-diagonals in NumPy, and the published evaluation loop of the segmental F1 (each predicted run in turn claims the true
run of the highest IoU, computed in floating point, and is a false positive when that one is taken or the IoU is below the
threshold).  The anti-diagonal form also serves the GPU tests where the table is large (1024 x 1024)."""
import numpy as np

MAX_SEGMENTS = 1024
MAX_CLASSES = 1024
MAX_THRESHOLDS = 8
RECORD = 5
STATE = 10
MAX_FRAMES = 1 << 22
EDIT_ONE = 1 << 32
TRIP = 256               # frames per trip of the kernel
(VIDEOS, OVERFLOW, EMPTY, SEG_PRED, SEG_TRUE, EDIT_DIST, EDIT_MAX, EDIT_Q, LABELLED, CORRECT) = range(STATE)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


# ---- the first statement ---------------------------------------------------------------------------------------------------------
def runs(values, C):
    """[(start, length, class)] of one video's frames, by a walk"""
    out, start, cur = [], 0, -1
    for f, v in enumerate(values):
        v = int(v)
        c = v if 0 <= v < C else -1
        if c != cur:
            if cur >= 0:
                out.append((start, f - start, cur))
            start, cur = f, c
    if cur >= 0:
        out.append((start, len(values) - start, cur))
    return out


def levenshtein(p, y):
    """the full table; p, y: sequences of classes"""
    m, n = len(p), len(y)
    D = np.zeros((m + 1, n + 1), np.int64)
    D[:, 0] = np.arange(m + 1)
    D[0, :] = np.arange(n + 1)
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            D[i, j] = min(D[i - 1, j] + 1, D[i, j - 1] + 1, D[i - 1, j - 1] + (p[i - 1] != y[j - 1]))
    return int(D[m, n])


def partner(p, Y, candidates=None):
    """(index, inter, union) of the partner of predicted run p among the true runs Y, or None"""
    ps, pe, best = p[0], p[0] + p[1], None
    for j in (range(len(Y)) if candidates is None else candidates):
        ys, ye = Y[j][0], Y[j][0] + Y[j][1]
        if Y[j][2] != p[2]:
            continue
        inter, union = max(0, min(pe, ye) - max(ps, ys)), max(pe, ye) - min(ps, ys)
        if best is None or inter * best[2] > best[1] * union:
            best = (j, inter, union)
    return best


def true_positives(P, Y, pcts):
    """tp per threshold: the distinct true runs that are the partner of at least one passing predicted run"""
    by_class = {}
    for j, y in enumerate(Y):
        by_class.setdefault(y[2], []).append(j)
    hit = [set() for _ in pcts]
    for p in P:
        best = partner(p, Y, by_class.get(p[2], ()))
        if best is None:
            continue
        for k, pct in enumerate(pcts):
            if 100 * best[1] >= pct * best[2]:
                hit[k].add(best[0])
    return [len(h) for h in hit]


def video(pred, label, C, pcts, distance=levenshtein):
    """the record of one video (already cut to its length): [m, n, D, frames_labelled, frames_correct, tp_0 ..]"""
    P, Y = runs(pred, C), runs(label, C)
    m, n = len(P), len(Y)
    labelled = sum(1 for v in label if 0 <= int(v) < C)
    correct = sum(1 for a, v in zip(pred, label) if 0 <= int(v) < C and int(a) == int(v))
    if m > MAX_SEGMENTS or n > MAX_SEGMENTS:
        return [m, n, -1, labelled, correct] + [-1] * len(pcts)
    D = distance([r[2] for r in P], [r[2] for r in Y])
    return [m, n, D, labelled, correct] + true_positives(P, Y, pcts)


def add_to_state(state, rec):
    m, n, D = (int(v) for v in rec[:3])
    state[VIDEOS] += 1
    state[LABELLED] += int(rec[3])
    state[CORRECT] += int(rec[4])
    if D < 0:
        state[OVERFLOW] += 1
        return
    M = max(m, n)
    state[SEG_PRED] += m
    state[SEG_TRUE] += n
    if M == 0:
        state[EMPTY] += 1
    else:
        state[EDIT_DIST] += D
        state[EDIT_MAX] += M
        state[EDIT_Q] += ((M - D) << 32) // M
    for k in range(len(rec) - RECORD):
        state[STATE + k] += int(rec[RECORD + k])


def video_length(lengths, b, frames):
    return frames if lengths is None else min(max(int(lengths[b]), 0), frames)


def evaluate(pred, label, C, pcts, lengths=None, state=None, distance=levenshtein):
    """(records int64 [B, RECORD + K], state int64 [STATE + K]) of pred, label int64 [B, T]; state: added to a copy"""
    B, T = pred.shape
    K = len(pcts)
    state = np.zeros(STATE + K, np.int64) if state is None else np.array(state, np.int64)
    records = np.zeros((B, RECORD + K), np.int64)
    for b in range(B):
        n = video_length(lengths, b, T)
        records[b] = video(pred[b, :n], label[b, :n], C, pcts, distance)
        add_to_state(state, records[b])
    return records, state


def encode(values, C, lengths=None, capacity=None, fill=-1):
    """(runs int32 [B, capacity, 3], counts int32 [B]); records at and behind the count keep `fill`"""
    B, T = values.shape
    capacity = T if capacity is None else capacity
    out, counts = np.full((B, capacity, 3), fill, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        r = runs(values[b, :video_length(lengths, b, T)], C)
        counts[b] = len(r)
        for k, run in enumerate(r[:capacity]):
            out[b, k] = run
    return out, counts


def report(state, pcts):
    """the report of the header, float64"""
    s = [int(v) for v in state]
    div = lambda a, b: float(a) / float(b) if b else 0.0
    scored = s[VIDEOS] - s[OVERFLOW] - s[EMPTY]
    out = {"edit": 100.0 * div(s[EDIT_Q], EDIT_ONE * scored),
           "edit_micro": 100.0 * (1.0 - s[EDIT_DIST] / s[EDIT_MAX]) if s[EDIT_MAX] else 0.0,
           "frame_accuracy": div(s[CORRECT], s[LABELLED]), "over_segmentation": div(s[SEG_PRED], s[SEG_TRUE]),
           "precision": {}, "recall": {}, "f1": {}}
    for pct, tp in zip(pcts, s[STATE:]):
        out["precision"][pct] = 100.0 * div(tp, s[SEG_PRED])
        out["recall"][pct] = 100.0 * div(tp, s[SEG_TRUE])
        out["f1"][pct] = 100.0 * div(2 * tp, s[SEG_PRED] + s[SEG_TRUE])
    return out


# ---- the second statement --------------------------------------------------------------------------------------------------------
def levenshtein_diagonals(p, y):
    """the same distance by anti-diagonals d = i + j, each a NumPy expression of the two before it"""
    p, y = np.asarray(p, np.int64), np.asarray(y, np.int64)
    m, n = len(p), len(y)
    d2 = d1 = None                                   # diagonals d - 2 and d - 1 as arrays over i = 0 .. m (unused cells stay 0)
    for d in range(m + n + 1):
        cur = np.zeros(m + 1, np.int64)
        lo, hi = max(0, d - n), min(m, d)
        if lo == 0:
            cur[0] = d
        if d <= m:
            cur[d] = d
        a, b = max(lo, 1), min(hi, d - 1)            # the inner cells: i >= 1 and j = d - i >= 1
        if a <= b:
            i = np.arange(a, b + 1)
            cost = (p[i - 1] != y[d - i - 1]).astype(np.int64)
            cur[i] = np.minimum(np.minimum(d1[i - 1], d1[i]) + 1, d2[i - 1] + cost)
        d2, d1 = d1, cur
    return int(d1[m])


def published_counts(P, Y, pct):
    """(tp, fp, fn) by the published loop: float IoU against every true run, zero for another class; the best one is claimed"""
    overlap = pct / 100.0
    tp = fp = 0
    used = np.zeros(len(Y), bool)
    if len(Y) == 0:
        return 0, len(P), 0
    y_start = np.array([y[0] for y in Y], np.float64)
    y_end = np.array([y[0] + y[1] for y in Y], np.float64)
    y_cls = np.array([y[2] for y in Y])
    for s, length, c in P:
        inter = np.minimum(s + length, y_end) - np.maximum(s, y_start)
        union = np.maximum(s + length, y_end) - np.minimum(s, y_start)
        iou = (inter / union) * (y_cls == c)
        j = int(np.argmax(iou))
        if iou[j] >= overlap and not used[j]:
            tp += 1
            used[j] = True
        else:
            fp += 1
    return tp, fp, len(Y) - int(used.sum())


# ---- data ------------------------------------------------------------------------------------------------------------------------
def make_pair(seed, frames, C, mean_run=12, flicker=0.04, unknown=0.02):
    """One seeded (pred, label) pair of int64 [frames]: label holds runs of about mean_run frames; pred is label with its
    boundaries moved by a few frames, short fragments of other classes flickered in and some frames unknown (-1, C or 2^40).
    Frame 0 of label is always known."""
    rng = np.random.default_rng(seed)
    label = np.empty(frames, np.int64)
    f = 0
    while f < frames:
        n = int(rng.integers(1, 2 * mean_run))
        label[f:f + n] = rng.integers(0, C)
        f += n
    pred = np.roll(label, int(rng.integers(-3, 4)))
    for f in np.nonzero(rng.random(frames) < flicker)[0]:
        pred[f:f + int(rng.integers(1, 4))] = rng.integers(0, C)
    bad = np.array([-1, C, 1 << 40], np.int64)
    where = rng.random(frames) < unknown
    pred[where] = bad[rng.integers(0, 3, int(where.sum()))]
    where = rng.random(frames) < unknown / 2
    where[:1] = False
    label[where] = bad[rng.integers(0, 3, int(where.sum()))]
    return pred, label


def make_batch(seed, batch, frames, C, **kw):
    pairs = [make_pair(1000 * seed + b, frames, C, **kw) for b in range(batch)]
    return np.stack([p for p, _ in pairs]), np.stack([l for _, l in pairs])


def frames_of(classes, frames=None, run=1):
    """int64 frames holding exactly the runs of `classes`, `run` frames each, one unknown frame between two runs of the same
    class, padded with -1 to `frames`"""
    out = []
    for k, c in enumerate(classes):
        if k and classes[k - 1] == c:
            out.append(-1)
        out.extend([int(c)] * run)
    frames = len(out) if frames is None else frames
    assert len(out) <= frames
    return np.array(out + [-1] * (frames - len(out)), np.int64)


# the seeded batches of tests/test_segments_gpu.py: (seed, batch, frames, C).  tests/test_segments_cpu.py asserts on the
# reference alone that none of their videos overflows or is empty and that each has at most a few hundred runs.
SEEDED = [(1, 3, 257, 4), (2, 2, 513, 12), (3, 5, 300, 12), (4, 1, 1500, 1024), (5, 4, 64, 2)]
