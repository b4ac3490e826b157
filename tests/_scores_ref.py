"""The rule of the score-based evaluation (include/qtcnn.h, csrc/scores.hip) as plain numpy, shared by
tests/test_scores_cpu.py (against the recorded scikit-learn values and against itself), tests/test_scores_gpu.py (the kernels,
integer for integer) and tests/golden/make_score_metrics_golden.py.

np.float32 for the two products (p K and conf M), Python integers for A2, float64 sums in the kernel's stated order (a
thread's K / 256 consecutive bins from the top down, then the halving tree over 256 partial sums; classes and calibration
bins in ascending order).  `update` takes the probabilities as an argument: the CPU tests pass a numpy softmax, the GPU
tests what `predict` wrote on the same device, so expf's rounding does not enter the comparison."""
import numpy as np

IGNORE = -100
LOGITS, PROBS = 0, 1
THREADS = 256
SCALARS = ("macro_auc", "weighted_auc", "macro_ap", "weighted_ap", "ece", "mce", "samples", "ignored", "invalid", "nan_rows",
           "classes_scored", "updates")


def cells(C, bits, M):
    return 2 * C * (1 << bits) + C + 3 * M + 5


def report_len(C, M):
    return 4 * C + 3 * M + 12


def q_of(p, bits):
    """min(K - 1, (int)(p * (float)K)) of f32 probabilities in [0, 1]"""
    K = 1 << bits
    return np.minimum(K - 1, (np.asarray(p, np.float32) * np.float32(K)).astype(np.int64))


def softmax_f32(z):
    """a numpy f32 softmax (max subtracted); NOT bit-identical to the kernel's expf, used where only the rule is tested"""
    z = np.asarray(z, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(z - z.max(1, keepdims=True), dtype=np.float32)
        return (e / e.sum(1, keepdims=True, dtype=np.float32)).astype(np.float32)


def row_classes(p, labels, C, kind, ignore_index=IGNORE):
    """0 counted, 1 ignored, 2 invalid, 3 nan: the first that applies, in the order ignored, invalid, nan"""
    y = np.asarray(labels, np.int64)
    p = np.asarray(p, np.float32)
    with np.errstate(invalid="ignore"):
        bad = np.isnan(p).any(1) if kind == LOGITS else ~((p >= 0) & (p <= 1)).all(1)
    cls = np.where(bad, 3, 0)
    cls = np.where((y < 0) | (y >= C), 2, cls)
    return np.where(y == ignore_index, 1, cls)


def update(state, given, p, labels, C, bits, M, kind, ignore_index=IGNORE, calls=1):
    """the state after one call, added to `state` (None: zeros).  given: the scores as given (z for logits, p for probs),
    p: the f32 probabilities [rows][C]."""
    K = 1 << bits
    st = np.zeros(cells(C, bits, M), np.int64) if state is None else np.asarray(state, np.int64).copy()
    s = np.asarray(given, np.float32)
    p = np.asarray(p, np.float32)
    y = np.asarray(labels, np.int64)
    cls = row_classes(p, y, C, kind, ignore_index)
    ok = cls == 0
    H = 2 * C * K
    if ok.any():
        pc, sc, yc = p[ok], s[ok], y[ok]
        n = len(yc)
        k = np.arange(C)[None, :]
        side = (k == yc[:, None]).astype(np.int64)
        np.add.at(st, ((k * 2 + side) * K + q_of(pc, bits)).reshape(-1), 1)
        sy = sc[np.arange(n), yc][:, None]
        rank = ((sc > sy) | ((sc == sy) & (k < yc[:, None]))).sum(1)
        np.add.at(st, H + rank, 1)
        pred = np.argmax(pc, 1)                                   # the first maximum; a counted row holds no NaN
        conf = pc[np.arange(n), pred]
        b = np.minimum(M - 1, (conf * np.float32(M)).astype(np.int64))
        cq = np.rint(np.clip(conf, np.float32(0), np.float32(1)) * np.float32(65536)).astype(np.int64)
        cal = H + C + 3 * b
        np.add.at(st, cal, 1)
        np.add.at(st, cal + 1, (pred == yc).astype(np.int64))
        np.add.at(st, cal + 2, cq)
    ctr = H + C + 3 * M
    for i in range(4):
        st[ctr + i] += int((cls == i).sum())
    st[ctr + 4] += calls
    return st


def _tree(partial):
    red = np.array(partial, np.float64)
    s = THREADS // 2
    while s >= 1:
        red[:s] += red[s:2 * s]
        s //= 2
    return float(red[0])


def report(state, C, bits, M):
    """(float64 [4C + 3M + 12], int64 curves [C][2][K]) from a state"""
    K = 1 << bits
    st = np.asarray(state, np.int64)
    H = 2 * C * K
    hist = st[:H].reshape(C, 2, K)
    rank, cal, ctr = st[H:H + C], st[H + C:H + C + 3 * M].reshape(M, 3), st[H + C + 3 * M:]
    rep = np.zeros(report_len(C, M))
    curves = np.zeros((C, 2, K), np.int64)
    nan = float("nan")
    per = K // THREADS if K >= THREADS else 1
    for k in range(C):
        neg, pos = hist[k, 0], hist[k, 1]
        P, N = int(pos.sum()), int(neg.sum())
        posbelow, negbelow = np.cumsum(pos) - pos, np.cumsum(neg) - neg
        tp, fp = P - posbelow, N - negbelow
        curves[k, 0], curves[k, 1] = tp, fp
        occupied = np.nonzero(pos)[0]
        a2 = sum(int(pos[b]) * (2 * int(negbelow[b]) + int(neg[b])) for b in occupied)
        rep[k] = float(a2) / float(2 * P * N) if P and N else nan
        partial = [0.0] * THREADS
        for b in occupied[::-1]:
            t_, f_ = float(tp[b]), float(fp[b])
            partial[b // per] += (float(pos[b]) / float(P)) * (t_ / (t_ + f_))
        rep[C + k] = _tree(partial) if P else nan
        rep[2 * C + k] = float(P)
    counted = int(ctr[0])
    cum = 0
    for k in range(C):
        cum += int(rank[k])
        rep[3 * C + k] = float(cum) / float(counted) if counted else nan
    o = 4 * C
    gaps = []
    for b in range(M):
        n, hit, cs = (int(v) for v in cal[b])
        acc = float(hit) / float(n) if n else 0.0
        conf = float(cs) / (65536.0 * float(n)) if n else 0.0
        rep[o + b], rep[o + M + b], rep[o + 2 * M + b] = float(n), acc, conf
        gaps.append((float(n), abs(acc - conf)))
    s = rep[o + 3 * M:]
    n = float(sum(g[0] for g in gaps))
    ece = mce = 0.0
    for w, g in gaps:
        if w > 0:
            ece += (w / n) * g
            mce = max(mce, g)
    ma = wa = sa = na = mp = wp = sp = npp = 0.0
    for k in range(C):
        a, ap, sup = rep[k], rep[C + k], rep[2 * C + k]
        if a == a:
            ma, wa, sa, na = ma + a, wa + sup * a, sa + sup, na + 1.0
        if ap == ap:
            mp, wp, sp, npp = mp + ap, wp + sup * ap, sp + sup, npp + 1.0
    s[0], s[1] = (ma / na, wa / sa) if na else (nan, nan)
    s[2], s[3] = (mp / npp, wp / sp) if npp else (nan, nan)
    s[4], s[5] = (ece, mce) if n > 0 else (nan, nan)
    s[6], s[7], s[8], s[9], s[10], s[11] = counted, ctr[1], ctr[2], ctr[3], na, ctr[4]
    return rep, curves


def scalars(rep, C, M):
    return dict(zip(SCALARS, np.asarray(rep)[4 * C + 3 * M:].tolist()))


def close(got, want, tol=1e-12):
    """|got - want| <= tol * max(1, |want|) elementwise, NaN only where NaN is wanted (the report's tolerance)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    m = ~np.isnan(want)
    return bool(np.all(np.abs(got[m] - want[m]) <= tol * np.maximum(1.0, np.abs(want[m]))))


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def make_logits(rows, C, seed, peak=4.0):
    """(z f32 [rows][C], labels int64 [rows]): seeded normal logits with the label's column raised by `peak` in about 70 %
    of the rows (a trained-looking model); peak = 0 gives flat scores"""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, C, size=rows).astype(np.int64)
    z = rng.standard_normal((rows, C)).astype(np.float32)
    lift = rng.random(rows) < 0.7
    z[np.arange(rows)[lift], y[lift]] += np.float32(peak)
    return z, y


def mix_in(s, y, C, kind, ignore_index=IGNORE):
    """Overwrites the first rows (as many as there are) with the cases a rule can get wrong; returns (s, y).  Row 0 keeps a
    valid label so that a batch of one row is counted."""
    s, y = s.copy(), y.copy()
    rows = len(y)
    one = np.float32(1.0)

    def put(i, row=None, label=None):
        if i < rows:
            if row is not None:
                s[i, :] = row
            if label is not None:
                y[i] = label

    hot = np.zeros(C, np.float32)
    if kind == PROBS:
        hot[C - 1] = one
        put(1, hot, C - 1)                                  # p exactly 1 and exactly 0
        put(2, np.full(C, 0.25, np.float32), C - 1)         # all tied: the rank is the label's index, pred is class 0
        put(3, None, ignore_index)
        put(4, None, C)
        put(5, None, -1)
        bad = np.full(C, 0.125, np.float32)
        bad[0] = np.float32(1.5)                            # a value above 1: a nan row
        put(6, bad, 0)
        bad = np.full(C, 0.125, np.float32)
        bad[C // 2] = np.nan
        put(7, bad, 0)
        put(8, bad, ignore_index)                           # ignored comes first
        put(9, bad, 2 ** 40)                                # invalid before nan
        neg = np.full(C, 0.5, np.float32)
        neg[C - 1] = np.float32(-0.0)                       # -0.0 is inside [0, 1]
        put(10, neg, 0)
        tie = np.full(C, 0.0625, np.float32)
        tie[0] = tie[C - 1] = np.float32(0.75)              # a tie at the top: the lower index ranks first
        put(11, tie, C - 1)
        put(12, tie, 0)
        put(13, np.full(C, 1.0 - 2.0 ** -24, np.float32), C // 2)
    else:
        hot[:] = np.float32(-200.0)
        hot[C - 1] = np.float32(50.0)                       # expf underflows: p exactly 0 and exactly 1
        put(1, hot, C - 1)
        put(2, np.zeros(C, np.float32), C - 1)              # all tied
        put(3, None, ignore_index)
        put(4, None, C)
        put(5, None, -1)
        bad = np.zeros(C, np.float32)
        bad[0] = np.inf                                     # softmax gives NaN
        put(6, bad, 0)
        bad = np.zeros(C, np.float32)
        bad[C // 2] = np.nan
        put(7, bad, 0)
        put(8, bad, ignore_index)
        put(9, bad, 2 ** 40)
        low = np.zeros(C, np.float32)
        low[C - 1] = -np.inf                                # a finite row: p = 0 there
        put(10, low, 0)
        tie = np.full(C, -1.0, np.float32)
        tie[0] = tie[C - 1] = np.float32(2.5)
        put(11, tie, C - 1)
        put(12, tie, 0)
        put(13, np.full(C, -np.inf, np.float32), 0)         # all -inf: NaN
    return s, y
