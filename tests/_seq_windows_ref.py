"""Plain statements of the sequence-window rules of include/qtcnn.h (qt_seq_windows_plan, qt_seq_gather_rows) in numpy, and a
Python walk of the three launches of csrc/seq_windows.hip.

`windows` is the reference's two loops as they stand: per clip, `for i in range(0, n - T + 1, stride)`, the window's labels
looked at as create_sequential_dataset.py:164-171 ("uniform": one distinct value, and a known one) or
prepare_sequential_dataset.py:46-62 ("last": the last frame's label, if it is a known class) do.  tests/golden/seq_windows.npz
holds what those two scripts themselves produced on small clips; tests/test_seq_windows_cpu.py compares.
`kernel_walk` follows the kernels instead: spans of SPAN positions, per (trip, wave) counts, one scan workgroup that takes
SCAN partials per trip, the scatter by slot.  Both give (starts int32, labels int64, count).
"""
import numpy as np

UNIFORM, LAST = 0, 1
RULES = {"uniform": UNIFORM, "last": LAST}
SPAN, THREADS, SCAN, WAVE = 1024, 256, 256, 64      # csrc/seq_windows.hip: SW_SPAN, SW_THREADS, SW_SCAN, the wave size
MAX_SEQ = 64


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int32)


def candidate_count(lengths, T, stride):
    return int(sum(max(0, (int(n) - T) // stride + 1) for n in lengths))


def windows(labels, lengths, T, stride, num_classes, rule, capacity=None):
    """the plain per-clip loop: (starts int32 [min(count, capacity)], labels int64 [same], count)"""
    labels = np.asarray(labels, dtype=np.int64)
    assert int(np.sum(lengths)) == labels.shape[0]
    starts, out = [], []
    begin = 0
    for n in lengths:
        n = int(n)
        clip = labels[begin:begin + n]
        for i in range(0, n - T + 1, stride):
            win = clip[i:i + T]
            if rule == UNIFORM:
                if len(np.unique(win)) != 1:
                    continue
            label = int(win[-1])
            if not 0 <= label < num_classes:
                continue
            starts.append(begin + i)
            out.append(label)
        begin += n
    count = len(starts)
    keep = count if capacity is None else min(count, capacity)
    return np.array(starts[:keep], dtype=np.int32), np.array(out[:keep], dtype=np.int64), count


def windows_vectorised(labels, lengths, T, stride, num_classes, rule, capacity=None):
    """`windows` without the Python loop, for the sizes at which the loop takes seconds; tests/test_seq_windows_cpu.py holds
    the two equal"""
    labels = np.asarray(labels, dtype=np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)
    N = labels.shape[0]
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    clip = np.repeat(np.arange(len(lengths)), lengths)
    p = np.arange(N)
    keep = (p + T <= offsets[clip + 1]) & ((p - offsets[clip]) % stride == 0)
    last = labels[np.minimum(p + T - 1, N - 1)]
    keep &= (last >= 0) & (last < num_classes)
    if rule == UNIFORM and T > 1:
        same = np.concatenate([[0], np.cumsum(labels[1:] == labels[:-1])])      # same[i]: equal neighbours before frame i
        keep &= same[np.minimum(p + T - 1, N - 1)] - same[p] == T - 1
    starts = p[keep]
    count = len(starts)
    n = count if capacity is None else min(count, capacity)
    return starts[:n].astype(np.int32), last[keep][:n], count


def kernel_walk(labels, lengths, T, stride, num_classes, rule, capacity=None, span=SPAN, threads=THREADS, scan=SCAN, wave=WAVE):
    """The launches of qt_seq_windows_plan in Python.  Returns (starts, labels, count, scan_trips)."""
    labels = np.asarray(labels, dtype=np.int64)
    frames = labels.shape[0]
    offsets = offsets_of(lengths)
    clips = len(lengths)
    capacity = candidate_count(lengths, T, stride) if capacity is None else capacity
    trips, waves = span // threads, threads // wave

    def window_label(lab, s0, i):
        p = s0 + i
        if p + T > frames:
            return -1
        v = lab[i + T - 1]
        if v < 0:
            return -1
        if rule == UNIFORM and any(lab[i + t] != v for t in range(T - 1)):
            return -1
        lo, hi = 0, clips
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            if offsets[mid] <= p:
                lo = mid
            else:
                hi = mid
        begin, end = int(offsets[lo]), min(int(offsets[lo + 1]), frames)
        if begin < 0 or begin > p or p + T > end or (p - begin) % stride:
            return -1
        return int(v)

    def span_windows(g):
        s0 = g * span
        n = min(span + T - 1, frames - s0)
        lab = [int(l) if 0 <= l < num_classes else -1 for l in labels[s0:s0 + n]]
        v = [[window_label(lab, s0, k * threads + t) for t in range(threads)] for k in range(trips)]
        wc = [[sum(1 for t in range(w * wave, (w + 1) * wave) if v[k][t] >= 0) for w in range(waves)] for k in range(trips)]
        return s0, v, wc

    spans = -(-frames // span)
    partial = [sum(sum(row) for row in span_windows(g)[2]) for g in range(spans)]       # launch 1
    carry, scan_trips = 0, 0                                                            # launch 2: one workgroup
    for base in range(0, spans, scan):
        chunk = partial[base:base + scan]
        run = 0
        for j, own in enumerate(chunk):
            partial[base + j] = carry + run
            run += own
        carry += run
        scan_trips += 1
    count = carry
    starts = np.full(capacity, -7, dtype=np.int32)                                      # launch 3
    out = np.full(capacity, -7, dtype=np.int64)
    for g in range(spans):
        s0, v, wc = span_windows(g)
        slot = partial[g]
        for k in range(trips):
            for w in range(waves):
                rank = 0
                for t in range(w * wave, (w + 1) * wave):
                    if v[k][t] >= 0:
                        mine = slot + sum(wc[k][:w]) + rank
                        rank += 1
                        if mine < capacity:
                            assert starts[mine] == -7
                            starts[mine], out[mine] = s0 + k * threads + t, v[k][t]
            slot += sum(wc[k])
    keep = min(count, capacity)
    assert (starts[keep:] == -7).all() and (starts[:keep] != -7).all()
    return starts[:keep], out[:keep], count, scan_trips


def random_case(seed, frames, clips, num_classes, run=6, unknown=0.1):
    """seeded labels in runs of about `run` equal values (so that uniform windows exist), a share `unknown` of them outside
    [0, num_classes) on either side, and `clips` lengths (some zero) that sum to `frames`"""
    rng = np.random.default_rng(seed)
    labels = np.repeat(rng.integers(0, num_classes, frames), rng.integers(1, 2 * run, frames))[:frames].astype(np.int64)
    bad = rng.random(frames) < unknown
    labels[bad] = rng.choice(np.array([-1, num_classes, -(1 << 40), 1 << 40], dtype=np.int64), int(bad.sum()))
    cuts = np.sort(rng.integers(0, frames + 1, max(clips - 1, 0)))
    lengths = np.diff(np.concatenate([[0], cuts, [frames]])).astype(np.int64)
    return labels, lengths


def gather_rows(src, starts, T):
    """src: any array [N, ...]; starts: ints.  The byte-exact gather [B, T, ...]; a start outside [0, N - T] is 0xFF bytes."""
    src = np.ascontiguousarray(src)
    N = src.shape[0]
    out = np.empty((len(starts), T) + src.shape[1:], dtype=src.dtype)
    as_bytes = out.view(np.uint8).reshape(len(starts), -1)
    for b, s in enumerate(starts):
        s = int(s)
        if 0 <= s <= N - T:
            out[b] = src[s:s + T]
        else:
            as_bytes[b] = 0xFF
    return out
