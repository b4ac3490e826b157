"""Segment-level evaluation on the GPU (csrc/segments.hip, <pkg>/segments.py): qt_segments_update and qt_segments_encode against
the plain rule of tests/_segments_ref.py, every output and the state compared for equality (every number is an integer: there
is nothing for a tolerance to cover), at the sizes where the trips, the ballots, the diagonals and the cap can go wrong.
Every buffer sits between poisoned guard bands (tests/_guard.py); the padding columns of ld > frames and the frames at and
beyond a video's length hold known classes that would add runs if they were read; inputs must come back unchanged.  Large
Levenshtein tables (up to 1024 x 1024) are the reference's anti-diagonal form, which tests/test_segments_cpu.py holds
against the full table."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _segments_ref as R
from _guard import Guard
from _util import pkg

pytestmark = pytest.mark.gpu
TRIP = R.TRIP
I64 = lambda *v: np.array(v, np.int64)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _api():
    M, Lm = pkg("segments"), pkg("_lib")
    return M, Lm, Lm.lib()


def _poisoned(values, C, lengths, pad):
    """values [B, T] in rows of T + pad columns; the padding and the frames at and beyond a video's length alternate between
    the known classes 0 and C - 1"""
    B, T = values.shape
    out = np.tile((np.arange(T + pad) % 2) * (C - 1), (B, 1)).astype(np.int64)
    for b in range(B):
        n = R.video_length(lengths, b, T)
        out[b, :n] = values[b, :n]
    return out


def run_update(dev, pred, label, C, pcts, lengths=None, state=None, pad=3, want_records=True):
    """qt_segments_update through ctypes; returns (records or None, state) as numpy arrays"""
    M, Lm, L = _api()
    B, T = pred.shape
    K = len(pcts)
    G = Guard(dev)
    d_pred = G.input("pred", torch.from_numpy(_poisoned(pred, C, lengths, pad)))
    d_label = G.input("label", torch.from_numpy(_poisoned(label, C, lengths, pad + 2)))
    d_len = G.input("lengths", None if lengths is None else torch.tensor(lengths, dtype=torch.int32))
    d_state = G.output("state", (R.STATE + K,), torch.int64, fill=0)
    if state is not None:
        d_state.copy_(torch.from_numpy(np.asarray(state, np.int64)))
    d_rec = G.output("records", (B, R.RECORD + K), torch.int64) if want_records else None
    desc = M.make_desc(B, T, C, pcts)
    need = L.qt_segments_workspace_bytes(ctypes.byref(desc))
    assert need == B * (R.RECORD + K) * 8
    d_work = G.workspace("workspace", need)
    Lm.check(L.qt_segments_update(ctypes.byref(desc), Lm.ptr(d_pred), T + pad, Lm.ptr(d_label), T + pad + 2, Lm.ptr(d_len),
                                  Lm.ptr(d_state), Lm.ptr(d_rec), Lm.ptr(d_work), need, Lm.stream_ptr()), "qt_segments_update")
    G.check()
    return (d_rec.cpu().numpy() if want_records else None), d_state.cpu().numpy()


def same_update(dev, pred, label, C, pcts, lengths=None, distance=R.levenshtein, what=None):
    """one call against the reference: records and state equal; returns (records, state)"""
    want_rec, want_state = R.evaluate(pred, label, C, pcts, lengths, distance=distance)
    rec, state = run_update(dev, pred, label, C, pcts, lengths)
    assert rec.tolist() == want_rec.tolist(), (what, "records")
    assert state.tolist() == want_state.tolist(), (what, "state")
    return rec, state


def run_encode(dev, values, C, lengths=None, capacity=None, pad=3):
    M, Lm, L = _api()
    B, T = values.shape
    capacity = T if capacity is None else capacity
    G = Guard(dev)
    d_val = G.input("values", torch.from_numpy(_poisoned(values, C, lengths, pad)))
    d_len = G.input("lengths", None if lengths is None else torch.tensor(lengths, dtype=torch.int32))
    d_runs = G.output("runs", (B, capacity, 3), torch.int32) if capacity else None
    d_counts = G.output("counts", (B,), torch.int32)
    desc = M.make_desc(B, T, C, capacity=capacity)
    Lm.check(L.qt_segments_encode(ctypes.byref(desc), Lm.ptr(d_val), T + pad, Lm.ptr(d_len), Lm.ptr(d_runs), Lm.ptr(d_counts),
                                  Lm.stream_ptr()), "qt_segments_encode")
    G.check()
    runs = d_runs.cpu().numpy() if capacity else np.zeros((B, 0, 3), np.int32)
    return runs, d_counts.cpu().numpy()


# ---- runs --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def run_videos(frames, C=3):
    """the videos whose runs can go wrong: seeded with unknown values -1, C and 2^40; all unknown; one run over every trip;
    a boundary exactly at a trip's edge; a gap exactly at it; a run per frame"""
    f = np.arange(frames)
    rows = [R.make_pair(40 + frames, frames, C, mean_run=5, unknown=0.1)[0],
            I64(-1, C, 1 << 40)[f % 3],
            np.full(frames, C - 1, np.int64),
            np.where(f < TRIP, 0, 1).astype(np.int64),
            np.where((f == TRIP) | (f == 2 * TRIP - 1), -1, 1).astype(np.int64),
            (f % 2).astype(np.int64),
            np.where(f % 64 == 63, 1 << 40, (f // 64) % 2).astype(np.int64)]
    values = np.stack(rows)
    values.setflags(write=False)
    return values


@pytest.mark.parametrize("frames", [0, 1, 255, 256, 257, 513])
def test_encode_equals_the_walk(frames):
    dev = _dev()
    C = 3
    values = run_videos(frames)
    B = values.shape[0]
    mixed = [0, frames, -2, frames + 7, frames // 2, TRIP, frames - 1][:B]
    for lengths in (None, mixed):
        _, full = R.encode(values, C, lengths)
        top = int(full.max())
        if lengths is None and frames:
            assert full.tolist()[1:4] == [0, 1, min(2, -(-frames // TRIP))] and full[5] == frames
        for capacity in sorted({0, max(top - 1, 0), top, top + 5}):
            want = R.encode(values, C, lengths, capacity)
            got = run_encode(dev, values, C, lengths, capacity)
            assert got[1].tolist() == want[1].tolist(), (lengths, capacity, "counts")
            assert R.bits(got[0]) == R.bits(want[0]), (lengths, capacity, "runs")


@pytest.mark.parametrize("frames", [0, 1, 255, 256, 257, 513])
def test_update_on_the_run_videos(frames):
    """the same videos through qt_segments_update, against themselves moved by one frame, with and without lengths"""
    dev = _dev()
    C = 3
    pred = run_videos(frames)
    label = np.roll(pred, 1, axis=1)
    B = pred.shape[0]
    pcts = (10, 25, 50)
    for lengths in (None, [0, frames, -2, frames + 7, frames // 2, TRIP, frames - 1][:B]):
        rec, state = same_update(dev, pred, label, C, pcts, lengths, distance=R.levenshtein_diagonals, what=(frames, lengths))
        assert state[R.OVERFLOW] == 0 and state[R.VIDEOS] == B
        if frames == 0:
            assert state[R.EMPTY] == B and not state[R.SEG_PRED:].any()
        elif lengths is None:
            assert state[R.EMPTY] == 1                           # the all-unknown video, and no other


# ---- edit ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edit_case(m, n):
    """three videos with m predicted and n true runs: repeated classes; disjoint alphabets (D = max(m, n)); identical
    sequences (D = 0) where m == n, a shared prefix otherwise.  Computed once, shared, never written."""
    rng = np.random.default_rng(100 * m + n)
    p, y = rng.integers(0, 3, m), rng.integers(0, 3, n)
    pairs = [(p, y), (rng.integers(0, 2, m), rng.integers(2, 5, n)), (p, p if m == n else np.concatenate([p, y])[:n])]
    T = max(len(R.frames_of(list(s))) for pair in pairs for s in pair)
    pred = np.stack([R.frames_of(list(a), T) for a, _ in pairs])
    label = np.stack([R.frames_of(list(b), T) for _, b in pairs])
    ref = R.evaluate(pred, label, 5, (10, 25, 50), distance=R.levenshtein_diagonals)
    for a in (pred, label) + ref:
        a.setflags(write=False)
    return pred, label, ref


@pytest.mark.parametrize("m,n", [(0, 0), (0, 3), (1, 1), (1, 300), (63, 65), (1023, 1024), (1024, 1024)])
def test_edit_distance_equals_the_table(m, n):
    dev = _dev()
    pred, label, (want_rec, want_state) = edit_case(m, n)
    M = max(m, n)
    assert want_rec[:, 0].tolist() == [m] * 3 and want_rec[:, 1].tolist() == [n] * 3
    assert want_rec[1, 2] == M and (want_rec[2, 2] == 0 if m == n else want_rec[2, 2] == abs(m - n))
    if m * n <= 65 * 65:                                         # small enough for the full table
        assert R.evaluate(pred, label, 5, (10, 25, 50))[0].tolist() == want_rec.tolist()
    rec, state = run_update(dev, pred, label, 5, (10, 25, 50))
    assert rec.tolist() == want_rec.tolist() and state.tolist() == want_state.tolist()
    assert state[R.OVERFLOW] == 0 and state[R.EMPTY] == (3 if M == 0 else 0)
    # the other way round: the table is not square
    rec, state = run_update(dev, label, pred, 5, (10, 25, 50))
    assert rec[:, 2].tolist() == want_rec[:, 2].tolist() and rec[:, 0].tolist() == [n] * 3 and rec[:, 1].tolist() == [m] * 3
    assert state[R.EDIT_Q] == want_state[R.EDIT_Q] and state[R.OVERFLOW] == 0


def test_one_overflowing_video_beside_normal_ones():
    dev = _dev()
    C, pcts = 4, (10, 50)
    many = R.frames_of([k % 2 for k in range(R.MAX_SEGMENTS + 1)])
    T = len(many)
    pred, label = R.make_batch(9, 3, T, C)
    _, normal = R.evaluate(pred[[0, 2]], label[[0, 2]], C, pcts, distance=R.levenshtein_diagonals)
    for side in (0, 1):                                          # m = 1025, then n = 1025
        pred, label = R.make_batch(9, 3, T, C)
        (pred, label)[side][1] = many
        rec, state = same_update(dev, pred, label, C, pcts, distance=R.levenshtein_diagonals)
        assert state[R.OVERFLOW] == 1 and state[R.EMPTY] == 0 and state[R.VIDEOS] == 3
        assert rec[1, 2] == -1 and rec[1, R.RECORD:].tolist() == [-1, -1] and R.MAX_SEGMENTS + 1 in rec[1, :2]
        moved = [k for k in range(R.STATE + 2) if k not in (R.VIDEOS, R.OVERFLOW, R.LABELLED, R.CORRECT)]
        assert state[moved].tolist() == normal[moved].tolist()   # nothing else moved
        assert state[R.LABELLED] == normal[R.LABELLED] + rec[1, 3] and rec[1, 3] > 0
    # exactly the cap on both sides is no overflow
    full = R.frames_of([k % 2 for k in range(R.MAX_SEGMENTS)])[None]
    rec, state = same_update(dev, full, full, 2, (50,), distance=R.levenshtein_diagonals)
    assert rec.tolist() == [[1024, 1024, 0, 1024, 1024, 1024]] and state[R.OVERFLOW] == 0


# ---- F1 --------------------------------------------------------------------------------------------------------------------------
def test_the_hand_worked_videos():
    """the videos of tests/test_segments_cpu.py in one batch, told apart by lengths; K = 8"""
    dev = _dev()
    videos = [(I64(0, 0, 1, 1, 1, 2), I64(0, 0, 0, 1, 1, 2)),                                   # one late boundary
              (I64(0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0), I64(*[0] * 11)),                          # a hold in three fragments
              (I64(-1, 1, 1, 1, 1, -1), I64(1, 1, -1, -1, 1, 1)),                                # a tie; 100 inter == 20 union
              (I64(1, -1, 1, 1, 1, 1, -1, -1), I64(1, 1, 1, -1, -1, 1, 1, 1))]                   # the tie seen in a count
    T = 11
    pred = np.stack([np.concatenate([p, np.zeros(T - len(p), np.int64)]) for p, _ in videos])
    label = np.stack([np.concatenate([l, np.zeros(T - len(l), np.int64)]) for _, l in videos])
    lengths = [len(p) for p, _ in videos]
    pcts = (10, 16, 17, 20, 21, 25, 50, 67)
    rec, state = same_update(dev, pred, label, 3, pcts, lengths)
    assert rec.tolist() == [[3, 3, 0, 6, 5, 3, 3, 3, 3, 3, 3, 3, 1],
                            [3, 1, 2, 11, 9, 1, 1, 1, 1, 1, 1, 0, 0],
                            [1, 2, 1, 4, 2, 1, 1, 1, 1, 0, 0, 0, 0],
                            [2, 2, 0, 6, 3, 1, 1, 1, 1, 1, 1, 0, 0]]
    assert state[:R.STATE].tolist() == [4, 0, 0, 9, 8, 3, 10, 2 * (1 << 32) + (1 << 32) // 3 + (1 << 31), 27, 19]
    assert state[R.OVERFLOW] == 0 and state[R.EMPTY] == 0


@pytest.mark.parametrize("case", range(len(R.SEEDED)))
def test_seeded_videos(case):
    """K = 1, and K = 8 with thresholds unsorted and duplicated"""
    dev = _dev()
    seed, batch, frames, C = R.SEEDED[case]
    pred, label = R.make_batch(seed, batch, frames, C)
    eight = (50, 10, 25, 10, 100, 1, 75, 50)
    rec8, state = same_update(dev, pred, label, C, eight, distance=R.levenshtein_diagonals)
    assert state[R.OVERFLOW] == 0 and state[R.EMPTY] == 0
    assert rec8[:, R.RECORD + 1].tolist() == rec8[:, R.RECORD + 3].tolist() and rec8[:, R.RECORD].tolist() == rec8[:, R.RECORD + 7].tolist()
    assert (rec8[:, R.RECORD + 5] >= rec8[:, R.RECORD + 1]).all() and state[R.STATE + 5] > state[R.STATE + 4]
    rec1, state = same_update(dev, pred, label, C, (50,), distance=R.levenshtein_diagonals)
    assert state[R.OVERFLOW] == 0 and state[R.EMPTY] == 0 and rec1[:, R.RECORD].tolist() == rec8[:, R.RECORD].tolist()
    # with lengths, every video still with a known label at frame 0
    lengths = [1 + (7 * b * frames) // (5 * batch) for b in range(batch)]
    _, state = same_update(dev, pred, label, C, (25,), lengths, distance=R.levenshtein_diagonals)
    assert state[R.OVERFLOW] == 0 and state[R.EMPTY] == 0


# ---- additivity ------------------------------------------------------------------------------------------------------------------
def test_the_state_is_additive_and_a_video_alone_gives_its_record():
    dev = _dev()
    seed, batch, frames, C = R.SEEDED[2]
    assert batch == 5
    pred, label = R.make_batch(seed, batch, frames, C)
    pcts = (10, 25, 50)
    rec, whole = same_update(dev, pred, label, C, pcts, distance=R.levenshtein_diagonals)
    assert whole[R.OVERFLOW] == 0 and whole[R.EMPTY] == 0
    _, part = run_update(dev, pred[:2], label[:2], C, pcts)
    _, split = run_update(dev, pred[2:], label[2:], C, pcts, state=part, want_records=False)
    assert split.tolist() == whole.tolist()
    _, part = run_update(dev, pred[2:], label[2:], C, pcts)
    _, other = run_update(dev, pred[:2], label[:2], C, pcts, state=part)
    assert other.tolist() == whole.tolist()
    alone, _ = run_update(dev, pred[3:4], label[3:4], C, pcts)
    assert alone[0].tolist() == rec[3].tolist()


# ---- the Python surface ------------------------------------------------------------------------------------------------------------
def test_segment_meter_on_strided_views():
    dev = _dev()
    P = pkg()
    seed, batch, frames, C = R.SEEDED[2]
    pred, label = R.make_batch(seed, batch, frames, C)
    pcts = (10, 25, 50)
    want_rec, want_state = R.evaluate(pred, label, C, pcts, distance=R.levenshtein_diagonals)
    wide_p = torch.full((batch, frames + 5), C - 1, dtype=torch.int64, device=dev)
    wide_l = torch.zeros((batch, frames + 9), dtype=torch.int64, device=dev)
    wide_p[:, :frames] = torch.from_numpy(pred).to(dev)
    wide_l[:, 4:4 + frames] = torch.from_numpy(label).to(dev)
    vp, vl = wide_p[:, :frames], wide_l[:, 4:4 + frames]
    assert not vp.is_contiguous() and vp.stride(0) == frames + 5 and vl.stride(0) == frames + 9

    meter = P.SegmentMeter(C, dev, thresholds=pcts)
    assert meter.update(vp, vl) is None
    assert meter.state.cpu().tolist() == want_state.tolist()
    got = meter.result()
    ref = R.report(want_state, pcts)
    for key in ("edit", "edit_micro", "frame_accuracy", "over_segmentation", "precision", "recall", "f1"):
        assert got[key] == ref[key], key
    assert got["videos"] == batch and got["videos_overflow"] == 0 and got["videos_empty"] == 0
    assert got["tp"] == dict(zip(pcts, want_state[R.STATE:].tolist())) and 0.0 < got["f1"][50] <= got["f1"][10] <= 100.0

    # two meters over a split, merged; records=True; lengths; reset
    a, b = P.SegmentMeter(C, dev, thresholds=pcts), P.SegmentMeter(C, dev, thresholds=pcts)
    rec_a = a.update(vp[:2], vl[:2], records=True)
    rec_b = b.update(vp[2:], vl[2:], records=True)
    assert rec_a.device == dev and torch.cat([rec_a, rec_b]).cpu().tolist() == want_rec.tolist()
    assert a.merge(b).state.cpu().tolist() == want_state.tolist()
    lengths = [0, frames, 17, frames + 3, -1]
    want_len = R.evaluate(pred, label, C, pcts, lengths, distance=R.levenshtein_diagonals)
    assert a.reset().state.cpu().tolist() == [0] * (R.STATE + 3)
    rec = a.update(vp, vl, lengths=torch.tensor(lengths, dtype=torch.int32, device=dev), records=True)
    assert rec.cpu().tolist() == want_len[0].tolist() and a.state.cpu().tolist() == want_len[1].tolist()
    assert a.result()["videos_empty"] == 2
    # a column view (stride 2 along frames) is copied, not misread
    every = torch.stack([torch.from_numpy(pred).to(dev), torch.from_numpy(label).to(dev)], dim=2)
    a.reset().update(every[:, :, 0], every[:, :, 1])
    assert a.state.cpu().tolist() == want_state.tolist()
    for bad in (vp.cpu(), vp.int(), vp[:, :-1], vp[0]):
        with pytest.raises(P.QtError):
            a.update(bad, vl)
    with pytest.raises(P.QtError):
        a.update(vp, vl, lengths=torch.zeros(batch, dtype=torch.int64, device=dev))
    with pytest.raises(P.QtError):
        a.merge(P.SegmentMeter(C, dev, thresholds=(50,)))
    assert a.state.cpu().tolist() == want_state.tolist()            # a refused call counts nothing


def test_segment_runs_equals_the_walk():
    dev = _dev()
    P = pkg()
    C = 3
    values = run_videos(513)
    B, T = values.shape
    wide = torch.zeros((B, T + 7), dtype=torch.int64, device=dev)
    wide[:, 2:2 + T] = torch.from_numpy(np.array(values)).to(dev)
    view = wide[:, 2:2 + T]
    runs, counts = P.segment_runs(view, C)
    want_runs, want_counts = R.encode(values, C)
    assert runs.dtype == torch.int32 and tuple(runs.shape) == (B, T, 3) and counts.cpu().tolist() == want_counts.tolist()
    got = runs.cpu().numpy()
    for b in range(B):                                           # records at and behind the count are not written
        assert got[b, :want_counts[b]].tolist() == want_runs[b, :want_counts[b]].tolist()
    lengths = [0, T, -2, T + 7, T // 2, TRIP, T - 1]
    runs, counts = P.segment_runs(view, C, lengths=torch.tensor(lengths, dtype=torch.int32, device=dev), capacity=4)
    want_runs, want_counts = R.encode(values, C, lengths, 4)
    assert counts.cpu().tolist() == want_counts.tolist()
    got = runs.cpu().numpy()
    for b in range(B):
        k = min(4, want_counts[b])
        assert got[b, :k].tolist() == want_runs[b, :k].tolist()
    runs, counts = P.segment_runs(view, C, capacity=0)
    assert tuple(runs.shape) == (B, 0, 3) and counts.cpu().tolist() == R.encode(values, C)[1].tolist()
