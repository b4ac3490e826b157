"""Segment-level evaluation, the parts that need no GPU: hand-worked videos with every number written out, the two statements
of tests/_segments_ref.py against each other, the seeded batches of the GPU tests (no overflow, no empty video, a few hundred
runs at most), the C ABI's declaration and every host-side refusal (pointers that are never dereferenced), the module's
argument checks, the report's arithmetic, the exports."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _segments_ref as R
from _util import PKG, ROOT, pkg

QT_ERR_INVALID_ARG, QT_ERR_UNSUPPORTED = -1, -3
I64 = lambda *v: np.array(v, np.int64)


# ---- hand-worked videos ----------------------------------------------------------------------------------------------------------
def test_one_late_boundary_by_hand():
    label, pred = I64(0, 0, 0, 1, 1, 2), I64(0, 0, 1, 1, 1, 2)
    assert R.runs(pred, 3) == [(0, 2, 0), (2, 3, 1), (5, 1, 2)] and R.runs(label, 3) == [(0, 3, 0), (3, 2, 1), (5, 1, 2)]
    # IoU 2/3, 2/3 and 1/1: all three pass up to 66 per cent (200 >= 198), only the last from 67 (200 < 201)
    assert R.video(pred, label, 3, (10, 25, 50, 66, 67, 100)) == [3, 3, 0, 6, 5, 3, 3, 3, 3, 1, 1]
    _, state = R.evaluate(pred[None], label[None], 3, (50, 67))
    assert state.tolist() == [1, 0, 0, 3, 3, 0, 3, 1 << 32, 6, 5, 3, 1]
    rep = R.report(state, (50, 67))
    assert rep["edit"] == 100.0 and rep["edit_micro"] == 100.0 and rep["f1"] == {50: 100.0, 67: 100.0 * (2 / 6)}
    assert rep["frame_accuracy"] == 5 / 6 and rep["over_segmentation"] == 1.0


def test_a_hold_in_three_fragments_by_hand():
    label = I64(*[0] * 11)
    pred = I64(0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0)
    assert R.runs(pred, 2) == [(0, 3, 0), (4, 3, 0), (8, 3, 0)] and R.runs(label, 2) == [(0, 11, 0)]
    # three predicted runs, one partner, IoU 3/11 each: it counts once at 10 and 25 (300 >= 275), not at 28 (300 < 308)
    assert R.video(pred, label, 2, (10, 25, 27, 28, 50)) == [3, 1, 2, 11, 9, 1, 1, 1, 0, 0]
    _, state = R.evaluate(pred[None], label[None], 2, (25, 50))
    assert state.tolist() == [1, 0, 0, 3, 1, 2, 3, (1 << 32) // 3, 11, 9, 1, 0]
    assert (1 << 32) // 3 == 1431655765
    rep = R.report(state, (25, 50))
    assert rep["edit"] == 100.0 * (1431655765 / (1 << 32)) and rep["edit_micro"] == 100.0 * (1 - 2 / 3)
    assert rep["precision"][25] == 100.0 * (1 / 3) and rep["recall"][25] == 100.0 and rep["f1"][25] == 50.0 and rep["f1"][50] == 0.0
    assert rep["over_segmentation"] == 3.0


def test_a_tie_goes_to_the_lower_index_and_equality_passes_by_hand():
    # one predicted run across two true runs of its class, IoU 1/5 with each: the partner is the first
    label, pred = I64(1, 1, -1, -1, 1, 1), I64(-1, 1, 1, 1, 1, -1)
    P, Y = R.runs(pred, 2), R.runs(label, 2)
    assert P == [(1, 4, 1)] and Y == [(0, 2, 1), (4, 2, 1)]
    assert R.partner(P[0], Y) == (0, 1, 5)
    # 100 * 1 == 20 * 5 exactly: passes at 20, not at 21
    assert R.video(pred, label, 2, (20, 21)) == [1, 2, 1, 4, 2, 1, 0]
    _, state = R.evaluate(pred[None], label[None], 2, (20, 21))
    assert state.tolist() == [1, 0, 0, 1, 2, 1, 2, 1 << 31, 4, 2, 1, 0]
    # the tie seen in a count: the straddling run (IoU 1/6 with both) and a second run (IoU 1/3) share true run 0, so tp = 1;
    # a tie that went to the higher index would give 2
    label, pred = I64(1, 1, 1, -1, -1, 1, 1, 1), I64(1, -1, 1, 1, 1, 1, -1, -1)
    P, Y = R.runs(pred, 2), R.runs(label, 2)
    assert P == [(0, 1, 1), (2, 4, 1)] and Y == [(0, 3, 1), (5, 3, 1)]
    assert R.partner(P[1], Y) == (0, 1, 6) and R.partner(P[0], Y) == (0, 1, 3)
    assert R.video(pred, label, 2, (10, 16, 17, 33, 34)) == [2, 2, 0, 6, 3, 1, 1, 1, 1, 0]
    assert [R.published_counts(P, Y, pct) for pct in (10, 17, 34)] == [(1, 1, 1), (1, 1, 1), (0, 2, 2)]


def test_gaps_unknowns_lengths_and_empty_videos_by_hand():
    C = 3
    # unknown values are a gap: two runs of one class around it; no partner without a run of the class
    label, pred = I64(2, 2, 3, 2, 1 << 40, -1), I64(0, 0, 0, 0, 0, 0)
    assert R.runs(label, C) == [(0, 2, 2), (3, 1, 2)] and R.video(pred, label, C, (1,)) == [1, 2, 2, 3, 0, 0]
    # an all-unknown video is empty: it adds to videos_empty and to no edit sum; a label-less video has no labelled frame
    rec, state = R.evaluate(I64(-1, 7, 3)[None], I64(3, 3, -5)[None], C, (50,))
    assert rec.tolist() == [[0, 0, 0, 0, 0, 0]] and state.tolist() == [1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    # lengths: clamped to 0 .. frames, frames beyond them are not looked at
    pred, label = np.stack([I64(0, 1, 2, 0)] * 4), np.stack([I64(0, 1, 1, 0)] * 4)
    rec, state = R.evaluate(pred, label, C, (50,), lengths=[-3, 2, 4, 9])
    assert rec.tolist() == [[0, 0, 0, 0, 0, 0], [2, 2, 0, 2, 2, 2], [4, 3, 1, 4, 3, 3], [4, 3, 1, 4, 3, 3]]
    assert state.tolist() == [4, 0, 1, 10, 8, 2, 10, (1 << 32) + 2 * ((3 << 32) // 4), 10, 8, 8]
    runs, counts = R.encode(pred, C, lengths=[-3, 2, 4, 9], capacity=3)
    assert counts.tolist() == [0, 2, 4, 4] and runs[2].tolist() == [[0, 1, 0], [1, 1, 1], [2, 1, 2]]
    assert runs[1].tolist() == [[0, 1, 0], [1, 1, 1], [-1, -1, -1]]


def test_overflow_by_hand():
    many = R.frames_of([k % 2 for k in range(R.MAX_SEGMENTS + 1)])
    few = R.frames_of([0], len(many), run=5)
    rec, state = R.evaluate(np.stack([many, few, few]), np.stack([few, few, many]), 2, (10, 50), distance=R.levenshtein_diagonals)
    assert rec[0].tolist() == [1025, 1, -1, 5, 3, -1, -1] and rec[2].tolist() == [1, 1025, -1, 1025, 3, -1, -1]
    assert rec[1].tolist() == [1, 1, 0, 5, 5, 1, 1]
    assert state.tolist() == [3, 2, 0, 1, 1, 0, 1, 1 << 32, 1035, 11, 1, 1]
    # exactly the cap is no overflow
    full = R.frames_of([k % 2 for k in range(R.MAX_SEGMENTS)])
    rec = R.video(full, full, 2, (50,), distance=R.levenshtein_diagonals)
    assert rec == [1024, 1024, 0, 1024, 1024, 1024]


# ---- the two statements ----------------------------------------------------------------------------------------------------------
def test_the_two_statements_agree():
    """a few thousand seeded pairs: the full table against the anti-diagonals, the distinct-partner count against the
    published claim-the-partner loop at 1, 10, 25, 50 and 100 per cent"""
    pcts = (1, 10, 25, 50, 100)
    rng = np.random.default_rng(7)
    seen_shared = seen_fp = 0
    for seed in range(3000):
        frames, C = int(rng.integers(1, 48)), int(rng.integers(1, 5))
        pred, label = R.make_pair(seed, frames, C, mean_run=int(rng.integers(1, 8)), flicker=0.1, unknown=0.05)
        if seed % 7 == 0:
            pred = label.copy()                                    # identical videos: every IoU is 1
        P, Y = R.runs(pred, C), R.runs(label, C)
        p, y = [r[2] for r in P], [r[2] for r in Y]
        assert R.levenshtein(p, y) == R.levenshtein_diagonals(p, y), seed
        tp = R.true_positives(P, Y, pcts)
        for k, pct in enumerate(pcts):
            assert R.published_counts(P, Y, pct) == (tp[k], len(P) - tp[k], len(Y) - tp[k]), (seed, pct)
        passing = sum(1 for r in P if (b := R.partner(r, Y)) is not None and 100 * b[1] >= 10 * b[2])
        seen_shared += passing > tp[1]
        seen_fp += tp[3] < len(P)
    assert seen_shared > 100 and seen_fp > 1000                   # partners are shared and runs do fail: the check has teeth


def test_levenshtein_known_values():
    for p, y, d in (("", "", 0), ("", "abc", 3), ("abc", "", 3), ("kitten", "sitting", 3), ("flaw", "lawn", 2),
                    ("abcabc", "abcabc", 0), ("aaaa", "bbbbbb", 6), ("aabbaa", "aba", 3)):
        p, y = [ord(c) for c in p], [ord(c) for c in y]
        assert R.levenshtein(p, y) == d and R.levenshtein_diagonals(p, y) == d, (p, y)


def test_the_seeded_batches_leave_nothing_out():
    """what the GPU tests rely on, asserted on the reference alone"""
    for seed, batch, frames, C in R.SEEDED:
        pred, label = R.make_batch(seed, batch, frames, C)
        rec, state = R.evaluate(pred, label, C, (10, 25, 50), distance=R.levenshtein_diagonals)
        assert state[R.OVERFLOW] == 0 and state[R.EMPTY] == 0 and state[R.VIDEOS] == batch
        assert rec[:, :2].max() <= 400 and rec[:, 1].min() >= 1 and rec[:, 3].min() >= 1
        assert 0 <= label[:, 0].min() and label[:, 0].max() < C
        assert (pred < 0).any() and (pred >= C).any()              # unknown frames of both kinds are there


# ---- header, module, library -----------------------------------------------------------------------------------------------------
def test_constants_are_the_kernels_and_the_modules():
    M = pkg("segments")
    assert (M.MAX_SEGMENTS, M.MAX_CLASSES, M.MAX_THRESHOLDS, M.RECORD, M.STATE, M.MAX_FRAMES, M.EDIT_ONE) == \
        (R.MAX_SEGMENTS, R.MAX_CLASSES, R.MAX_THRESHOLDS, R.RECORD, R.STATE, R.MAX_FRAMES, R.EDIT_ONE)
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    define = lambda name: int(re.search(rf"#define {name} (\d+)", header).group(1))
    assert (define("QT_SEGMENTS_MAX"), define("QT_SEGMENTS_MAX_CLASSES"), define("QT_SEGMENTS_MAX_THRESHOLDS"),
            define("QT_SEGMENTS_RECORD"), define("QT_SEGMENTS_STATE")) == (M.MAX_SEGMENTS, M.MAX_CLASSES, M.MAX_THRESHOLDS, M.RECORD,
                                                                            M.STATE)
    assert len(M.STATE_FIELDS) == M.STATE and len(M.RECORD_FIELDS) == M.RECORD
    src = open(os.path.join(ROOT, PKG, "csrc", "segments.hip")).read()
    const = lambda name: int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))
    assert const("SG_THREADS") == const("SG_TRIP") == R.TRIP


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    declared = set(re.findall(r"\b(qt_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(os.path.join(ROOT, PKG, "libqtcnn_hip.so"))
    for symbol in ("qt_segments_workspace_bytes", "qt_segments_update", "qt_segments_encode"):
        assert symbol in declared and hasattr(lib, symbol), symbol
    M = pkg("segments")
    fields = re.search(r"typedef struct qt_segments_desc \{(.*?)\} qt_segments_desc;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields)
    got = [(name, int(dim) if dim else None) for name, dim in re.findall(r"^\s*int\s+(\w+)(?:\[(\d+)\])?;", fields, re.M)]
    assert len(got) == len(re.findall(r";", fields))               # every field is an int or an array of them
    want = [(n, t._length_ if hasattr(t, "_length_") else None) for n, t in M.SegmentsDesc._fields_]
    assert got == want
    for _, t in M.SegmentsDesc._fields_:
        assert (t._type_ if hasattr(t, "_length_") else t) is ctypes.c_int
    assert ctypes.sizeof(M.SegmentsDesc) == 4 * (4 + 8 + 1) and M.SegmentsDesc.pct.offset == 16 and M.SegmentsDesc.capacity.offset == 48
    P = pkg()
    assert P.SegmentMeter is M.SegmentMeter and P.segment_runs is M.segment_runs
    assert "SegmentMeter" in P.__all__ and "segment_runs" in P.__all__


def _lib():
    M = pkg("segments")
    L = pkg("_lib").lib()
    return M, L


def _refused(L, rc, word, status=QT_ERR_INVALID_ARG):
    assert rc == status and word in L.qt_last_error(), (rc, L.qt_last_error())


def test_update_argument_checks_need_no_device():
    """every refusal comes before the first device call: the pointers are never dereferenced"""
    M, L = _lib()
    D = lambda batch=4, frames=100, C=12, pcts=(10, 25, 50): M.make_desc(batch, frames, C, pcts)
    pred, label, lengths, state, records, work = (0x10000000 * k for k in range(1, 7))
    good = dict(pred=pred, ld_pred=100, label=label, ld_label=100, lengths=lengths, state=state, records=records, work=work,
                bytes=4 * 8 * 8)

    def call(desc, **kw):
        a = {**good, **kw}
        return L.qt_segments_update(ctypes.byref(desc), a["pred"], a["ld_pred"], a["label"], a["ld_label"], a["lengths"], a["state"],
                                    a["records"], a["work"], a["bytes"], None)

    assert L.qt_segments_workspace_bytes(ctypes.byref(D())) == 4 * 8 * 8
    assert L.qt_segments_workspace_bytes(ctypes.byref(D(batch=7, pcts=(50,)))) == 7 * 6 * 8
    _refused(L, L.qt_segments_update(None, pred, 100, label, 100, lengths, state, records, work, 256, None), b"null descriptor")
    for batch in (0, -3):
        _refused(L, call(D(batch=batch)), b"batch")
    _refused(L, call(D(frames=-1), ld_pred=0, ld_label=0), b"frames")
    for C in (0, -1, 1025):
        _refused(L, call(D(C=C)), b"num_classes")
    desc = D()
    for K in (0, -1, 9):
        desc.num_thresholds = K
        _refused(L, call(desc), b"num_thresholds")
    for pct in (0, -5, 101):
        _refused(L, call(D(pcts=(10, pct, 50))), b"pct[1]")
    desc = D(pcts=(10,))
    desc.pct[1] = 1000                                              # beyond K: not read
    _refused(L, call(desc, state=None), b"null state")
    _refused(L, call(D(), ld_pred=99), b"ld_pred")
    _refused(L, call(D(), ld_label=99), b"ld_label")
    for name in ("pred", "label", "state"):
        _refused(L, call(D(), **{name: None}), b"null " + name.encode())
    _refused(L, call(D(), work=None), b"null workspace")
    for name, off in (("pred", 4), ("label", 4), ("state", 4), ("records", 4), ("work", 4), ("lengths", 2)):
        _refused(L, call(D(), **{name: good[name] + off}), b"aligned")
    for nbytes in (0, 4 * 8 * 8 - 1):
        _refused(L, call(D(), bytes=nbytes), b"workspace")
    _refused(L, call(D(batch=1 << 12, frames=(1 << 10) + 1), ld_pred=2000, ld_label=2000, bytes=1 << 30), b"frames", QT_ERR_UNSUPPORTED)
    _refused(L, call(D(batch=1, frames=(1 << 22) + 1), ld_pred=1 << 23, ld_label=1 << 23), b"frames", QT_ERR_UNSUPPORTED)


def test_encode_argument_checks_need_no_device():
    M, L = _lib()
    D = lambda batch=4, frames=100, C=12, capacity=16: M.make_desc(batch, frames, C, capacity=capacity)
    values, lengths, runs, counts = (0x10000000 * k for k in range(1, 5))
    good = dict(values=values, ld=100, lengths=lengths, runs=runs, counts=counts)

    def call(desc, **kw):
        a = {**good, **kw}
        return L.qt_segments_encode(ctypes.byref(desc), a["values"], a["ld"], a["lengths"], a["runs"], a["counts"], None)

    _refused(L, L.qt_segments_encode(None, values, 100, lengths, runs, counts, None), b"null descriptor")
    for batch in (0, -3):
        _refused(L, call(D(batch=batch)), b"batch")
    _refused(L, call(D(frames=-1)), b"frames")
    for C in (0, -1, 1025):
        _refused(L, call(D(C=C)), b"num_classes")
    _refused(L, call(D(capacity=-1)), b"capacity")
    _refused(L, call(D(), ld=99), b"ld")
    _refused(L, call(D(), values=None), b"null values")
    _refused(L, call(D(), counts=None), b"null counts")
    _refused(L, call(D(), runs=None), b"null runs")
    for name, off in (("values", 4), ("lengths", 2), ("runs", 2), ("counts", 1)):
        _refused(L, call(D(), **{name: good[name] + off}), b"aligned")
    _refused(L, call(D(batch=1 << 12, frames=(1 << 10) + 1), ld=2000), b"frames", QT_ERR_UNSUPPORTED)
    # the thresholds are update's business: encode does not read them
    desc = D(batch=0)
    desc.num_thresholds = 0
    _refused(L, call(desc), b"batch")


def test_module_argument_checks_need_no_device():
    P = pkg()
    for bad in (dict(num_classes=0), dict(num_classes=1025), dict(num_classes=12.0), dict(num_classes=True), dict(thresholds=()),
                dict(thresholds=(0,)), dict(thresholds=(101,)), dict(thresholds=(10, 25.0)), dict(thresholds=(True,)),
                dict(thresholds=tuple(range(1, 10))), dict(thresholds=50)):
        with pytest.raises(ValueError):
            P.SegmentMeter(**{"num_classes": 12, "device": "cuda:0", **bad})
    # no torch fallback
    with pytest.raises(P.QtError, match="AMD GPU"):
        P.SegmentMeter(12, "cpu")
    with pytest.raises(P.QtError, match="no CPU or torch fallback"):
        P.segment_runs(torch.zeros(2, 5, dtype=torch.int64), 12)
    with pytest.raises(P.QtError, match="tensor"):
        P.segment_runs([[0, 1]], 12)
    with pytest.raises(ValueError):
        P.segment_runs(torch.zeros(2, 5, dtype=torch.int64), 0)
    # update's own checks come before anything touches a device: a meter without one
    M = pkg("segments")
    meter = object.__new__(M.SegmentMeter)
    meter.num_classes, meter.thresholds, meter.device = 12, (50,), torch.device("cuda:0")
    with pytest.raises(P.QtError, match="no CPU or torch fallback"):
        meter.update(torch.zeros(2, 5, dtype=torch.int64), torch.zeros(2, 5, dtype=torch.int64))
    with pytest.raises(P.QtError, match="tensor"):
        meter.update(None, None)


def test_report_arithmetic_on_a_hand_filled_state():
    M = pkg("segments")
    #        videos ovf empty seg_p seg_t dist max  edit_q               lab  cor  tp10 tp50
    state = [10,    2,  3,    40,   30,   12,  48,  3 * (1 << 32) + (1 << 31), 200, 150, 24, 9]
    r = M.report(state, (10, 50))
    assert r["edit"] == 100.0 * (3.5 / 5) and r["edit_micro"] == 100.0 * (1 - 12 / 48)
    assert r["precision"] == {10: 100.0 * (24 / 40), 50: 100.0 * (9 / 40)} and r["recall"] == {10: 100.0 * (24 / 30), 50: 100.0 * (9 / 30)}
    assert r["f1"] == {10: 100.0 * (48 / 70), 50: 100.0 * (18 / 70)}
    assert r["tp"] == {10: 24, 50: 9} and r["fp"] == {10: 16, 50: 31} and r["fn"] == {10: 6, 50: 21}
    assert r["frame_accuracy"] == 0.75 and r["over_segmentation"] == 40 / 30
    assert [r[k] for k in M.STATE_FIELDS] == state[:10] and r["thresholds"] == (10, 50)
    ref = R.report(state, (10, 50))
    for key in ("edit", "edit_micro", "frame_accuracy", "over_segmentation", "precision", "recall", "f1"):
        assert r[key] == ref[key], key
    # zero denominators give 0.0
    z = M.report([0] * 11, (25,))
    assert (z["edit"], z["edit_micro"], z["frame_accuracy"], z["over_segmentation"]) == (0.0, 0.0, 0.0, 0.0)
    assert z["precision"] == {25: 0.0} and z["recall"] == {25: 0.0} and z["f1"] == {25: 0.0}
    # only overflowing and empty videos: nothing is scored
    z = M.report([3, 1, 2, 0, 0, 0, 0, 0, 7, 0, 0], (25,))
    assert z["edit"] == 0.0 and z["frame_accuracy"] == 0.0
    # predicted runs without true ones
    z = M.report([1, 0, 0, 4, 0, 4, 4, 0, 0, 0, 0], (25,))
    assert z["over_segmentation"] == 0.0 and z["recall"][25] == 0.0 and z["precision"][25] == 0.0 and z["edit_micro"] == 0.0
    with pytest.raises(ValueError):
        M.report([0] * 12, (25,))


def test_the_documents_speak_of_the_meter():
    for doc, word in (("DESIGN.md", "qt_segments_update"), ("INTEGRATION.md", "SegmentMeter("), ("README.md", "segments.py"),
                      ("EXPERIMENTS.md", "bench_segments.py")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc
