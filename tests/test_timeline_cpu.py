"""Pose timeline, the parts that need no GPU: the plain loops of tests/_timeline_ref.py against themselves for every split of a
stream into two and three calls, their array form against the loops, hand-written cases of the debounce and of q, the C ABI's
declaration and every host-side refusal (pointers that are never dereferenced), the module's argument checks, the exports."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import _timeline_ref as R
from _util import PKG, ROOT, pkg

QT_ERR_INVALID_ARG, QT_ERR_UNSUPPORTED = -1, -3
F32 = np.float32


def _run_split(probs, pred_conf, cuts, W, C, min_run, min_conf, capacity):
    """smooth + decode over consecutive calls cut at `cuts`; decode runs on the given (pred, conf), not on smooth's"""
    B, T = probs.shape[:2]
    hist, count = None, None
    state, segments = np.zeros((B, R.STATE), np.int64), np.full((B, capacity, 4), -7, np.int64)
    parts = []
    for a, b in zip([0] + cuts, cuts + [T]):
        sm, pr, cf, hist, count = R.smooth(probs[:, a:b], W, hist, count)
        stable, state, segments = R.decode(pred_conf[0][:, a:b], pred_conf[1][:, a:b], C, min_run, min_conf, state, segments,
                                           flush=(b == T))
        parts.append((sm, pr, cf, stable))
    joined = [np.concatenate([p[i] for p in parts], axis=1) for i in range(4)]
    return joined + [hist, count, state, segments]


def test_every_split_of_a_stream_gives_the_bits_of_one_call():
    T, C, W = 40, 2, 4
    probs = R.make_probs(3, 1, T, C)
    probs[0, 7] = np.nan
    probs[0, 20] = np.inf
    labels = R.make_labels(4, 1, T, C, run=6)
    whole = _run_split(probs, labels, [], W, C, 3, 0.5, 16)
    assert whole[6][:, R.TOTAL].min() >= 3                       # there is something to compare
    cuts = [[a] for a in range(1, T)] + [[a, b] for a, b in itertools.combinations(range(1, T), 2)]
    assert len(cuts) == 39 + 741
    for cut in cuts:
        got = _run_split(probs, labels, cut, W, C, 3, 0.5, 16)
        for name, w, g in zip(("smoothed", "pred", "confidence", "stable", "hist", "count", "state", "segments"), whole, got):
            assert R.bits(w) == R.bits(g), (cut, name)


def test_array_form_equals_the_loop():
    for seed, (B, T, C, W) in enumerate([(1, 1, 1, 1), (2, 7, 3, 1), (3, 9, 12, 5), (1, 4, 13, 8), (2, R.TILE + 3, 5, 7),
                                         (1, 70, 17, 64), (2, 3, 2, 64)]):
        probs = R.make_probs(10 + seed, B, T, C)
        probs[0, T // 2] = np.nan                               # a NaN row, an inf row, exact ties
        probs[-1, T // 3] = np.inf
        probs[0, 0] = F32(0.25)
        probs[0, T - 1, C // 2:] = probs[0, T - 1, C // 2]
        for hist, count in ((None, None), (R.make_probs(20 + seed, B, max(W - 1, 1), C)[:, :W - 1],
                                           np.array([0, W + 3, 1][:B], np.int32))):
            want, got = R.smooth(probs, W, hist, count), R.smooth_vectorised(probs, W, hist, count)
            for name, w, g in zip(("smoothed", "pred", "confidence", "hist_out", "count"), want, got):
                assert w.dtype == g.dtype and R.bits(w) == R.bits(g), (B, T, C, W, name)
            assert T < 4 or (np.isnan(want[0]).any() and np.isinf(want[0]).any())
    # the NaN is the stated one, a window of one is the input itself, -0.0 included
    p = np.array([[[-0.0, np.nan, 0.5]]], F32)
    out, pred, conf, _, _ = R.smooth(p, 1)
    assert R.bits(out[0, 0, [0, 2]]) == R.bits(p[0, 0, [0, 2]]) and out.view(np.uint32)[0, 0, 1] == 0x7FC00000
    assert pred[0, 0] == 1 and conf.view(np.uint32)[0, 0] == 0x7FC00000


def test_smooth_rule_by_hand():
    p = np.array([[[1, 0], [0, 1], [0, 1], [0.5, 0.5], [0, 1]]], F32)
    out, pred, conf, hist, count = R.smooth(p, 3)
    assert out[0].tolist() == [[1, 0], [0.5, 0.5], [F32(1) / F32(3), F32(2) / F32(3)], [F32(0.5) / F32(3), F32(2.5) / F32(3)],
                               [F32(0.5) / F32(3), F32(2.5) / F32(3)]]
    assert pred[0].tolist() == [0, 0, 1, 1, 1]                   # the tie of frame 1 goes to the lower index
    assert conf[0].tolist() == [1, 0.5, F32(2) / F32(3), F32(2.5) / F32(3), F32(2.5) / F32(3)]
    assert hist[0].tolist() == [[0, 1], [0.5, 0.5]] and count.tolist() == [2]
    # the order of the adds matters, and it is oldest first: (1e8 + 1) - 1e8 is 0 in f32, 1e8 - 1e8 + 1 is 1
    p = np.array([[[1e8], [1.0], [-1e8]]], F32)
    assert R.smooth(p, 3)[0][0, 2, 0] == F32(0) and R.smooth(p[:, ::-1], 3)[0][0, 2, 0] == F32(0)
    p = np.array([[[1e8], [-1e8], [1.0]]], F32)
    assert R.smooth(p, 3)[0][0, 2, 0] == F32(1) / F32(3)
    # a NaN row reaches exactly the W frames that read it
    p = R.make_probs(1, 1, 12, 3)
    p[0, 4] = np.nan
    assert np.isnan(R.smooth(p, 3)[0][0]).all(axis=1).tolist() == [4 <= f < 7 for f in range(12)]


def _decode1(pred, conf, min_run, min_conf=0.5, C=4, capacity=8, flush=True, state=None, segments=None):
    state = np.zeros((1, R.STATE), np.int64) if state is None else state
    segments = np.full((1, capacity, 4), -7, np.int64) if segments is None else segments
    return R.decode(np.array([pred], np.int64), np.array([conf], F32), C, min_run, min_conf, state, segments, flush=flush)


def test_debounce_by_hand():
    hi = 0.75
    # min_run 1: stable is the gated class itself; one segment per run of it
    stable, state, seg = _decode1([2, 2, 3, 3, 3, 1], [hi] * 6, 1)
    assert stable[0].tolist() == [2, 2, 3, 3, 3, 1]
    assert R.segment_list(state, seg) == [(0, 2, 2, hi), (2, 3, 3, hi), (5, 1, 1, hi)]
    # min_run 3: nothing before the third frame in a row; a flicker shorter than min_run leaves stable alone
    stable, state, seg = _decode1([2, 2, 2, 2, 0, 0, 2, 2, 1, 1, 1, 1], [hi] * 12, 3)
    assert stable[0].tolist() == [-1, -1, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1]
    assert R.segment_list(state, seg) == [(2, 8, 2, hi), (10, 2, 1, hi)]
    assert seg[0, 2:].tolist() == [[-7] * 4] * 6                 # records behind the total are not written
    # min_run unknown frames (low confidence, a class outside [0, C), a NaN confidence) end the segment: a gap
    stable, state, seg = _decode1([1, 1, 1, 1, 9, 1, 1, 1, 1, 1], [hi, hi, hi, 0.25, hi, np.nan, hi, hi, hi, hi], 3)
    assert stable[0].tolist() == [-1, -1, 1, 1, 1, -1, -1, -1, 1, 1]
    assert [s[:3] for s in R.segment_list(state, seg)] == [(2, 3, 1), (8, 2, 1)]
    assert seg[0, 0, 3] == 2 * R.q(hi) + R.q(0.25)              # a frame of the segment counts with its own confidence
    # fewer than min_run unknown frames do not
    stable, _, _ = _decode1([1, 1, 1, 9, 9, 1], [hi] * 6, 3)
    assert stable[0].tolist() == [-1, -1, 1, 1, 1, 1]
    # without flush the open segment stays open, and a second flush adds nothing
    stable, state, seg = _decode1([1, 1, 1], [hi] * 3, 2, flush=False)
    assert state[0].tolist() == [3, 2, 2, 3, 1, 2, 2 * R.q(hi), 0] and seg[0, 0].tolist() == [-7] * 4
    _, state, seg = R.decode(np.zeros((1, 0), np.int64), np.zeros((1, 0), F32), 4, 2, 0.5, state, seg, flush=True)
    assert state[0].tolist() == [3, 2, 2, 3, 3, 0, 0, 1] and seg[0, 0].tolist() == [1, 2, 1, 2 * R.q(hi)]
    _, again, seg2 = R.decode(np.zeros((1, 0), np.int64), np.zeros((1, 0), F32), 4, 2, 0.5, state, seg, flush=True)
    assert again.tolist() == state.tolist() and R.bits(seg2) == R.bits(seg)
    # after a flush the label stays; frames that go on with it are a new segment from their own number
    _, state, seg = _decode1([1, 1, 0], [hi] * 3, 2, flush=True, state=state, segments=seg)
    assert R.segment_list(state, seg) == [(1, 2, 1, hi), (3, 3, 1, hi)]
    # capacity below the count: the first records, the full total
    _, state, seg = _decode1([0, 1, 2, 3, 0, 1], [hi] * 6, 1, capacity=2)
    assert state[0, R.TOTAL] == 6 and seg[0].tolist() == [[0, 1, 0, R.q(hi)], [1, 1, 1, R.q(hi)]]
    # the run saturates
    state = np.array([[5, 2, 2, R.RUN_MAX - 1, 0, 5, 0, 0]], np.int64)
    _, state, _ = _decode1([1, 1, 1], [hi] * 3, 2, state=state, flush=False)
    assert state[0, R.RUN] == R.RUN_MAX


def test_q():
    assert [R.q(x) for x in (0.0, 1.0, 1.5, np.inf, -0.25, -np.inf, np.nan, -0.0)] == [0, 65536, 65536, 65536, 0, 0, 0, 0]
    assert R.q(0.5) == 32768 and R.q(F32(1) / F32(65536)) == 1 and R.q(F32(1.5) / F32(65536)) == 2 and R.q(F32(2.5) / F32(65536)) == 2
    assert R.q(np.nextafter(F32(1), F32(0))) == 65536            # rint of 65535.996


def test_constants_are_the_kernels_and_the_modules():
    M = pkg("timeline")
    assert (M.TILE, M.TRIP, M.MAX_WINDOW, M.MAX_CLASSES, M.STATE, M.MAX_FRAMES, M.CONF_ONE) == \
        (R.TILE, R.TRIP, R.MAX_WINDOW, R.MAX_CLASSES, R.STATE, R.MAX_FRAMES, R.CONF_ONE)
    src = open(os.path.join(ROOT, PKG, "csrc", "timeline.hip")).read()
    const = lambda name: int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))
    assert (const("TL_TILE"), const("TL_TRIP"), const("TL_MAX_W"), const("TL_MAX_C")) == (R.TILE, R.TRIP, R.MAX_WINDOW, R.MAX_CLASSES)
    assert const("TL_AHEAD") == R.AHEAD
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    define = lambda name: int(re.search(rf"#define {name} (\d+)", header).group(1))
    assert (define("QT_TIMELINE_TILE"), define("QT_TIMELINE_TRIP"), define("QT_TIMELINE_MAX_WINDOW"),
            define("QT_TIMELINE_MAX_CLASSES"), define("QT_TIMELINE_STATE")) == (R.TILE, R.TRIP, R.MAX_WINDOW, R.MAX_CLASSES, R.STATE)
    assert len(M.STATE_FIELDS) == R.STATE
    assert (R.TILE + R.MAX_WINDOW - 1) * R.MAX_CLASSES * 4 <= 32 * 1024


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    declared = set(re.findall(r"\b(qt_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(os.path.join(ROOT, PKG, "libqtcnn_hip.so"))
    for symbol in ("qt_timeline_smooth", "qt_timeline_decode"):
        assert symbol in declared and hasattr(lib, symbol), symbol
    M = pkg("timeline")
    fields = re.search(r"typedef struct qt_timeline_desc \{(.*?)\} qt_timeline_desc;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields)
    assert re.findall(r"\b(\w+)\s*;", fields) == [n for n, _ in M.TimelineDesc._fields_]
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float}
    assert [ctype[t] for t, _ in re.findall(r"^\s*(int|float)\s+(\w+);", fields, re.M)] == [t for _, t in M.TimelineDesc._fields_]
    P = pkg()
    assert P.PoseTimeline is M.PoseTimeline and "PoseTimeline" in P.__all__


def _lib():
    M = pkg("timeline")
    L = pkg("_lib").lib()
    return M, L


def test_smooth_argument_checks_need_no_device():
    """every refusal comes before the first device call: the pointers are never dereferenced"""
    M, L = _lib()
    D = lambda batch=2, frames=100, C=12, W=15: M.TimelineDesc(batch, frames, C, W, 5, 0.5, 64, 0)
    probs, hin, cin, hout, cout, sm, pred, conf = (0x10000000 * k for k in range(1, 9))
    good = dict(probs=probs, ld=12, hin=hin, cin=cin, hout=hout, cout=cout, sm=sm, ld_s=12, pred=pred, conf=conf)

    def call(desc, **kw):
        a = {**good, **kw}
        return L.qt_timeline_smooth(ctypes.byref(desc), a["probs"], a["ld"], a["hin"], a["cin"], a["hout"], a["cout"], a["sm"],
                                    a["ld_s"], a["pred"], a["conf"], None)

    def refused(rc, word, status=QT_ERR_INVALID_ARG):
        assert rc == status and word in L.qt_last_error(), (rc, L.qt_last_error())

    refused(L.qt_timeline_smooth(None, probs, 12, hin, cin, hout, cout, sm, 12, pred, conf, None), b"null descriptor")
    for batch in (0, -3):
        refused(call(D(batch=batch)), b"batch")
    for frames in (-1, 0):
        refused(call(D(frames=frames)), b"frames")
    desc = D(frames=0)
    desc.flush = 1                                               # flush is decode's: zero frames stay refused here
    refused(call(desc), b"frames")
    for C in (0, -1, 65):
        refused(call(D(C=C), ld=70, ld_s=70), b"num_classes")
    for W in (0, -1, 65):
        refused(call(D(W=W)), b"window")
    refused(call(D(), ld=11), b"ld")
    refused(call(D(), ld_s=11), b"ld_smoothed")
    for name in ("probs", "pred", "conf"):
        refused(call(D(), **{name: None}), b"null")
    for name, off in (("probs", 2), ("sm", 1), ("conf", 3), ("pred", 4), ("hin", 2), ("hout", 1), ("cin", 2), ("cout", 3)):
        refused(call(D(), **{name: good[name] + off}), b"aligned")
    for half in ("hin", "cin", "hout", "cout"):
        refused(call(D(), **{half: None}), b"half a history pair")
    nbytes = 2 * 14 * 12 * 4
    refused(call(D(), hout=hin + nbytes - 4), b"overlap")
    refused(call(D(), hout=hin - nbytes + 4), b"overlap")
    refused(call(D(), cout=cin + 4), b"overlap")
    refused(call(D(), sm=probs + (200 * 12 - 1) * 4), b"overlap")
    refused(call(D(), sm=probs - (200 * 12 - 1) * 4), b"overlap")
    refused(call(D(), ld=16, sm=probs + (199 * 16 + 11) * 4), b"overlap")
    refused(call(D(batch=1 << 12, frames=(1 << 10) + 1)), b"frames", QT_ERR_UNSUPPORTED)
    refused(call(D(batch=1, frames=(1 << 22) + 1)), b"frames", QT_ERR_UNSUPPORTED)


def test_decode_argument_checks_need_no_device():
    M, L = _lib()

    def D(batch=2, frames=100, C=12, min_run=5, min_conf=0.5, capacity=64, flush=0):
        return M.TimelineDesc(batch, frames, C, 15, min_run, min_conf, capacity, flush)

    pred, conf, state, stable, seg = (0x10000000 * k for k in range(1, 6))
    good = dict(pred=pred, conf=conf, state=state, stable=stable, seg=seg)

    def call(desc, **kw):
        a = {**good, **kw}
        return L.qt_timeline_decode(ctypes.byref(desc), a["pred"], a["conf"], a["state"], a["stable"], a["seg"], None)

    def refused(rc, word, status=QT_ERR_INVALID_ARG):
        assert rc == status and word in L.qt_last_error(), (rc, L.qt_last_error())

    refused(L.qt_timeline_decode(None, pred, conf, state, stable, seg, None), b"null descriptor")
    for batch in (0, -3):
        refused(call(D(batch=batch)), b"batch")
    refused(call(D(frames=-1)), b"frames")
    refused(call(D(frames=-1, flush=1)), b"frames")
    refused(call(D(frames=0)), b"flush")
    for C in (0, -1, 65):
        refused(call(D(C=C)), b"num_classes")
    for min_run in (0, -2):
        refused(call(D(min_run=min_run)), b"min_run")
    refused(call(D(min_conf=float("nan"))), b"min_confidence")
    refused(call(D(capacity=-1)), b"capacity")
    refused(call(D(), seg=None), b"segments")
    for name in ("pred", "conf", "state", "stable"):
        refused(call(D(), **{name: None}), b"null")
    refused(call(D(frames=0, flush=1), state=None), b"null state")
    for name, off in (("pred", 4), ("conf", 2), ("state", 4), ("stable", 4), ("seg", 4)):
        refused(call(D(), **{name: good[name] + off}), b"aligned")
    refused(call(D(batch=1 << 12, frames=(1 << 10) + 1)), b"frames", QT_ERR_UNSUPPORTED)
    # a window outside 1 .. 64 is smooth's business: decode does not read it
    desc = D(batch=0)
    desc.window = 0
    refused(call(desc), b"batch")


def test_module_argument_checks_need_no_device():
    P = pkg()
    for bad in (dict(num_classes=0), dict(num_classes=65), dict(num_classes=12.0), dict(num_classes=True), dict(streams=0),
                dict(window=0), dict(window=65), dict(min_run=0), dict(capacity=-1), dict(min_confidence=float("nan")),
                dict(class_names=["a", "b"])):
        with pytest.raises(ValueError):
            P.PoseTimeline(**{"num_classes": 12, "device": "cuda:0", **bad})
    # no torch fallback
    with pytest.raises(P.QtError, match="AMD GPU"):
        P.PoseTimeline(12, "cpu")


def test_the_documents_speak_of_the_timeline():
    for doc, word in (("DESIGN.md", "no such step exists"), ("INTEGRATION.md", "timeline.update(probs)"), ("README.md", "PoseTimeline"),
                      ("EXPERIMENTS.md", "Pose timeline")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc
