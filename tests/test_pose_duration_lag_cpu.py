"""Fixed-lag pose-order decoding with hold durations, the parts that need no GPU: the loops of tests/_pose_duration_lag_ref.py
against the whole-video loops of tests/_pose_duration_ref.py on every prefix, against themselves under every two-call split,
against the plain fixed-lag decoder's loops where the two rules must coincide (D = 1, dur all zero), the two size queries on
hand-computed cases, every host-side refusal (pointers that are never dereferenced), the exports, the documents, and what the
feature is for: on seeded tracks the live path with durations scores no worse than the plain live path, and mostly better."""
import ctypes
import os
import re

import numpy as np
import pytest

import _pose_duration_lag_ref as DL
import _pose_duration_ref as Q
import _pose_lag_ref as G
import _pose_order_ref as R
import _segments_ref as SEG
from _util import PKG, ROOT, pkg

QT_ERR_INVALID_ARG, QT_ERR_UNSUPPORTED = -1, -3
F32 = np.float32


def _chain(S, C, stay=-39, advance=-300):
    return R.cyclic_prior([s % C for s in range(S)], stay, advance, skip=-600, other=-1500)


def _case(seed, B, T, C, S, D):
    """probs with a NaN row, zero rows and tie rows; a chain; a box-like dur with a dent, its suffix maximum, an init"""
    probs = R.make_probs(seed, B, T, C, run=5)
    probs[0, min(5, T - 1)] = np.nan
    probs[B - 1, T // 3:T // 3 + 2] = 0
    probs[0, T // 2:T // 2 + 4] = F32(1.0 / C)
    sc, tr = _chain(S, C)
    dur = Q.hold_prior(S, D, min(2, D), max(D - 1, min(2, D)), inside=-10, outside=-4000)
    dur[:, D // 2] = -3
    dur[S - 1] = -7                                              # a flat row: every length ties
    return probs, sc, tr, dur, Q.suffix_max(dur), -np.arange(S) * 50


# ---- the loops against the whole-video decoder's -------------------------------------------------------------------------------
@pytest.mark.parametrize("D,T", [(1, 40), (3, 40), (8, 40), (128, 150)])
def test_every_emitted_frame_is_the_whole_video_decoder_on_a_prefix(D, T):
    """lag_path[g] and lag_start[g] are path[g] and start[g] of the whole-video loops on the first min(g + lag, T - 1) + 1
    frames, score[f] their score on the first f + 1 frames; with dur_open given, NULL, and without init"""
    B, C, S = 2, 5, 6
    probs, sc, tr, dur, open_, init = _case(11 + D, B, T, C, S, D)
    for use_open, use_init in ((open_, init), (None, None)):
        whole = [Q.decode(probs[:, :L], sc, tr, dur, use_init, use_open) for L in range(1, T + 1)]     # prefix L at [L - 1]
        for lag in (0, 1, 5, 63):
            g0, (path, start, filtered, score), state = DL.decode(probs, sc, tr, dur, use_init, use_open, lag=lag, flush=True)
            assert g0 == 0 and path.shape == start.shape == filtered.shape == score.shape == (B, T) and state["seen"] == T
            for g in range(T):
                w = whole[min(g + lag, T - 1)]
                assert path[:, g].tolist() == w[0][:, g].tolist() and start[:, g].tolist() == w[1][:, g].tolist(), (lag, g)
                assert score[:, g].tolist() == whole[g][2].tolist() and filtered[:, g].tolist() == whole[g][0][:, g].tolist()
    assert len(set(path[0].tolist())) >= 3


@pytest.mark.parametrize("D", [1, 3, 8])
def test_every_two_call_split_is_one_call(D):
    B, T, C, S = 2, 40, 5, 6
    probs, sc, tr, dur, open_, init = _case(3 + D, B, T, C, S, D)
    for lag in (0, 1, 5, 63):
        _, want, want_state = DL.decode(probs, sc, tr, dur, init, open_, lag=lag, flush=True)
        for cut in range(1, T):
            g0, got, state, calls = DL.split(DL.decode, probs, [cut], sc, tr, dur, init, open_, lag=lag)
            assert g0 == 0 and all(R.bits(a) == R.bits(b) for a, b in zip(got, want)), (lag, cut)
            DL.same_state(state, want_state)
            assert calls[0][1][0].shape[1] == max(0, cut - lag)
        # no flush leaves the last lag frames pending; a flush alone brings them
        g0, first, state = DL.decode(probs, sc, tr, dur, init, open_, lag=lag, flush=False)
        assert first[0].shape[1] == max(0, T - lag)
        g0, rest, state = DL.decode(probs[:, :0], sc, tr, dur, init, open_, lag=lag, flush=True, state=state)
        assert g0 == max(0, T - lag) and rest[2].shape[1] == 0
        assert all(R.bits(np.concatenate([a, b], axis=1)) == R.bits(w) for a, b, w in zip(first[:2], rest[:2], want[:2]))
        DL.same_state(state, want_state)


def test_a_long_table_under_split_and_the_packed_carry():
    """D = 128 over 150 frames: the ring wraps; the carry goes through its bytes between the calls"""
    B, T, C, S, D, lag = 2, 150, 5, 6, 128, 16
    probs, sc, tr, dur, open_, init = _case(2, B, T, C, S, D)
    _, want, want_state = DL.decode(probs, sc, tr, dur, init, open_, lag=lag, flush=True)
    for cuts in ([1], [127], [128], [129], [40, 41, 140]):
        state, outs = None, []
        for a, b in zip([0] + cuts, cuts + [T]):
            _, o, state = DL.decode(probs[:, a:b], sc, tr, dur, init, open_, lag=lag, flush=b == T, state=state)
            raw = DL.pack_carry(state, S, D, lag)
            assert raw.shape == (B, DL.carry_stride(S, D, lag))
            state = DL.unpack_carry(raw.tobytes(), B, S, D, lag, state["seen"])
            outs.append(o)
        assert all(R.bits(np.concatenate([o[i] for o in outs], axis=1)) == R.bits(want[i]) for i in range(4)), cuts
        DL.same_state(state, want_state)


@pytest.mark.parametrize("S,C", [(1, 1), (6, 5), (12, 12), (17, 17)])
def test_a_table_of_one_frame_is_the_plain_lag_decoder(S, C):
    """D = 1 and dur all zero: lag_path and filtered are the plain fixed-lag loops', ties included"""
    T = 37
    probs = R.make_probs(5 * S + T, 2, T, C, run=4)
    probs[0, 5] = np.nan
    probs[1, 9:14] = F32(0.25)
    sc, tr = _chain(S, C)
    init = -np.arange(S) * 37
    dur = np.zeros((S, 1), np.int32)
    for trans in (tr, np.zeros_like(tr)):
        for use_init in (None, init):
            for lag in (0, 1, 5, 63):
                _, (path, start, filtered, _), _ = DL.decode(probs, sc, trans, dur, use_init, lag=lag, flush=True)
                _, (want, want_filtered), _ = G.decode(probs, sc, trans, use_init, lag=lag, flush=True)
                assert R.bits(path) == R.bits(want) and R.bits(filtered) == R.bits(want_filtered), (S, lag)
                assert (start == np.arange(T)[None, :]).all()


# ---- what it is for ---------------------------------------------------------------------------------------------------------------
LIVE_SEEDS = (4, 7, 16, 20, 23, 26, 27, 28, 30, 31)


def test_the_live_path_with_durations_beats_the_plain_live_path():
    """tracks whose labels hold every step for 9 frames, with a tenth of the frames sent off, decoded 16 frames behind the
    camera.  Of the seeds 0 .. 31 those are kept for which (1) no interior run of the labels is shorter than 4, so the box says
    something true, and (2) the plain fixed-lag path does hold an interior run shorter than 4.  On them Edit and F1@50 of the
    joined duration-lag path are no worse than the plain lag path's, and strictly better on at least half."""
    C = S = 6
    T, D, lag = 150, 16, 16
    sc, tr = R.cyclic_prior(range(C), -39, -300, skip=-600, other=-1500)
    dur = Q.hold_prior(S, D, 4, D)
    interior = lambda row: Q.runs_of(row)[1:-1]
    kept, better = [], 0
    for seed in range(32):
        probs, lead = Q.make_tracks(seed, 1, T, C, run=9)
        _, (plain, _), _ = G.split(G.decode, probs, list(range(1, T)), sc, tr, None, lag=lag)[:3]
        if not (min(r[1] for r in interior(lead[0])) >= 4 and min(r[1] for r in interior(plain[0])) < 4):   # (1) and (2)
            continue
        kept.append(seed)
        _, (path, _, _, _), _ = DL.split(DL.decode, probs, list(range(1, T)), sc, tr, dur, None, Q.suffix_max(dur), lag=lag)[:3]
        scores = []
        for p in (plain, path):
            _, state = SEG.evaluate(sc.astype(np.int64)[p], lead, C, [50])
            rep = SEG.report(state, [50])
            scores.append((rep["edit"], rep["f1"][50]))
        assert scores[1][0] >= scores[0][0] and scores[1][1] >= scores[0][1], (seed, scores)
        better += scores[1][0] > scores[0][0] and scores[1][1] > scores[0][1]
    assert tuple(kept) == LIVE_SEEDS and len(kept) >= 8
    assert 2 * better >= len(kept)


# ---- the library -------------------------------------------------------------------------------------------------------------------
def _lib():
    M = pkg("pose_order")
    L = pkg("_lib").lib()
    return M, L


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    declared = set(re.findall(r"\b(qt_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(os.path.join(ROOT, PKG, "libqtcnn_hip.so"))
    for symbol in ("qt_pose_duration_lag_carry_bytes", "qt_pose_duration_lag_workspace_bytes", "qt_pose_duration_lag_decode"):
        assert symbol in declared and hasattr(lib, symbol), symbol
    M, P = pkg("pose_order"), pkg()
    fields = re.search(r"typedef struct qt_pose_duration_lag_desc \{(.*?)\} qt_pose_duration_lag_desc;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields)
    names = [n for decl in fields.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [n for n, _ in M.PoseDurationLagDesc._fields_]
    assert [t for _, t in M.PoseDurationLagDesc._fields_] == [ctypes.c_int] * 7 + [ctypes.c_longlong]
    src = open(os.path.join(ROOT, PKG, "csrc", "pose_duration_lag.hip")).read()
    assert '#include "pose_chain.h"' in src and not re.search(r"_LOG2\[256\]\s*=|\b\w*_FLOOR\s*=(?!=)", re.sub(r"//[^\n]*", "", src))
    assert "getenv" not in src and "qt_env" not in src                                # one route
    assert "constexpr int PC_MAX_D = 128;" in open(os.path.join(ROOT, PKG, "csrc", "pose_duration_chain.h")).read()
    assert P.PoseDurationLagDecoder is M.PoseDurationLagDecoder and "PoseDurationLagDecoder" in P.__all__


def test_size_queries_by_hand():
    M, L = _lib()
    D = lambda batch=2, frames=1, C=12, S=12, dmax=64, lag=16, flush=0, seen=0: \
        M.PoseDurationLagDesc(batch, frames, C, S, dmax, lag, flush, seen)
    carry = lambda **kw: L.qt_pose_duration_lag_carry_bytes(ctypes.byref(D(**kw)))
    room = lambda **kw: L.qt_pose_duration_lag_workspace_bytes(ctypes.byref(D(**kw)))
    # per stream 8 S + 8 D S + 2 lag S + 2, rounded up to 8
    assert carry(batch=1, S=1, dmax=1, lag=0) == 24                                   # 8 + 8 + 0 + 2 -> 24
    assert carry(batch=1, S=1, dmax=1, lag=3) == 24                                   # 8 + 8 + 6 + 2
    assert carry(batch=1, S=1, dmax=1, lag=4) == 32                                   # 8 + 8 + 8 + 2 -> 32
    assert carry(batch=2, S=12, dmax=64, lag=16) == 2 * (96 + 6144 + 384 + 8)         # .. + 2 -> 8
    assert carry(batch=3, S=64, dmax=128, lag=63) == 3 * (512 + 65536 + 8064 + 8)
    assert carry(batch=1, S=13, dmax=24, lag=5, frames=7, seen=99, flush=1) == 104 + 2496 + 130 + 6
    for S, dmax, lag in ((1, 1, 0), (3, 5, 5), (12, 64, 16), (13, 24, 63), (64, 128, 63)):
        assert carry(batch=5, S=S, dmax=dmax, lag=lag) == 5 * DL.carry_stride(S, dmax, lag) and DL.carry_stride(S, dmax, lag) % 8 == 0
    # uint16 [batch][n][S] and [batch][n], each rounded up to 8; nothing for a flush alone
    assert room(batch=1, frames=1, S=1) == 8 + 8
    assert room(batch=16, frames=1, S=12) == 384 + 32
    assert room(batch=2, frames=3, S=13) == 160 + 16                                  # 156 -> 160, 12 -> 16
    assert room(batch=3, frames=300, S=64) == 115200 + 1800
    assert room(batch=2, frames=0, flush=1, seen=40) == 0 and carry(batch=2, frames=0, flush=1, seen=40) > 0
    assert room(batch=2, frames=5, S=3) == DL.workspace_bytes(2, 5, 3) == 64 + 24
    for bad in (dict(batch=0), dict(frames=-1), dict(frames=0), dict(C=0), dict(C=65), dict(S=0), dict(S=65), dict(dmax=0),
                dict(dmax=129), dict(lag=-1), dict(lag=64), dict(seen=-1), dict(batch=2, frames=(1 << 19) + 1),
                dict(seen=1 << 36), dict(seen=(1 << 36) - 1, frames=2)):
        assert carry(**bad) == 0 and room(**bad) == 0, bad
    assert carry(seen=(1 << 36) - 1, frames=1) > 0
    assert L.qt_pose_duration_lag_carry_bytes(None) == 0 and L.qt_pose_duration_lag_workspace_bytes(None) == 0


def test_argument_checks_need_no_device():
    """every refusal comes before the first device call: the pointers are never dereferenced"""
    M, L = _lib()
    D = lambda batch=2, frames=300, C=12, S=12, dmax=16, lag=16, flush=0, seen=50: \
        M.PoseDurationLagDesc(batch, frames, C, S, dmax, lag, flush, seen)
    names = ("probs", "sc", "trans", "init", "dur", "dur_open", "cin", "cout", "path", "start", "filt", "score", "ws")
    good = {n: 0x10000000 * k for k, n in enumerate(names, 1)}
    good.update(ld=12, ws_bytes=1 << 24)
    probs, sc, trans, init, dur, dur_open, cin, cout = (good[n] for n in names[:8])

    def call(desc, **kw):
        a = {**good, **kw}
        return L.qt_pose_duration_lag_decode(None if desc is None else ctypes.byref(desc), a["probs"], a["ld"], a["sc"], a["trans"],
                                             a["init"], a["dur"], a["dur_open"], a["cin"], a["cout"], a["path"], a["start"],
                                             a["filt"], a["score"], a["ws"], a["ws_bytes"], None)

    def refused(rc, word, status=QT_ERR_INVALID_ARG):
        assert rc == status and word in L.qt_last_error(), (rc, L.qt_last_error())

    refused(call(None), b"null descriptor")
    for batch in (0, -3):
        refused(call(D(batch=batch)), b"batch")
    refused(call(D(frames=-1)), b"frames")
    refused(call(D(frames=-1, flush=1)), b"frames")
    refused(call(D(frames=0)), b"flush")
    for C in (0, -1, 65):
        refused(call(D(C=C), ld=70), b"num_classes")
    for S in (0, -1, 65):
        refused(call(D(S=S)), b"num_states")
    for dmax in (0, -1, 129, 1 << 20):
        refused(call(D(dmax=dmax)), b"max_duration")
    for lag in (-1, 64, 1000):
        refused(call(D(lag=lag)), b"lag")
    refused(call(D(seen=-1)), b"seen")
    refused(call(D(), ld=11), b"ld")
    for name, word in (("probs", b"null probs"), ("sc", b"null state_class"), ("trans", b"null trans"), ("dur", b"null dur"),
                       ("cout", b"null carry_out")):
        refused(call(D(), **{name: None}), word)
    refused(call(D(), path=None), b"null lag_path")                                 # count = 300 > 0
    refused(call(D(seen=3, frames=13, lag=16), path=None, cin=None), b"carry_in")   # count == 0: lag_path may be null, the carry not
    refused(call(D(), cin=None), b"null carry_in")
    refused(call(D(seen=0, frames=20, lag=16), path=None, cin=None), b"null lag_path")   # seen == 0: no carry_in; count = 4
    refused(call(D(frames=0, flush=1, seen=9), path=None, probs=None), b"null lag_path")  # a flush alone still emits
    for name, off in (("probs", 2), ("sc", 1), ("trans", 3), ("init", 2), ("dur", 2), ("dur_open", 1), ("cin", 4), ("cout", 4),
                      ("path", 4), ("start", 4), ("filt", 2), ("score", 4), ("ws", 4)):
        refused(call(D(), **{name: good[name] + off}), b"aligned")
    need = L.qt_pose_duration_lag_workspace_bytes(ctypes.byref(D()))
    assert need == 2 * 300 * 12 * 2 + 2 * 300 * 2
    refused(call(D(), ws_bytes=need - 1), b"workspace")
    refused(call(D(), ws_bytes=0), b"workspace")
    refused(call(D(), ws=None), b"workspace")
    carry = 2 * DL.carry_stride(12, 16, 16)
    assert carry == L.qt_pose_duration_lag_carry_bytes(ctypes.byref(D()))
    refused(call(D(), cin=cout + carry - 8), b"carry_in must not overlap carry_out")
    refused(call(D(), cin=cout), b"carry_in must not overlap carry_out")
    refused(call(D(), cout=cin + 8), b"carry_in must not overlap carry_out")
    rows = 2 * 300
    for name, nbytes in (("path", rows * 8), ("start", rows * 8), ("filt", rows * 8), ("score", rows * 8), ("cout", carry),
                         ("ws", need)):
        refused(call(D(), **{name: probs + (rows * 12 - 2) * 4}), b"overlap")
        refused(call(D(), **{name: probs - nbytes + 8}), b"overlap")
        refused(call(D(), **{name: sc + 40}), b"overlap")
        refused(call(D(), **{name: trans + (144 - 2) * 4}), b"overlap")
        refused(call(D(), **{name: init}), b"overlap")
        refused(call(D(), **{name: dur + (12 * 16 - 2) * 4}), b"overlap")
        refused(call(D(), **{name: dur_open + 8}), b"overlap")
        if name != "cout":
            refused(call(D(), **{name: cin + carry - 8}), b"overlap")
            refused(call(D(), **{name: cout + 8}), b"overlap")
    refused(call(D(), start=good["path"] + 8), b"overlap")
    refused(call(D(), filt=good["start"] + 800), b"overlap")
    refused(call(D(), score=good["filt"] + 8), b"overlap")
    refused(call(D(), ws=good["score"] + 8), b"overlap")
    refused(call(D(batch=1 << 10, frames=(1 << 10) + 1)), b"frames", QT_ERR_UNSUPPORTED)
    refused(call(D(batch=1, frames=(1 << 20) + 1)), b"frames", QT_ERR_UNSUPPORTED)
    refused(call(D(seen=(1 << 36) - 299)), b"seen", QT_ERR_UNSUPPORTED)
    refused(call(D(batch=1, frames=(1 << 20) + 1, dmax=129)), b"max_duration")
    # a flush alone asks for no workspace and no probs: the next check is reached
    refused(call(D(frames=0, flush=1), probs=None, ws=None, ws_bytes=0, cin=cout), b"carry_in must not overlap")
    # with seen == 0 carry_in is not looked at; the optional ones may be null
    refused(call(D(seen=0, frames=1), cin=cout, filt=cout + 8), b"carry_out must not overlap filtered")
    refused(call(D(), init=None, dur_open=None, start=None, filt=None, score=None, path=None), b"null lag_path")


def test_module_argument_checks_need_no_device():
    P = pkg()
    sc, trans = P.cyclic_prior(range(4), -10, -100)
    dur = P.hold_prior(4, 8, 2, 6)
    for bad in (dict(dur=dur[:3]), dict(dur=dur.astype(float)), dict(dur=dur - 1), dict(dur=np.zeros((4, 129), int)),
                dict(dur_open="prefix_max"), dict(dur_open=dur[:, :7]), dict(trans=trans[:3]), dict(init=[0, 0, 0]),
                dict(streams=0), dict(state_class=[0, 1, 2, 64]), dict(class_names=["a", "b", "c"]),
                dict(lag=-1), dict(lag=64), dict(lag=2.0), dict(lag=True), dict(lag=None)):
        with pytest.raises(ValueError, match="PoseDurationLagDecoder"):
            P.PoseDurationLagDecoder(**{"state_class": sc, "trans": trans, "dur": dur, "device": "cuda:0", "lag": 5, **bad})
    with pytest.raises(P.QtError, match="AMD GPU"):      # no torch fallback
        P.PoseDurationLagDecoder(sc, trans, dur, "cpu", 5)


def test_the_documents_speak_of_the_duration_lag_decoder():
    for doc, word in (("DESIGN.md", "qt_pose_duration_lag_decode"), ("DESIGN.md", "pose_duration_lag.hip"),
                      ("INTEGRATION.md", "PoseDurationLagDecoder("), ("INTEGRATION.md", "- lag_start"),
                      ("README.md", "pose_duration_lag.hip"), ("README.md", "PoseDurationLagDecoder"),
                      ("EXPERIMENTS.md", "qt_pose_duration_lag_decode"),
                      (os.path.join(PKG, "pose_order.py"), "PoseDurationLagDecoder("),
                      (os.path.join("include", "qtcnn.h"), "qt_pose_duration_lag_decode"),
                      (os.path.join("scripts", "bench_pose_duration_lag.py"), "PoseDurationLagDecoder(")):
        assert word in open(os.path.join(ROOT, doc)).read(), (doc, word)
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, PKG, "pose_order.py")).read())
    assert "streaming, fixed-lag and split calls" not in text
    assert "Not built for the chain with durations:" in text and "fixed-lag posteriors with durations" in text
