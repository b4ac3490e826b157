"""Pose-order decoding with hold durations, the parts that need no GPU: the loops of tests/_pose_duration_ref.py against the
plain decoder's loops where the two rules must coincide (geometric durations, D = 1), against themselves (lengths, a stream
alone), the box prior on seeded tracks, the host helpers and the run-length count on hand-written tables, the C ABI's
declaration and every host-side refusal (pointers that are never dereferenced), the exports and the documents."""
import ctypes
import os
import re

import numpy as np
import pytest

import _pose_duration_ref as Q
import _pose_order_ref as R
import _segments_ref as G
from _util import PKG, ROOT, pkg

QT_ERR_INVALID_ARG, QT_ERR_UNSUPPORTED = -1, -3
F32 = np.float32


def _chain(S, C, stay=-39, advance=-850):
    return R.cyclic_prior([s % C for s in range(S)], stay, advance, skip=-3000, other=-20000)


# ---- the rule against the plain decoder's -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 7, 128])
def test_geometric_durations_score_what_the_plain_decoder_scores(D):
    """dur[j][d - 1] = (d - 1) stay with trans[j][j] = stay and dur_open = dur: a hold split into segments costs what it costs
    inside one, so the best score is the plain decoder's for every D (carry[:, 1] from a zero carry, its delta's maximum)"""
    M = pkg("pose_order")
    stay = M.prob_score(0.9)
    assert stay == -39 and (128 - 1) * stay >= R.TRANS_FLOOR
    for seed, (B, T, C, S) in enumerate([(2, 150, 5, 6), (1, 40, 12, 12), (1, 1, 3, 3)]):
        probs = R.make_probs(70 + seed, B, T, C, run=9)
        sc, tr = _chain(S, C, stay=stay)
        init = -np.arange(S) * 41
        dur = Q.geometric_durations(stay, S, D)
        _, _, score = Q.decode(probs, sc, tr, dur, init, dur_open=dur)
        want = R.decode(probs, sc, tr, init)[3][:, 1]
        assert score.dtype == np.int64 and score.tolist() == want.tolist(), (D, B, T)
        assert Q.decode(probs, sc, tr, dur, init)[2].tolist() == want.tolist()           # dur_open None is dur


def test_a_hold_in_one_segment_or_in_several():
    """ten frames that favour state 0, by hand.  With geometric durations every split of the hold into segments scores alike
    for every D, and the lowest d wins every tie: the segments are of one frame each, and start says so.  With a table that
    admits segments of exactly 4 the hold is 4 + 4 + 2, the last one cut by the video and scored by dur_open."""
    stay = -39
    probs = np.full((1, 10, 2), F32(0.1), F32)
    probs[0, :, 0] = F32(0.9)
    sc, tr = R.cyclic_prior([0, 1], stay, -850)
    e0 = int(R.q(F32(0.9)))
    for D in (1, 4, 16):
        path, start, score = Q.decode(probs, sc, tr, Q.geometric_durations(stay, 2, D))
        assert score.tolist() == [10 * e0 + 10 * stay] and path[0].tolist() == [0] * 10                  # beta[0] = max_i trans[i][0] = stay
        assert start[0].tolist() == list(range(10)), D
    dur = Q.hold_prior(2, 4, 4, 4)
    path, start, score = Q.decode(probs, sc, tr, dur, dur_open=Q.suffix_max(dur))
    assert path[0].tolist() == [0] * 10 and start[0].tolist() == [0, 0, 0, 0, 4, 4, 4, 4, 8, 8]            # (1 + 4 + 4 + 1 has a join more)
    assert score.tolist() == [10 * e0 + 3 * stay]


@pytest.mark.parametrize("S,C", [(1, 1), (6, 5), (12, 12), (17, 17)])
def test_a_table_of_one_frame_is_the_plain_decoder(S, C):
    """D = 1 and dur all zero: path is the bytes of the plain decoder's path; the tie rules coincide (rows of equal
    probabilities, NaN rows and an all-zero trans make ties)"""
    for T in (1, 2, 37):
        probs = R.make_probs(5 * S + T, 2, T, C, run=4)
        if T > 20:
            probs[0, 5] = np.nan
            probs[1, 9:14] = F32(0.25)
        sc, tr = _chain(S, C)
        init = -np.arange(S) * 37
        dur = np.zeros((S, 1), np.int32)
        for trans in (tr, np.zeros_like(tr)):
            for use_init in (None, init):
                path, start, score = Q.decode(probs, sc, trans, dur, use_init)
                want = R.decode(probs, sc, trans, use_init)
                assert R.bits(path) == R.bits(want[0]) and score.tolist() == want[3][:, 1].tolist(), (S, T)
                assert (start == np.arange(T)[None, :]).all()


def test_lengths_cut_a_stream_and_a_stream_alone_is_itself():
    B, T, C, S, D = 3, 60, 5, 6, 8
    probs = R.make_probs(9, B, T, C, run=5)
    sc, tr = _chain(S, C, advance=-300)
    dur = Q.hold_prior(S, D, 3, 7, inside=-10, outside=-4000)
    dur[:, 4] = -3
    open_ = Q.suffix_max(dur)
    init = -np.arange(S) * 50
    lengths = np.array([T, 1, 23], np.int32)
    path, start, score = Q.decode(probs, sc, tr, dur, init, open_, lengths)
    for b, L in enumerate(lengths):
        alone = Q.decode(probs[b:b + 1, :L], sc, tr, dur, init, open_)
        assert R.bits(path[b, :L]) == R.bits(alone[0][0]) and R.bits(start[b, :L]) == R.bits(alone[1][0]) and score[b] == alone[2][0]
        assert (path[b, L:] == -1).all() and (start[b, L:] == -1).all()
    whole = Q.decode(probs, sc, tr, dur, init, open_)
    for b in range(B):
        alone = Q.decode(probs[b:b + 1], sc, tr, dur, init, open_)
        assert all(R.bits(w[b:b + 1]) == R.bits(a) for w, a in zip(whole, alone))
    # lengths outside 1 .. frames are clamped into it
    wild = Q.decode(probs, sc, tr, dur, init, open_, np.array([T + 9, -4, 0], np.int32))
    tame = Q.decode(probs, sc, tr, dur, init, open_, np.array([T, 1, 1], np.int32))
    assert all(R.bits(w) == R.bits(t) for w, t in zip(wild, tame))
    assert len(set(path[0].tolist())) >= 4 and (start[0, 1:] >= start[0, :-1]).all()


def test_dur_open_is_read_at_the_two_cuts_only():
    """holds of 2, 5, 5 and 3 frames under a box of 5 .. 6: the interior holds pay dur, the first and the last, which the video
    cuts, pay dur_open (the suffix maximum: nothing); with dur_open NULL they pay for being short"""
    C = S = 3
    lead = [0] * 2 + [1] * 5 + [2] * 5 + [0] * 3
    probs = np.full((1, len(lead), C), F32(0.05), F32)
    probs[0, np.arange(len(lead)), lead] = F32(0.9)
    sc, tr = R.cyclic_prior(range(C), -39, -200)
    dur = Q.hold_prior(S, 6, 5, 6, inside=0, outside=-9000)
    path, start, score = Q.decode(probs, sc, tr, dur, dur_open=Q.suffix_max(dur))
    assert path[0].tolist() == lead and start[0].tolist() == [0] * 2 + [2] * 5 + [7] * 5 + [12] * 3
    e = int(R.q(F32(0.9)))
    assert score.tolist() == [15 * e + (-39) + 3 * (-200)]                          # no duration is charged: beta[0] is one stay
    charged = Q.decode(probs, sc, tr, dur)                                          # dur_open NULL: the cut holds of 2 and 3 pay
    assert charged[2][0] < score[0]


# ---- the box prior ----------------------------------------------------------------------------------------------------------------
BOX_SEEDS = (4, 7, 16, 20, 23, 26, 27, 28)


def test_a_box_prior_removes_the_short_visits():
    """tracks whose labels hold every step for 9 frames, with a tenth of the frames sent off; a prior loose enough that the
    plain decoder follows some of them.  The seeds are kept for which (1) no interior run of the labels is shorter than 4, so the
    box says something true, and (2) the plain decoder's path does hold an interior run shorter than 4.  Then no interior run
    of the duration path is shorter than 4, and Edit and F1@50 against the labels are no worse than the plain decoder's."""
    C = S = 6
    T, D = 150, 16
    sc, tr = R.cyclic_prior(range(C), -39, -300, skip=-600, other=-1500)
    dur = Q.hold_prior(S, D, 4, D)
    interior = lambda row: Q.runs_of(row)[1:-1]
    better = 0
    for seed in BOX_SEEDS:
        probs, lead = Q.make_tracks(seed, 1, T, C, run=9)
        assert R.bits(probs) == R.bits(R.make_probs(seed, 1, T, C, run=9))
        plain = R.decode(probs, sc, tr)[0]
        assert min(r[1] for r in interior(lead[0])) >= 4, seed                                   # (1)
        assert min(r[1] for r in interior(plain[0])) < 4, seed                                   # (2)
        path, start, _ = Q.decode(probs, sc, tr, dur, dur_open=Q.suffix_max(dur))
        assert min(r[1] for r in interior(path[0])) >= 4, seed
        scores = []
        for p in (plain, path):
            _, state = G.evaluate(sc.astype(np.int64)[p], lead, C, [50])
            rep = G.report(state, [50])
            scores.append((rep["edit"], rep["f1"][50]))
        assert scores[1][0] >= scores[0][0] and scores[1][1] >= scores[0][1], (seed, scores)
        better += scores[1] != scores[0]
    assert better >= len(BOX_SEEDS) // 2


# ---- host helpers and the count -----------------------------------------------------------------------------------------------------
def test_host_helpers_on_hand_written_tables():
    M = pkg("pose_order")
    box = M.hold_prior(2, 6, 2, 4)
    assert box.dtype == np.int32 and box.tolist() == [[-65536, 0, 0, 0, -65536, -65536]] * 2
    assert M.hold_prior(1, 3, 2, 9, inside=-5, outside=-70).tolist() == [[-70, -5, -5]]
    assert R.bits(M.hold_prior(3, 7, 2, 5, -1, -99)) == R.bits(Q.hold_prior(3, 7, 2, 5, -1, -99))
    geo = M.geometric_durations(-39, 2, 4)
    assert geo.dtype == np.int32 and geo.tolist() == [[0, -39, -78, -117]] * 2
    assert R.bits(M.geometric_durations(-39, 3, 128)) == R.bits(Q.geometric_durations(-39, 3, 128))
    assert M.geometric_durations(-65536, 1, 2).tolist() == [[0, -65536]] and M.geometric_durations(-516, 1, 128)[0, -1] == -65532
    with pytest.raises(ValueError):
        M.geometric_durations(-517, 1, 128)                                       # 127 * -517 leaves the range
    counts = np.array([[1, 3, 0, 0], [0, 0, 0, 0], [5, 0, 0, 2]])
    got = M.duration_prior(counts)                                                # pseudo 1: (2 4 1 1) / 8, 1 / 4, (6 1 1 3) / 11
    assert got.dtype == np.int32 and got[0].tolist() == [-511, -255, -767, -767] and got[1].tolist() == [-511] * 4
    assert got[2].tolist() == [int(M.prob_score(F32(v / 11))) for v in (6, 1, 1, 3)]
    assert R.bits(got) == R.bits(Q.duration_prior(counts))
    bare = M.duration_prior(counts, pseudo_count=0)
    assert bare[0].tolist() == [-511, -106, -8192, -8192] and bare[1].tolist() == [-8192] * 4
    assert R.bits(bare) == R.bits(Q.duration_prior(counts, 0)) and R.bits(M.duration_prior(counts, 0.5)) == R.bits(Q.duration_prior(counts, 0.5))
    for bad in (lambda: M.hold_prior(0, 4, 1, 2), lambda: M.hold_prior(65, 4, 1, 2), lambda: M.hold_prior(2, 129, 1, 2),
                lambda: M.hold_prior(2, 0, 1, 2), lambda: M.hold_prior(2, 4, 3, 2), lambda: M.hold_prior(2, 4, 0, 2),
                lambda: M.hold_prior(2, 4, 1, 2, inside=1), lambda: M.hold_prior(2, 4, 1, 2, outside=-65537),
                lambda: M.hold_prior(2, 4, 1.0, 2), lambda: M.geometric_durations(1, 2, 4), lambda: M.geometric_durations(-1.5, 2, 4),
                lambda: M.geometric_durations(-1, 2, 129), lambda: M.duration_prior(np.zeros((2, 3))),
                lambda: M.duration_prior([[1, -1]]), lambda: M.duration_prior([1, 2]), lambda: M.duration_prior([[1, 2]], -1.0),
                lambda: M.duration_prior(np.zeros((2, 129), int))):
        with pytest.raises(ValueError):
            bad()
    assert Q.suffix_max([[-5, -1, -7, -3], [0, -2, -2, -9]]).tolist() == [[-1, -1, -3, -3], [0, -2, -2, -9]]


def test_run_lengths_counted_by_hand():
    S, D = 3, 4
    #       first run (not counted) | 1 x 3 | 2 x 4 = D | 0 x 5 = D + 1 | 1 x 1 | last run (not counted)
    a = [0, 0] + [1] * 3 + [2] * 4 + [0] * 5 + [1] + [2, 2]
    want = np.zeros((S, D), np.int64)
    want[1, 2] += 1
    want[2, 3] += 1
    want[0, 3] += 1
    want[1, 0] += 1
    assert Q.count_durations(np.array([a]), S, D).tolist() == want.tolist()
    # a -1 tail: with lengths the run in front of it is the stream's last; without, the -1 ends it and it counts
    tail = a + [-1] * 4
    assert Q.count_durations(np.array([tail]), S, D, lengths=[len(a)]).tolist() == want.tolist()
    more = want.copy()
    more[2, 1] += 1
    assert Q.count_durations(np.array([tail]), S, D).tolist() == more.tolist()
    # entries outside [0, S) end a run and count nowhere; a run that follows one at frame 0 does not start at frame 0
    b = [7, 1, 1, -1, 1, 1, 1, 3, 0, 0, 2]
    wb = np.zeros((S, D), np.int64)
    wb[1, 1] += 1
    wb[1, 2] += 1
    wb[0, 1] += 1
    assert Q.count_durations(np.array([b]), S, D).tolist() == wb.tolist()
    # two streams, and counts that add up; one run over the whole stream counts nowhere
    both = np.array([a[:11], b])
    first = Q.count_durations(both, S, D)
    assert Q.count_durations(both, S, D, counts=first).tolist() == (2 * first).tolist()
    assert not Q.count_durations(np.array([[1] * 9]), S, D).any() and not Q.count_durations(np.array([[1]]), S, D).any()
    assert Q.count_durations(np.array([a]), S, D, lengths=[1]).sum() == 0


# ---- the library -------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    declared = set(re.findall(r"\b(qt_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(os.path.join(ROOT, PKG, "libqtcnn_hip.so"))
    for symbol in ("qt_pose_duration_workspace_bytes", "qt_pose_duration_decode", "qt_pose_duration_count"):
        assert symbol in declared and hasattr(lib, symbol), symbol
    M = pkg("pose_order")
    fields = re.search(r"typedef struct qt_pose_duration_desc \{(.*?)\} qt_pose_duration_desc;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields)
    assert re.findall(r"\b(\w+)\s*;", fields) == [n for n, _ in M.PoseDurationDesc._fields_]
    assert all(t is ctypes.c_int for _, t in M.PoseDurationDesc._fields_)
    src = open(os.path.join(ROOT, PKG, "csrc", "pose_duration.hip")).read()
    assert '#include "pose_chain.h"' in src and not re.search(r"_LOG2\[256\]\s*=|\b\w*_FLOOR\s*=(?!=)", re.sub(r"//[^\n]*", "", src))
    assert int(re.search(r"#define QT_POSE_DUR_MAX (\d+)", header).group(1)) == M.DUR_MAX == Q.DUR_MAX == \
        int(re.search(r"constexpr int PC_MAX_D = (\d+);", open(os.path.join(ROOT, PKG, "csrc", "pose_duration_chain.h")).read()).group(1))
    P = pkg()
    assert P.PoseDurationDecoder is M.PoseDurationDecoder and P.duration_prior is M.duration_prior
    assert P.hold_prior is M.hold_prior and P.geometric_durations is M.geometric_durations
    assert {"PoseDurationDecoder", "duration_prior", "hold_prior", "geometric_durations"} <= set(P.__all__)


def _lib():
    M = pkg("pose_order")
    L = pkg("_lib").lib()
    return M, L


def _refused(L, rc, word, status=QT_ERR_INVALID_ARG):
    assert rc == status and word in L.qt_last_error(), (rc, L.qt_last_error())


def test_workspace_query():
    M, L = _lib()
    q = lambda *a: L.qt_pose_duration_workspace_bytes(ctypes.byref(M.PoseDurationDesc(*a)))
    assert q(3, 100, 12, 12, 64) == 3 * 100 * 12 * 2 and q(1, 1, 1, 1, 1) == 8 and q(1, 5, 3, 3, 128) == 32
    for bad in ((0, 100, 12, 12, 64), (3, 0, 12, 12, 64), (3, 100, 65, 12, 64), (3, 100, 12, 65, 64), (3, 100, 12, 12, 0),
                (3, 100, 12, 12, 129), (3, 100, 12, 12, -1), (1 << 10, (1 << 10) + 1, 12, 12, 64)):
        assert q(*bad) == 0, bad
    assert L.qt_pose_duration_workspace_bytes(None) == 0


def test_decode_argument_checks_need_no_device():
    """every refusal comes before the first device call: the pointers are never dereferenced"""
    M, L = _lib()
    D = lambda batch=2, frames=100, C=12, S=12, dmax=16: M.PoseDurationDesc(batch, frames, C, S, dmax)
    names = ("probs", "sc", "trans", "init", "dur", "dur_open", "lengths", "path", "start", "score", "ws")
    good = {n: 0x10000000 * k for k, n in enumerate(names, 1)}
    good.update(ld=12, ws_bytes=1 << 24)

    def call(desc, **kw):
        a = {**good, **kw}
        return L.qt_pose_duration_decode(ctypes.byref(desc), a["probs"], a["ld"], a["sc"], a["trans"], a["init"], a["dur"],
                                         a["dur_open"], a["lengths"], a["path"], a["start"], a["score"], a["ws"], a["ws_bytes"],
                                         None)

    refused = lambda rc, word, status=QT_ERR_INVALID_ARG: _refused(L, rc, word, status)
    refused(L.qt_pose_duration_decode(None, *[good[n] for n in ("probs", "ld", "sc", "trans", "init", "dur", "dur_open", "lengths",
                                                               "path", "start", "score", "ws", "ws_bytes")], None), b"null descriptor")
    for batch in (0, -3):
        refused(call(D(batch=batch)), b"batch")
    for frames in (0, -1):
        refused(call(D(frames=frames)), b"frames")
    for C in (0, -1, 65):
        refused(call(D(C=C), ld=70), b"num_classes")
    for S in (0, -1, 65):
        refused(call(D(S=S)), b"num_states")
    for dmax in (0, -1, 129, 1 << 20):
        refused(call(D(dmax=dmax)), b"max_duration")
    refused(call(D(), ld=11), b"ld")
    for name, word in (("probs", b"null probs"), ("sc", b"null state_class"), ("trans", b"null trans"), ("dur", b"null dur"),
                       ("path", b"null path")):
        refused(call(D(), **{name: None}), word)
    for name, off in (("probs", 2), ("sc", 1), ("trans", 3), ("init", 2), ("dur", 2), ("dur_open", 1), ("lengths", 3), ("path", 4),
                      ("start", 4), ("score", 4), ("ws", 4)):
        refused(call(D(), **{name: good[name] + off}), b"aligned")
    need = L.qt_pose_duration_workspace_bytes(ctypes.byref(D()))
    assert need == 2 * 100 * 12 * 2
    refused(call(D(), ws_bytes=need - 1), b"workspace")
    refused(call(D(), ws_bytes=0), b"workspace")
    refused(call(D(), ws=None), b"workspace")
    rows = 2 * 100
    for out, nbytes in (("path", rows * 8), ("start", rows * 8), ("score", 2 * 8), ("ws", need)):
        refused(call(D(), **{out: good["probs"] + (rows * 12 - 2) * 4}), b"overlap")
        refused(call(D(), **{out: good["probs"] - nbytes + 8}), b"overlap")
        refused(call(D(), **{out: good["sc"] + 40}), b"overlap")
        refused(call(D(), **{out: good["trans"] + (144 - 2) * 4}), b"overlap")
        refused(call(D(), **{out: good["init"]}), b"overlap")
        refused(call(D(), **{out: good["dur"] + (12 * 16 - 2) * 4}), b"overlap")
        refused(call(D(), **{out: good["dur_open"] + 8}), b"overlap")
        refused(call(D(), **{out: good["lengths"]}), b"overlap")
    refused(call(D(), ld=16, path=good["probs"] + (199 * 16 + 10) * 4), b"overlap")
    refused(call(D(), start=good["path"] + 8), b"overlap")
    refused(call(D(), score=good["start"] + 800), b"overlap")
    refused(call(D(), ws=good["score"] + 8), b"overlap")
    refused(call(D(batch=1 << 10, frames=(1 << 10) + 1)), b"frames", QT_ERR_UNSUPPORTED)
    refused(call(D(batch=1, frames=(1 << 20) + 1)), b"frames", QT_ERR_UNSUPPORTED)
    # the optional ones may be null: the next check is reached
    refused(call(D(), init=None, dur_open=None, lengths=None, start=None, score=None, path=None), b"null path")


def test_count_argument_checks_need_no_device():
    M, L = _lib()
    D = lambda batch=2, frames=100, C=1, S=12, dmax=16: M.PoseDurationDesc(batch, frames, C, S, dmax)
    path, lengths, counts = 0x10000000, 0x20000000, 0x30000000
    call = lambda desc, path=path, ld=100, lengths=lengths, counts=counts: \
        L.qt_pose_duration_count(ctypes.byref(desc), path, ld, lengths, counts, None)
    refused = lambda rc, word, status=QT_ERR_INVALID_ARG: _refused(L, rc, word, status)
    refused(L.qt_pose_duration_count(None, path, 100, lengths, counts, None), b"null descriptor")
    refused(call(D(batch=0)), b"batch")
    refused(call(D(frames=0)), b"frames")
    refused(call(D(S=65)), b"num_states")
    refused(call(D(C=0)), b"num_classes")
    for dmax in (0, 129):
        refused(call(D(dmax=dmax)), b"max_duration")
    refused(call(D(), ld=99), b"ld_path")
    refused(call(D(), path=None), b"null path")
    refused(call(D(), counts=None), b"null counts")
    for kw in (dict(path=path + 4), dict(counts=counts + 4), dict(lengths=lengths + 2)):
        refused(call(D(), **kw), b"aligned")
    refused(call(D(), counts=path + 199 * 8), b"overlap")
    refused(call(D(), ld=150, counts=path + 249 * 8), b"overlap")
    refused(call(D(), counts=path - 12 * 16 * 8 + 8), b"overlap")
    refused(call(D(), counts=lengths), b"overlap")
    refused(call(D(batch=1, frames=(1 << 20) + 1), ld=1 << 21), b"frames", QT_ERR_UNSUPPORTED)


def test_module_argument_checks_need_no_device():
    P = pkg()
    sc, trans = P.cyclic_prior(range(4), -10, -100)
    dur = P.hold_prior(4, 8, 2, 6)
    for bad in (dict(dur=dur[:3]), dict(dur=dur.astype(float)), dict(dur=dur - 1), dict(dur=-dur - 1), dict(dur=dur[0]),
                dict(dur=np.zeros((4, 129), int)), dict(dur=np.zeros((4, 0), int)), dict(dur_open="prefix_max"),
                dict(dur_open=dur[:, :7]), dict(dur_open=dur + 1), dict(dur_open=dur.astype(float)),
                dict(trans=trans[:3]), dict(init=[0, 0, 0]), dict(streams=0), dict(state_class=[0, 1, 2, 64]),
                dict(class_names=["a", "b", "c"])):
        with pytest.raises(ValueError):
            P.PoseDurationDecoder(**{"state_class": sc, "trans": trans, "dur": dur, "device": "cuda:0", **bad})
    with pytest.raises(P.QtError, match="AMD GPU"):      # no torch fallback
        P.PoseDurationDecoder(sc, trans, dur, "cpu")


def test_the_documents_speak_of_the_duration_decoder():
    for doc, word in (("DESIGN.md", "qt_pose_duration_decode"), ("DESIGN.md", "pose_duration.hip"),
                      ("INTEGRATION.md", "PoseDurationDecoder("), ("INTEGRATION.md", "count_durations"),
                      ("README.md", "pose_duration.hip"), ("README.md", "PoseDurationDecoder"),
                      ("EXPERIMENTS.md", "qt_pose_duration_decode"),
                      (os.path.join(PKG, "pose_order.py"), "PoseDurationDecoder("),
                      (os.path.join("scripts", "bench_pose_duration.py"), "PoseDurationDecoder(")):
        assert word in open(os.path.join(ROOT, doc)).read(), (doc, word)
