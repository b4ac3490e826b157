"""Pose-order posteriors, the parts that need no GPU: the float64 loops of tests/_pose_posterior_ref.py against an enumeration of
every path, the f32 loops and the tiled restatement against the float64 loops, the rule's corner statements (a row sums to one,
the last frame's posterior is its filtered row, a split changes nothing), the C ABI's declaration and every host-side refusal
(pointers that are never dereferenced), the module's argument checks, the exports and the documents."""
import ctypes
import os
import re

import numpy as np
import pytest

import _pose_order_ref as O
import _pose_posterior_ref as R
from _util import PKG, ROOT, pkg, pose_chain_header

QT_ERR_INVALID_ARG, QT_ERR_UNSUPPORTED = -1, -3
F32 = np.float32


def _case(seed, B, T, C, S, run=3):
    probs = O.make_probs(seed, B, T, C, run=run)
    sc, trans = O.cyclic_prior([s % C for s in range(S)], -30, -600, skip=-3000, other=-20000)
    return probs, sc, trans


def test_the_loops_equal_an_enumeration_of_every_path():
    """S = 3, n = 5: 243 paths, their weights summed in float64"""
    probs, sc, trans = _case(5, 1, 5, 3, 3, run=2)
    probs[0, 3] = F32(0.2)
    for init in (None, np.array([0, -700, -90])):
        post, filt, ev = R.brute_force(probs[0], sc, trans, init)
        got = R.loops64(probs, sc, trans, init)
        assert np.abs(got[0][0] - post).max() <= 1e-12 and np.abs(got[1][0] - filt).max() <= 1e-12
        assert abs(got[3][0] - ev) <= 1e-12 * max(1.0, abs(ev))
        assert abs(got[4][0, 1] - ev) <= 1e-12 * max(1.0, abs(ev)) and got[4][0, 0] == 5
        assert np.abs(got[2][0] - post).max() <= 1e-12               # one state per class here
    assert (post.argmax(axis=1) != filt.argmax(axis=1)).any() or np.abs(post - filt).max() > 1e-3    # smoothing is not filtering


def test_the_tiled_form_agrees_with_the_loops():
    for seed, (B, T, C, S) in enumerate([(2, 23, 5, 6), (1, 23, 3, 3), (2, 23, 12, 12)]):
        probs, sc, trans = _case(40 + seed, B, T, C, S)
        probs[0, 5] = np.nan
        probs[-1, 11:14] = F32(0.25)
        init = -np.arange(S) * 37
        stay = np.full_like(trans, -65536)
        np.fill_diagonal(stay, 0)
        for trans_used in (trans, np.zeros_like(trans), stay):
            carry = np.array([[9.0, -123.5] + [-(float((7 * s * s) % 9)) for s in range(S)]] * B)
            for c in (None, carry):
                want = R.loops64(probs, sc, trans_used, init, c)
                for tile in (1, 2, 5, R.TILE):
                    got = R.tiled(probs, sc, trans_used, init, c, tile=tile)
                    for name, w, g in zip(("posterior", "filtered", "class_posterior", "evidence", "carry"), want, got):
                        scale = max(1.0, float(np.abs(w).max())) if name in ("evidence", "carry") else 1.0
                        assert np.abs(w - g).max() <= 1e-10 * scale, (B, T, S, tile, name, float(np.abs(w - g).max()))


def test_rows_sum_to_one_and_the_last_frame_is_filtered():
    probs, sc, trans = _case(7, 2, 30, 4, 6)
    probs[0, 10] = np.nan
    probs[1, 4] = 0.0
    for F, tol in ((np.float64, 1e-13), (F32, 6 * 2.0 ** -22)):
        post, filt, cls, ev, carry = R.loops(probs, sc, trans, F=F)
        assert post.dtype == F and np.isfinite(post).all() and np.isfinite(filt).all() and np.isfinite(ev).all()
        for rows in (post, filt, cls):
            assert np.abs(rows.sum(axis=-1, dtype=np.float64) - 1.0).max() <= tol
        assert O.bits(post[:, -1]) == O.bits(filt[:, -1])
        assert cls.shape == (2, 30, 4) and np.abs(cls[..., 0] - (post[..., 0].astype(np.float64) + post[..., 4])).max() <= tol
    a, b = R.loops64(probs, sc, trans), R.loops32(probs, sc, trans)
    assert max(np.abs(a[i] - b[i]).max() for i in range(3)) <= 1e-4 and np.abs(a[3] - b[3]).max() <= 1e-4 * np.abs(a[3]).max()


def test_an_all_floor_table_and_rows_nothing_is_infinite():
    """every transition -65536 and every probability NaN: 288 bits down per frame, and every row is still a distribution (the
    start vector of zeros weighs 5, which the first frame's c takes in)"""
    S = 5
    probs = np.full((1, 40, S), np.nan, F32)
    trans = np.full((S, S), -65536)
    for F in (np.float64, F32):
        post, filt, cls, ev, carry = R.loops(probs, np.arange(S), trans, F=F)
        assert np.abs(post - 0.2).max() <= 1e-6 and np.abs(filt - 0.2).max() <= 1e-6
        assert abs(ev[0] - (40 * (-32 - 256 + np.log2(5)) + np.log2(5))) <= 1e-3 and carry[0, 1] == ev[0]
        got = R.tiled(probs, np.arange(S), trans, tile=7, F=F)
        assert np.abs(got[0] - 0.2).max() <= 1e-6 and abs(got[3][0] - ev[0]) <= 1e-3


def test_every_split_of_a_stream_gives_the_bits_of_one_call():
    """filtered, the evidence total and the carry in bits, in f32 as in float64; the last call's posterior is the one-call
    posterior on its frames"""
    T, C = 24, 5
    probs, sc, trans = _case(3, 1, T, C, 6, run=4)
    probs[0, 7] = np.nan
    init = np.array([0, -100, -200, -300, -400, -500])
    for F in (np.float64, F32):
        whole = R.loops(probs, sc, trans, init, F=F)
        for cut in range(1, T):
            first = R.loops(probs[:, :cut], sc, trans, init, F=F)
            second = R.loops(probs[:, cut:], sc, trans, init, first[4], F=F)
            assert O.bits(np.concatenate([first[1], second[1]], axis=1)) == O.bits(whole[1]), cut
            assert O.bits(second[4]) == O.bits(whole[4]) and O.bits(second[0]) == O.bits(whole[0][:, cut:]), cut


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    declared = set(re.findall(r"\b(qt_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(os.path.join(ROOT, PKG, "libqtcnn_hip.so"))
    for symbol in ("qt_pose_posterior_workspace_bytes", "qt_pose_posterior"):
        assert symbol in declared and hasattr(lib, symbol), symbol
    P, M = pkg(), pkg("pose_order")
    assert P.PosePosterior is M.PosePosterior and "PosePosterior" in P.__all__
    src = pose_chain_header() + open(os.path.join(ROOT, PKG, "csrc", "pose_posterior.hip")).read()
    body = re.search(r"PC_LOG2\[256\] = \{(.*?)\};", src, re.S).group(1)
    assert [int(v) for v in re.findall(r"\d+", body)] == list(O.LOG2_TABLE)
    const = lambda name: int(re.search(rf"constexpr int {name} = (-?\d+);", src).group(1))
    assert (const("PC_TILE"), const("PC_MAX_S"), const("PC_MAX_C"), const("PC_FLOOR"), const("PC_TRANS_FLOOR")) == \
        (O.TILE, O.MAX_STATES, O.MAX_CLASSES, O.SCORE_FLOOR, O.TRANS_FLOOR)
    for S in (1, 2, 3, 11, 12, 13, 16, 17, 45, 46, 63, 64):
        assert M.posterior_scan_trip_tiles(S) == max(1, min(const("PP_SCAN_MAX_TILES"), const("PP_SCAN_FLOATS") // (S * S)))


def _lib():
    M = pkg("pose_order")
    L = pkg("_lib").lib()
    return M, L


def test_workspace_query():
    M, L = _lib()
    q = lambda *a: L.qt_pose_posterior_workspace_bytes(ctypes.byref(M.PoseOrderDesc(*a)))
    for frames in (1, 2, R.TILE):
        assert q(3, frames, 12, 12) == 0
    B, T, S, tiles = 3, 2 * R.TILE + 3, 12, 3
    assert q(B, T, 12, S) == B * tiles * (S * 8 + 8 + S * S * 4 + S * 4 + S * 4)
    assert q(1, R.TILE + 1, 64, 64) == 2 * (64 * 8 + 8 + 64 * 64 * 4 + 64 * 4 + 64 * 4)
    assert q(0, 100, 12, 12) == 0 and q(1, 100, 12, 65) == 0 and q(1, 100, 0, 12) == 0 and q(2, 1 << 20, 12, 12) == 0
    assert L.qt_pose_posterior_workspace_bytes(None) == 0


def test_argument_checks_need_no_device():
    """every refusal comes before the first device call: the pointers are never dereferenced"""
    M, L = _lib()
    D = lambda batch=2, frames=100, C=12, S=12: M.PoseOrderDesc(batch, frames, C, S)
    probs, sc, trans, init, carry, post, filt, cls, ev, ws = (0x10000000 * k for k in range(1, 11))
    good = dict(probs=probs, ld=12, sc=sc, trans=trans, init=init, carry=carry, post=post, filt=filt, cls=cls, ev=ev, ws=ws,
                ws_bytes=1 << 24)

    def call(desc, **kw):
        a = {**good, **kw}
        return L.qt_pose_posterior(ctypes.byref(desc), a["probs"], a["ld"], a["sc"], a["trans"], a["init"], a["carry"], a["post"],
                                   a["filt"], a["cls"], a["ev"], a["ws"], a["ws_bytes"], None)

    def refused(rc, word, status=QT_ERR_INVALID_ARG):
        assert rc == status and word in L.qt_last_error(), (rc, L.qt_last_error())

    refused(L.qt_pose_posterior(None, probs, 12, sc, trans, init, carry, post, filt, cls, ev, ws, 1 << 24, None), b"null descriptor")
    for batch in (0, -3):
        refused(call(D(batch=batch)), b"batch")
    for frames in (0, -1):
        refused(call(D(frames=frames)), b"frames")
    for C in (0, -1, 65):
        refused(call(D(C=C), ld=70), b"num_classes")
    for S in (0, -1, 65):
        refused(call(D(S=S)), b"num_states")
    refused(call(D(), ld=11), b"ld")
    for name in ("probs", "sc", "trans", "carry", "post"):
        refused(call(D(), **{name: None}), b"null")
    refused(call(D(), post=None), b"null posterior")
    for name, off in (("probs", 2), ("sc", 1), ("trans", 3), ("init", 2), ("post", 1), ("filt", 2), ("cls", 3), ("carry", 4),
                      ("ev", 4), ("ws", 4)):
        refused(call(D(), **{name: good[name] + off}), b"aligned")
    need = L.qt_pose_posterior_workspace_bytes(ctypes.byref(D()))
    assert need > 0
    refused(call(D(), ws_bytes=need - 1), b"workspace")
    refused(call(D(), ws_bytes=0), b"workspace")
    refused(call(D(), ws=None), b"workspace")
    rows = 2 * 100
    for out, nbytes in (("carry", 2 * 14 * 8), ("post", rows * 12 * 4), ("filt", rows * 12 * 4), ("cls", rows * 12 * 4),
                        ("ev", 2 * 8), ("ws", need)):
        refused(call(D(), **{out: probs + (rows * 12 - 2) * 4}), b"overlap")
        refused(call(D(), **{out: probs - nbytes + 8}), b"overlap")
        refused(call(D(), **{out: sc + 40}), b"overlap")
        refused(call(D(), **{out: trans + (144 - 2) * 4}), b"overlap")
        refused(call(D(), **{out: init}), b"overlap")
    refused(call(D(), ld=16, post=probs + (199 * 16 + 10) * 4), b"overlap")
    refused(call(D(), filt=post + 8), b"overlap")
    refused(call(D(), cls=filt + rows * 12 * 4 - 8), b"overlap")
    refused(call(D(), ev=carry + 8), b"overlap")
    refused(call(D(batch=1 << 10, frames=(1 << 10) + 1)), b"frames", QT_ERR_UNSUPPORTED)
    refused(call(D(batch=1, frames=(1 << 20) + 1)), b"frames", QT_ERR_UNSUPPORTED)
    # the short route asks for no workspace: a null one is not refused for being null (the next check is reached)
    refused(call(D(frames=R.TILE), ws=None, ws_bytes=0, post=None), b"null posterior")


def test_module_argument_checks_need_no_device():
    P = pkg()
    sc, trans = P.cyclic_prior(range(4), -10, -100)
    for bad in (dict(state_class=[]), dict(state_class=list(range(65)), trans=np.zeros((65, 65), int)), dict(state_class=[0, 1, 2, 64]),
                dict(state_class=[0, -1, 2, 3]), dict(state_class=np.zeros(4)), dict(trans=trans[:3]), dict(trans=trans.astype(float)),
                dict(trans=trans - 65536), dict(trans=-trans), dict(init=[0, 0, 0]), dict(init=np.array([0, 0, 0, 1])),
                dict(init=np.zeros(4)), dict(streams=0), dict(streams=True), dict(streams=2.0), dict(class_names=["a", "b", "c"])):
        with pytest.raises(ValueError, match="PosePosterior"):
            P.PosePosterior(**{"state_class": sc, "trans": trans, "device": "cuda:0", **bad})
    with pytest.raises(P.QtError, match="AMD GPU"):      # no torch fallback
        P.PosePosterior(sc, trans, "cpu")


def test_the_documents_speak_of_the_posterior():
    for doc, word in (("DESIGN.md", "Pose posterior"), ("DESIGN.md", "(L, +)"), ("README.md", "PosePosterior"),
                      ("EXPERIMENTS.md", "Pose posterior"), ("INTEGRATION.md", "posterior.smooth("),
                      (os.path.join("scripts", "bench_pose_posterior.py"), "qt_pose_posterior")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc
    for doc in ("DESIGN.md", os.path.join(PKG, "pose_order.py")):
        text = open(os.path.join(ROOT, doc)).read()
        assert "Not built: forward-backward posteriors" not in text, doc
