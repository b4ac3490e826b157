"""Fixed-lag pose-order posteriors and revised paths, the parts that need no GPU: the loops of tests/_pose_lag_ref.py against the
full posterior / decode of every prefix, the rule's corner statements (lag 0 is filtered, a lag that reaches the end is the full
answer, a split changes no bit), the arithmetic of the emitted span, the C ABI's declaration, every host-side refusal (pointers
that are never dereferenced), the size queries, the module's argument checks, the exports and the documents."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import _pose_lag_ref as G
import _pose_order_ref as O
import _pose_posterior_ref as R
from _util import PKG, ROOT, pkg

QT_ERR_INVALID_ARG, QT_ERR_UNSUPPORTED = -1, -3
F32, F64 = np.float32, np.float64


def _case(seed, B, T, C, S, run=3):
    probs = O.make_probs(seed, B, T, C, run=run)
    sc, trans = O.cyclic_prior([s % C for s in range(S)], -30, -600, skip=-3000, other=-20000)
    return probs, sc, trans


def test_every_lagged_row_is_the_full_posterior_of_its_prefix():
    """23 frames, S = 3: lagged[g] is row g of the float64 posterior of frames [0, min(g + lag, last)], lag_path[g] is path[g] of
    the decode of that prefix"""
    T = 23
    probs, sc, trans = _case(11, 2, T, 3, 3, run=2)
    probs[0, 9] = np.nan
    for init in (None, np.array([0, -700, -90])):
        prefix = [R.loops64(probs[:, :w + 1], sc, trans, init) for w in range(T)]
        paths = [O.decode(probs[:, :w + 1], sc, trans, init) for w in range(T)]
        for lag in (0, 1, 5, 22, 40):
            g0, (lagged, cls, filt, ev), state = G.smooth(probs, sc, trans, init, lag=lag, flush=True)
            p0, (path, pfilt), pstate = G.decode(probs, sc, trans, init, lag=lag, flush=True)
            assert g0 == 0 and p0 == 0 and lagged.shape == (2, T, 3) and path.shape == (2, T)
            for g in range(T):
                w = min(g + lag, T - 1)
                assert np.abs(lagged[:, g] - prefix[w][0][:, g]).max() <= 1e-12, (lag, g)
                assert np.abs(cls[:, g] - prefix[w][2][:, g]).max() <= 1e-12, (lag, g)
                assert (path[:, g] == paths[w][0][:, g]).all(), (lag, g)
            assert np.abs(filt - prefix[-1][1]).max() <= 1e-12 and (pfilt == paths[-1][1]).all()
            assert np.abs(ev - prefix[-1][3]).max() <= 1e-12 * np.abs(ev).max()
            if lag == 0:
                assert O.bits(lagged) == O.bits(filt) and (path == pfilt).all()
            if lag >= T - 1:
                assert np.abs(lagged - prefix[-1][0]).max() <= 1e-12 and (path == paths[-1][0]).all()
            assert state["seen"] == T and (pstate["delta"].max(axis=1) == 0).all()
            assert (pstate["offset"] == paths[-1][3][:, 1]).all() and (pstate["delta"] == paths[-1][3][:, 2:]).all()


def test_a_short_flush_is_the_posterior_rule_in_bits():
    """one call with flush and n <= lag + 1: the f32 loops give the bits of the posterior's f32 loops"""
    probs, sc, trans = _case(3, 2, 9, 4, 6)
    for F in (F32, F64):
        want = R.loops(probs, sc, trans, None, F=F)
        _, (lagged, cls, filt, ev), _ = G.smooth(probs, sc, trans, None, lag=8, flush=True, F=F)
        assert O.bits(lagged) == O.bits(want[0]) and O.bits(filt) == O.bits(want[1]) and O.bits(cls) == O.bits(want[2])
        assert O.bits(ev) == O.bits(want[3])


def test_every_split_keeps_the_bits():
    """a 40-frame stream at lag 5, flush on the last call: every split into two calls and into three gives the one-call outputs
    and state, in bits for the f32 (and float64) loops and exactly for the integers"""
    T, lag = 40, 5
    probs, sc, trans = _case(21, 2, T, 4, 5)
    probs[1, 17] = 0.0
    init = np.array([0, -40, -900, -5, -300])
    whole32 = G.split(G.smooth, probs, [], sc, trans, init, lag=lag, F=F32)
    whole64 = G.split(G.smooth, probs, [], sc, trans, init, lag=lag, F=F64)
    wholei = G.split(G.decode, probs, [], sc, trans, init, lag=lag)
    assert whole32[1][0].shape == (2, T, 5) and wholei[1][0].shape == (2, T)
    threes = [c for c in itertools.combinations(range(1, T), 2)]
    for cuts in [[c] for c in range(1, T)] + [list(c) for c in threes]:
        full = len(cuts) == 1 or cuts in ([1, 2], [5, 6], [5, 10], [6, 11], [4, 39], [38, 39], [13, 30], [20, 26])
        for whole, F in ((whole32, F32),) + (((whole64, F64),) if full else ()):
            g0, joined, state, calls = G.split(G.smooth, probs, cuts, sc, trans, init, lag=lag, F=F)
            assert g0 == 0 and all(O.bits(a) == O.bits(b) for a, b in zip(joined[:3], whole[1][:3])), cuts
            G.same_state(state, whole[2])
            assert np.abs(joined[3] - whole[1][3]).max() <= 1e-9 * np.abs(whole[1][3]).max()
            spans = [G.span(a, b - a, lag, k == len(cuts)) for k, (a, b) in enumerate(zip([0] + cuts, cuts + [T]))]
            assert [c[1][0].shape[1] for c in calls] == [g1 - g0 for g0, g1 in spans] and [c[0] for c in calls] == [g0 for g0, _ in spans]
        g0, joined, state, _ = G.split(G.decode, probs, cuts, sc, trans, init, lag=lag)
        assert g0 == 0 and (joined[0] == wholei[1][0]).all() and (joined[1] == wholei[1][1]).all(), cuts
        G.same_state(state, wholei[2])


def test_a_flush_without_frames_and_a_stream_without_flush():
    """no flush: the last lag frames stay pending; a later call with frames == 0 and flush emits them, conditioned on the same
    frames as a flush in the last call"""
    T, lag = 17, 4
    probs, sc, trans = _case(8, 1, T, 3, 4)
    for fn in (G.smooth, G.decode):
        kw = dict(F=F32) if fn is G.smooth else {}
        _, want, want_state = fn(probs, sc, trans, None, lag=lag, flush=True, **kw)
        g0, first, state = fn(probs, sc, trans, None, lag=lag, flush=False, **kw)
        assert g0 == 0 and first[0].shape[1] == T - lag
        g0, rest, state = fn(probs[:, :0], sc, trans, None, lag=lag, flush=True, state=state, **kw)
        assert g0 == T - lag and rest[0].shape[1] == lag and rest[2 if fn is G.smooth else 1].shape[1] == 0
        assert O.bits(np.concatenate([first[0], rest[0]], axis=1)) == O.bits(want[0])
        G.same_state(state, want_state)


def test_the_emitted_span():
    assert G.span(0, 1, 16, False) == (0, 0) and G.span(15, 1, 16, False) == (0, 0) and G.span(16, 1, 16, False) == (0, 1)
    assert G.span(17, 1, 16, False) == (1, 2) and G.span(17, 0, 16, True) == (1, 17) and G.span(3, 0, 16, True) == (0, 3)
    assert G.span(0, 5, 0, False) == (0, 5) and G.span(7, 5, 0, True) == (7, 12) and G.span(0, 0, 3, True) == (0, 0)
    for lag in (0, 1, 5, 63):
        for sizes in ([1] * 12, [3, 1, 7, 64, 2], [70], [lag + 1, lag, 1]):
            seen, nxt = 0, 0
            for k, n in enumerate(sizes):
                g0, g1 = G.span(seen, n, lag, k == len(sizes) - 1)
                assert g0 == nxt and g1 >= g0                   # the calls' spans adjoin
                seen, nxt = seen + n, g1
            assert nxt == sum(sizes)


def _lib():
    M = pkg("pose_order")
    L = pkg("_lib").lib()
    return M, L


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    declared = set(re.findall(r"\b(qt_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(os.path.join(ROOT, PKG, "libqtcnn_hip.so"))
    for symbol in ("qt_pose_lag_smooth", "qt_pose_lag_decode", "qt_pose_lag_smooth_carry_bytes", "qt_pose_lag_decode_carry_bytes",
                   "qt_pose_lag_smooth_workspace_bytes", "qt_pose_lag_decode_workspace_bytes"):
        assert symbol in declared and hasattr(lib, symbol), symbol
    assert int(re.search(r"#define QT_POSE_LAG_MAX (\d+)", header).group(1)) == G.LAG_MAX == pkg("pose_order").LAG_MAX
    P, M = pkg(), pkg("pose_order")
    for name in ("PoseLagSmoother", "PoseLagDecoder"):
        assert getattr(P, name) is getattr(M, name) and name in P.__all__


def test_size_queries(monkeypatch):
    M, L = _lib()
    D = lambda batch=2, frames=1, C=12, S=12, lag=16, flush=0, seen=0: M.PoseLagDesc(batch, frames, C, S, lag, flush, seen)
    queries = (L.qt_pose_lag_smooth_carry_bytes, L.qt_pose_lag_decode_carry_bytes, L.qt_pose_lag_smooth_workspace_bytes,
               L.qt_pose_lag_decode_workspace_bytes)
    monkeypatch.delenv("QTCNN_POSE_LAG", raising=False)
    for S, lag in ((1, 0), (1, 1), (3, 5), (12, 16), (13, 63), (64, 63)):
        assert L.qt_pose_lag_smooth_carry_bytes(ctypes.byref(D(batch=3, S=S, lag=lag))) == 3 * G.smooth_carry_stride(S, lag)
        assert L.qt_pose_lag_decode_carry_bytes(ctypes.byref(D(batch=3, S=S, lag=lag))) == 3 * G.decode_carry_stride(S, lag)
        assert G.smooth_carry_stride(S, lag) % 8 == 0 and G.decode_carry_stride(S, lag) % 8 == 0
    for bad in (D(batch=0), D(frames=-1), D(frames=0), D(C=0), D(C=65), D(S=0), D(S=65), D(lag=-1), D(lag=64), D(seen=-1),
                D(batch=2, frames=(1 << 19) + 1)):
        for query in queries:
            assert query(ctypes.byref(bad)) == 0
    for query in queries:
        assert query(None) == 0
    # the live route (few dependent steps, or forced) needs no workspace; the batch route's is 8-byte aligned
    for d in (D(frames=1), D(frames=1, lag=63), D(frames=3, lag=4), D(frames=0, flush=1, seen=40), D(frames=16, lag=0)):
        assert L.qt_pose_lag_smooth_workspace_bytes(ctypes.byref(d)) == 0 and L.qt_pose_lag_decode_workspace_bytes(ctypes.byref(d)) == 0
    for frames, lag in itertools.product((1, 2, 3, 4, 16, 17, 64, 240, 241, 4096, 4097), (0, 1, 5, 16, 63)):
        d = D(frames=frames, lag=lag)
        assert (L.qt_pose_lag_smooth_workspace_bytes(ctypes.byref(d)) == 0) == G.live("smooth", frames, lag), (frames, lag)
        assert (L.qt_pose_lag_decode_workspace_bytes(ctypes.byref(d)) == 0) == G.live("decode", frames, lag), (frames, lag)
    for S in (1, 3, 12, 13, 64):
        d = D(batch=3, frames=300, S=S)
        ws, wd = L.qt_pose_lag_smooth_workspace_bytes(ctypes.byref(d)), L.qt_pose_lag_decode_workspace_bytes(ctypes.byref(d))
        assert ws >= 3 * 300 * S * 6 and ws % 8 == 0 and wd >= 3 * 300 * (S + 4) and wd % 8 == 0
        monkeypatch.setenv("QTCNN_POSE_LAG", "1")
        assert L.qt_pose_lag_smooth_workspace_bytes(ctypes.byref(d)) == 0 and L.qt_pose_lag_decode_workspace_bytes(ctypes.byref(d)) == 0
        monkeypatch.setenv("QTCNN_POSE_LAG", "2")
        assert L.qt_pose_lag_smooth_workspace_bytes(ctypes.byref(d)) == ws
        assert L.qt_pose_lag_smooth_workspace_bytes(ctypes.byref(D(batch=3, frames=1, S=S))) == (3 * S * 6 + 7) // 8 * 8
        monkeypatch.delenv("QTCNN_POSE_LAG")


def test_argument_checks_need_no_device(monkeypatch):
    """every refusal comes before the first device call: the pointers are never dereferenced"""
    monkeypatch.delenv("QTCNN_POSE_LAG", raising=False)
    M, L = _lib()
    D = lambda batch=2, frames=300, C=12, S=12, lag=16, flush=0, seen=50: M.PoseLagDesc(batch, frames, C, S, lag, flush, seen)
    probs, sc, trans, init, cin, cout, out, cls, filt, ev, ws = (0x10000000 * k for k in range(1, 12))
    good = dict(probs=probs, ld=12, sc=sc, trans=trans, init=init, cin=cin, cout=cout, out=out, cls=cls, filt=filt, ev=ev, ws=ws,
                ws_bytes=1 << 24)

    def smooth(desc, **kw):
        a = {**good, **kw}
        return L.qt_pose_lag_smooth(None if desc is None else ctypes.byref(desc), a["probs"], a["ld"], a["sc"], a["trans"], a["init"],
                                    a["cin"], a["cout"], a["out"], a["cls"], a["filt"], a["ev"], a["ws"], a["ws_bytes"], None)

    def decode(desc, **kw):
        a = {**good, **kw}
        return L.qt_pose_lag_decode(None if desc is None else ctypes.byref(desc), a["probs"], a["ld"], a["sc"], a["trans"], a["init"],
                                    a["cin"], a["cout"], a["out"], a["filt"], a["ws"], a["ws_bytes"], None)

    def refused(rc, word, status=QT_ERR_INVALID_ARG):
        assert rc == status and word in L.qt_last_error(), (rc, L.qt_last_error())

    rows = 2 * 300                                                                  # D(): both calls on the batch route
    for call, carry, need, outs in (
            (smooth, 2 * G.smooth_carry_stride(12, 16), L.qt_pose_lag_smooth_workspace_bytes(ctypes.byref(D())),
             (("out", rows * 12 * 4), ("cls", rows * 12 * 4), ("filt", rows * 12 * 4), ("ev", 16))),
            (decode, 2 * G.decode_carry_stride(12, 16), L.qt_pose_lag_decode_workspace_bytes(ctypes.byref(D())),
             (("out", rows * 8), ("filt", rows * 8)))):
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
        for lag in (-1, 64, 1000):
            refused(call(D(lag=lag)), b"lag")
        refused(call(D(seen=-1)), b"seen")
        refused(call(D(), ld=11), b"ld")
        for name in ("probs", "sc", "trans", "cout"):
            refused(call(D(), **{name: None}), b"null")
        refused(call(D(), out=None), b"null lag")                                   # count = 300 > 0
        refused(call(D(seen=3, frames=13, lag=16), out=None, cin=None), b"carry_in")    # count == 0: out may be null, the carry not
        refused(call(D(), cin=None), b"null carry_in")
        refused(call(D(seen=0, frames=20, lag=16), out=None, cin=None), b"null lag")    # seen == 0: no carry_in; count = 4
        refused(call(D(frames=0, flush=1, seen=9), out=None, probs=None), b"null lag")  # a flush alone still emits
        for name, off in (("probs", 2), ("sc", 1), ("trans", 3), ("init", 2), ("out", 1), ("filt", 2), ("cin", 4), ("cout", 4),
                          ("ws", 4)) + ((("cls", 3), ("ev", 4)) if call is smooth else ()):
            refused(call(D(), **{name: good[name] + off}), b"aligned")
        assert need > 0 and need % 8 == 0
        refused(call(D(), ws_bytes=need - 1), b"workspace")
        refused(call(D(), ws_bytes=0), b"workspace")
        refused(call(D(), ws=None), b"workspace")
        refused(call(D(), cin=cout + carry - 8), b"carry_in must not overlap carry_out")
        refused(call(D(), cin=cout), b"carry_in must not overlap carry_out")
        refused(call(D(), cout=cin + 8), b"carry_in must not overlap carry_out")
        for name, nbytes in outs + (("cout", carry), ("ws", need)):
            refused(call(D(), **{name: probs + (rows * 12 - 2) * 4}), b"overlap")
            refused(call(D(), **{name: probs - nbytes + 8}), b"overlap")
            refused(call(D(), **{name: sc + 40}), b"overlap")
            refused(call(D(), **{name: trans + (144 - 2) * 4}), b"overlap")
            refused(call(D(), **{name: init}), b"overlap")
            if name != "cout":
                refused(call(D(), **{name: cin + carry - 8}), b"overlap")
                refused(call(D(), **{name: cout + 8}), b"overlap")
        refused(call(D(), filt=out + 8), b"overlap")
        refused(call(D(batch=1 << 10, frames=(1 << 10) + 1)), b"frames", QT_ERR_UNSUPPORTED)
        refused(call(D(batch=1, frames=(1 << 20) + 1)), b"frames", QT_ERR_UNSUPPORTED)
        # the live route asks for no workspace: a null one is not refused for being null (the next check is reached)
        refused(call(D(frames=1), ws=None, ws_bytes=0, cin=cout), b"carry_in must not overlap")
        # with seen == 0 carry_in is not looked at
        refused(call(D(seen=0, frames=1), cin=cout, filt=cout + 8), b"carry_out must not overlap filtered")


def test_module_argument_checks_need_no_device():
    P = pkg()
    sc, trans = P.cyclic_prior(range(4), -10, -100)
    for cls in (P.PoseLagSmoother, P.PoseLagDecoder):
        for bad in (dict(state_class=[]), dict(state_class=[0, 1, 2, 64]), dict(trans=trans[:3]), dict(trans=-trans),
                    dict(init=[0, 0, 0]), dict(streams=0), dict(streams=True), dict(class_names=["a", "b", "c"]),
                    dict(lag=-1), dict(lag=64), dict(lag=2.0), dict(lag=True), dict(lag=None)):
            with pytest.raises(ValueError, match=cls.__name__):
                cls(**{"state_class": sc, "trans": trans, "device": "cuda:0", "lag": 5, **bad})
        with pytest.raises(P.QtError, match="AMD GPU"):      # no torch fallback
            cls(sc, trans, "cpu", 5)


def test_the_documents_speak_of_the_fixed_lag():
    for doc, word in (("DESIGN.md", "Fixed-lag"), ("DESIGN.md", "QTCNN_POSE_LAG"), ("README.md", "PoseLagSmoother"),
                      ("EXPERIMENTS.md", "Fixed-lag"), ("INTEGRATION.md", "PoseLagSmoother("), ("INTEGRATION.md", "PoseLagDecoder("),
                      (os.path.join("scripts", "bench_pose_lag.py"), "qt_pose_lag_smooth")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc
    for doc in ("DESIGN.md", os.path.join(PKG, "pose_order.py")):
        text = open(os.path.join(ROOT, doc)).read()
        assert "fixed-lag revision of earlier calls' paths" not in text and "fixed-lag smoothing across calls" not in text, doc
