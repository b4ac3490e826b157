"""Pose-order posteriors with hold durations, the parts that need no GPU: the float64 loops of
tests/_pose_duration_posterior_ref.py against brute-force enumeration of every segmentation, against the plain chain's loops
where the two rules must coincide (D = 1; geometric durations with one segment per hold), their invariants, the mixed-precision
loops beside them, the host helper expected_duration_prior, the C ABI's declaration and every host-side refusal (pointers that
are never dereferenced), the exports and the documents."""
import ctypes
import os
import re

import numpy as np
import pytest

import _pose_duration_posterior_ref as P
import _pose_duration_ref as Q
import _pose_order_ref as R
import _pose_posterior_ref as PL
from _util import PKG, ROOT, pkg

QT_ERR_INVALID_ARG, QT_ERR_UNSUPPORTED = -1, -3
F32 = np.float32


def _chain(S, C, stay=-39, advance=-300):
    return R.cyclic_prior([s % C for s in range(S)], stay, advance, skip=-800, other=-3000)


def _durations(S, D, seed):
    rng = np.random.default_rng(seed)
    return (-rng.integers(0, 700, (S, D))).astype(np.int32)


# ---- the rule against enumeration -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,D", [(5, 2, 3), (6, 3, 2), (4, 3, 4), (1, 2, 3)])
def test_loops64_is_the_sum_over_every_segmentation(T, S, D):
    C = S
    probs = R.make_probs(10 * T + S, 1, T, C, run=2)
    sc, tr = R.cyclic_prior(range(S), -39, -300, other=-900)
    dur = _durations(S, D, T)
    for init in (None, -np.arange(S) * 41):
        for dur_open in (None, Q.suffix_max(dur)):
            post, cls, begin, ev, counts, endp = P.loops64(probs, sc, tr, dur, init, dur_open)
            b_post, b_begin, b_endp, b_ev, b_counts = P.brute(probs[0], sc, tr, dur, init, dur_open)
            for name, got, want in (("posterior", post[0], b_post), ("begin", begin[0], b_begin), ("endp", endp[0], b_endp),
                                    ("evidence", ev[0], b_ev), ("dur_counts", counts, b_counts)):
                assert np.abs(got - want).max() <= 1e-12, (name, T, S, D, init is None, dur_open is None)
            assert np.abs(cls[0] - post[0]).max() == 0                    # state j emits class j
            assert T < 4 or counts.sum() > 1e-3


def test_a_table_of_one_frame_is_the_plain_chain():
    """D = 1 and dur all zero: every frame is a segment, and posterior and evidence are the plain chain's from a zeroed carry"""
    for S, C, B, T in ((1, 1, 1, 3), (6, 5, 2, 40), (12, 12, 1, 150)):
        probs = R.make_probs(3 * S + T, B, T, C, run=4)
        sc, tr = _chain(S, C)
        for init in (None, -np.arange(S) * 37):
            post, cls, begin, ev, counts, _ = P.loops64(probs, sc, tr, np.zeros((S, 1), np.int32), init)
            want = PL.loops64(probs, sc, tr, init)
            assert np.abs(post - want[0]).max() <= 1e-9 and np.abs(cls - want[2]).max() <= 1e-9, (S, T)
            assert np.abs(ev - want[3]).max() <= 1e-9 * max(1.0, np.abs(want[3]).max())
            assert np.abs(begin - post).max() <= 1e-9                      # a hold begins at every frame it covers
            assert abs(counts.sum() - B * max(T - 2, 0)) <= 1e-9           # every interior frame is an uncut segment


def test_geometric_durations_with_one_segment_per_hold_are_the_plain_chain():
    """dur[j][d - 1] = (d - 1) stay, dur_open NULL and D >= T, with -65536 on the diagonal of the duration chain's trans (a hold
    has one segmentation: joining two segments of one state costs 256 bits) and stay on the diagonal of the plain chain's"""
    stay = -39
    for S, C, B, T in ((2, 2, 1, 9), (6, 5, 2, 60), (12, 12, 1, 128)):
        D = max(T, 2)
        assert (D - 1) * stay >= R.TRANS_FLOOR
        probs = R.make_probs(7 * S + T, B, T, C, run=5)
        sc, plain = _chain(S, C, stay=stay)
        single = np.array(plain)
        np.fill_diagonal(single, R.TRANS_FLOOR)
        init = -np.arange(S) * 29
        # the plain chain's first frame may follow a stay from the start vector; give both chains the same start scores
        post, cls, _, ev, _, _ = P.loops64(probs, sc, single, Q.geometric_durations(stay, S, D), init)
        start = PL.L((init[:, None] + single) / 256.0, 0, np.float64)
        want = _plain_from(probs, sc, plain, (start[0] + start[1]))
        assert np.abs(post - want[0]).max() <= 1e-9, (S, T)
        assert (np.abs(ev - want[1]) / np.maximum(1.0, np.abs(want[1]))).max() <= 1e-9


def _plain_from(probs, sc, trans, bt0):
    """the plain chain's forward-backward in float64 from given scores Bt[0][j] before the first frame (posterior, evidence)"""
    B, T, C = probs.shape
    S = len(sc)
    Tm = R.clamp_trans(trans) / 256.0
    post, ev = np.empty((B, T, S)), np.empty(B)
    lse = lambda x, axis: np.log2(np.exp2(x - x.max(axis=axis, keepdims=True)).sum(axis=axis)) + x.max(axis=axis)
    for b in range(B):
        E = R.emissions(probs[b], sc) / 256.0
        a = np.empty((T, S))
        a[0] = bt0 + E[0]
        for f in range(1, T):
            a[f] = lse(a[f - 1][:, None] + Tm, 0) + E[f]
        be = np.zeros((T, S))
        for f in range(T - 2, -1, -1):
            be[f] = lse(Tm + (E[f + 1] + be[f + 1])[None, :], 1)
        ev[b] = lse(a[-1], 0)
        post[b] = np.exp2(a + be - ev[b])
    return post, ev


def test_the_plain_helper_is_the_plain_chain():
    """_plain_from from L_i (start[i] + T[i][j]) is tests/_pose_posterior_ref.py's loops64"""
    S = C = 5
    probs = R.make_probs(2, 2, 30, C, run=4)
    sc, tr = _chain(S, C)
    init = -np.arange(S) * 29
    start = PL.L((init[:, None] + tr) / 256.0, 0, np.float64)
    got, want = _plain_from(probs, sc, tr, start[0] + start[1]), PL.loops64(probs, sc, tr, init)
    assert np.abs(got[0] - want[0]).max() <= 1e-9 and np.abs(got[1] - want[3]).max() <= 1e-9


# ---- invariants --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,D,T", [(3, 3, 4, 30), (12, 12, 16, 200), (17, 12, 8, 70)])
def test_invariants(S, C, D, T):
    B = 3
    probs = R.make_probs(S + D + T, B, T, C)
    probs[0, T // 2] = np.nan
    sc, tr = _chain(S, C)
    dur = _durations(S, D, 5)
    open_ = Q.suffix_max(dur)
    lengths = np.array([T, 1, T // 2 + 1], np.int32)
    init = -np.arange(S) * 17
    post, cls, begin, ev, counts, endp = P.loops64(probs, sc, tr, dur, init, open_, lengths)
    _, _, score = Q.decode(probs, sc, tr, dur, init, open_, lengths)
    for b, n in enumerate(lengths):
        assert np.abs(post[b, :n].sum(axis=1) - 1).max() <= 1e-9 and np.abs(cls[b, :n].sum(axis=1) - 1).max() <= 1e-9
        assert not post[b, n:].any() and not begin[b, n:].any() and not cls[b, n:].any()
        assert np.abs(begin[b].sum(axis=0) - endp[b].sum(axis=0)).max() <= 1e-9          # every hold that begins also ends
        assert ev[b] >= score[b] / 256.0 - 1e-9                                          # the best path is one of the sum
        alone = P.loops64(probs[b:b + 1, :n], sc, tr, dur, init, open_)
        assert R.bits(alone[0][0]) == R.bits(post[b, :n]) and R.bits(alone[3]) == R.bits(ev[b:b + 1])
    assert (post >= 0).all() and counts.shape == (S, D) and (counts >= 0).all()
    # the precision of the rule, beside the rule: f32 inside an L, double levels
    mixed = P.loops_mixed(probs, sc, tr, dur, init, open_, lengths)
    assert mixed[0].dtype == F32 and mixed[2].dtype == F32 and mixed[3].dtype == np.float64 and mixed[4].dtype == np.float64
    assert max(np.abs(m - w).max() for m, w in zip(mixed[:3], (post, cls, begin))) <= 1e-4
    assert (np.abs(mixed[3] - ev) / np.maximum(1.0, np.abs(ev))).max() <= 1e-6


# ---- the host helper ---------------------------------------------------------------------------------------------------------------
def test_expected_duration_prior():
    M = pkg("pose_order")
    counts = np.array([[1, 3, 0, 0], [0, 0, 0, 0], [5, 0, 0, 2]])
    for pseudo in (1.0, 0, 0.5):
        got = M.expected_duration_prior(counts.astype(np.float64), pseudo)
        assert got.dtype == np.int32 and R.bits(got) == R.bits(M.duration_prior(counts, pseudo))
        assert R.bits(M.expected_duration_prior(counts, pseudo)) == R.bits(got)          # integers are real numbers too
    soft = M.expected_duration_prior(np.array([[0.5, 1.5], [0.25, 0.25]]), pseudo_count=0)
    assert soft.tolist() == [[-511, -106], [-255, -255]]                         # prob_score of 1/4, 3/4 and 1/2
    assert M.expected_duration_prior(np.zeros((2, 3)), 0).tolist() == [[-8192] * 3] * 2
    for bad in (lambda: M.expected_duration_prior([[1.0, -0.5]]), lambda: M.expected_duration_prior([[1.0, np.nan]]),
                lambda: M.expected_duration_prior([[np.inf, 1.0]]), lambda: M.expected_duration_prior([1.0, 2.0]),
                lambda: M.expected_duration_prior(np.zeros((2, 129))), lambda: M.expected_duration_prior(np.zeros((65, 2))),
                lambda: M.expected_duration_prior(np.zeros((0, 2))), lambda: M.expected_duration_prior(np.zeros((2, 2), complex)),
                lambda: M.expected_duration_prior([["a", "b"]]), lambda: M.expected_duration_prior([[1.0, 2.0]], -1.0),
                lambda: M.expected_duration_prior([[1.0, 2.0]], float("inf")), lambda: M.expected_duration_prior([[1.0, 2.0]], True),
                lambda: M.expected_duration_prior([[1.0, 2.0]], "1")):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError):
        M.duration_prior(np.zeros((2, 3)))                                 # the integer helper keeps refusing floats


# ---- the library -------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    declared = set(re.findall(r"\b(qt_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(os.path.join(ROOT, PKG, "libqtcnn_hip.so"))
    for symbol in ("qt_pose_duration_posterior_workspace_bytes", "qt_pose_duration_posterior"):
        assert symbol in declared and hasattr(lib, symbol), symbol
    src = open(os.path.join(ROOT, PKG, "csrc", "pose_duration_posterior.hip")).read()
    assert '#include "pose_chain.h"' in src and not re.search(r"_LOG2\[256\]\s*=|\b\w*_FLOOR\s*=(?!=)", re.sub(r"//[^\n]*", "", src))
    P_, M = pkg(), pkg("pose_order")
    assert P_.PoseDurationPosterior is M.PoseDurationPosterior and P_.expected_duration_prior is M.expected_duration_prior
    assert {"PoseDurationPosterior", "expected_duration_prior"} <= set(P_.__all__)
    assert issubclass(M.PoseDurationPosterior, M._PoseDurationTables) and issubclass(M.PoseDurationDecoder, M._PoseDurationTables)


def _lib():
    M = pkg("pose_order")
    L = pkg("_lib").lib()
    return M, L


def test_workspace_query():
    M, L = _lib()
    q = lambda *a: L.qt_pose_duration_posterior_workspace_bytes(ctypes.byref(M.PoseDurationDesc(*a)))
    assert q(3, 100, 12, 12, 64) == 8 * (2 * 3 * 100 * 12 + 3 * 12 * 64) and q(1, 1, 1, 1, 1) == 24
    for bad in ((0, 100, 12, 12, 64), (3, 0, 12, 12, 64), (3, 100, 65, 12, 64), (3, 100, 12, 65, 64), (3, 100, 12, 12, 0),
                (3, 100, 12, 12, 129), (3, 100, 12, 12, -1), (1 << 10, (1 << 10) + 1, 12, 12, 64)):
        assert q(*bad) == 0, bad
    assert L.qt_pose_duration_posterior_workspace_bytes(None) == 0


def test_argument_checks_need_no_device():
    """every refusal comes before the first device call: the pointers are never dereferenced"""
    M, L = _lib()
    D = lambda batch=2, frames=100, C=12, S=12, dmax=16: M.PoseDurationDesc(batch, frames, C, S, dmax)
    names = ("probs", "sc", "trans", "init", "dur", "dur_open", "lengths", "posterior", "cls", "begin", "ev", "counts", "ws")
    order = ("probs", "ld", "sc", "trans", "init", "dur", "dur_open", "lengths", "posterior", "cls", "begin", "ev", "counts", "ws",
             "ws_bytes")
    good = {n: 0x10000000 * k for k, n in enumerate(names, 1)}
    good.update(ld=12, ws_bytes=1 << 24)

    def call(desc, **kw):
        a = {**good, **kw}
        return L.qt_pose_duration_posterior(ctypes.byref(desc), *[a[n] for n in order], None)

    def refused(rc, word, status=QT_ERR_INVALID_ARG):
        assert rc == status and word in L.qt_last_error(), (rc, L.qt_last_error())

    refused(L.qt_pose_duration_posterior(None, *[good[n] for n in order], None), b"null descriptor")
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
    for name, word in (("probs", b"null probs"), ("sc", b"null state_class"), ("trans", b"null trans"), ("dur", b"null dur")):
        refused(call(D(), **{name: None}), word)
    refused(call(D(), posterior=None, counts=None), b"null posterior and null dur_counts")
    for name, off in (("probs", 2), ("sc", 1), ("trans", 3), ("init", 2), ("dur", 2), ("dur_open", 1), ("lengths", 3),
                      ("posterior", 2), ("cls", 1), ("begin", 3), ("ev", 4), ("counts", 4), ("ws", 4)):
        refused(call(D(), **{name: good[name] + off}), b"aligned")
    need = L.qt_pose_duration_posterior_workspace_bytes(ctypes.byref(D()))
    assert need == 8 * (2 * 2 * 100 * 12 + 2 * 12 * 16)
    refused(call(D(), ws_bytes=need - 1), b"workspace")
    refused(call(D(), ws_bytes=0), b"workspace")
    refused(call(D(), ws=None), b"workspace")
    rows = 2 * 100
    for out, nbytes in (("posterior", rows * 12 * 4), ("cls", rows * 12 * 4), ("begin", rows * 12 * 4), ("ev", 2 * 8),
                        ("counts", 12 * 16 * 8), ("ws", need)):
        refused(call(D(), **{out: good["probs"] + (rows * 12 - 2) * 4}), b"overlap")
        refused(call(D(), **{out: good["probs"] - nbytes + 8}), b"overlap")
        refused(call(D(), **{out: good["sc"] + 40}), b"overlap")
        refused(call(D(), **{out: good["trans"] + (144 - 2) * 4}), b"overlap")
        refused(call(D(), **{out: good["init"]}), b"overlap")
        refused(call(D(), **{out: good["dur"] + (12 * 16 - 2) * 4}), b"overlap")
        refused(call(D(), **{out: good["dur_open"] + 8}), b"overlap")
        refused(call(D(), **{out: good["lengths"]}), b"overlap")
    refused(call(D(), ld=16, posterior=good["probs"] + (199 * 16 + 10) * 4), b"overlap")
    refused(call(D(), cls=good["posterior"] + 8), b"overlap")
    refused(call(D(), begin=good["cls"] + rows * 12 * 4 - 8), b"overlap")
    refused(call(D(), ev=good["begin"] + 800), b"overlap")
    refused(call(D(), counts=good["ev"] + 8), b"overlap")
    refused(call(D(), ws=good["counts"] + 8), b"overlap")
    refused(call(D(batch=1 << 10, frames=(1 << 10) + 1)), b"frames", QT_ERR_UNSUPPORTED)
    refused(call(D(batch=1, frames=(1 << 20) + 1)), b"frames", QT_ERR_UNSUPPORTED)
    # the optional ones may be null: the next check is reached (the workspace's)
    refused(call(D(), init=None, dur_open=None, lengths=None, cls=None, begin=None, ev=None, counts=None, ws_bytes=8), b"workspace")
    refused(call(D(), init=None, dur_open=None, lengths=None, posterior=None, cls=None, begin=None, ev=None, ws_bytes=8), b"workspace")


def test_module_argument_checks_need_no_device():
    P_ = pkg()
    sc, trans = P_.cyclic_prior(range(4), -10, -100)
    dur = P_.hold_prior(4, 8, 2, 6)
    for bad in (dict(dur=dur[:3]), dict(dur=dur.astype(float)), dict(dur=dur - 1), dict(dur=-dur - 1), dict(dur=dur[0]),
                dict(dur=np.zeros((4, 129), int)), dict(dur=np.zeros((4, 0), int)), dict(dur_open="prefix_max"),
                dict(dur_open=dur[:, :7]), dict(dur_open=dur + 1), dict(dur_open=dur.astype(float)),
                dict(trans=trans[:3]), dict(init=[0, 0, 0]), dict(streams=0), dict(state_class=[0, 1, 2, 64]),
                dict(class_names=["a", "b", "c"])):
        with pytest.raises(ValueError, match="PoseDurationPosterior"):
            P_.PoseDurationPosterior(**{"state_class": sc, "trans": trans, "dur": dur, "device": "cuda:0", **bad})
    with pytest.raises(P_.QtError, match="AMD GPU"):      # no torch fallback
        P_.PoseDurationPosterior(sc, trans, dur, "cpu")


def test_the_documents_speak_of_the_duration_posterior():
    for doc, word in (("DESIGN.md", "qt_pose_duration_posterior"), ("DESIGN.md", "pose_duration_posterior.hip"),
                      ("INTEGRATION.md", "PoseDurationPosterior("), ("INTEGRATION.md", "expected_duration_prior"),
                      ("README.md", "pose_duration_posterior.hip"), ("README.md", "PoseDurationPosterior"),
                      ("EXPERIMENTS.md", "qt_pose_duration_posterior"),
                      (os.path.join(PKG, "pose_order.py"), "PoseDurationPosterior("),
                      (os.path.join("scripts", "bench_pose_duration_posterior.py"), "PoseDurationPosterior(")):
        assert word in open(os.path.join(ROOT, doc)).read(), (doc, word)
