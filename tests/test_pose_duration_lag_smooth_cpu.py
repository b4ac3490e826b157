"""Fixed-lag pose-order posteriors with hold durations, the parts that need no GPU: the loops of
tests/_pose_duration_lag_posterior_ref.py, which keep a bounded carry, against the whole-video loops of
tests/_pose_duration_posterior_ref.py on every prefix, bit for bit and in both precisions (contract 1 is a property of the
rule); against themselves under splits into calls, outputs and carry; against the plain chain's fixed-lag loops where the two
rules coincide; what the feature is for on seeded tracks; the two size queries by hand, every host-side refusal (pointers that
are never dereferenced), the stream limit, the exports and the documents."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import _pose_duration_lag_posterior_ref as LS
import _pose_duration_lag_ref as DL
import _pose_duration_posterior_ref as P
import _pose_duration_ref as Q
import _pose_lag_ref as G
import _pose_order_ref as R
from _util import PKG, ROOT, pkg

QT_ERR_INVALID_ARG, QT_ERR_UNSUPPORTED = -1, -3
F32, F64 = np.float32, np.float64
CASES = [(3, 3, 4, 23, 5), (5, 4, 7, 40, 16), (4, 4, 1, 20, 3), (6, 6, 12, 30, 0), (3, 2, 5, 12, 63)]     # (S, C, D, T, lag)


@functools.lru_cache(maxsize=None)
def _case(S, C, D, T, B=2):
    """probs with a NaN row, zero rows and tie rows; a chain; seeded durations with forbidden lengths and a dur_open of its own;
    an init.  Computed once, shared, never written"""
    probs = R.make_probs(100 * S + 10 * D + T, B, T, C, run=4)
    probs[0, min(5, T - 1)] = np.nan
    probs[B - 1, T // 3:T // 3 + 2] = 0
    probs[0, T // 2:T // 2 + 3] = F32(1.0 / C)
    sc, tr = R.cyclic_prior([s % C for s in range(S)], -39, -300, skip=-600, other=-1500)
    dur, open_ = LS.durations(S, D)
    probs.setflags(write=False)
    return probs, sc, tr, dur, -np.arange(S) * 50, open_


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape and R.bits(got) == R.bits(want), what


# ---- contract 1: a property of the rule --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,D,T,lag", CASES)
@pytest.mark.parametrize("F", [F64, F32])
def test_every_emitted_row_is_the_whole_video_loops_on_a_prefix(S, C, D, T, lag, F):
    probs, sc, tr, dur, init, open_ = _case(S, C, D, T)
    for use_init, use_open in ((init, open_), (None, None)):
        whole = [P.loops(probs[:, :n], sc, tr, dur, use_init, use_open, F=F) for n in range(1, T + 1)]    # prefix n at [n - 1]
        g0, (lagged, cls, begin, filtered, evidence), state = LS.smooth(probs, sc, tr, dur, use_init, use_open, lag=lag, flush=True,
                                                                        F=F)
        assert g0 == 0 and lagged.shape == begin.shape == filtered.shape == probs.shape[:2] + (S,) and state["seen"] == T
        for g in range(T):
            w = whole[min(g + lag, T - 1)]
            what = (S, D, lag, g, use_init is None)
            _same(lagged[:, g], w[0][:, g], what + ("lagged",))
            _same(cls[:, g], w[1][:, g], what + ("class",))
            _same(begin[:, g], w[2][:, g], what + ("begin",))
            _same(filtered[:, g], whole[g][0][:, g], what + ("filtered",))
            _same(evidence[:, g], whole[g][3], what + ("evidence",))
    assert len({int(j) for j in lagged[0].argmax(axis=-1)}) >= 2


@pytest.mark.parametrize("n", [1, 5, 17])
def test_a_one_call_flush_within_the_lag_is_the_whole_video_loops(n):
    S, C, D, T, lag = CASES[1]
    probs, sc, tr, dur, init, open_ = _case(S, C, D, T)
    for F in (F64, F32):
        _, (lagged, cls, begin, _, evidence), _ = LS.smooth(probs[:, :n], sc, tr, dur, init, open_, lag=lag, flush=True, F=F)
        want = P.loops(probs[:, :n], sc, tr, dur, init, open_, F=F)
        _same(lagged, want[0], n), _same(cls, want[1], n), _same(begin, want[2], n), _same(evidence[:, -1], want[3], n)


@pytest.mark.parametrize("S,C,D,T,lag", CASES)
def test_lag_zero_is_filtered(S, C, D, T, lag):
    probs, sc, tr, dur, init, open_ = _case(S, C, D, T)
    _, (lagged, _, _, filtered, _), _ = LS.smooth(probs, sc, tr, dur, init, open_, lag=0, flush=False, F=F32)
    _same(lagged, filtered, (S, D))


# ---- contract 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [F64, F32])
def test_splits_are_one_call(F):
    """every two-call split and a three-call split of 40 frames, a flush alone, and one frame per call: the outputs and the
    carry of one call, bit for bit; the carry goes through its bytes"""
    S, C, D, T, lag = CASES[1]
    probs, sc, tr, dur, init, open_ = _case(S, C, D, T)
    args = (sc, tr, dur, init, open_)
    _, want, want_state = LS.smooth(probs, *args, lag=lag, flush=True, F=F)
    for cuts in [[c] for c in range(1, T)] + [[7, 24]]:
        g0, got, state, calls = LS.split(LS.smooth, probs, cuts, *args, lag=lag, F=F)
        assert g0 == 0 and calls[0][1][0].shape[1] == max(0, cuts[0] - lag)
        for a, b in zip(got, want):
            _same(a, b, cuts)
        LS.same_state(state, want_state)
    # one frame per call without a flush leaves the last lag frames pending; a flush alone brings them
    g0, first, state, _ = LS.split(LS.smooth, probs, list(range(1, T)), *args, flush_last=False, lag=lag, F=F)
    assert first[0].shape[1] == T - lag and first[3].shape[1] == T
    g0, rest, state = LS.smooth(probs[:, :0], *args, lag=lag, flush=True, state=state, F=F)
    assert g0 == T - lag and rest[0].shape[1] == lag and rest[3].shape[1] == 0
    for a, b, w in zip(first, rest, want):
        _same(np.concatenate([a, b], axis=1), w, "flush alone")
    LS.same_state(state, want_state)
    # the packed carry: the integers of the state, its levels as the kernel keeps them, zeros in the padding
    raw = LS.pack_carry(state, S, D, lag)
    assert raw.shape == (probs.shape[0], LS.carry_stride(S, D, lag))
    fields = LS.unpack_carry(raw.tobytes(), probs.shape[0], S, D, lag, T)
    LS.same_carry(fields, LS.carry_fields(state, S, D, lag), 0.0)
    assert (fields["e"] == np.stack([R.emissions(probs[b, T - lag:], sc) for b in range(probs.shape[0])])).all()
    assert (fields["cum"] == np.stack([R.emissions(probs[b], sc).sum(axis=0) for b in range(probs.shape[0])])).all()


# ---- where the rules coincide ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C", [(1, 1), (6, 5), (12, 12)])
def test_a_table_of_one_frame_is_the_plain_lagged_posterior(S, C):
    T = 37
    probs = R.make_probs(5 * S + T, 2, T, C, run=4)
    probs[0, 5] = np.nan
    sc, tr = R.cyclic_prior([s % C for s in range(S)], -39, -300, skip=-600, other=-1500)
    dur = np.zeros((S, 1), np.int32)
    for init in (None, -np.arange(S) * 37):
        for lag in (0, 1, 5, 63):
            _, (lagged, cls, begin, filtered, _), _ = LS.smooth(probs, sc, tr, dur, init, lag=lag, flush=True, F=F64)
            _, (want, want_cls, want_filtered, _), _ = G.smooth(probs, sc, tr, init, lag=lag, flush=True, F=F64)
            assert np.abs(lagged - want).max() <= 1e-9 and np.abs(cls - want_cls).max() <= 1e-9, (S, lag)
            assert np.abs(filtered - want_filtered).max() <= 1e-9
            assert np.abs(begin - lagged).max() <= 1e-9                    # a hold begins at every frame it covers


# ---- what it is for ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_the_lagged_posterior_follows_the_lagged_path(seed):
    """holds of 9 frames with 0.97 on the true class, a tenth of the frames replaced by Dirichlet(1) rows, 16 frames behind the
    camera: the most probable step of every lagged row is the step of the revised path, and the confidence a loop would print
    beside it never falls below a half"""
    S = C = 6
    T, D, lag = 90, 16, 16
    sc, tr = R.cyclic_prior(range(6), -39, -300, skip=-800, other=-3000)
    dur = np.full((S, D), R.TRANS_FLOOR, np.int32)
    dur[:, 3:16] = 0                                                       # lengths 4 .. 16
    open_ = Q.suffix_max(dur)
    truth = (np.arange(T) // 9) % C
    probs = np.full((1, T, C), F32(0.03 / (C - 1)), F32)
    probs[0, np.arange(T), truth] = F32(0.97)
    rng = np.random.default_rng(seed)
    off = rng.random(T) < 0.1
    probs[0, off] = rng.dirichlet(np.ones(C), int(off.sum())).astype(F32)
    _, (lagged, _, begin, _, _), _ = LS.split(LS.smooth, probs, list(range(1, T)), sc, tr, dur, None, open_, lag=lag, F=F32)[:3]
    _, (path, _, _, _), _ = DL.split(DL.decode, probs, list(range(1, T)), sc, tr, dur, None, open_, lag=lag)[:3]
    assert (lagged.argmax(axis=-1) == path).all(), np.argwhere(lagged.argmax(axis=-1) != path).tolist()
    confidence = np.take_along_axis(lagged, path[..., None], axis=-1)[..., 0]
    print(f"pose_duration_lag_smooth use, seed {seed}: lowest confidence {confidence.min():.3f}")
    assert confidence.min() >= 0.5
    assert (begin >= 0).all() and (begin <= 1 + 2.0 ** -20).all()


# ---- the library -------------------------------------------------------------------------------------------------------------------
def _lib():
    M = pkg("pose_order")
    L = pkg("_lib").lib()
    return M, L


NAMES = ("qt_pose_duration_lag_smooth_carry_bytes", "qt_pose_duration_lag_smooth_workspace_bytes", "qt_pose_duration_lag_smooth")


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    declared = set(re.findall(r"\b(qt_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(os.path.join(ROOT, PKG, "libqtcnn_hip.so"))
    for symbol in NAMES:
        assert symbol in declared and hasattr(lib, symbol), symbol
    assert len(re.findall(r"typedef struct qt_pose_duration_lag_desc \{", header)) == 1            # the descriptor is reused
    M, P_ = pkg("pose_order"), pkg()
    src = open(os.path.join(ROOT, PKG, "csrc", "pose_duration_lag_posterior.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert '#include "pose_duration_sweep.h"' in src and "getenv" not in src and "qt_env" not in src    # one route
    assert "atomic" not in code.replace("std::atomic", "") and "exp2f" not in code and "log2f" not in code   # the sweeps' own arithmetic
    sweep = open(os.path.join(ROOT, PKG, "csrc", "pose_duration_sweep.h")).read()
    for shared in ("pp_group_L", "pp_length_L", "pp_evidence", "pp_owner_step", "pp_row", "pp_class_sum"):
        assert re.search(r"(double|float) " + shared + r"\(", sweep) and shared + "(" in code.replace("<LPS>", ""), shared
    assert P_.PoseDurationLagSmoother is M.PoseDurationLagSmoother and "PoseDurationLagSmoother" in P_.__all__
    assert issubclass(M.PoseDurationLagSmoother, (M._LagState, M._PoseDurationTables))
    assert M.MAX_SMOOTH_STREAM_FRAMES == 1 << 20 == LS.MAX_STREAM


def _desc(M):
    return lambda batch=2, frames=1, C=12, S=12, dmax=64, lag=16, flush=0, seen=0: \
        M.PoseDurationLagDesc(batch, frames, C, S, dmax, lag, flush, seen)


def test_size_queries_by_hand():
    M, L = _lib()
    D = _desc(M)
    carry = lambda **kw: L.qt_pose_duration_lag_smooth_carry_bytes(ctypes.byref(D(**kw)))
    room = lambda **kw: L.qt_pose_duration_lag_smooth_workspace_bytes(ctypes.byref(D(**kw)))
    # per stream 8 S + 8 D S + 16 lag S + 8 S + 8 + 2 lag S, rounded up to 8
    assert carry(batch=1, S=1, dmax=1, lag=0) == 8 + 8 + 0 + 8 + 8
    assert carry(batch=1, S=1, dmax=1, lag=3) == 8 + 8 + 48 + 8 + 8 + 8                # 6 -> 8
    assert carry(batch=1, S=1, dmax=1, lag=4) == 8 + 8 + 64 + 8 + 8 + 8
    assert carry(batch=2, S=12, dmax=64, lag=16) == 2 * (96 + 6144 + 3072 + 96 + 8 + 384) == 2 * 9800
    assert carry(batch=3, S=64, dmax=128, lag=63) == 3 * (512 + 65536 + 64512 + 512 + 8 + 8064)
    assert carry(batch=1, S=13, dmax=24, lag=5, frames=7, seen=99, flush=1) == 104 + 2496 + 1040 + 104 + 8 + 130 + 6
    for S, dmax, lag in ((1, 1, 0), (3, 5, 5), (12, 64, 16), (13, 24, 63), (64, 128, 63)):
        assert carry(batch=5, S=S, dmax=dmax, lag=lag) == 5 * LS.carry_stride(S, dmax, lag) and LS.carry_stride(S, dmax, lag) % 8 == 0
    # four [batch][n][S] arrays of 8 bytes, Z [batch][n], int16 [batch][n][S] rounded up to 8; nothing for a flush alone
    assert room(batch=1, frames=1, S=1) == 32 + 8 + 8
    assert room(batch=16, frames=1, S=12) == 16 * 12 * 32 + 128 + 384
    assert room(batch=2, frames=3, S=13) == 2496 + 48 + 160                            # 156 -> 160
    assert room(batch=3, frames=300, S=64) == 32 * 57600 + 7200 + 115200
    assert room(batch=2, frames=0, flush=1, seen=40) == 0 and carry(batch=2, frames=0, flush=1, seen=40) > 0
    assert room(batch=2, frames=5, S=3) == LS.workspace_bytes(2, 5, 3) == 960 + 80 + 64
    for bad in (dict(batch=0), dict(frames=-1), dict(frames=0), dict(C=0), dict(C=65), dict(S=0), dict(S=65), dict(dmax=0),
                dict(dmax=129), dict(lag=-1), dict(lag=64), dict(seen=-1), dict(batch=2, frames=(1 << 19) + 1),
                dict(seen=1 << 20), dict(seen=(1 << 20) - 1, frames=2), dict(seen=1 << 36)):
        assert carry(**bad) == 0 and room(**bad) == 0, bad
    assert carry(seen=(1 << 20) - 1, frames=1) > 0 and carry(batch=1, frames=1 << 20) > 0
    assert L.qt_pose_duration_lag_smooth_carry_bytes(None) == 0 and L.qt_pose_duration_lag_smooth_workspace_bytes(None) == 0


def test_argument_checks_need_no_device():
    """every refusal comes before the first device call: the pointers are never dereferenced"""
    M, L = _lib()
    D = lambda batch=2, frames=300, C=12, S=12, dmax=16, lag=16, flush=0, seen=50: \
        M.PoseDurationLagDesc(batch, frames, C, S, dmax, lag, flush, seen)
    names = ("probs", "sc", "trans", "init", "dur", "dur_open", "cin", "cout", "lagged", "cls", "begin", "filt", "ev", "ws")
    good = {n: 0x10000000 * k for k, n in enumerate(names, 1)}
    good.update(ld=12, ws_bytes=1 << 26)
    probs, sc, trans, init, dur, dur_open, cin, cout = (good[n] for n in names[:8])

    def call(desc, **kw):
        a = {**good, **kw}
        return L.qt_pose_duration_lag_smooth(None if desc is None else ctypes.byref(desc), a["probs"], a["ld"], a["sc"], a["trans"],
                                             a["init"], a["dur"], a["dur_open"], a["cin"], a["cout"], a["lagged"], a["cls"],
                                             a["begin"], a["filt"], a["ev"], a["ws"], a["ws_bytes"], None)

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
    refused(call(D(), lagged=None), b"null lagged")                                  # count = 300 > 0
    refused(call(D(seen=3, frames=13, lag=16), lagged=None, cin=None), b"carry_in")  # count == 0: lagged may be null, the carry not
    refused(call(D(), cin=None), b"null carry_in")
    refused(call(D(seen=0, frames=20, lag=16), lagged=None, cin=None), b"null lagged")    # seen == 0: no carry_in; count = 4
    refused(call(D(frames=0, flush=1, seen=9), lagged=None, probs=None), b"null lagged")  # a flush alone still emits
    for name, off in (("probs", 2), ("sc", 1), ("trans", 3), ("init", 2), ("dur", 2), ("dur_open", 1), ("cin", 4), ("cout", 4),
                      ("lagged", 2), ("cls", 1), ("begin", 3), ("filt", 2), ("ev", 4), ("ws", 4)):
        refused(call(D(), **{name: good[name] + off}), b"aligned")
    need = L.qt_pose_duration_lag_smooth_workspace_bytes(ctypes.byref(D()))
    assert need == 32 * 2 * 300 * 12 + 8 * 600 + 2 * 2 * 300 * 12
    refused(call(D(), ws_bytes=need - 1), b"workspace")
    refused(call(D(), ws_bytes=0), b"workspace")
    refused(call(D(), ws=None), b"workspace")
    carry = 2 * LS.carry_stride(12, 16, 16)
    assert carry == L.qt_pose_duration_lag_smooth_carry_bytes(ctypes.byref(D()))
    refused(call(D(), cin=cout + carry - 8), b"carry_in must not overlap carry_out")
    refused(call(D(), cin=cout), b"carry_in must not overlap carry_out")
    refused(call(D(), cout=cin + 8), b"carry_in must not overlap carry_out")
    rows = 2 * 300
    sizes = (("lagged", rows * 48), ("cls", rows * 48), ("begin", rows * 48), ("filt", rows * 48), ("ev", rows * 8),
             ("cout", carry), ("ws", need))
    for name, nbytes in sizes:
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
    outs = [n for n, _ in sizes if n != "cout"]
    for a, first in enumerate(outs):                                                 # every output against every other
        for second in outs[a + 1:]:
            refused(call(D(), **{second: good[first] + 8}), b"overlap")
    refused(call(D(batch=1 << 10, frames=(1 << 10) + 1)), b"frames", QT_ERR_UNSUPPORTED)
    refused(call(D(batch=1, frames=(1 << 20) + 1)), b"frames", QT_ERR_UNSUPPORTED)
    refused(call(D(seen=(1 << 20) - 299)), b"seen", QT_ERR_UNSUPPORTED)              # the stream limit
    refused(call(D(seen=(1 << 20) + 1, frames=0, flush=1), probs=None), b"seen", QT_ERR_UNSUPPORTED)
    refused(call(D(seen=(1 << 20) - 300), ws=None), b"workspace")                    # the last frame that is handled
    refused(call(D(batch=1, frames=(1 << 20) + 1, dmax=129)), b"max_duration")
    # a flush alone asks for no workspace and no probs: the next check is reached
    refused(call(D(frames=0, flush=1), probs=None, ws=None, ws_bytes=0, cin=cout), b"carry_in must not overlap")
    # with seen == 0 carry_in is not looked at; the optional ones may be null
    refused(call(D(seen=0, frames=1), cin=cout, filt=cout + 8), b"carry_out must not overlap filtered")
    refused(call(D(), init=None, dur_open=None, cls=None, begin=None, filt=None, ev=None, lagged=None), b"null lagged")


def test_module_argument_checks_need_no_device():
    P_ = pkg()
    sc, trans = P_.cyclic_prior(range(4), -10, -100)
    dur = P_.hold_prior(4, 8, 2, 6)
    for bad in (dict(dur=dur[:3]), dict(dur=dur.astype(float)), dict(dur=dur - 1), dict(dur=np.zeros((4, 129), int)),
                dict(dur_open="prefix_max"), dict(dur_open=dur[:, :7]), dict(trans=trans[:3]), dict(init=[0, 0, 0]),
                dict(streams=0), dict(state_class=[0, 1, 2, 64]), dict(class_names=["a", "b", "c"]),
                dict(lag=-1), dict(lag=64), dict(lag=2.0), dict(lag=True), dict(lag=None)):
        with pytest.raises(ValueError, match="PoseDurationLagSmoother"):
            P_.PoseDurationLagSmoother(**{"state_class": sc, "trans": trans, "dur": dur, "device": "cuda:0", "lag": 5, **bad})
    with pytest.raises(P_.QtError, match="AMD GPU"):      # no torch fallback
        P_.PoseDurationLagSmoother(sc, trans, dur, "cpu", 5)
    src = open(os.path.join(ROOT, PKG, "pose_order.py")).read()
    body = src[src.index("class PoseDurationLagSmoother"):src.index("class _Learner")]
    assert "MAX_SMOOTH_STREAM_FRAMES" in body and ".cpu()" not in body and ".item()" not in body and "synchronize" not in body
    for method in ("def push(self, probs, flush=False, by_class=False, begin=False, filtered=False, evidence=False)",
                   "def confidence(self, lagged, lag_path)", "def holds(self, lagged_begin)"):
        assert method in body, method


def test_the_documents_speak_of_the_duration_lag_smoother():
    for doc, word in (("DESIGN.md", "qt_pose_duration_lag_smooth"), ("DESIGN.md", "pose_duration_lag_posterior.hip"),
                      ("README.md", "pose_duration_lag_posterior.hip"), ("README.md", "PoseDurationLagSmoother"),
                      ("README.md", "bench_pose_duration_lag_posterior.py"),
                      ("EXPERIMENTS.md", "Fixed-lag pose-duration posteriors"),
                      (os.path.join(PKG, "pose_order.py"), "PoseDurationLagSmoother("),
                      (os.path.join("include", "qtcnn.h"), "qt_pose_duration_lag_smooth"),
                      (os.path.join("scripts", "bench_pose_duration_lag_posterior.py"), "PoseDurationLagSmoother(")):
        assert word in open(os.path.join(ROOT, doc)).read(), (doc, word)
    for doc in ("README.md", "DESIGN.md"):
        text = re.sub(r"\s+", " ", open(os.path.join(ROOT, doc)).read())
        for sentence in re.findall(r"Not built[^.]*\.", text):
            assert "fixed-lag posteriors with durations" not in sentence and "a fixed-lag form, one wave" not in sentence, (doc, sentence)
