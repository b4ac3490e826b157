"""The learner of the chain with hold durations, the parts that need no GPU: the float64 loops of
tests/_pose_duration_prior_ref.py against brute-force enumeration of every segmentation, the identities that tie the expected
transition counts to the posterior's begin and endp, the plain learner's counts where the two rules coincide (D = 1), the hard
counts, the M-step restated, the learning test on the reference alone, the C ABI's declarations and every host-side refusal
(pointers that are never dereferenced), the exports, the Python refusals and the documents.

The learning test: seeded tracks with holds of 9 frames, a cyclic chain without self-joins, dur uniform over 24 lengths.  In
float64 and with the rule's own precision alike, on all 12 seeds, the evidence per frame rises at every one of four iterations,
the first gains 0.337 bit per frame or more, and every step's most likely length becomes 9."""
import ctypes
import os
import re

import numpy as np
import pytest

import _pose_duration_posterior_ref as P
import _pose_duration_prior_ref as A
import _pose_duration_ref as Q
import _pose_order_ref as R
import _pose_prior_ref as PR
from _util import PKG, ROOT, pkg

QT_ERR_INVALID_ARG, QT_ERR_UNSUPPORTED = -1, -3
F32 = np.float32
SYMBOLS = ("qt_pose_duration_prior_workspace_bytes", "qt_pose_duration_prior_expect", "qt_pose_duration_prior_count_paths",
           "qt_pose_duration_prior_update")


def _chain(S, C, stay=-39, advance=-300):
    return R.cyclic_prior([s % C for s in range(S)], stay, advance, skip=-800, other=-3000)


def _durations(S, D, seed):
    rng = np.random.default_rng(seed)
    return (-rng.integers(0, 700, (S, D))).astype(np.int32)


# ---- the rule against enumeration -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,D", [(5, 2, 3), (4, 3, 3), (5, 3, 2), (3, 2, 2), (2, 2, 2), (1, 2, 3)])
def test_loops64_is_the_sum_over_every_segmentation(T, S, D):
    probs = R.make_probs(10 * T + S, 1, T, S, run=2)
    sc, tr = R.cyclic_prior(range(S), -39, -300, other=-900)
    dur = _durations(S, D, T)
    for init in (None, -np.arange(S) * 41):
        for dur_open in (None, Q.suffix_max(dur)):
            got = A.loops64(probs, sc, tr, dur, init, dur_open)
            want = A.brute(probs[0], sc, tr, dur, init, dur_open)
            for name, g, w in zip(("trans_counts", "start_counts", "dur_counts"), got, want):
                assert np.abs(g - w).max() <= 1e-12, (name, T, S, D, init is None, dur_open is None)
            assert abs(got[3][0] - want[3]) <= 1e-12 and got[3][1] == T
            if T == 1:
                assert not got[0].any()
            if T <= 2:
                assert not got[2].any()
            assert T < 3 or got[0].sum() > 1e-3


# ---- the identities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,D,T", [(3, 3, 4, 30), (12, 12, 16, 120), (17, 12, 8, 70)])
def test_identities(S, C, D, T):
    B = 3
    probs = R.make_probs(S + D + T, B, T, C)
    probs[0, T // 2] = np.nan
    sc, tr = _chain(S, C)
    dur = _durations(S, D, 5)
    open_ = Q.suffix_max(dur)
    lengths = np.array([T, 1, T // 2 + 1], np.int32)
    init = -np.arange(S) * 17
    args = (probs, sc, tr, dur, init, open_, lengths)
    tc, st, dc, totals = A.loops64(*args)
    post, cls, begin, ev, counts, endp = P.loops64(*args)
    assert np.abs(tc.sum(axis=0) - begin[:, 1:].sum(axis=(0, 1))).max() <= 1e-9              # column sums: begin, f >= 1
    ends = sum(endp[b, :n - 1].sum(axis=0) for b, n in enumerate(lengths))                   # endp[f], f = 1 .. T_b - 1
    assert np.abs(tc.sum(axis=1) - ends).max() <= 1e-9                                       # row sums
    assert abs(st.sum() - B) <= 1e-9
    assert R.bits(dc) == R.bits(counts)                                                      # the posterior reference's, bit for bit
    assert totals[0] == ev[0] + ev[1] + ev[2] and totals[1] == lengths.sum()
    # a stream alone is its share of the batch
    tcs, sts, dcs, evs, n_of = A.per_stream(*args)
    for b, n in enumerate(lengths):
        alone = A.loops64(probs[b:b + 1, :n], sc, tr, dur, init, open_)
        assert R.bits(alone[0]) == R.bits(tcs[b]) and R.bits(alone[1]) == R.bits(sts[b]) and R.bits(alone[2]) == R.bits(dcs[b])
    # the precision of the rule, beside the rule
    mixed = A.loops_mixed(*args)
    for m, w in zip(mixed[:3], (tc, st, dc)):
        assert m.dtype == np.float64 and (np.abs(m - w) / np.maximum(1.0, w)).max() <= 1e-4
    assert abs(mixed[3][0] - totals[0]) <= 1e-6 * max(1.0, abs(totals[0]))


def test_a_table_of_one_frame_is_the_plain_learner():
    """D = 1 and dur all zero: every frame is a segment, and the expected transition and start counts are the plain chain's"""
    for S, C, B, T in ((1, 1, 1, 3), (6, 5, 2, 40), (12, 12, 1, 150)):
        probs = R.make_probs(3 * S + T, B, T, C, run=4)
        sc, tr = _chain(S, C)
        for init in (None, -np.arange(S) * 37):
            tc, st, dc, totals = A.loops64(probs, sc, tr, np.zeros((S, 1), np.int32), init)
            want = PR.loops64(probs, sc, tr, init)
            assert np.abs(tc - want[0]).max() <= 1e-9 and np.abs(st - want[1]).max() <= 1e-9, (S, T)
            assert abs(totals[0] - want[2][0]) <= 1e-9 * max(1.0, abs(want[2][0])) and totals[1] == want[2][1]
            assert abs(dc.sum() - B * max(T - 2, 0)) <= 1e-9


# ---- hard counts ------------------------------------------------------------------------------------------------------------------
def test_hard_counts_of_runs():
    S, D = 5, 6
    rng = np.random.default_rng(4)
    path = np.repeat(rng.integers(-1, S + 1, (3, 40)), 3, axis=1)[:, :97].astype(np.int64)   # runs of 3, 6, .. ; labels -1 and S
    lengths = np.array([97, 1, 50], np.int32)
    tc, st, dc, totals = A.count_paths(path, S, D, None, lengths)
    assert R.bits(dc) == R.bits(Q.count_durations(path, S, D, lengths).astype(np.float64))
    want = np.zeros((S, S))
    for b, n in enumerate(lengths):
        for f in range(1, n):
            i, j = path[b, f - 1], path[b, f]
            if i != j and 0 <= i < S and 0 <= j < S:
                want[i, j] += 1
    assert R.bits(tc) == R.bits(want) and not np.diag(tc).any() and tc.sum() > 10
    assert totals.tolist() == [0.0, 148.0] and st.sum() == sum(0 <= path[b, 0] < S for b in range(3))


def test_hard_counts_of_the_decoders_segments():
    """holds of 20 frames under D = 8: the decoder joins segments of one step, which count on the diagonal"""
    S = C = 4
    D = 8
    probs, lead = Q.make_tracks(2, 3, 90, C, run=20)
    sc, tr = R.cyclic_prior(range(S), -20, -300, other=-3000)
    dur = Q.hold_prior(S, D, 2, D, inside=-10, outside=-4000)
    lengths = np.array([90, 47, 1], np.int32)
    path, start, _ = Q.decode(probs, sc, tr, dur, None, Q.suffix_max(dur), lengths)
    tc, st, dc, totals = A.count_paths(path, S, D, start, lengths)
    segments = joins = inner = 0
    for b, n in enumerate(lengths):
        cuts = [f for f in range(1, n) if start[b, f] == f]
        assert all(e - s <= D for s, e in zip([0] + cuts, cuts + [n]))
        segments += len(cuts) + 1
        inner += max(len(cuts) - 1, 0)
        joins += sum(path[b, f] == path[b, f - 1] for f in cuts)
    assert joins >= 5 and np.diag(tc).sum() == joins and tc.sum() == segments - 3 and dc.sum() == inner
    assert st.sum() == 3 and totals[1] == 138
    runs = A.count_paths(path, S, D, None, lengths)
    assert not np.diag(runs[0]).any() and runs[0].sum() < tc.sum()


# ---- the M-step -------------------------------------------------------------------------------------------------------------------
def test_m_step_restated():
    M = pkg("pose_order")
    rng = np.random.default_rng(9)
    S, D = 5, 24
    counts = rng.random((S, D)) * 3
    counts[1] = 0
    counts[2, 5:] = 0
    dur = np.full((S, D), -1174, np.int64)
    for pseudo in (1.0, 0.01, 0.0):
        got = A.dur_rows(counts, dur, None, pseudo)
        want = M.expected_duration_prior(counts, pseudo)
        rows = [j for j in range(S) if pseudo > 0 or counts[j].sum() > 0]
        assert R.bits(got[rows].astype(np.int32)) == R.bits(want[rows])
    kept = A.dur_rows(counts, dur, None, 0.0)
    assert (kept[1] == -1174).all() and (kept[2, 5:] == R.SCORE_FLOOR).all()              # an empty row stays; a zero scores -8192
    forbidden = np.array(dur)
    forbidden[:, ::3] = R.TRANS_FLOOR
    got = A.dur_rows(counts, forbidden, None, 0.5)
    assert (got[:, ::3] == R.TRANS_FLOOR).all() and (got[:, 1::3] > R.TRANS_FLOOR).all()
    mass = np.exp2(np.where(forbidden > R.TRANS_FLOOR, got, -np.inf) / 256.0).sum(axis=1)
    assert np.abs(mass - 1).max() <= 0.01                                                  # the allowed lengths share the row
    assert R.bits(A.suffix_max(got)) == R.bits(Q.suffix_max(got))
    # trans and init are the plain learner's M-step
    tcounts, scounts = rng.random((S, S)), rng.random(S)
    sc, tr = R.cyclic_prior(range(S), -39, -300, other=R.TRANS_FLOOR)
    new = A.m_step(tcounts, scounts, counts, tr, None, dur, pseudo_count=0.25, learn_init=True)
    want = PR.m_step(tcounts, scounts, tr, None, None, 0.25, True)
    assert R.bits(new[0]) == R.bits(want[0]) and R.bits(new[1]) == R.bits(want[1]) and (new[0][tr == R.TRANS_FLOOR] == R.TRANS_FLOOR).all()


# ---- learning ---------------------------------------------------------------------------------------------------------------------
def learning_case(seed):
    """(videos, state_class, trans, dur): the issue's setup"""
    probs, _ = Q.make_tracks(seed, 6, 160, 6, run=9)
    sc, tr = R.cyclic_prior(range(6), stay=R.TRANS_FLOOR, advance=-64, skip=-1024, other=R.TRANS_FLOOR)
    return [(probs, None)], sc, tr, np.full((6, 24), -1174, np.int32)


def learning_run(seed, F):
    videos, sc, tr, dur = learning_case(seed)
    out = A.fit(videos, sc, tr, dur, iterations=4, pseudo_count=0.0, dur_pseudo_count=0.01, F=F)
    return [bits / frames for bits, frames in out[4]], out[2].argmax(axis=1) + 1


def learns(per_frame, modes):
    return bool((np.diff(per_frame) > 0).all() and per_frame[1] - per_frame[0] >= 0.33 and (modes == 9).all())


def test_learning_on_the_reference():
    assert -1174 == int(np.rint(-256 * np.log2(24)))                        # a normalised start
    qualified = 0
    for seed in range(12):
        per_frame, modes = learning_run(seed, np.float64)
        if not learns(per_frame, modes):
            continue
        qualified += 1
        mixed, mixed_modes = learning_run(seed, F32)
        print(f"pose_duration_prior learning seed {seed}: float64 {np.round(per_frame, 4).tolist()} mixed "
              f"{np.round(mixed, 4).tolist()} modes {mixed_modes.tolist()}")
        assert len(mixed) == 5 and learns(mixed, mixed_modes), (seed, mixed, mixed_modes)
    assert qualified >= 10, qualified


# ---- the library ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    declared = set(re.findall(r"\b(qt_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(os.path.join(ROOT, PKG, "libqtcnn_hip.so"))
    for symbol in SYMBOLS:
        assert symbol in declared and hasattr(lib, symbol), symbol
    for word in ("xi_f[i][j]", "sum_i xi_f[i][j] = begin[f][j]", "sum_j xi_f[i][j] = endp[f][i]", "sum_i start_counts[i] = 1",
                 "T = 1 adds zeros to trans_counts", "T <= 2 adds zeros to dur_counts"):
        assert word in re.sub(r"\s*\n \*\s*", " ", header), word
    csrc = os.path.join(ROOT, PKG, "csrc")
    src = open(os.path.join(csrc, "pose_duration_prior.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert '#include "pose_duration_sweep.h"' in src and not re.search(r"_LOG2\[256\]\s*=|\b\w*_FLOOR\s*=(?!=)", code)
    assert "atomicAdd(&pq_hist" in code and not re.search(r"atomicAdd\([^)]*(double|float)", code)      # integer atomics only
    assert "hipMemset" not in code and "Synchronize" not in code
    # one sweep for the posterior and the learner, one M-step row for both learners
    sweep = open(os.path.join(csrc, "pose_duration_sweep.h")).read()
    assert '#include "pose_chain.h"' in sweep and "template <bool SMALL, bool LEARN>" in sweep
    post = open(os.path.join(csrc, "pose_duration_posterior.hip")).read()
    assert '#include "pose_duration_sweep.h"' in post and "length_L" not in post and "length_L" not in code
    assert "pc_update_row" in open(os.path.join(csrc, "pose_chain.h")).read()
    assert "pc_update_row(" in code and "pc_update_row(" in open(os.path.join(csrc, "pose_prior.hip")).read()
    P_, M = pkg(), pkg("pose_order")
    assert P_.PoseDurationLearner is M.PoseDurationLearner and "PoseDurationLearner" in P_.__all__
    assert issubclass(M.PoseDurationLearner, M._PoseDurationTables)
    for cls in (M.PoseDurationDecoder, M.PoseDurationPosterior, M.PoseDurationLagDecoder):
        assert callable(getattr(cls, "load_tables")), cls
    for method in ("zero", "accumulate", "accumulate_paths", "update", "fit", "totals", "tables"):
        assert callable(getattr(M.PoseDurationLearner, method)), method


def _lib():
    M = pkg("pose_order")
    L = pkg("_lib").lib()
    return M, L


def _refused(L, rc, word, status=QT_ERR_INVALID_ARG):
    assert rc == status and word in L.qt_last_error(), (rc, word, L.qt_last_error())


def test_workspace_query():
    M, L = _lib()
    q = lambda *a: L.qt_pose_duration_prior_workspace_bytes(ctypes.byref(M.PoseDurationDesc(*a)))
    assert q(3, 100, 12, 12, 64) == 8 * (2 * 3 * 100 * 12 + 3 * (144 + 12 + 12 * 64 + 1)) and q(1, 1, 1, 1, 1) == 8 * (2 + 4)
    assert q(1, 9000, 64, 64, 128) % 8 == 0
    for bad in ((0, 100, 12, 12, 64), (3, 0, 12, 12, 64), (3, 100, 65, 12, 64), (3, 100, 12, 65, 64), (3, 100, 12, 12, 0),
                (3, 100, 12, 12, 129), (3, 100, 12, 12, -1), (1 << 10, (1 << 10) + 1, 12, 12, 64)):
        assert q(*bad) == 0, bad
    assert L.qt_pose_duration_prior_workspace_bytes(None) == 0


def test_expect_argument_checks_need_no_device():
    """every refusal comes before the first device call: the pointers are never dereferenced"""
    M, L = _lib()
    D = lambda batch=2, frames=100, C=12, S=12, dmax=16: M.PoseDurationDesc(batch, frames, C, S, dmax)
    names = ("probs", "sc", "trans", "init", "dur", "dur_open", "lengths", "tc", "st", "dc", "totals", "ws")
    order = ("probs", "ld", "sc", "trans", "init", "dur", "dur_open", "lengths", "tc", "st", "dc", "totals", "ws", "ws_bytes")
    good = {n: 0x10000000 * k for k, n in enumerate(names, 1)}
    good.update(ld=12, ws_bytes=1 << 24)
    refused = lambda rc, word, status=QT_ERR_INVALID_ARG: _refused(L, rc, word, status)

    def call(desc, **kw):
        a = {**good, **kw}
        return L.qt_pose_duration_prior_expect(ctypes.byref(desc), *[a[n] for n in order], None)

    refused(L.qt_pose_duration_prior_expect(None, *[good[n] for n in order], None), b"null descriptor")
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
                       ("tc", b"null trans_counts"), ("dc", b"null dur_counts"), ("totals", b"null totals")):
        refused(call(D(), **{name: None}), word)
    for name, off in (("probs", 2), ("sc", 1), ("trans", 3), ("init", 2), ("dur", 2), ("dur_open", 1), ("lengths", 3),
                      ("tc", 4), ("st", 4), ("dc", 4), ("totals", 4), ("ws", 4)):
        refused(call(D(), **{name: good[name] + off}), b"aligned")
    need = L.qt_pose_duration_prior_workspace_bytes(ctypes.byref(D()))
    assert need == 8 * (2 * 2 * 100 * 12 + 2 * (144 + 12 + 12 * 16 + 1))
    refused(call(D(), ws_bytes=need - 1), b"workspace")
    refused(call(D(), ws_bytes=0), b"workspace")
    refused(call(D(), ws=None), b"workspace")
    rows = 2 * 100
    sizes = (("tc", 144 * 8), ("st", 12 * 8), ("dc", 12 * 16 * 8), ("totals", 16), ("ws", need))
    for out, nbytes in sizes:
        refused(call(D(), **{out: good["probs"] + (rows * 12 - 2) * 4}), b"overlap")
        refused(call(D(), **{out: good["probs"] - nbytes + 8}), b"overlap")
        refused(call(D(), **{out: good["sc"] + 40}), b"overlap")
        refused(call(D(), **{out: good["trans"] + (144 - 2) * 4}), b"overlap")
        refused(call(D(), **{out: good["init"]}), b"overlap")
        refused(call(D(), **{out: good["dur"] + (12 * 16 - 2) * 4}), b"overlap")
        refused(call(D(), **{out: good["dur_open"] + 8}), b"overlap")
        refused(call(D(), **{out: good["lengths"]}), b"overlap")
        for other, other_bytes in sizes:
            if other != out:
                refused(call(D(), **{out: good[other] + other_bytes - 8}), b"overlap")
    refused(call(D(batch=1 << 10, frames=(1 << 10) + 1)), b"frames", QT_ERR_UNSUPPORTED)
    refused(call(D(batch=1, frames=(1 << 20) + 1)), b"frames", QT_ERR_UNSUPPORTED)
    # the optional ones may be null: the next check is reached (the workspace's)
    refused(call(D(), init=None, dur_open=None, lengths=None, st=None, ws_bytes=8), b"workspace")


def test_count_paths_argument_checks_need_no_device():
    M, L = _lib()
    D = lambda batch=2, frames=100, C=1, S=12, dmax=16: M.PoseDurationDesc(batch, frames, C, S, dmax)
    names = ("path", "start", "lengths", "tc", "st", "dc", "totals", "ws")
    order = ("path", "start", "ld", "lengths", "tc", "st", "dc", "totals", "ws", "ws_bytes")
    good = {n: 0x10000000 * k for k, n in enumerate(names, 1)}
    good.update(ld=100, ws_bytes=1 << 24)
    refused = lambda rc, word, status=QT_ERR_INVALID_ARG: _refused(L, rc, word, status)

    def call(desc, **kw):
        a = {**good, **kw}
        return L.qt_pose_duration_prior_count_paths(ctypes.byref(desc), *[a[n] for n in order], None)

    refused(L.qt_pose_duration_prior_count_paths(None, *[good[n] for n in order], None), b"null descriptor")
    refused(call(D(batch=0)), b"batch")
    refused(call(D(frames=0)), b"frames")
    refused(call(D(S=65)), b"num_states")
    refused(call(D(dmax=129)), b"max_duration")
    refused(call(D(), ld=99), b"ld_path")
    for name, word in (("path", b"null path"), ("tc", b"null trans_counts"), ("dc", b"null dur_counts"), ("totals", b"null totals")):
        refused(call(D(), **{name: None}), word)
    for name, off in (("path", 4), ("start", 4), ("lengths", 2), ("tc", 4), ("st", 4), ("dc", 4), ("totals", 4), ("ws", 4)):
        refused(call(D(), **{name: good[name] + off}), b"aligned")
    need = 2 * 1 * (144 + 12 * 16) * 4
    assert need <= L.qt_pose_duration_prior_workspace_bytes(ctypes.byref(D()))
    refused(call(D(), ws_bytes=need - 1), b"workspace")
    refused(call(D(), ws=None), b"workspace")
    for out in ("tc", "st", "dc", "totals", "ws"):
        refused(call(D(), **{out: good["path"] + 8}), b"overlap")
        refused(call(D(), **{out: good["start"] + 200 * 8 - 8}), b"overlap")
        refused(call(D(), **{out: good["lengths"]}), b"overlap")
    refused(call(D(), st=good["tc"] + 8), b"overlap")
    refused(call(D(), totals=good["dc"] + 8), b"overlap")
    refused(call(D(), ws=good["totals"] + 8), b"overlap")
    refused(call(D(batch=1, frames=(1 << 20) + 1), ld=1 << 21), b"frames", QT_ERR_UNSUPPORTED)
    refused(call(D(), start=None, lengths=None, st=None, ws_bytes=8), b"workspace")
    for frames in (1024, 1025):                                         # a chunk of 1024 frames per workgroup
        want = 2 * (1 + (frames > 1024)) * (144 + 12 * 16) * 4
        refused(call(D(frames=frames), ld=frames, ws_bytes=want - 1), b"workspace")
        assert want <= L.qt_pose_duration_prior_workspace_bytes(ctypes.byref(D(frames=frames)))


def test_update_argument_checks_need_no_device():
    M, L = _lib()
    names = ("tc", "st", "dc", "allowed", "dur_allowed", "trans_in", "init_in", "dur_in", "trans_out", "init_out", "dur_out",
             "open_out")
    good = {n: 0x10000000 * k for k, n in enumerate(names, 1)}
    refused = lambda rc, word, status=QT_ERR_INVALID_ARG: _refused(L, rc, word, status)

    def call(S=12, D=16, pseudo=0.5, dur_pseudo=1.0, **kw):
        a = {**good, **kw}
        return L.qt_pose_duration_prior_update(S, D, a["tc"], a["st"], a["dc"], a["allowed"], a["dur_allowed"], pseudo, dur_pseudo,
                                               a["trans_in"], a["init_in"], a["dur_in"], a["trans_out"], a["init_out"],
                                               a["dur_out"], a["open_out"], None)

    for S in (0, -1, 65):
        refused(call(S=S), b"num_states")
    for D in (0, -1, 129):
        refused(call(D=D), b"max_duration")
    for v in (-1.0, float("nan"), float("inf")):
        refused(call(pseudo=v), b"pseudo_count")
        refused(call(dur_pseudo=v), b"dur_pseudo_count")
    for name, word in (("tc", b"null trans_counts"), ("allowed", b"null allowed"), ("trans_in", b"null trans_in"),
                       ("trans_out", b"null trans_out"), ("dc", b"null dur_counts"), ("dur_allowed", b"null dur_allowed"),
                       ("dur_in", b"null dur_in"), ("dur_out", b"null dur_out")):
        refused(call(**{name: None}), word)
    refused(call(st=None), b"null start_counts")
    for name, off in (("tc", 4), ("st", 4), ("dc", 4), ("allowed", 2), ("dur_allowed", 1), ("trans_in", 3), ("init_in", 2),
                      ("dur_in", 2), ("trans_out", 1), ("init_out", 2), ("dur_out", 2), ("open_out", 3)):
        refused(call(**{name: good[name] + off}), b"aligned")
    for out in ("trans_out", "init_out", "dur_out", "open_out"):
        for src in ("tc", "st", "dc", "allowed", "dur_allowed", "trans_in", "init_in", "dur_in"):
            refused(call(**{out: good[src] + 8}), b"overlap")
    refused(call(init_out=good["trans_out"] + 8), b"overlap")
    refused(call(open_out=good["dur_out"]), b"overlap")
    refused(call(dur_out=good["trans_out"] + 16), b"overlap")
    refused(call(open_out=good["dur_in"]), b"overlap")                  # dur_open_out has no table it may be


def test_module_argument_checks_need_no_device():
    P_ = pkg()
    sc, trans = P_.cyclic_prior(range(4), -10, -100)
    dur = P_.hold_prior(4, 8, 2, 6)
    for bad in (dict(dur=dur[:3]), dict(dur=dur.astype(float)), dict(dur=dur - 1), dict(dur=np.zeros((4, 129), int)),
                dict(dur_open="prefix_max"), dict(dur_open=dur[:, :7]), dict(trans=trans[:3]), dict(init=[0, 0, 0]),
                dict(state_class=[0, 1, 2, 64]), dict(class_names=["a", "b", "c"]), dict(pseudo_count=-1.0),
                dict(pseudo_count=float("nan")), dict(pseudo_count=True), dict(dur_pseudo_count=-0.5),
                dict(dur_pseudo_count=float("inf")), dict(dur_pseudo_count="1")):
        with pytest.raises(ValueError, match="PoseDurationLearner"):
            P_.PoseDurationLearner(**{"state_class": sc, "trans": trans, "dur": dur, "device": "cuda:0", **bad})
    with pytest.raises(P_.QtError, match="AMD GPU"):      # no torch fallback
        P_.PoseDurationLearner(sc, trans, dur, "cpu")
    with pytest.raises(TypeError):
        P_.PoseDurationLearner(sc, trans, dur, "cuda:0", streams=2)       # a learner owns no streams


def test_the_documents_speak_of_the_duration_learner():
    for doc, word in (("DESIGN.md", "qt_pose_duration_prior_expect"), ("DESIGN.md", "pose_duration_prior.hip"),
                      ("DESIGN.md", "pose_duration_sweep.h"), ("INTEGRATION.md", "PoseDurationLearner("),
                      ("INTEGRATION.md", "load_tables("), ("README.md", "pose_duration_prior.hip"),
                      ("README.md", "PoseDurationLearner"), ("README.md", "bench_pose_duration_prior.py"),
                      ("EXPERIMENTS.md", "qt_pose_duration_prior_expect"),
                      (os.path.join(PKG, "pose_order.py"), "PoseDurationLearner("),
                      (os.path.join("scripts", "bench_pose_duration_prior.py"), "PoseDurationLearner(")):
        assert word in open(os.path.join(ROOT, doc)).read(), (doc, word)
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, PKG, "pose_order.py")).read())
    assert "a full Baum-Welch learner over durations" not in text
    assert "Not built for the chain with durations:" in text and "fixed-lag posteriors with durations" in text
    assert "trans[j][j] = -65536" in text and "normalised dur" in text
