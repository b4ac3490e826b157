"""The score-based evaluation, the parts that need no GPU: tests/_scores_ref.py reproduces what scikit-learn returned on the
quantised scores (tests/golden/score_metrics.npz); the restatement agrees with itself under every split of a batch and under
merging; the score key at its edges; the C ABI's declarations, size queries and host-side argument checks; the module's
constructor and device checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _scores_ref as R
from _util import PKG, ROOT, pkg

NEW_SYMBOLS = ["qt_scores_state_bytes", "qt_scores_report_bytes", "qt_scores_update", "qt_scores_finalize"]
QT_ERR_INVALID_ARG, QT_ERR_UNSUPPORTED = -1, -3
SCORES = pkg("scores")            # every test here needs the module


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "score_metrics.npz"))


def test_fixture_has_the_five_cases(golden):
    shapes = [(int(golden["num_classes"][i]), golden[f"labels{i}"].shape[0], int(golden["bits"][i])) for i in range(5)]
    assert shapes == [(12, 1000, 12), (12, 300, 4), (2, 65, 12), (5, 64, 4), (3, 7, 12)]
    absent = [int(np.isnan(golden[f"ap{i}"]).sum()) for i in range(5)]
    assert absent == [0, 2, 0, 1, 1]
    p3 = golden["probs3"]
    assert len(np.unique(R.q_of(p3[:, 4], 4))) == 1 and len(np.unique(R.q_of(p3[:, 4], 12))) == 1    # all scores in one bin
    for i in range(5):
        p = golden[f"probs{i}"]
        assert p.dtype == np.float32 and golden[f"labels{i}"].dtype == np.int64
        srt = np.sort(p, 1)
        assert not (srt[:, 1:] == srt[:, :-1]).any()             # top-k was recorded on untied rows


@pytest.mark.parametrize("i", range(5))
def test_restatement_reproduces_scikit_learn_on_the_quantised_scores(golden, i):
    C, bits, M = int(golden["num_classes"][i]), int(golden["bits"][i]), 15
    p, y = golden[f"probs{i}"], golden[f"labels{i}"]
    st = R.update(None, p, p, y, C, bits, M, R.PROBS)
    rep, curves = R.report(st, C, bits, M)
    assert R.close(rep[:C], golden[f"auc{i}"]), np.nanmax(np.abs(rep[:C] - golden[f"auc{i}"]))
    assert R.close(rep[C:2 * C], golden[f"ap{i}"]), np.nanmax(np.abs(rep[C:2 * C] - golden[f"ap{i}"]))
    assert np.array_equal(rep[2 * C:3 * C], np.bincount(y, minlength=C))
    want = golden[f"topk{i}"]
    for j in range(3):
        if not np.isnan(want[j]):
            assert R.close(rep[3 * C + j], want[j]), (j, rep[3 * C + j], want[j])
    assert rep[4 * C - 1] == 1.0                                  # top-C holds every counted row
    s = R.scalars(rep, C, M)
    assert s["samples"] == len(y) and s["updates"] == 1 and s["classes_scored"] == int((~np.isnan(golden[f"auc{i}"])).sum())
    assert R.close(s["macro_auc"], np.nanmean(golden[f"auc{i}"])) and R.close(s["macro_ap"], np.nanmean(golden[f"ap{i}"]))
    # the curves: cumulative from the top, bin 0 holds the totals
    sup = np.bincount(y, minlength=C)
    assert np.array_equal(curves[:, 0, 0], sup) and np.array_equal(curves[:, 1, 0], len(y) - sup)
    assert (np.diff(curves, axis=2) <= 0).all()


def test_calibration_and_rank_on_a_hand_made_batch():
    C, bits, M = 3, 4, 4
    p = np.array([[0.5, 0.25, 0.25],      # pred 0, conf .5 -> bin 2, label 0: hit, rank 0
                  [0.25, 0.5, 0.25],      # pred 1, conf .5 -> bin 2, label 2: miss, rank 2 (0.25 tie: class 0 is in front)
                  [0.0, 0.0, 1.0],        # pred 2, conf 1 -> bin 3 (clamped), label 2: hit, rank 0
                  [0.375, 0.375, 0.25]],  # pred 0 (tie: lower index), conf .375 -> bin 1, label 1: miss, rank 1
                 np.float32)
    y = np.array([0, 2, 2, 1])
    st = R.update(None, p, p, y, C, bits, M, R.PROBS)
    H = 2 * C * 16
    assert st[H:H + C].tolist() == [2, 1, 1]
    assert st[H + C:H + C + 3 * M].reshape(M, 3).tolist() == [[0, 0, 0], [1, 0, 24576], [2, 1, 65536], [1, 1, 65536]]
    assert st[H + C + 3 * M:].tolist() == [4, 0, 0, 0, 1]
    hist = st[:H].reshape(C, 2, 16)
    assert hist[2, 1].nonzero()[0].tolist() == [4, 15] and hist[2, 1, 15] == 1 and hist[0, 0, 0] == 1 and hist[0, 1, 8] == 1
    rep, _ = R.report(st, C, bits, M)
    assert rep[3 * C:4 * C].tolist() == [0.5, 0.75, 1.0]
    s = R.scalars(rep, C, M)
    assert rep[4 * C:4 * C + 3 * M].tolist() == [0, 1, 2, 1, 0, 0, 0.5, 1, 0, 0.375, 0.5, 1]
    assert s["ece"] == 0.25 * 0.375 and s["mce"] == 0.375


@pytest.mark.parametrize("kind", [R.LOGITS, R.PROBS])
def test_every_split_of_a_batch_gives_the_state_of_one_call(kind):
    C, bits, M, rows = 5, 6, 7, 40
    z, y = R.make_logits(rows, C, seed=11)
    s = z if kind == R.LOGITS else R.softmax_f32(z)
    s, y = R.mix_in(s, y, C, kind)
    p = R.softmax_f32(s) if kind == R.LOGITS else s
    one = R.update(None, s, p, y, C, bits, M, kind)
    ctr = one[-5:].tolist()
    assert ctr[0] + ctr[1] + ctr[2] + ctr[3] == rows and min(ctr[:4]) >= 2 and ctr[4] == 1    # every row class occurs
    for a in range(1, rows):
        two = R.update(R.update(None, s[:a], p[:a], y[:a], C, bits, M, kind), s[a:], p[a:], y[a:], C, bits, M, kind)
        assert np.array_equal(two[:-1], one[:-1]) and two[-1] == 2, a
        for b in range(a + 1, rows):
            st = None
            for lo, hi in ((0, a), (a, b), (b, rows)):
                st = R.update(st, s[lo:hi], p[lo:hi], y[lo:hi], C, bits, M, kind)
            assert np.array_equal(st[:-1], one[:-1]) and st[-1] == 3, (a, b)
    # merge is the sum of the states
    half = R.update(None, s[:17], p[:17], y[:17], C, bits, M, kind) + R.update(None, s[17:], p[17:], y[17:], C, bits, M, kind)
    assert np.array_equal(half[:-1], one[:-1])
    ra, rb = R.report(one, C, bits, M), R.report(half, C, bits, M)
    assert np.array_equal(ra[0][:-1].view(np.uint64), rb[0][:-1].view(np.uint64)) and np.array_equal(ra[1], rb[1])


def test_score_key_at_its_edges():
    for bits in (4, 12, 14):
        K = 1 << bits
        p = np.array([0.0, 2.0 ** -14, 1.0 - 2.0 ** -24, 1.0], np.float32)
        assert p[2] < 1.0
        assert R.q_of(p, bits).tolist() == [0, K >> 14, K - 1, K - 1]
    lo = np.arange(16, dtype=np.float32) / np.float32(16)            # the lower edge of every bin for bits = 4
    assert R.q_of(lo, 4).tolist() == list(range(16))
    assert R.q_of(np.nextafter(lo[1:], np.float32(0)), 4).tolist() == list(range(15))      # just below an edge: the bin below
    assert R.q_of(np.nextafter(lo, np.float32(1)), 4).tolist() == list(range(16))
    assert R.q_of(np.float32(-0.0), 4) == 0


def test_report_edge_states():
    C, bits, M = 4, 4, 3
    rep, curves = R.report(np.zeros(R.cells(C, bits, M), np.int64), C, bits, M)
    assert np.isnan(rep[:2 * C]).all() and not rep[2 * C:3 * C].any() and np.isnan(rep[3 * C:4 * C]).all()
    assert not rep[4 * C:4 * C + 3 * M].any() and np.isnan(rep[4 * C + 3 * M:4 * C + 3 * M + 6]).all()
    assert rep[4 * C + 3 * M + 6:].tolist() == [0] * 6 and not curves.any()
    p = np.array([[1, 0, 0, 0], [1, 0, 0, 0]], np.float32)             # one class only: AUC undefined everywhere it has no
    rep, _ = R.report(R.update(None, p, p, [0, 0], C, bits, M, R.PROBS), C, bits, M)       # negatives or no positives
    assert np.isnan(rep[:C]).all() and rep[C] == 1.0 and np.isnan(rep[C + 1:2 * C]).all()
    s = R.scalars(rep, C, M)
    assert np.isnan(s["macro_auc"]) and s["macro_ap"] == 1.0 and s["classes_scored"] == 0 and s["ece"] == 0.0
    p = np.array([[0.75, 0.25], [0.25, 0.75], [0.75, 0.25]], np.float32)                  # a perfect and a tied ranking
    rep, _ = R.report(R.update(None, p, p, [0, 1, 0], 2, 4, 2, R.PROBS), 2, 4, 2)
    assert rep[:4].tolist() == [1.0, 1.0, 1.0, 1.0]
    p = np.full((4, 2), 0.5, np.float32)
    rep, _ = R.report(R.update(None, p, p, [0, 1, 0, 1], 2, 4, 2, R.PROBS), 2, 4, 2)
    assert rep[:4].tolist() == [0.5, 0.5, 0.5, 0.5] and rep[3 * 2:4 * 2].tolist() == [0.5, 1.0]


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    declared = set(re.findall(r"\b(qt_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(os.path.join(ROOT, PKG, "libqtcnn_hip.so"))
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
    assert "qt_scores_desc" in header and re.search(r"#define\s+QT_SCORES_MAX_CLASSES\s+64\b", header)
    S = pkg("scores")
    for name, value in (("MAX_CLASSES", S.MAX_CLASSES), ("MAX_CAL_BINS", S.MAX_CAL_BINS), ("MIN_BITS", S.MIN_BITS),
                        ("MAX_BITS", S.MAX_BITS)):
        assert re.search(rf"#define\s+QT_SCORES_{name}\s+{value}\b", header), name
    assert [f[0] for f in S.ScoresDesc._fields_] == ["dtype", "kind", "bits", "cal_bins", "route", "ignore_index"]


def test_size_queries():
    S = pkg("scores")
    L = pkg("_lib").lib()
    for C in (1, 2, 12, 64):
        for bits in (4, 12, 14):
            for M in (1, 15, 64):
                assert L.qt_scores_state_bytes(C, bits, M) == 8 * (2 * C * (1 << bits) + C + 3 * M + 5) == 8 * R.cells(C, bits, M)
                assert L.qt_scores_report_bytes(C, M) == 8 * (4 * C + 3 * M + 12) == 8 * R.report_len(C, M)
    for C, bits, M in ((0, 12, 15), (-3, 12, 15), (65, 12, 15), (12, 3, 15), (12, 15, 15), (12, 12, 0), (12, 12, 65)):
        assert L.qt_scores_state_bytes(C, bits, M) == 0, (C, bits, M)
    for C, M in ((0, 15), (65, 15), (12, 0), (12, 65), (-1, -1)):
        assert L.qt_scores_report_bytes(C, M) == 0, (C, M)


def test_host_side_argument_checks_need_no_device():
    S = pkg("scores")
    L = pkg("_lib").lib()
    z, y, st, rp, cv = 0x10000, 0x30000, 0x40000, 0x80000, 0x90000   # never dereferenced

    def desc(dtype=0, kind=0, bits=12, cal_bins=15, route=0, ignore=-100):
        return S.ScoresDesc(dtype, kind, bits, cal_bins, route, ignore)

    base = dict(desc=desc(), scores=z, ld=12, labels=y, rows=4, C=12, state=st)

    def upd(**kw):
        a = dict(base, **kw)
        d = a["desc"]
        return L.qt_scores_update(None if d is None else ctypes.byref(d), a["scores"], a["ld"], a["labels"], a["rows"], a["C"],
                                  a["state"], None)

    def refused(status, **kw):
        assert L.qt_scores_finalize(None, 12, 12, 15, rp, None, None) == QT_ERR_INVALID_ARG   # leaves another call's message behind
        got = upd(**kw)
        msg = L.qt_last_error()
        assert got == status, (kw, got, msg)
        assert msg and b"qt_scores_update" in msg, (kw, msg)

    refused(QT_ERR_INVALID_ARG, desc=None)
    for bad in (dict(kind=2), dict(kind=-1), dict(bits=3), dict(bits=15), dict(cal_bins=0), dict(cal_bins=65), dict(route=3),
                dict(route=-1)):
        refused(QT_ERR_INVALID_ARG, desc=desc(**bad))
    refused(QT_ERR_INVALID_ARG, scores=None)
    refused(QT_ERR_INVALID_ARG, labels=None)
    refused(QT_ERR_INVALID_ARG, state=None)
    refused(QT_ERR_INVALID_ARG, ld=11)
    assert b"stride" in L.qt_last_error()
    refused(QT_ERR_INVALID_ARG, rows=0)
    refused(QT_ERR_INVALID_ARG, rows=-4)
    refused(QT_ERR_INVALID_ARG, C=0, ld=0)
    for name, bad in (("scores", z + 2), ("labels", y + 4), ("state", st + 4)):
        refused(QT_ERR_INVALID_ARG, **{name: bad})
    refused(QT_ERR_UNSUPPORTED, C=65, ld=65)
    assert b"64" in L.qt_last_error()
    refused(QT_ERR_UNSUPPORTED, rows=(1 << 22) + 1)
    refused(QT_ERR_UNSUPPORTED, desc=desc(dtype=1))                                   # bf16 scores
    # the finalize
    fin = L.qt_scores_finalize
    assert fin(None, 12, 12, 15, rp, None, None) == QT_ERR_INVALID_ARG and b"qt_scores_finalize" in L.qt_last_error()
    assert fin(st, 12, 12, 15, None, cv, None) == QT_ERR_INVALID_ARG
    assert fin(st, 0, 12, 15, rp, cv, None) == QT_ERR_INVALID_ARG
    assert fin(st, 12, 3, 15, rp, cv, None) == QT_ERR_INVALID_ARG
    assert fin(st, 12, 15, 15, rp, cv, None) == QT_ERR_INVALID_ARG
    assert fin(st, 12, 12, 0, rp, cv, None) == QT_ERR_INVALID_ARG
    assert fin(st, 12, 12, 65, rp, cv, None) == QT_ERR_INVALID_ARG
    assert fin(st + 4, 12, 12, 15, rp, cv, None) == QT_ERR_INVALID_ARG
    assert fin(st, 12, 12, 15, rp + 4, cv, None) == QT_ERR_INVALID_ARG
    assert fin(st, 12, 12, 15, rp, cv + 4, None) == QT_ERR_INVALID_ARG
    assert fin(st, 65, 12, 15, rp, cv, None) == QT_ERR_UNSUPPORTED and b"qt_scores_finalize" in L.qt_last_error()


def test_module_constructor_and_device_checks():
    P = pkg()
    assert "ScoreMeter" in P.__all__ and P.ScoreMeter is pkg("scores").ScoreMeter
    for bad in (0, -1, 65, 12.0, True, None):
        with pytest.raises(ValueError):
            P.ScoreMeter(bad, "cuda:0")
    for kw in (dict(bits=3), dict(bits=15), dict(bits=12.0), dict(cal_bins=0), dict(cal_bins=65), dict(class_names=["a", "b"])):
        with pytest.raises(ValueError):
            P.ScoreMeter(3, "cuda:0", **kw)
    with pytest.raises(P.QtError):                  # no torch fallback
        P.ScoreMeter(12, "cpu")
