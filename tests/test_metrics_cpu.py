"""The evaluation report, the parts that need no GPU: tests/_metrics_ref.py reproduces what the reference's own evaluate_model
returned (tests/golden/eval_metrics.npz) and what scikit-learn computes, a deliberately wrong macro average is caught; an f32
restatement of the softmax meets the derived bound and one without the maximum subtraction misses it; the C ABI's
declarations, size queries and host-side argument checks; the module's constructor and device checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _metrics_ref as R
from _util import PKG, ROOT, pkg

NEW_SYMBOLS = ["qt_metrics_state_bytes", "qt_metrics_report_bytes", "qt_metrics_update", "qt_metrics_finalize"]
QT_ERR_INVALID_ARG, QT_ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "eval_metrics.npz"))


def _case(golden, i):
    C = int(golden["num_classes"][i])
    z, y = golden[f"logits{i}"], golden[f"labels{i}"]
    return C, z, y, golden[f"scalars{i}"], golden[f"cm{i}"]


def test_fixture_has_the_five_cases(golden):
    shapes = [(int(golden["num_classes"][i]), golden[f"labels{i}"].shape[0]) for i in range(len(golden["cases"]))]
    assert shapes == [(12, 4099), (12, 300), (2, 65), (5, 64), (3, 7)]
    absent = []
    for i in range(5):
        C, z, y, _, cm = _case(golden, i)
        assert z.dtype == np.float32 and z.shape == (len(y), C) and y.dtype == np.int64
        assert bool((z * 2 == np.round(z * 2)).all()), "logits are multiples of 0.5"
        srt = np.sort(z, 1)
        assert int((srt[:, -1] == srt[:, -2]).sum()) > 0 or len(y) < 10, "ties at the maximum occur"
        absent.append(C - cm.shape[0])
    assert absent == [0, 2, 0, 2, 1]


@pytest.mark.parametrize("i", range(5))
def test_reference_reproduces_the_recorded_outputs_of_evaluate_model(golden, i):
    C, z, y, want, cm = _case(golden, i)
    st = R.count(y, R.argmax_ref(z), C)
    assert np.array_equal(R.present_submatrix(st[:C * C].reshape(C, C)), cm)
    assert st[C * C:].tolist() == [len(y), 0, 0, 1]
    s = R.scalars(R.report(st, C), C)
    got = [s["accuracy"], s["weighted_precision"], s["weighted_recall"], s["weighted_f1"], s["r2"]]
    assert R.close(got, want), (got, want.tolist())
    assert s["samples"] == len(y) and s["classes_present"] == cm.shape[0]


@pytest.mark.parametrize("i", range(5))
def test_reference_matches_scikit_learn(golden, i):
    M = pytest.importorskip("sklearn.metrics")
    C, z, y, _, _ = _case(golden, i)
    p = R.argmax_ref(z)
    st = R.count(y, p, C)
    rep = R.report(st, C)
    s = R.scalars(rep, C)
    assert np.array_equal(R.present_submatrix(st[:C * C].reshape(C, C)), M.confusion_matrix(y, p))
    assert R.close(s["accuracy"], M.accuracy_score(y, p))
    for avg in ("weighted", "macro"):
        pr, rc, f1, _ = M.precision_recall_fscore_support(y, p, average=avg, zero_division=0)
        assert R.close([s[f"{avg}_precision"], s[f"{avg}_recall"], s[f"{avg}_f1"]], [pr, rc, f1]), avg
    pr, rc, f1, sup = M.precision_recall_fscore_support(y, p, labels=list(range(C)), average=None, zero_division=0)
    assert R.close(rep[:4 * C], np.concatenate([pr, rc, f1, sup.astype(np.float64)]))
    assert R.close(s["r2"], M.r2_score(y, p))


def test_a_macro_average_over_all_classes_is_caught(golden):
    C, z, y, _, _ = _case(golden, 1)     # classes 3 and 7 absent
    st = R.count(y, R.argmax_ref(z), C)
    good, bad = R.scalars(R.report(st, C), C), R.scalars(R.report(st, C, macro_over_all_classes=True), C)
    for k in ("macro_precision", "macro_recall", "macro_f1"):
        assert not R.close(bad[k], good[k]) and abs(bad[k] - good[k] * 10 / 12) < 1e-12, k
    for k in ("accuracy", "weighted_f1", "r2"):
        assert bad[k] == good[k]
    M = pytest.importorskip("sklearn.metrics")
    pr, _, _, _ = M.precision_recall_fscore_support(y, R.argmax_ref(z), average="macro", zero_division=0)
    assert R.close(good["macro_precision"], pr) and not R.close(bad["macro_precision"], pr)


def test_report_edge_states():
    C = 4
    empty = R.scalars(R.report(np.zeros(C * C + 4, np.int64), C), C)
    assert all(np.isnan(empty[k]) for k in R.SCALARS[:8]) and empty["samples"] == 0 and empty["classes_present"] == 0
    assert not R.report(np.zeros(C * C + 4, np.int64), C)[:4 * C].any()
    one = R.scalars(R.report(R.count([2], [2], C), C), C)
    assert one["accuracy"] == 1.0 and one["macro_f1"] == 1.0 and np.isnan(one["r2"]) and one["classes_present"] == 1
    single = R.scalars(R.report(R.count([1, 1, 1], [1, 1, 1], C), C), C)
    assert single["r2"] == 1.0 and single["accuracy"] == 1.0           # SS_tot == 0 and SS_res == 0
    off = R.scalars(R.report(R.count([1, 1, 1], [1, 2, 1], C), C), C)
    assert off["r2"] == 0.0 and off["classes_present"] == 2            # SS_tot == 0, SS_res != 0
    st = R.count([0, -100, 7, -5, 1, 2 ** 40], [0, 1, 1, 1, 9, 0], C)
    assert st[C * C:].tolist() == [1, 1, 4, 1] and int(st[:C * C].sum()) == 1


@pytest.mark.parametrize("rows,C", R.SHAPES)
@pytest.mark.parametrize("scale", [1.0, 20.0, 90.0])
def test_f32_restatement_of_the_softmax_meets_the_bound(rows, C, scale):
    z = R.make_logits(rows, C, seed=rows + C, scale=scale / 3.0, step=0.25)
    p, bound = R.softmax_ref(z)
    r = R.ratio(R.softmax_f32(z), p, bound)
    assert r <= 1.0, r


def test_a_softmax_without_maximum_subtraction_misses_the_bound():
    z = R.make_logits(7, 12, seed=5, scale=30.0)     # |z| up to 90: exp overflows f32 without the subtraction
    z[0, 0], z[3, 5] = 90.0, -90.0
    assert float(np.abs(z).max()) == 90.0
    p, bound = R.softmax_ref(z)
    assert R.ratio(R.softmax_f32(z), p, bound) <= 1.0
    assert R.ratio(R.softmax_f32(z, subtract_max=False), p, bound) > 1.0
    small = R.make_logits(7, 12, seed=5)             # (harmless where nothing overflows)
    ps, bs = R.softmax_ref(small)
    assert R.ratio(R.softmax_f32(small, subtract_max=False), ps, bs) <= 1.0


def test_nan_pattern_of_the_restatement_is_torchs():
    z = R.make_logits(5, 12, seed=8)
    z[1, 3] = np.nan
    z[2, 7] = np.inf
    z[3, 2] = -np.inf
    z[4, :] = -np.inf
    want = R.nan_pattern(z)
    assert want.all(1).tolist() == [False, True, True, False, True] and want.any(1).tolist() == want.all(1).tolist()
    assert np.array_equal(np.isnan(R.softmax_f32(z)), want)


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    declared = set(re.findall(r"\b(qt_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(os.path.join(ROOT, PKG, "libqtcnn_hip.so"))
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
    assert "qt_metrics_desc" in header and re.search(r"#define\s+QT_METRICS_MAX_CLASSES\s+1024\b", header)


def test_size_queries():
    M = pkg("metrics")
    L = pkg("_lib").lib()
    for C in (1, 2, 12, 64, 65, 1024):
        assert L.qt_metrics_state_bytes(C) == 8 * (C * C + 4)
        assert L.qt_metrics_report_bytes(C) == 8 * (4 * C + 12)
    for C in (0, -3, 1025):
        assert L.qt_metrics_state_bytes(C) == 0 and L.qt_metrics_report_bytes(C) == 0


def test_host_side_argument_checks_need_no_device():
    M = pkg("metrics")
    L = pkg("_lib").lib()
    z, p_in, y, st, pr, cf, po, rp = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000   # never dereferenced
    good = M.MetricsDesc(0, -100)
    base = dict(desc=good, logits=z, ld=12, pred_in=None, labels=y, rows=4, C=12, state=st, probs=pr, ld_probs=12, conf=cf,
                pred_out=po)

    def upd(**kw):
        a = dict(base, **kw)
        d = a["desc"]
        return L.qt_metrics_update(None if d is None else ctypes.byref(d), a["logits"], a["ld"], a["pred_in"], a["labels"],
                                   a["rows"], a["C"], a["state"], a["probs"], a["ld_probs"], a["conf"], a["pred_out"], None)

    def refused(status, **kw):
        assert L.qt_metrics_finalize(None, 12, rp, None) == QT_ERR_INVALID_ARG      # leaves another call's message behind
        got = upd(**kw)
        msg = L.qt_last_error()
        assert got == status, (kw, got, msg)
        assert msg and b"qt_metrics_update" in msg, (kw, msg)

    refused(QT_ERR_INVALID_ARG, desc=None)
    refused(QT_ERR_INVALID_ARG, pred_in=p_in)                                        # both inputs
    refused(QT_ERR_INVALID_ARG, logits=None)                                         # neither
    refused(QT_ERR_INVALID_ARG, logits=None, pred_in=p_in, conf=None, pred_out=None)   # probs without logits
    refused(QT_ERR_INVALID_ARG, logits=None, pred_in=p_in, probs=None, pred_out=None)  # confidence without logits
    refused(QT_ERR_INVALID_ARG, state=None)                                          # labels without a state
    refused(QT_ERR_INVALID_ARG, labels=None)                                         # a state without labels
    refused(QT_ERR_INVALID_ARG, labels=None, state=None, probs=None, conf=None, pred_out=None)     # nothing to produce
    refused(QT_ERR_INVALID_ARG, ld=11)
    assert b"stride" in L.qt_last_error()
    refused(QT_ERR_INVALID_ARG, ld_probs=11)
    refused(QT_ERR_INVALID_ARG, rows=0)
    refused(QT_ERR_INVALID_ARG, rows=-4)
    refused(QT_ERR_INVALID_ARG, C=0, ld=0, ld_probs=0)
    for name, bad in (("logits", z + 2), ("probs", pr + 1), ("conf", cf + 2), ("labels", y + 4), ("state", st + 4),
                      ("pred_out", po + 4)):
        refused(QT_ERR_INVALID_ARG, **{name: bad})
    refused(QT_ERR_INVALID_ARG, logits=None, pred_in=p_in + 4, probs=None, conf=None, pred_out=None)
    refused(QT_ERR_UNSUPPORTED, C=1025, ld=1025, ld_probs=1025)
    assert b"1024" in L.qt_last_error()
    refused(QT_ERR_UNSUPPORTED, rows=(1 << 22) + 1)
    refused(QT_ERR_UNSUPPORTED, desc=M.MetricsDesc(1, -100))                         # bf16 logits
    # the finalize
    assert L.qt_metrics_finalize(None, 12, rp, None) == QT_ERR_INVALID_ARG and b"qt_metrics_finalize" in L.qt_last_error()
    assert L.qt_metrics_finalize(st, 12, None, None) == QT_ERR_INVALID_ARG
    assert L.qt_metrics_finalize(st, 0, rp, None) == QT_ERR_INVALID_ARG
    assert L.qt_metrics_finalize(st + 4, 12, rp, None) == QT_ERR_INVALID_ARG
    assert L.qt_metrics_finalize(st, 12, rp + 4, None) == QT_ERR_INVALID_ARG
    assert L.qt_metrics_finalize(st, 1025, rp, None) == QT_ERR_UNSUPPORTED


def test_module_constructor_and_device_checks():
    P = pkg()
    assert "EvalMeter" in P.__all__ and "predict" in P.__all__
    assert pkg("quadtree_from_scratch.models").EvalMeter is P.EvalMeter
    assert pkg("threed_cnn.models").EvalMeter is P.EvalMeter
    for bad in (0, -1, 1025, 12.0, True, None):
        with pytest.raises(ValueError):
            P.EvalMeter(bad, "cuda:0")
    with pytest.raises(ValueError):
        P.EvalMeter(3, "cuda:0", class_names=["a", "b"])
    # no torch fallback
    with pytest.raises(P.QtError):
        P.EvalMeter(12, "cpu")
    with pytest.raises(P.QtError):
        P.predict(torch.zeros(4, 12))
    with pytest.raises(P.QtError):
        P.predict([[0.0, 1.0]])
