"""Score-based evaluation on the device: top-k accuracy, one-vs-rest ROC / AUC, average precision and calibration
(csrc/scores.hip), the figures that need the scores where EvalMeter (metrics.py) counts hard decisions.

    meter = ScoreMeter(num_classes, device, class_names=class_names)
    with torch.no_grad():
        for images, features, labels in val_loader:
            meter.update(model(images.to(device), features.to(device)), labels.to(device))
    report = meter.result()                          # the one host sync
    report["top_k"][1], report["auc"], report["macro"]["average_precision"], report["calibration"]["ece"]
    fpr, tpr, thresholds = meter.roc_curve(3)

Scores are f32 [rows, C] (any row stride, C <= 64, rows <= 2^22 per call): logits, of which the kernel forms the softmax
`predict` writes, or with probs= probabilities used as given (e.g. PoseTimeline's smoothed rows).  Probabilities are
quantised to K = 2^bits bins; AUC and average precision are those of the quantised scores, exactly and independent of the
order of execution.  There is no torch fallback: CPU tensors and other dtypes raise QtError.  include/qtcnn.h states the
layouts and every formula.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._abi import ScoresDesc, bind  # noqa: F401  (<module>.bind is _abi.bind)
from ._lib import QtError
from .loss import _row_major
from .metrics import MAX_ROWS, _check_index_vector

MAX_CLASSES = 64            # QT_SCORES_MAX_CLASSES
MAX_CAL_BINS = 64           # QT_SCORES_MAX_CAL_BINS
MIN_BITS, MAX_BITS = 4, 14  # QT_SCORES_MIN_BITS, QT_SCORES_MAX_BITS
LOGITS, PROBS = 0, 1        # QT_SCORES_LOGITS, QT_SCORES_PROBS
ROUTE_AUTO, ROUTE_DIRECT, ROUTE_PRIVATE = 0, 1, 2
COUNTERS = ("samples", "ignored", "invalid", "nan_rows", "updates")
SCALARS = ("macro_auc", "weighted_auc", "macro_ap", "weighted_ap", "ece", "mce", "samples", "ignored", "invalid", "nan_rows",
           "classes_scored", "updates")


def _int_in(value, lo, hi, what):
    if isinstance(value, bool) or not isinstance(value, int) or not lo <= value <= hi:
        raise ValueError(f"ScoreMeter: {what} must be an integer in {lo} .. {hi} (got {value!r})")
    return value


class ScoreMeter:
    """Top-k accuracy, one-vs-rest AUC / average precision and calibration of one validation pass, counted in device memory.

    `state` is an int64 tensor of 2 C K + C + 3 M + 5 additive counts (K = 2^bits, M = cal_bins; include/qtcnn.h).  It is
    additive: `merge(other)` adds another meter's counts, and under data parallelism
    `torch.distributed.all_reduce(meter.state)` before `result()` gives the report of all ranks' samples.  `update` launches
    one kernel and reads nothing back; `result()` is the one host sync."""

    def __init__(self, num_classes, device, bits=12, cal_bins=15, ignore_index=-100, class_names=None):
        C = _int_in(num_classes, 1, MAX_CLASSES, "num_classes")
        self.bits = _int_in(bits, MIN_BITS, MAX_BITS, "bits")
        self.cal_bins = _int_in(cal_bins, 1, MAX_CAL_BINS, "cal_bins")
        if class_names is not None:
            class_names = [str(c) for c in class_names]
            if len(class_names) != C:
                raise ValueError(f"ScoreMeter: {len(class_names)} class names for {C} classes")
        device = torch.device(device)
        if device.type != "cuda":
            raise QtError("ScoreMeter lives on an AMD GPU (device must be cuda:N); no CPU fallback")
        self.num_classes = C
        self.ignore_index = int(ignore_index)
        self.class_names = class_names
        self.route = ROUTE_AUTO      # qt_scores_desc.route; scripts/bench_scores.py forces one route per meter to time it
        K, M = 1 << self.bits, self.cal_bins
        self._hist = 2 * C * K
        self._cells = self._hist + C + 3 * M + len(COUNTERS)
        self._rep = 4 * C + 3 * M + len(SCALARS)
        # one allocation: the counts, then the report qt_scores_finalize writes, then its integer curves.  result() copies
        # the slice from the rank table to the report's end: one copy that leaves the histograms where they are
        self._buf = torch.zeros(self._cells + self._rep + self._hist, dtype=torch.int64, device=device)
        self.state = self._buf[:self._cells]
        self._report = self._buf[self._cells:self._cells + self._rep].view(torch.float64)
        self._curves = self._buf[self._cells + self._rep:]

    def reset(self):
        self.state.zero_()

    def merge(self, other):
        """add another meter's counts (same classes, bits and bins; copied to this meter's device when it lives on another)"""
        if (not isinstance(other, ScoreMeter) or other.num_classes != self.num_classes or other.bits != self.bits
                or other.cal_bins != self.cal_bins):
            raise QtError("ScoreMeter.merge: needs a ScoreMeter with the same number of classes, bits and cal_bins")
        self.state.add_(other.state.to(self.state.device))
        return self

    def update(self, logits=None, labels=None, *, probs=None):
        """Count one batch: logits f32 [rows, C], or probs= f32 [rows, C] used as given, and labels int64 [rows], all on the
        meter's device.  Returns None and reads nothing back."""
        what = "ScoreMeter.update"
        if (logits is None) == (probs is None):
            raise QtError(f"{what}: give either logits or probs=")
        if labels is None:
            raise QtError(f"{what}: needs labels")
        s, kind = (logits, LOGITS) if probs is None else (probs, PROBS)
        name = "logits" if probs is None else "probs"
        dev, C = self.state.device, self.num_classes
        if not isinstance(s, torch.Tensor):
            raise QtError(f"{what}: {name} must be a tensor")
        if s.device != dev:
            raise QtError(f"{what}: {name} must be on {dev} (got {s.device}); there is no CPU or torch fallback")
        if s.dtype != torch.float32:
            raise QtError(f"{what}: f32 {name} only (got {s.dtype})")
        if s.dim() != 2 or not 1 <= s.shape[0] <= MAX_ROWS or s.shape[1] != C:
            raise QtError(f"{what}: needs {name} [rows, {C}] with 1 <= rows <= {MAX_ROWS} (got {tuple(s.shape)})")
        labels = _check_index_vector(labels, "labels", s.shape[0], dev, what)
        s = _row_major(s.detach())
        L = _lib.lib()
        with torch.cuda.device(dev):
            desc = ScoresDesc(_lib.QT_F32, kind, self.bits, self.cal_bins, self.route, self.ignore_index)
            _lib.check(L.qt_scores_update(ctypes.byref(desc), _lib.ptr(s), s.stride(0), _lib.ptr(labels), s.shape[0], C,
                                          _lib.ptr(self.state), _lib.stream_ptr()), "qt_scores_update")

    def _finalize(self, curves):
        L = _lib.lib()
        with torch.cuda.device(self.state.device):
            _lib.check(L.qt_scores_finalize(_lib.ptr(self.state), self.num_classes, self.bits, self.cal_bins,
                                            _lib.ptr(self._report), _lib.ptr(self._curves) if curves else None,
                                            _lib.stream_ptr()), "qt_scores_finalize")

    def result(self):
        """The report as a dict: auc, average_precision (float64 [C], NaN where undefined), support (int64 [C]),
        macro / weighted {auc, average_precision}, top_k (float64 [C]: top_k[k - 1] is the top-k accuracy), calibration
        {count, accuracy, confidence (per bin), ece, mce}, samples, ignored, invalid, nan_rows, classes_scored, updates
        (, names)."""
        C, M = self.num_classes, self.cal_bins
        self._finalize(False)
        host = self._buf[self._hist:self._cells + self._rep].cpu().numpy()      # the one copy
        rep = host[self._cells - self._hist:].view(np.float64)
        s = dict(zip(SCALARS, rep[4 * C + 3 * M:].tolist()))
        cal = rep[4 * C:4 * C + 3 * M]
        out = {"auc": rep[:C].copy(), "average_precision": rep[C:2 * C].copy(), "support": rep[2 * C:3 * C].astype(np.int64),
               "macro": {"auc": s["macro_auc"], "average_precision": s["macro_ap"]},
               "weighted": {"auc": s["weighted_auc"], "average_precision": s["weighted_ap"]},
               "top_k": rep[3 * C:4 * C].copy(),
               "calibration": {"count": cal[:M].astype(np.int64), "accuracy": cal[M:2 * M].copy(),
                               "confidence": cal[2 * M:].copy(), "ece": s["ece"], "mce": s["mce"]}}
        for k in ("samples", "ignored", "invalid", "nan_rows", "classes_scored", "updates"):
            out[k] = int(s[k])
        if self.class_names is not None:
            out["names"] = list(self.class_names)
        return out

    def _class_curves(self, k):
        """(tp, fp, bins): the cumulative counts at the occupied bins of class k, from the highest bin down; P = tp[-1]"""
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < self.num_classes:
            raise ValueError(f"ScoreMeter: class index must be an integer in 0 .. {self.num_classes - 1} (got {k!r})")
        K = 1 << self.bits
        self._finalize(True)
        c = self._curves[2 * K * k:2 * K * (k + 1)].cpu().numpy().reshape(2, K)
        tot = np.append(c[0] + c[1], 0)
        bins = np.nonzero(tot[:-1] > tot[1:])[0][::-1]
        return c[0][bins], c[1][bins], bins

    def roc_curve(self, k):
        """(fpr, tpr, thresholds) of class k against the rest, as sklearn.metrics.roc_curve(y == k, q / K,
        drop_intermediate=False) returns them: thresholds descending over the occupied bins, led by the point (0, 0) at
        threshold inf.  NaN rates when the class (or the rest) has no sample."""
        tp, fp, bins = self._class_curves(k)
        P, N = (int(tp[-1]), int(fp[-1])) if len(bins) else (0, 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            tpr = np.concatenate([[0.0], tp / np.float64(P)])
            fpr = np.concatenate([[0.0], fp / np.float64(N)])
        return fpr, tpr, np.concatenate([[np.inf], bins / np.float64(1 << self.bits)])

    def pr_curve(self, k):
        """(precision, recall, thresholds) of class k against the rest, as sklearn.metrics.precision_recall_curve(y == k,
        q / K) returns them: thresholds ascending over the occupied bins, closed by the point (1, 0)."""
        tp, fp, bins = self._class_curves(k)
        P = int(tp[-1]) if len(bins) else 0
        with np.errstate(invalid="ignore", divide="ignore"):
            precision = np.concatenate([(tp / (tp + fp).astype(np.float64))[::-1], [1.0]])
            recall = np.concatenate([(tp / np.float64(P))[::-1], [0.0]])
        return precision, recall, bins[::-1] / np.float64(1 << self.bits)
