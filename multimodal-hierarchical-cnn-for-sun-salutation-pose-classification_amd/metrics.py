"""Evaluation report on the device: confusion matrix, precision / recall / F1, R^2 and softmax confidence
(csrc/metrics.hip).

The reference's evaluation (comparative analysis/analysis.py:60-109; the same confusion matrix in
3dcnn/train_3D_Quadtree_cnn_model.py:248 and VIT/fact_model_train.py:153) copies labels and predictions to the host every
batch and hands them to scikit-learn.  Here the counts stay in device memory for the whole evaluation:

    meter = EvalMeter(num_classes, device, class_names=class_names)
    with torch.no_grad():
        for images, features, labels in val_loader:
            meter.update(model(images.to(device), features.to(device)), labels.to(device))
    report = meter.result()                          # the one host sync
    report["accuracy"], report["precision"], report["recall"], report["f1"], report["r2"], report["confusion_matrix"]

and the video loop's softmax / max / .item() per frame (experiment/test_on_video_cnn.py:274-278) is one launch per batch:

    probs, confidence, pred = predict(model(frames, features))

Logits are f32 [rows, C] (any row stride, C <= 1024, rows <= 2^22 per call), labels and predictions int64 [rows].  A row
whose label is `ignore_index` is counted as ignored, a label or a given prediction outside [0, C) as invalid; neither
reaches the matrix.  There is no torch fallback: CPU tensors and other dtypes raise QtError.  include/qtcnn.h states the
layouts and every formula.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._abi import MetricsDesc, bind  # noqa: F401  (<module>.bind is _abi.bind)
from ._lib import QtError
from .loss import _row_major

MAX_CLASSES = 1024          # QT_METRICS_MAX_CLASSES
MAX_ROWS = 1 << 22
SCALARS = ("accuracy", "weighted_precision", "weighted_recall", "weighted_f1", "macro_precision", "macro_recall", "macro_f1",
           "r2", "samples", "ignored", "invalid", "classes_present")


def _check_logits(logits, what, C=None):
    if not isinstance(logits, torch.Tensor):
        raise QtError(f"{what}: logits must be a tensor")
    if logits.device.type != "cuda":
        raise QtError(f"{what}: logits must be on an AMD GPU (got {logits.device}); there is no CPU or torch fallback")
    if logits.dtype != torch.float32:
        raise QtError(f"{what}: f32 logits only (got {logits.dtype})")
    if logits.dim() != 2 or not 1 <= logits.shape[0] <= MAX_ROWS:
        raise QtError(f"{what}: needs logits [rows, C] with 1 <= rows <= {MAX_ROWS} (got {tuple(logits.shape)})")
    if not 1 <= logits.shape[1] <= MAX_CLASSES:
        raise QtError(f"{what}: C = {logits.shape[1]} classes; 1 .. {MAX_CLASSES} are handled")
    if C is not None and logits.shape[1] != C:
        raise QtError(f"{what}: the meter has {C} classes, the logits {logits.shape[1]}")


def _check_index_vector(t, name, rows, dev, what):
    if not isinstance(t, torch.Tensor):
        raise QtError(f"{what}: {name} must be a tensor")
    if t.device != dev:
        raise QtError(f"{what}: {name} must be on {dev} (got {t.device}); there is no CPU or torch fallback")
    if t.dtype != torch.int64:
        raise QtError(f"{what}: int64 {name} only (got {t.dtype})")
    if t.dim() != 1 or (rows is not None and t.shape[0] != rows) or not 1 <= t.shape[0] <= MAX_ROWS:
        raise QtError(f"{what}: {name} must have shape [{'rows' if rows is None else rows}] with 1 <= rows <= {MAX_ROWS} "
                      f"(got {tuple(t.shape)})")
    return t.contiguous()


def _update(logits, predictions, labels, state, C, ignore_index, want_probs):
    """one qt_metrics_update launch on checked operands; returns (probs, confidence, pred) or None"""
    L = _lib.lib()
    z = None if logits is None else _row_major(logits.detach())
    rows, dev = (z.shape[0], z.device) if z is not None else (predictions.shape[0], predictions.device)
    with torch.cuda.device(dev):
        out = (None, None, None)
        if want_probs:
            out = (torch.empty(rows, C, dtype=torch.float32, device=dev), torch.empty(rows, dtype=torch.float32, device=dev),
                   torch.empty(rows, dtype=torch.int64, device=dev))
        desc = MetricsDesc(_lib.QT_F32, ignore_index)
        _lib.check(L.qt_metrics_update(ctypes.byref(desc), _lib.ptr(z), z.stride(0) if z is not None else 0,
                                       _lib.ptr(predictions), _lib.ptr(labels), rows, C, _lib.ptr(state), _lib.ptr(out[0]), C,
                                       _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.stream_ptr()), "qt_metrics_update")
    return out if want_probs else None


def predict(logits):
    """(probs f32 [rows, C], confidence f32 [rows], pred int64 [rows]) of f32 logits on the GPU: torch.softmax(logits, 1),
    its maximum's value and torch.max(logits, 1)'s index, in one launch and without a host read."""
    _check_logits(logits, "predict")
    return _update(logits, None, None, None, logits.shape[1], -100, True)


class EvalMeter:
    """The evaluation report of one validation pass, counted in device memory.

    `state` is an int64 tensor of num_classes^2 + 4 additive counts (the confusion matrix, row = true class, then rows
    counted / ignored / invalid and the number of updates).  It is additive: `merge(other)` adds another meter's counts,
    and under data parallelism `torch.distributed.all_reduce(meter.state)` before `result()` gives the report of all
    ranks' samples.  `update` launches one kernel and reads nothing back; `result()` is the one host sync."""

    def __init__(self, num_classes, device, ignore_index=-100, class_names=None):
        if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 1 <= num_classes <= MAX_CLASSES:
            raise ValueError(f"EvalMeter: num_classes must be an integer in 1 .. {MAX_CLASSES} (got {num_classes!r})")
        if class_names is not None:
            class_names = [str(c) for c in class_names]
            if len(class_names) != num_classes:
                raise ValueError(f"EvalMeter: {len(class_names)} class names for {num_classes} classes")
        device = torch.device(device)
        if device.type != "cuda":
            raise QtError("EvalMeter lives on an AMD GPU (device must be cuda:N); no CPU fallback")
        self.num_classes = num_classes
        self.ignore_index = int(ignore_index)
        self.class_names = class_names
        C = num_classes
        self._cells = C * C + 4
        # one allocation: the counts, then the report qt_metrics_finalize writes, so that result() is one copy
        self._buf = torch.zeros(self._cells + 4 * C + len(SCALARS), dtype=torch.int64, device=device)
        self.state = self._buf[:self._cells]
        self._report = self._buf[self._cells:].view(torch.float64)

    def reset(self):
        self.state.zero_()

    def merge(self, other):
        """add another meter's counts (same class count; copied to this meter's device when it lives on another)"""
        if not isinstance(other, EvalMeter) or other.num_classes != self.num_classes:
            raise QtError("EvalMeter.merge: needs an EvalMeter with the same number of classes")
        self.state.add_(other.state.to(self.state.device))
        return self

    def update(self, logits=None, labels=None, *, predictions=None, probs=False):
        """Count one batch.  logits f32 [rows, C] or predictions= int64 [rows] (e.g. what the fused loss wrote to its
        predictions= tensor), and labels int64 [rows], all on the meter's device.  Returns None, or with probs=True (logits
        only) the tensors (probs [rows, C], confidence [rows], pred [rows]) of `predict`."""
        what = "EvalMeter.update"
        if (logits is None) == (predictions is None):
            raise QtError(f"{what}: give either logits or predictions=")
        if labels is None:
            raise QtError(f"{what}: needs labels (predict(logits) gives probabilities without counting)")
        if probs and logits is None:
            raise QtError(f"{what}: probs=True needs logits")
        dev = self.state.device
        if logits is not None:
            _check_logits(logits, what, self.num_classes)
            if logits.device != dev:
                raise QtError(f"{what}: logits must be on {dev} (got {logits.device})")
            rows = logits.shape[0]
        else:
            predictions = _check_index_vector(predictions, "predictions", None, dev, what)
            rows = predictions.shape[0]
        labels = _check_index_vector(labels, "labels", rows, dev, what)
        return _update(logits, predictions, labels, self.state, self.num_classes, self.ignore_index, bool(probs))

    def _read(self):
        """finalize launch, then one copy: (counts int64 [C*C + 4], report float64 [4C + 12]) as numpy arrays"""
        L = _lib.lib()
        with torch.cuda.device(self.state.device):
            _lib.check(L.qt_metrics_finalize(_lib.ptr(self.state), self.num_classes, _lib.ptr(self._report),
                                             _lib.stream_ptr()), "qt_metrics_finalize")
        host = self._buf.cpu().numpy()
        return host[:self._cells], host[self._cells:].view(np.float64)

    def result(self):
        """The report as a dict: accuracy, precision, recall, f1 (the weighted values, under analysis.py's key names), r2,
        confusion_matrix (numpy int64 [C, C], row = true class), per_class {precision, recall, f1, support (, names)},
        macro {precision, recall, f1}, samples, ignored, invalid, classes_present, updates."""
        C = self.num_classes
        counts, rep = self._read()
        s = dict(zip(SCALARS, rep[4 * C:].tolist()))
        per_class = {"precision": rep[:C].copy(), "recall": rep[C:2 * C].copy(), "f1": rep[2 * C:3 * C].copy(),
                     "support": rep[3 * C:4 * C].astype(np.int64)}
        if self.class_names is not None:
            per_class["names"] = list(self.class_names)
        return {"accuracy": s["accuracy"], "precision": s["weighted_precision"], "recall": s["weighted_recall"],
                "f1": s["weighted_f1"], "r2": s["r2"], "confusion_matrix": counts[:C * C].reshape(C, C).copy(),
                "per_class": per_class,
                "macro": {"precision": s["macro_precision"], "recall": s["macro_recall"], "f1": s["macro_f1"]},
                "samples": int(s["samples"]), "ignored": int(s["ignored"]), "invalid": int(s["invalid"]),
                "classes_present": int(s["classes_present"]), "updates": int(counts[C * C + 3])}

    def confusion_matrix(self, present_only=True):
        """numpy int64 matrix, row = true class.  present_only: only the classes that occur in the labels or in the
        predictions, in ascending order -- the shape sklearn.metrics.confusion_matrix(y_true, y_pred) returns when some
        classes are absent.  A host sync, like result()."""
        C = self.num_classes
        cm = self.state[:C * C].cpu().numpy().reshape(C, C)
        if not present_only:
            return cm
        keep = np.nonzero(cm.sum(0) + cm.sum(1))[0]
        return cm[np.ix_(keep, keep)]
