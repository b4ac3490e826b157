"""Segment-level evaluation on the device: the segmental edit score and the segmental F1 at IoU thresholds
(csrc/segments.hip).

PoseTimeline, PoseOrderDecoder, PosePosterior, PoseLagSmoother / PoseLagDecoder and PoseOrderLearner all serve one aim: turn
a flickering per-frame argmax into the right poses, in the right order, once each.  EvalMeter and ScoreMeter count frames and
cannot see whether they achieve it: a prediction that is 95 % frame-accurate but splits every pose hold into five fragments
scores almost as a clean one.  The yardsticks of the action-segmentation literature for exactly this are the segmental edit
score and the segmental F1 at an IoU threshold (Lea et al., CVPR 2017; the MS-TCN evaluation: Edit, F1@10/25/50).  The
reference has no such step.  Here the counts stay in device memory for the whole evaluation, as EvalMeter's do:

    raw, smooth, ordered = (SegmentMeter(num_classes, device, thresholds=(10, 25, 50)) for _ in range(3))
    for frames, features, labels in validation_videos:              # labels int64 [videos, frames] on the device
        probs, _, pred = predict(model(frames, features))           # a raw predict(...)[2] ...
        raw.update(pred.view_as(labels), labels)
        _, _, stable = timeline.reset().update(probs.view(*labels.shape, -1))
        smooth.update(stable, labels)                               # ... PoseTimeline's `stable` ...
        path, _ = decoder.decode(probs.view(*labels.shape, -1))
        ordered.update(decoder.state_class[path], labels)           # ... and decoder.state_class[path] from PoseOrderDecoder.decode
    for name, meter in (("argmax", raw), ("timeline", smooth), ("pose order", ordered)):
        r = meter.result()                                          # the one host sync
        print(name, r["edit"], [r["f1"][k] for k in (10, 25, 50)])

`update` takes int64 [videos, frames] tensors (any row stride) of WHOLE videos and an optional int32 `lengths` [videos]; a
value outside [0, num_classes) is unknown: it belongs to no run and, as a label, to no frame count.  A video with more than
1024 runs on either side overflows: it is counted in `videos_overflow` and in the frame counts only.  include/qtcnn.h states
the rule in full.  `state` is additive int64, so `merge`, `torch.distributed.all_reduce(meter.state)` and any split of the
videos into calls give the same bits.  `segment_runs` is the run extraction on its own (ground-truth segments to draw).

Not built: streaming a video across calls, per-class segment scores, boundary-distance metrics, round-count error.  There is
no torch fallback: CPU tensors and other dtypes raise QtError.
"""
import ctypes

import torch

from . import _lib
from ._abi import SegmentsDesc, bind  # noqa: F401  (<module>.bind is _abi.bind)
from ._lib import QtError

MAX_SEGMENTS = 1024         # QT_SEGMENTS_MAX
MAX_CLASSES = 1024          # QT_SEGMENTS_MAX_CLASSES
MAX_THRESHOLDS = 8          # QT_SEGMENTS_MAX_THRESHOLDS
RECORD = 5                  # QT_SEGMENTS_RECORD
STATE = 10                  # QT_SEGMENTS_STATE
MAX_FRAMES = 1 << 22
EDIT_ONE = 1 << 32          # edit_q counts a video's edit score in units of 2^-32
RECORD_FIELDS = ("m", "n", "edit_distance", "frames_labelled", "frames_correct")
STATE_FIELDS = ("videos", "videos_overflow", "videos_empty", "seg_pred", "seg_true", "edit_dist", "edit_max", "edit_q",
                "frames_labelled", "frames_correct")


def make_desc(batch, frames, num_classes, thresholds=(50,), capacity=0):
    pct = (ctypes.c_int * 8)(*thresholds)
    return SegmentsDesc(batch, frames, num_classes, len(thresholds), pct, capacity)


def _ratio(num, den):
    """num / den in float64; a zero denominator gives 0.0"""
    return float(num) / float(den) if den else 0.0


def report(state, thresholds):
    """The report of one copy of the state (a sequence of STATE + K integers): plain float64 arithmetic, no kernel.  A zero
    denominator gives 0.0.  `f1`, `precision`, `recall`, `tp`, `fp` and `fn` are dicts keyed by threshold (per cent)."""
    s = [int(v) for v in state]
    K = len(thresholds)
    if len(s) != STATE + K:
        raise ValueError(f"report: the state has {len(s)} integers, {STATE} + {K} thresholds are expected")
    out = dict(zip(STATE_FIELDS, s[:STATE]))
    scored = out["videos"] - out["videos_overflow"] - out["videos_empty"]
    seg_pred, seg_true = out["seg_pred"], out["seg_true"]
    out["edit"] = 100.0 * _ratio(out["edit_q"], EDIT_ONE * scored)
    out["edit_micro"] = 100.0 * (1.0 - out["edit_dist"] / out["edit_max"]) if out["edit_max"] else 0.0
    out["frame_accuracy"] = _ratio(out["frames_correct"], out["frames_labelled"])
    out["over_segmentation"] = _ratio(seg_pred, seg_true)
    out["thresholds"] = tuple(thresholds)
    for key in ("tp", "fp", "fn", "precision", "recall", "f1"):
        out[key] = {}
    for pct, tp in zip(thresholds, s[STATE:]):
        out["tp"][pct], out["fp"][pct], out["fn"][pct] = tp, seg_pred - tp, seg_true - tp
        out["precision"][pct] = 100.0 * _ratio(tp, seg_pred)
        out["recall"][pct] = 100.0 * _ratio(tp, seg_true)
        out["f1"][pct] = 100.0 * _ratio(2 * tp, seg_pred + seg_true)
    return out


def _check_classes(who, num_classes):
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 1 <= num_classes <= MAX_CLASSES:
        raise ValueError(f"{who}: num_classes must be an integer in 1 .. {MAX_CLASSES} (got {num_classes!r})")
    return num_classes


def _check_videos(t, name, what, dev=None, shape=None):
    """an int64 [videos, frames] device tensor whose rows are dense (any row stride >= frames); copied if they are not"""
    if not isinstance(t, torch.Tensor):
        raise QtError(f"{what}: {name} must be a tensor")
    if t.device.type != "cuda" or (dev is not None and t.device != dev):
        raise QtError(f"{what}: {name} must be on {dev or 'an AMD GPU'} (got {t.device}); there is no CPU or torch fallback")
    if t.dtype != torch.int64:
        raise QtError(f"{what}: int64 {name} only (got {t.dtype})")
    if t.dim() != 2 or t.shape[0] < 1:
        raise QtError(f"{what}: {name} must be [videos, frames] with at least one video (got {list(t.shape)})")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise QtError(f"{what}: {name} has shape {list(t.shape)}, pred has {list(shape)}")
    if max(t.shape[0], t.shape[0] * t.shape[1]) > MAX_FRAMES:
        raise QtError(f"{what}: {t.shape[0]} videos of {t.shape[1]} frames; at most {MAX_FRAMES} frames (and videos) per call")
    t = t.detach()
    B, T = t.shape
    if T and (t.stride(1) != 1 or (B > 1 and t.stride(0) < T)):
        t = t.contiguous()
    return t


def _row_stride(t):
    return max(t.stride(0), t.shape[1]) if t.shape[0] > 1 else t.shape[1]


def _check_lengths(lengths, videos, dev, what):
    if lengths is None:
        return None
    if not isinstance(lengths, torch.Tensor):
        raise QtError(f"{what}: lengths must be a tensor")
    if lengths.device != dev:
        raise QtError(f"{what}: lengths must be on {dev} (got {lengths.device}); there is no CPU or torch fallback")
    if lengths.dtype != torch.int32:
        raise QtError(f"{what}: int32 lengths only (got {lengths.dtype})")
    if tuple(lengths.shape) != (videos,):
        raise QtError(f"{what}: lengths must have shape [{videos}] (got {list(lengths.shape)})")
    return lengths.contiguous()


class SegmentMeter:
    """The segment-level report of one validation pass, counted in device memory.

    `state` is an int64 tensor of 10 + K additive counts (STATE_FIELDS, then tp per threshold).  `merge(other)` adds another
    meter's counts, and under data parallelism `torch.distributed.all_reduce(meter.state)` before `result()` gives the report
    of all ranks' videos.  `update` launches two kernels and reads nothing back; `result()` is the one host sync."""

    def __init__(self, num_classes, device, thresholds=(10, 25, 50)):
        self.num_classes = _check_classes("SegmentMeter", num_classes)
        try:
            thresholds = tuple(thresholds)
        except TypeError:
            raise ValueError(f"SegmentMeter: thresholds must be a sequence of integers (got {thresholds!r})") from None
        if not 1 <= len(thresholds) <= MAX_THRESHOLDS:
            raise ValueError(f"SegmentMeter: {len(thresholds)} thresholds; 1 .. {MAX_THRESHOLDS} are handled")
        for pct in thresholds:
            if isinstance(pct, bool) or not isinstance(pct, int) or not 1 <= pct <= 100:
                raise ValueError(f"SegmentMeter: thresholds are integers in 1 .. 100 per cent (got {pct!r})")
        self.thresholds = thresholds
        device = torch.device(device)
        if device.type != "cuda":
            raise QtError("SegmentMeter lives on an AMD GPU (device must be cuda:N); no CPU fallback")
        self.state = torch.zeros(STATE + len(thresholds), dtype=torch.int64, device=device)
        self.device = self.state.device
        self._work = None

    def reset(self):
        self.state.zero_()
        return self

    def merge(self, other):
        """add another meter's counts (same classes and thresholds; copied to this meter's device when it lives on another)"""
        if not isinstance(other, SegmentMeter) or other.num_classes != self.num_classes or other.thresholds != self.thresholds:
            raise QtError("SegmentMeter.merge: needs a SegmentMeter with the same number of classes and the same thresholds")
        self.state.add_(other.state.to(self.device))
        return self

    def update(self, pred, label, lengths=None, records=False):
        """Count `videos` whole videos.  pred, label: int64 [videos, frames] on the meter's device, any row stride; lengths:
        int32 [videos] or None (every video has `frames` frames).  Returns None, or with records=True the per-video records
        int64 [videos, 5 + K] = (m, n, D, frames_labelled, frames_correct, tp per threshold) as a device tensor."""
        what = "SegmentMeter.update"
        pred = _check_videos(pred, "pred", what, self.device)
        label = _check_videos(label, "label", what, self.device, pred.shape)
        B, T = pred.shape
        lengths = _check_lengths(lengths, B, self.device, what)
        K = len(self.thresholds)
        desc = make_desc(B, T, self.num_classes, self.thresholds)
        L = _lib.lib()
        need = L.qt_segments_workspace_bytes(ctypes.byref(desc))
        if self._work is None or self._work.numel() * 8 < need:
            self._work = torch.empty(need // 8, dtype=torch.int64, device=self.device)   # (kept: the stream orders its reuse)
        out = torch.empty(B, RECORD + K, dtype=torch.int64, device=self.device) if records else None
        with torch.cuda.device(self.device):
            _lib.check(L.qt_segments_update(ctypes.byref(desc), _lib.ptr(pred), _row_stride(pred), _lib.ptr(label),
                                            _row_stride(label), _lib.ptr(lengths), _lib.ptr(self.state), _lib.ptr(out),
                                            _lib.ptr(self._work), self._work.numel() * 8, _lib.stream_ptr()), "qt_segments_update")
        return out

    def result(self):
        """The report as a dict (the one host sync): edit, edit_micro, f1 / precision / recall / tp / fp / fn keyed by
        threshold, frame_accuracy, over_segmentation, and the counts of STATE_FIELDS.  A zero denominator gives 0.0."""
        return report(self.state.cpu().tolist(), self.thresholds)


def segment_runs(values, num_classes, lengths=None, capacity=None):
    """(runs int32 [videos, capacity, 3] = (start, length, class), counts int32 [videos]) of int64 [videos, frames] values on
    the GPU, device tensors both, nothing read back.  capacity: runs kept per video (default: frames, which holds them all);
    counts is the true number of runs, records at and behind it are not written."""
    what = "segment_runs"
    _check_classes(what, num_classes)
    values = _check_videos(values, "values", what)
    B, T = values.shape
    dev = values.device
    lengths = _check_lengths(lengths, B, dev, what)
    if capacity is None:
        capacity = T
    if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 0:
        raise ValueError(f"{what}: capacity must be a non-negative integer (got {capacity!r})")
    runs = torch.empty(B, capacity, 3, dtype=torch.int32, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    desc = make_desc(B, T, num_classes, capacity=capacity)
    L = _lib.lib()
    with torch.cuda.device(dev):
        _lib.check(L.qt_segments_encode(ctypes.byref(desc), _lib.ptr(values), _row_stride(values), _lib.ptr(lengths),
                                        _lib.ptr(runs) if capacity else None, _lib.ptr(counts), _lib.stream_ptr()),
                   "qt_segments_encode")
    return runs, counts
