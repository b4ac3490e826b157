"""Pose timeline on the device: smoothed probabilities, a debounced label per frame, and the segments "which pose from when to
when" (csrc/timeline.hip).  The reference has no such step: experiment/test_on_video_cnn.py:274-292 draws each frame's raw
argmax, so at every pose boundary of a Sun Salutation its caption flickers between two classes.  Here the video loop stays
on the device to its end:

    timeline = PoseTimeline(num_classes, device, window=15, min_run=5, min_confidence=0.5, class_names=class_names)
    for frames, landmarks, detected in video:                       # chunks of any length
        probs, _, _ = predict(model(pre(frames), pose(landmarks, detected)))
        pred, confidence, stable = timeline.update(probs)           # two launches, nothing read back
        out = annotator.draw(frames, landmarks, detected, stable, confidence)
    timeline.finish()                                               # end of the video: close the open segment
    for start, length, label, mean_confidence in timeline.segments()[0]:   # the one host sync
        ...
    counts, dwell = timeline.transitions()                          # [C, C] label-to-label counts, frames per class

`update` takes f32 probabilities [streams, frames, C] (or [frames, C] with one stream) on the GPU.  A frame's smoothed row
is the mean of the last `window` rows of its stream (fewer at its start), summed afresh per frame from the oldest to the
newest; `pred` is its argmax in the loss head's order and `confidence` its value.  `stable` follows `pred` once the same
class (with confidence >= min_confidence) has been seen `min_run` frames in a row, -1 before that and after `min_run`
unknown frames, which FrameAnnotator draws as no caption.  A stream handed over in any split into calls gives the same bits
as one call; the W - 1 previous rows and eight integers per stream are carried in device memory.  include/qtcnn.h states
both rules.  Limits: C <= 64, window <= 64, 2^22 frames per call.

Not built: EMA or majority-vote smoothing, a centred (look-ahead) window, C > 64.  Decoding over a pose-order prior and counting
Sun Salutation rounds are pose_order.py's (PoseOrderDecoder), which takes this module's smoothed rows.  There is no torch
fallback: CPU tensors and other dtypes raise QtError.
"""
import ctypes

import torch

from . import _lib
from ._abi import TimelineDesc, bind  # noqa: F401  (<module>.bind is _abi.bind)
from ._lib import QtError

MAX_CLASSES = 64            # QT_TIMELINE_MAX_CLASSES
MAX_WINDOW = 64             # QT_TIMELINE_MAX_WINDOW
TILE = 64                   # QT_TIMELINE_TILE
TRIP = 64                   # QT_TIMELINE_TRIP
STATE = 8                   # QT_TIMELINE_STATE
MAX_FRAMES = 1 << 22
CONF_ONE = 65536            # q(1.0): seg_conf_sum counts confidences in units of 1 / 65536
STATE_FIELDS = ("frames_seen", "stable_plus_1", "cand_plus_1", "run", "seg_start", "seg_len", "seg_conf_sum", "segments_total")


def _int_in(name, v, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
        raise ValueError(f"PoseTimeline: {name} must be an integer {'>= ' + str(lo) if hi is None else f'in {lo} .. {hi}'} (got {v!r})")
    return v


class PoseTimeline:
    """The timeline of `streams` videos (or camera feeds), kept in device memory: two history buffers of W - 1 rows per
    stream that `update` reads and writes in turn, eight int64 of state per stream, and the segment records int64
    [streams, capacity, 4] = (start, length, label, conf_sum).  `update` and `finish` launch kernels and read nothing back;
    `segments()` is the one host sync.  See the module text."""

    def __init__(self, num_classes, device, streams=1, window=15, min_run=5, min_confidence=0.0, capacity=4096, class_names=None):
        self.num_classes = _int_in("num_classes", num_classes, 1, MAX_CLASSES)
        self.streams = _int_in("streams", streams, 1, MAX_FRAMES)
        self.window = _int_in("window", window, 1, MAX_WINDOW)
        self.min_run = _int_in("min_run", min_run, 1, (1 << 31) - 1)
        self.capacity = _int_in("capacity", capacity, 0, (1 << 31) - 1)
        min_confidence = float(min_confidence)
        if min_confidence != min_confidence:
            raise ValueError("PoseTimeline: min_confidence is NaN")
        self.min_confidence = min_confidence
        if class_names is not None:
            class_names = [str(c) for c in class_names]
            if len(class_names) != num_classes:
                raise ValueError(f"PoseTimeline: {len(class_names)} class names for {num_classes} classes")
        self.class_names = class_names
        device = torch.device(device)
        if device.type != "cuda":
            raise QtError("PoseTimeline lives on an AMD GPU (device must be cuda:N); no CPU fallback")
        S, C, back = self.streams, self.num_classes, self.window - 1
        self._hist = torch.zeros(2, S, max(back, 1), C, dtype=torch.float32, device=device) if back else None
        self._counts = torch.zeros(2, S, dtype=torch.int32, device=device) if back else None
        self._cur = 0
        # one allocation: the state, then the records, so that segments() is one copy
        self._buf = torch.zeros(S * (STATE + 4 * self.capacity), dtype=torch.int64, device=device)
        self.state = self._buf[:S * STATE].view(S, STATE)
        self.records = self._buf[S * STATE:].view(S, self.capacity, 4)
        self.device = self._buf.device

    def reset(self):
        """every stream starts anew: empty history, zeroed state (no host sync; the records are simply no longer counted)"""
        self.state.zero_()
        if self._counts is not None:
            self._counts.zero_()
        return self

    def _desc(self, frames, flush):
        return TimelineDesc(self.streams, frames, self.num_classes, self.window, self.min_run, self.min_confidence,
                            self.capacity, int(flush))

    def update(self, probs, smoothed=False):
        """probs: f32 [streams, frames, C], or [frames, C] when there is one stream, on the timeline's device.  Returns
        (pred int64, confidence f32, stable int64), each [streams, frames] (or [frames]), and with smoothed=True the
        smoothed rows in the shape of probs as a fourth."""
        what = "PoseTimeline.update"
        if not isinstance(probs, torch.Tensor):
            raise QtError(f"{what}: probs must be a tensor")
        if probs.device.type != "cuda" or probs.device != self.device:
            raise QtError(f"{what}: probs must be on {self.device} (got {probs.device}); there is no CPU or torch fallback")
        if probs.dtype != torch.float32:
            raise QtError(f"{what}: f32 probabilities only (got {probs.dtype})")
        S, C = self.streams, self.num_classes
        flat = probs.dim() == 2
        if flat and S == 1:
            probs = probs.unsqueeze(0)
        if probs.dim() != 3 or probs.shape[0] != S or probs.shape[2] != C or probs.shape[1] < 1:
            raise QtError(f"{what}: probs must be [{S}, frames, {C}]{' or [frames, ' + str(C) + ']' if S == 1 else ''} with "
                          f"frames >= 1 (got {list(probs.shape)})")
        T = probs.shape[1]
        if S * T > MAX_FRAMES:
            raise QtError(f"{what}: {S * T} frames; at most {MAX_FRAMES} are handled in one call")
        probs = probs.detach()
        if probs.stride(2) != 1 or probs.stride(1) < C or (S > 1 and probs.stride(0) != T * probs.stride(1)):
            probs = probs.contiguous()
        lead = (T,) if flat else (S, T)
        dev = self.device
        pred = torch.empty(lead, dtype=torch.int64, device=dev)
        conf = torch.empty(lead, dtype=torch.float32, device=dev)
        stable = torch.empty(lead, dtype=torch.int64, device=dev)
        rows = torch.empty(lead + (C,), dtype=torch.float32, device=dev) if smoothed else None
        if self._hist is not None:
            r, w = self._cur, 1 - self._cur
            hist = (self._hist[r], self._counts[r], self._hist[w], self._counts[w])
        else:
            hist = (None, None, None, None)
        desc = self._desc(T, False)
        L = _lib.lib()
        with torch.cuda.device(dev):
            _lib.check(L.qt_timeline_smooth(ctypes.byref(desc), _lib.ptr(probs), probs.stride(1), *(_lib.ptr(t) for t in hist),
                                            _lib.ptr(rows), C, _lib.ptr(pred), _lib.ptr(conf), _lib.stream_ptr()),
                       "qt_timeline_smooth")
            _lib.check(L.qt_timeline_decode(ctypes.byref(desc), _lib.ptr(pred), _lib.ptr(conf), _lib.ptr(self.state),
                                            _lib.ptr(stable), _lib.ptr(self.records), _lib.stream_ptr()), "qt_timeline_decode")
        if self._hist is not None:
            self._cur = 1 - self._cur       # only now: a refused call leaves the history it read as the current one
        return (pred, conf, stable, rows) if smoothed else (pred, conf, stable)

    def finish(self):
        """end of the video: close every stream's open segment (one launch, nothing read back; calling it twice adds nothing)"""
        desc = self._desc(0, True)
        L = _lib.lib()
        with torch.cuda.device(self.device):
            _lib.check(L.qt_timeline_decode(ctypes.byref(desc), None, None, _lib.ptr(self.state), None, _lib.ptr(self.records),
                                            _lib.stream_ptr()), "qt_timeline_decode")
        return self

    def segments(self, as_tensors=False):
        """The closed segments of every stream, in order of their start: the one host sync.  Per stream a list of
        (start, length, label, mean_confidence) -- label is the class name when the timeline has class_names -- or with
        as_tensors=True a dict of CPU tensors start / length / label / conf_sum int64 [n] and mean_confidence float64 [n].
        Raises QtError when a stream closed more segments than `capacity` records hold."""
        S = self.streams
        host = self._buf.cpu()
        state, records = host[:S * STATE].view(S, STATE), host[S * STATE:].view(S, self.capacity, 4)
        out = []
        for s in range(S):
            total = int(state[s, STATE - 1])
            if total > self.capacity:
                raise QtError(f"PoseTimeline.segments: stream {s} closed {total} segments, the buffer holds capacity = "
                              f"{self.capacity}; build the timeline with a larger capacity")
            rec = records[s, :total]
            mean = rec[:, 3].double() / (CONF_ONE * rec[:, 1].double())
            if as_tensors:
                out.append({"start": rec[:, 0].clone(), "length": rec[:, 1].clone(), "label": rec[:, 2].clone(),
                            "conf_sum": rec[:, 3].clone(), "mean_confidence": mean})
            else:
                name = (lambda k: self.class_names[k]) if self.class_names is not None else int
                out.append([(int(a), int(n), name(int(k)), float(m)) for (a, n, k, _), m in zip(rec.tolist(), mean.tolist())])
        return out

    def transitions(self):
        """(counts int64 [C, C], dwell int64 [C]) over all streams, on the device and without a host sync: counts[i, j] is how
        often a segment of class i is followed by a segment of class j in its stream's list (a gap in between or not), dwell[k]
        the frames spent in segments of class k.  Plain torch on the records: once per video.  Open segments are not in
        the list before finish(); records beyond `capacity` do not exist and are not counted."""
        C = self.num_classes
        total = self.state[:, STATE - 1].clamp(max=self.capacity)
        slot = torch.arange(self.capacity, device=self.device)
        have = slot[None, :] < total[:, None]                                      # [S, capacity]
        label = self.records[:, :, 2].clamp(0, C - 1)
        dwell = torch.zeros(C, dtype=torch.int64, device=self.device)
        dwell.index_add_(0, label.reshape(-1), (self.records[:, :, 1] * have).reshape(-1))
        counts = torch.zeros(C * C, dtype=torch.int64, device=self.device)
        if self.capacity > 1:
            pair = (label[:, :-1] * C + label[:, 1:]).reshape(-1)
            counts.index_add_(0, pair, have[:, 1:].reshape(-1).to(torch.int64))
        return counts.view(C, C), dwell
