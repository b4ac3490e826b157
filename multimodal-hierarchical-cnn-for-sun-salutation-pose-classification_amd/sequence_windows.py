"""Sequence windows on the device: from labelled clips to the [B,T,...] samples of CnnLstm, Quadtree3DCNN and Ji3DCNN without
a stored copy of every window.  The reference materialises each window on disk (sqn process/create_sequential_dataset.py:154-205
copies 10 frames per window at stride 1; cnn+lstm/prepare_sequential_dataset.py:36-112 stores T normalised f32 frames per
window) and its loaders read one such file per sample.  Here every clip is held on the device once, as uint8 frames and raw
pose rows; a window is T consecutive rows and a sample is a gather (csrc/seq_windows.hip):

    win  = SequenceWindows(seq_len=4, stride=2, label="last", num_classes=K)   # or label="uniform"
    plan = win.plan(frame_labels, clip_lengths)     # int64 [N] on the GPU; lengths: host ints / CPU tensor [C]
    plan.starts, plan.labels                        # int32 / int64 views of length plan.count, on the device
    plan.count                                      # Python int; the one host sync, once per dataset, on first use
    idx    = torch.randperm(plan.count, device=dev)[:B]                 # the loader's shuffle
    frames = win.gather(clip_frames_u8, plan, idx)                      # [B,T,H,W,3] -> FramePreprocessor -> [B,T,3,224,224]
    numer  = win.gather_features(raw_rows, plan, idx, mode="standardize", means=m, stds=s)   # [B,T,F]
    labels = plan.labels[idx]

The frames of all clips are concatenated along the first axis, each clip in temporal order; a window never crosses a clip
boundary.  label="uniform" keeps a window iff its T labels are equal and in [0, num_classes) (create_sequential_dataset.py:
164-171); label="last" gives it its last frame's label and keeps it iff that is in [0, num_classes)
(prepare_sequential_dataset.py:46-62).  The kept starts come in ascending frame order, the reference's order.  `gather` takes
any contiguous per-frame tensor (uint8 [N,H,W,3], f32 [N,3,224,224], landmarks [N,33,4], ...); `gather_features` takes f32 rows
of any width up to 1024 (47 and 443 are in use) and applies the modes of PoseFeatures with the window's label, which is what
gives the 443 columns their class-mean and standardize modes; `fit_class_stats` is PoseFeatures.fit for any width.  A start
outside the source makes that window 0xFF bytes (NaN as a float); a label outside the tables makes it NaN.  include/qtcnn.h
states every rule.

Against the reference: it drops the frames that have no label from its table BEFORE it windows
(create_sequential_dataset.py:125-127), so its windows run over the remaining frames and may bridge the gap.  That stays the
caller's filter: `keep = frame_labels >= 0`, then frame_labels[keep], the per-frame arrays [keep] and the clip lengths counted
over keep.  Here "no label" is only ever a value outside [0, num_classes).  Not built: file I/O and label joins, splitting into
train / val / test, the loader's pad-or-truncate of a stored sequence of another length (windows made here always have T
frames).  There is no torch fallback: CPU tensors and other dtypes raise QtError.
"""
import ctypes

import torch

from . import _lib
from ._abi import SeqFeaturesDesc, SeqGatherDesc, SeqWindowsDesc, bind  # noqa: F401  (<module>.bind is _abi.bind)
from ._lib import QtError
from .pose import _MODES, class_stats

QT_SEQ_LABEL_UNIFORM, QT_SEQ_LABEL_LAST = 0, 1
MAX_FRAMES = 1 << 22
MAX_SEQ_LEN = 64
MAX_FEATURES = 1024
_RULES = {"uniform": QT_SEQ_LABEL_UNIFORM, "last": QT_SEQ_LABEL_LAST}


def _device_tensor(t, name, dtype=None, dev=None):
    if not isinstance(t, torch.Tensor):
        raise QtError(f"SequenceWindows: {name} must be a tensor")
    if dtype is not None and t.dtype != dtype:
        raise QtError(f"SequenceWindows: {name} must be {dtype} (got {t.dtype})")
    if t.device.type != "cuda" or (dev is not None and t.device != dev):
        raise QtError(f"SequenceWindows: {name} must be on {'an AMD GPU' if dev is None else dev} (got {t.device}); there is "
                      "no CPU or torch fallback")
    return t


def candidate_count(clip_lengths, seq_len, stride):
    """sum over the clips of max(0, (n - seq_len) // stride + 1): the window starts there are before any label is read"""
    return sum(max(0, (int(n) - seq_len) // stride + 1) for n in clip_lengths)


def fit_class_stats(raw, labels, num_classes):
    """PoseFeatures.fit for rows of any width: raw f32 [N,F] with NaNs and labels int64 [N], on the GPU -> (means, stds) f32
    [num_classes,F]: per class and column the mean and the population standard deviation + 1e-6 over the values that are
    not NaN; a cell without a value gets mean 0 and std 1; rows whose label is outside [0, num_classes) are left out.  Torch
    float64 operations on the device, once per dataset, no kernel; for F = 47 the same bits as PoseFeatures.fit."""
    raw = _device_tensor(raw, "raw", torch.float32)
    labels = _device_tensor(labels, "labels", torch.int64, raw.device)
    if raw.dim() != 2 or raw.shape[1] < 1 or labels.dim() != 1 or labels.shape[0] != raw.shape[0]:
        raise QtError(f"fit_class_stats: needs raw [N,F] and labels [N] (got {list(raw.shape)} / {list(labels.shape)})")
    if num_classes < 1:
        raise ValueError("fit_class_stats: num_classes must be positive")
    return class_stats(raw, labels, num_classes)


class WindowPlan:
    """The kept windows of a dataset: `starts` int32 and `labels` int64, views of length `count` of device buffers of the
    candidate count.  `count` is read from the device at its first use (the one host synchronisation) and kept."""

    def __init__(self, seq_len, frames, starts, labels, count):
        self.seq_len, self.frames = seq_len, frames
        self._starts, self._labels = starts, labels
        self._count_dev = count if isinstance(count, torch.Tensor) else None
        self._count = None if isinstance(count, torch.Tensor) else int(count)
        self.device = starts.device

    @property
    def capacity(self):
        return int(self._starts.shape[0])

    @property
    def count(self):
        if self._count is None:
            self._count = int(self._count_dev.item())
        return self._count

    @property
    def starts(self):
        return self._starts[:self.count]

    @property
    def labels(self):
        return self._labels[:self.count]

    def __len__(self):
        return self.count


class SequenceWindows:
    """seq_len: frames per window, 1 .. 64; stride: step between candidate starts inside a clip; label: "uniform" or "last";
    num_classes: labels outside [0, num_classes) are "no label".  See the module text."""

    def __init__(self, seq_len, stride=1, label="uniform", num_classes=None):
        if label not in _RULES:
            raise ValueError(f"SequenceWindows: label must be one of {sorted(_RULES)} (got {label!r})")
        if not 1 <= int(seq_len) <= MAX_SEQ_LEN:
            raise ValueError(f"SequenceWindows: seq_len must be 1 .. {MAX_SEQ_LEN} (got {seq_len})")
        if int(stride) < 1:
            raise ValueError(f"SequenceWindows: stride must be positive (got {stride})")
        if num_classes is None or int(num_classes) < 1:
            raise ValueError(f"SequenceWindows: num_classes must be positive (got {num_classes})")
        self.seq_len, self.stride, self.label, self.num_classes = int(seq_len), int(stride), label, int(num_classes)

    def plan(self, frame_labels, clip_lengths):
        """frame_labels: int64 [N] on the GPU, the frames of all clips one after the other; clip_lengths: the clips' frame
        counts, host ints or a CPU tensor [C], non-negative, summing to N.  Returns a WindowPlan."""
        what = "SequenceWindows.plan"
        if not isinstance(frame_labels, torch.Tensor) or frame_labels.dim() != 1:
            raise QtError(f"{what}: frame_labels must be a tensor [N]")
        if isinstance(clip_lengths, torch.Tensor):
            if clip_lengths.device.type != "cpu" or clip_lengths.dim() != 1 or clip_lengths.is_floating_point():
                raise ValueError(f"{what}: clip_lengths must be host ints or a CPU integer tensor [C]")
            clip_lengths = clip_lengths.tolist()
        lengths = [int(n) for n in clip_lengths]
        N = int(frame_labels.shape[0])
        if not lengths or min(lengths) < 0:
            raise ValueError(f"{what}: clip_lengths must be non-negative and there must be a clip")
        if sum(lengths) != N:
            raise ValueError(f"{what}: clip_lengths sum to {sum(lengths)}, frame_labels has {N} frames")
        frame_labels = _device_tensor(frame_labels, "frame_labels", torch.int64).contiguous()
        dev = frame_labels.device
        if not 1 <= N <= MAX_FRAMES:
            raise QtError(f"{what}: {N} frames; 1 .. {MAX_FRAMES} are handled in one plan")
        capacity = candidate_count(lengths, self.seq_len, self.stride)
        if capacity == 0:   # no clip reaches seq_len frames: nothing to ask the device
            return WindowPlan(self.seq_len, N, torch.empty(0, dtype=torch.int32, device=dev),
                              torch.empty(0, dtype=torch.int64, device=dev), 0)
        offsets = torch.zeros(len(lengths) + 1, dtype=torch.int64)
        offsets[1:] = torch.cumsum(torch.tensor(lengths, dtype=torch.int64), 0)
        offsets = offsets.to(torch.int32).to(dev)
        starts = torch.empty(capacity, dtype=torch.int32, device=dev)
        labels = torch.empty(capacity, dtype=torch.int64, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        L = _lib.lib()
        desc = SeqWindowsDesc(N, len(lengths), self.seq_len, self.stride, self.num_classes, capacity, _RULES[self.label])
        nbytes = L.qt_seq_windows_workspace_bytes(ctypes.byref(desc))
        workspace = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(L.qt_seq_windows_plan(ctypes.byref(desc), _lib.ptr(frame_labels), _lib.ptr(offsets), _lib.ptr(starts),
                                             _lib.ptr(labels), _lib.ptr(count), _lib.ptr(workspace), nbytes, _lib.stream_ptr()),
                       "qt_seq_windows_plan")
        return WindowPlan(self.seq_len, N, starts, labels, count)

    def _batch(self, plan, idx, dev, what):
        """(starts int32 [B], idx as int64) of the windows idx of plan"""
        if not isinstance(plan, WindowPlan) or plan.seq_len != self.seq_len:
            raise QtError(f"{what}: plan must be a WindowPlan made with seq_len {self.seq_len}")
        if plan.device != dev:
            raise QtError(f"{what}: the plan lives on {plan.device}, the source on {dev}")
        if plan.capacity == 0:
            raise QtError(f"{what}: the plan has no windows")
        idx = _device_tensor(idx, "idx", None, dev)
        if idx.dim() != 1 or idx.shape[0] < 1 or idx.dtype not in (torch.int64, torch.int32):
            raise QtError(f"{what}: idx must be an int64 or int32 tensor [B], B >= 1 (got {idx.dtype} {list(idx.shape)})")
        idx = idx.long()
        return plan._starts[idx], idx      # (the whole buffers: no need for `count`, no host synchronisation)

    @staticmethod
    def _out(out, shape, dtype, dev, what):
        if out is None:
            return torch.empty(shape, dtype=dtype, device=dev)
        _device_tensor(out, "out", dtype, dev)
        if tuple(out.shape) != tuple(shape) or not out.is_contiguous():
            raise QtError(f"{what}: out must be a contiguous tensor of shape {list(shape)} (got {list(out.shape)})")
        return out

    def gather(self, src, plan, idx, out=None):
        """src: a contiguous tensor on the GPU whose first dimension is the frame axis, [N,*tail], any dtype; idx: int64 [B]
        on the GPU, indices into the plan's windows.  Returns [B,T,*tail] in src's dtype: window idx[b]'s
        T consecutive frames; `out`: a contiguous tensor of that shape to write instead."""
        what = "SequenceWindows.gather"
        src = _device_tensor(src, "src")
        if src.dim() < 1 or src.numel() == 0 or not src.is_contiguous():
            raise QtError(f"{what}: src must be contiguous, [N,*tail] with no empty dimension (got {list(src.shape)}, "
                          f"contiguous: {src.is_contiguous()})")
        dev = src.device
        starts, _ = self._batch(plan, idx, dev, what)
        if src.shape[0] != plan.frames:
            raise QtError(f"{what}: src has {src.shape[0]} frames, the plan was made for {plan.frames}")
        B = int(starts.shape[0])
        out = self._out(out, (B, self.seq_len) + tuple(src.shape[1:]), src.dtype, dev, what)
        desc = SeqGatherDesc(int(src.shape[0]), src.numel() // src.shape[0] * src.element_size(), B, self.seq_len)
        L = _lib.lib()
        with torch.cuda.device(dev):
            _lib.check(L.qt_seq_gather_rows(ctypes.byref(desc), _lib.ptr(src), _lib.ptr(starts), _lib.ptr(out),
                                            _lib.stream_ptr()), "qt_seq_gather_rows")
        return out

    def gather_features(self, raw, plan, idx, mode="zero", means=None, stds=None, out=None):
        """raw: f32 [N,F] on the GPU, the stored pose rows of every frame with their NaNs, F <= 1024; mode: "raw", "zero",
        "class_mean" or "standardize" as in PoseFeatures, with means (both class modes) and stds ("standardize") f32 [K,F]
        on the GPU; the label of a window is the plan's.  Returns f32 [B,T,F]."""
        what = "SequenceWindows.gather_features"
        if mode not in _MODES:
            raise ValueError(f"{what}: mode must be one of {sorted(_MODES)} (got {mode!r})")
        need_means, need_stds = mode in ("class_mean", "standardize"), mode == "standardize"
        if (need_means and means is None) or (need_stds and stds is None):
            raise ValueError(f"{what}: mode {mode!r} needs {'means' if means is None else 'stds'}")
        raw = _device_tensor(raw, "raw", torch.float32)
        if raw.dim() != 2 or not 1 <= raw.shape[1] <= MAX_FEATURES or raw.shape[0] < 1 or not raw.is_contiguous():
            raise QtError(f"{what}: raw must be a contiguous [N,F] with 1 <= F <= {MAX_FEATURES} (got {list(raw.shape)})")
        dev, F = raw.device, int(raw.shape[1])
        starts, idx = self._batch(plan, idx, dev, what)
        if raw.shape[0] != plan.frames:
            raise QtError(f"{what}: raw has {raw.shape[0]} frames, the plan was made for {plan.frames}")
        labels, K = None, 0
        if need_means:
            labels = plan._labels[idx]
            means = _device_tensor(means, "means", torch.float32, dev).contiguous()
            K = int(means.shape[0])
            if means.dim() != 2 or means.shape[1] != F or K < 1:
                raise QtError(f"{what}: means must be [K,{F}] (got {list(means.shape)})")
            if need_stds:
                stds = _device_tensor(stds, "stds", torch.float32, dev).contiguous()
                if stds.shape != means.shape:
                    raise QtError(f"{what}: means and stds must have one shape")
        B = int(starts.shape[0])
        out = self._out(out, (B, self.seq_len, F), torch.float32, dev, what)
        desc = SeqFeaturesDesc(int(raw.shape[0]), F, B, self.seq_len, _MODES[mode], K)
        L = _lib.lib()
        with torch.cuda.device(dev):
            _lib.check(L.qt_seq_gather_features(ctypes.byref(desc), _lib.ptr(raw), _lib.ptr(starts), _lib.ptr(labels),
                                                _lib.ptr(means if need_means else None), _lib.ptr(stds if need_stds else None),
                                                _lib.ptr(out), _lib.stream_ptr()), "qt_seq_gather_features")
        return out
