"""The 47-float pose vector on the device: landmarks to features and the loaders' NaN imputation, one HIP kernel
(csrc/pose.hip) behind the two places the reference makes the vector per sample on a CPU core:

    pose = PoseFeatures("zero")                                   # inference: test_on_video_cnn.py:126-202, :257-261
    numerical = pose.from_landmarks(landmarks.to(device), detected.to(device))     # [N,33,4] -> [N,47]

    means, stds = load_class_stats("class_feature_means.json", "class_feature_stds.json")
    pose = PoseFeatures("standardize", means.to(device), stds.to(device))          # training: the loaders' __getitem__
    numerical = pose.impute(raw.to(device), labels.to(device))    # [N,47] or [B,T,47] stored vectors, NaNs included

`landmarks` holds MediaPipe's x, y, z, visibility of the 33 pose landmarks; a frame without a pose has detected == 0 (its
landmark values are not read).  Modes: "raw" (NaNs stay: dataset preparation), "zero" (NaN -> 0: inference and
cnn+lstm/dataloader.py:64-65), "class_mean" (NaN -> the class's mean: the 2-D loaders), "standardize" (that, then
(v - mean) / std, 0 where std < 1e-6: 3dcnn/dataloaders.py:125-135).  A [B,T,...] input takes one label per sequence.
include/qtcnn.h states the rule of every column.

Against the reference: joint angles are atan2(|ba x bc|, ba . bc) in f32 where the reference takes arccos of the
normalised dot product in float64 (the same angle; exactly collinear points give 0 or 180 where numpy's arccos can return
NaN; a zero-length limb is NaN in both).  A label outside the tables makes that row NaN; the reference's loaders fall back to
zeros for an unknown class without a word.  Not built: MediaPipe itself, left/right landmark swapping under a horizontal
flip (the reference does not do it either), writing the head's packed layout directly.  There is no torch fallback: CPU
tensors and other dtypes raise QtError.
"""
import ctypes
import json

import torch

from . import _lib
from ._abi import PoseDesc, bind  # noqa: F401  (<module>.bind is _abi.bind)
from ._lib import QtError

NUM_LANDMARKS, NUM_FEATURES = 33, 47   # QT_POSE_LANDMARKS, QT_POSE_FEATURES
MAX_ROWS = 1 << 22
QT_POSE_RAW, QT_POSE_ZERO, QT_POSE_CLASS_MEAN, QT_POSE_STANDARDIZE = 0, 1, 2, 3
_MODES = {"raw": QT_POSE_RAW, "zero": QT_POSE_ZERO, "class_mean": QT_POSE_CLASS_MEAN, "standardize": QT_POSE_STANDARDIZE}

FEATURE_NAMES = tuple(
    [f"LM{j}_visibility" for j in range(NUM_LANDMARKS)]
    + ["LEFT_ELBOW_ANGLE", "RIGHT_ELBOW_ANGLE", "LEFT_SHOULDER_ANGLE", "RIGHT_SHOULDER_ANGLE", "LEFT_KNEE_ANGLE",
       "RIGHT_KNEE_ANGLE", "LEFT_HIP_ANGLE", "RIGHT_HIP_ANGLE", "TORSO_VERTICAL_ANGLE", "TORSO_HORIZONTAL_ALIGNMENT",
       "DIST_LR_WRIST_NORM", "DIST_LR_ANKLE_NORM", "DIST_L_WRIST_HIP_NORM", "TORSO_VAR_XY_RATIO"])
assert len(FEATURE_NAMES) == NUM_FEATURES


def _device_tensor(t, name, dtype, dev=None):
    if not isinstance(t, torch.Tensor):
        raise QtError(f"PoseFeatures: {name} must be a tensor")
    if t.dtype != dtype:
        raise QtError(f"PoseFeatures: {name} must be {dtype} (got {t.dtype})")
    if t.device.type != "cuda" or (dev is not None and t.device != dev):
        raise QtError(f"PoseFeatures: {name} must be on {'an AMD GPU' if dev is None else dev} (got {t.device}); there is no "
                      "CPU or torch fallback")
    return t


def load_class_stats(means_json, stds_json=None, class_names=None):
    """The reference's class_feature_means.json / class_feature_stds.json ({class: {feature: value}}, written by
    1_prepare_still_image_dataset.py:324-349) as CPU f32 [K,47] tensors: (means, stds), stds None without a stds file.
    Row k is class_names[k]; by default the classes of the means file sorted, as the loaders number them
    (sorted(os.listdir(...)) / sorted(data.keys())).  Columns are matched BY NAME against FEATURE_NAMES.  The reference's
    loaders index the stored vector by the key's position in the JSON object instead (`for i, feature_name in
    enumerate(means_for_class.keys())`), which is the same thing only when the JSON's key order is the column order; a
    file whose keys are in another order is read correctly here and wrongly there.  A missing class or feature is a
    QtError."""
    def read(path):
        with open(path) as f:
            data = json.load(f)
        if not isinstance(data, dict) or not data:
            raise QtError(f"load_class_stats: {path} does not hold a {{class: {{feature: value}}}} object")
        return data

    means = read(means_json)
    stds = read(stds_json) if stds_json is not None else None
    names = sorted(means.keys()) if class_names is None else list(class_names)

    def table(data, path):
        t = torch.empty(len(names), NUM_FEATURES, dtype=torch.float64)
        for k, cls in enumerate(names):
            if cls not in data:
                raise QtError(f"load_class_stats: class {cls!r} is not in {path}")
            for c, feat in enumerate(FEATURE_NAMES):
                if feat not in data[cls]:
                    raise QtError(f"load_class_stats: feature {feat!r} of class {cls!r} is not in {path}")
                t[k, c] = float(data[cls][feat])
        return t.to(torch.float32)

    return table(means, means_json), (table(stds, stds_json) if stds is not None else None)


def class_stats(raw, labels, num_classes):
    """The rule of PoseFeatures.fit for any column count: raw f32 [N,F], labels int64 [N], both checked by the caller ->
    (means, stds) f32 [num_classes,F].  Torch float64 on raw's device."""
    v = raw.double()
    member = torch.nn.functional.one_hot(labels.clamp(0, num_classes - 1), num_classes).double()
    member = member * ((labels >= 0) & (labels < num_classes)).double()[:, None]      # [N,K]
    valid = (~torch.isnan(v)).double()                                                # [N,F]
    v0 = torch.nan_to_num(v, nan=0.0)
    count = member.t() @ valid                                                        # [K,F]
    n = count.clamp_min(1.0)
    mean = (member.t() @ (v0 * valid)) / n
    dev2 = (v0 - member @ mean) ** 2 * valid     # each row against its own class's mean
    std = torch.sqrt((member.t() @ dev2) / n) + 1e-6
    empty = count == 0
    mean = torch.where(empty, torch.zeros_like(mean), mean)
    std = torch.where(empty, torch.ones_like(std), std)
    return mean.float(), std.float()


class PoseFeatures:
    """mode: "zero", "raw", "class_mean" or "standardize"; means (both class modes) and stds ("standardize"): f32 [K,47]
    on the GPU the inputs will be on.  See the module text."""

    def __init__(self, mode="zero", means=None, stds=None):
        if mode not in _MODES:
            raise ValueError(f"PoseFeatures: mode must be one of {sorted(_MODES)} (got {mode!r})")
        self.mode = mode
        need_means = mode in ("class_mean", "standardize")
        need_stds = mode == "standardize"
        for t, name, need in ((means, "means", need_means), (stds, "stds", need_stds)):
            if need and t is None:
                raise ValueError(f"PoseFeatures: mode {mode!r} needs {name}")
            if t is not None and (not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != NUM_FEATURES
                                  or t.shape[0] < 1):
                raise ValueError(f"PoseFeatures: {name} must be a [K,{NUM_FEATURES}] tensor")
        if need_stds and stds.shape != means.shape:
            raise ValueError("PoseFeatures: means and stds must have one shape")
        self.means = means.detach().contiguous() if need_means else None
        self.stds = stds.detach().contiguous() if need_stds else None

    @staticmethod
    def fit(raw, labels, num_classes):
        """The class tables of 1_prepare_still_image_dataset.py:324-340 from raw vectors on the GPU: raw f32 [N,47] with
        NaNs, labels int64 [N] -> (means, stds) f32 [num_classes,47]: per class and feature the mean and the population
        standard deviation + 1e-6 over the values that are not NaN; a cell without a value gets mean 0 and std 1.  Rows
        whose label is outside [0, num_classes) are left out.  Torch float64 operations on the device: this runs once per
        dataset, is not a hot path and has no kernel of its own."""
        raw = _device_tensor(raw, "raw", torch.float32)
        labels = _device_tensor(labels, "labels", torch.int64, raw.device)
        if raw.dim() != 2 or raw.shape[1] != NUM_FEATURES or labels.dim() != 1 or labels.shape[0] != raw.shape[0]:
            raise QtError(f"PoseFeatures.fit: needs raw [N,{NUM_FEATURES}] and labels [N] (got {list(raw.shape)} / "
                          f"{list(labels.shape)})")
        if num_classes < 1:
            raise ValueError("PoseFeatures.fit: num_classes must be positive")
        return class_stats(raw, labels, num_classes)

    def _run(self, landmarks, detected, raw, labels, out, rows, rows_per_label, dev, what):
        if not 1 <= rows <= MAX_ROWS:
            raise QtError(f"{what}: {rows} rows; 1 .. {MAX_ROWS} are handled in one call")
        by_class = self.means is not None
        if by_class:
            if labels is None:
                raise QtError(f"{what}: mode {self.mode!r} needs labels")
            labels = _device_tensor(labels, "labels", torch.int64, dev).contiguous()
            if labels.dim() != 1 or labels.shape[0] * rows_per_label != rows:
                raise QtError(f"{what}: labels must have shape [{rows // rows_per_label}] (got {list(labels.shape)})")
            means = _device_tensor(self.means, "means", torch.float32, dev)
            stds = None if self.stds is None else _device_tensor(self.stds, "stds", torch.float32, dev)
        else:
            labels = means = stds = None
        L = _lib.lib()
        desc = PoseDesc(rows, _MODES[self.mode], rows_per_label, int(means.shape[0]) if by_class else 0)
        with torch.cuda.device(dev):
            _lib.check(L.qt_pose_features(ctypes.byref(desc), _lib.ptr(landmarks), _lib.ptr(detected), _lib.ptr(raw),
                                          _lib.ptr(labels), _lib.ptr(means), _lib.ptr(stds), _lib.ptr(out),
                                          _lib.stream_ptr()), "qt_pose_features")
        return out

    def from_landmarks(self, landmarks, detected=None, labels=None):
        """landmarks: f32 [N,33,4] or [B,T,33,4] on the GPU (x, y, z, visibility); detected: uint8 or bool [N] / [B,T], zero
        where no pose was found (None: found everywhere); labels: int64 [N] / [B] (one per sequence), read in the two class
        modes only.  Returns f32 [N,47] / [B,T,47]."""
        what = "PoseFeatures.from_landmarks"
        landmarks = _device_tensor(landmarks, "landmarks", torch.float32)
        dev = landmarks.device
        if landmarks.dim() not in (3, 4) or tuple(landmarks.shape[-2:]) != (NUM_LANDMARKS, 4) or landmarks.numel() == 0:
            raise QtError(f"{what}: landmarks must be [N,33,4] or [B,T,33,4], no empty dimension (got {list(landmarks.shape)})")
        lead = tuple(landmarks.shape[:-2])
        rows = landmarks.numel() // (NUM_LANDMARKS * 4)
        landmarks = landmarks.contiguous()
        if landmarks.data_ptr() % 16:
            landmarks = landmarks.clone()   # (a view that starts inside an allocation)
        if detected is not None:
            if isinstance(detected, torch.Tensor) and detected.dtype == torch.bool:
                detected = detected.to(torch.uint8)
            detected = _device_tensor(detected, "detected", torch.uint8, dev).contiguous()
            if tuple(detected.shape) != lead:
                raise QtError(f"{what}: detected must have shape {list(lead)} (got {list(detected.shape)})")
        out = torch.empty(lead + (NUM_FEATURES,), dtype=torch.float32, device=dev)
        return self._run(landmarks, detected, None, labels, out, rows, lead[1] if len(lead) == 2 else 1, dev, what)

    def impute(self, raw, labels=None, out=None):
        """raw: f32 [N,47] or [B,T,47] on the GPU, the stored vectors with their NaNs; labels as in from_landmarks; out:
        None (a new tensor) or a contiguous f32 tensor of raw's shape, which may be raw itself (in place)."""
        what = "PoseFeatures.impute"
        raw = _device_tensor(raw, "raw", torch.float32)
        dev = raw.device
        if raw.dim() not in (2, 3) or raw.shape[-1] != NUM_FEATURES or raw.numel() == 0:
            raise QtError(f"{what}: raw must be [N,47] or [B,T,47], no empty dimension (got {list(raw.shape)})")
        lead = tuple(raw.shape[:-1])
        if out is None:
            out = torch.empty(raw.shape, dtype=torch.float32, device=dev)
        else:
            _device_tensor(out, "out", torch.float32, dev)
            if out.shape != raw.shape or not out.is_contiguous():
                raise QtError(f"{what}: out must be a contiguous tensor of raw's shape {list(raw.shape)}")
        src = raw.contiguous()   # raw itself when it is contiguous: then out may be raw
        return self._run(None, None, src, labels, out, raw.numel() // NUM_FEATURES, lead[1] if len(lead) == 2 else 1, dev, what)
