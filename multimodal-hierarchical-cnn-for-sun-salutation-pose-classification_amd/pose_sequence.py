"""Sequence pose features on the device: the 443 columns per frame of the reference's sequence pipeline
(sqn process/processing_image_sequence.py:96-247, driven per clip by the loop at :374-441; stored as a sequence's
features.npy by create_sequential_dataset.py:179-181), one HIP kernel (csrc/pose_seq.hip) in place of a Python dict of 443
entries per frame:

    seq = SequencePoseFeatures("zero", frame_size=(640, 480))           # NaN -> 0, as cnn+lstm/dataloader.py:64-65
    features = seq.from_landmarks(landmarks.to(device), detected.to(device))       # [B,T,33,4] -> [B,T,443]

`landmarks` holds MediaPipe's x, y, z, visibility of the 33 pose landmarks of every frame of B clips; a frame without a pose
has detected == 0 (its landmark values are not used) and becomes 443 NaNs ("raw") or zeros ("zero").  The frame size
(W, H) is one per call (`frame_size`) or one per clip (`sizes`, int32 [B,2] on the GPU).  Columns (SEQUENCE_FEATURE_NAMES, the
reference's dict order): the landmarks as given, ten visibility-gated joint angles in pixel space, three distances over a
body scale, hip-relative coordinates, per-landmark velocity and acceleration over the two previous frames of the clip in
which a pose was found, a torso variance ratio.  include/qtcnn.h states the rule of every column.

A live loop that gets its frames in chunks carries the two previous detected frames of every clip in a history:

    hist = seq.history(batch=B, device=device)
    for chunk, found in stream:                                         # [B,t,33,4], [B,t]; any t >= 1
        features = seq.from_landmarks(chunk, found, history=hist)       # the same bits as one call over the whole clip
    hist.reset(mask)                                                    # bool [B]: these clips start anew

Against the reference: angles are atan2(|ba x bc|, ba . bc) in f32 where the reference takes arccos of the clipped cosine
in float64 (the same angle); a NaN visibility is not visible (the reference's `<` gate lets it through); one frame size per
clip, where the reference reads every image's own shape.  Class-mean and standardize imputation for the 443 columns and the
sliding-window grouping of create_sequential_dataset.py are sequence_windows.py (SequenceWindows.gather_features, .plan).
Not built: MediaPipe itself.  There is no torch fallback: CPU tensors and other dtypes raise QtError.
"""
import ctypes

import torch

from . import _lib
from ._abi import PoseSeqDesc, bind  # noqa: F401  (<module>.bind is _abi.bind)
from ._lib import QtError
from .pose import NUM_LANDMARKS, QT_POSE_RAW, QT_POSE_ZERO

NUM_SEQUENCE_FEATURES = 443   # QT_POSE_SEQ_FEATURES
MAX_FRAMES = 1 << 22
_MODES = {"raw": QT_POSE_RAW, "zero": QT_POSE_ZERO}

ANGLE_NAMES = ("LEFT_ELBOW_ANGLE", "RIGHT_ELBOW_ANGLE", "LEFT_SHOULDER_ANGLE", "RIGHT_SHOULDER_ANGLE", "LEFT_KNEE_ANGLE",
               "RIGHT_KNEE_ANGLE", "LEFT_HIP_ANGLE", "RIGHT_HIP_ANGLE", "TORSO_VERTICAL_ANGLE", "TORSO_HORIZONTAL_ALIGNMENT")
SEQUENCE_FEATURE_NAMES = tuple(
    [f"LM{j}_{c}" for j in range(NUM_LANDMARKS) for c in ("norm_x", "norm_y", "norm_z", "visibility")]
    + list(ANGLE_NAMES) + ["DIST_LR_WRIST_NORM", "DIST_LR_ANKLE_NORM", "DIST_L_WRIST_HIP_NORM"]
    + [f"LM{j}_rel_{c}_norm" for j in range(NUM_LANDMARKS) for c in "xyz"]
    + [f"LM{j}_{c}_px" for j in range(NUM_LANDMARKS) for c in ("vx", "vy", "vz", "ax", "ay", "az")]
    + ["TORSO_VAR_XY_RATIO"])
assert len(SEQUENCE_FEATURE_NAMES) == NUM_SEQUENCE_FEATURES


def _device_tensor(t, name, dtype, dev=None):
    if not isinstance(t, torch.Tensor):
        raise QtError(f"SequencePoseFeatures: {name} must be a tensor")
    if t.dtype != dtype:
        raise QtError(f"SequencePoseFeatures: {name} must be {dtype} (got {t.dtype})")
    if t.device.type != "cuda" or (dev is not None and t.device != dev):
        raise QtError(f"SequencePoseFeatures: {name} must be on {'an AMD GPU' if dev is None else dev} (got {t.device}); "
                      "there is no CPU or torch fallback")
    return t


class SequenceHistory:
    """The last two detected frames of `batch` clips between calls: two buffers of landmarks f32 [batch,2,33,4] (slot 0 the
    most recent) and counts uint8 [batch], one read and the other written by a call, then swapped.  `frames` / `counts`
    are the current state."""

    def __init__(self, batch, device):
        device = torch.device(device)
        if batch < 1:
            raise ValueError("SequenceHistory: batch must be positive")
        if device.type != "cuda":
            raise QtError(f"SequenceHistory: the buffers live on an AMD GPU (got {device})")
        self._frames = torch.zeros(2, batch, 2, NUM_LANDMARKS, 4, dtype=torch.float32, device=device)
        self._counts = torch.zeros(2, batch, dtype=torch.uint8, device=device)
        self._cur = 0
        self.batch, self.device = batch, self._frames.device

    @property
    def frames(self):
        return self._frames[self._cur]

    @property
    def counts(self):
        return self._counts[self._cur]

    def reset(self, mask=None):
        """Forget the history of every clip, or of the clips where the bool [batch] tensor `mask` is set (no host sync)."""
        if mask is None:
            self.counts.zero_()
        else:
            mask = _device_tensor(mask, "mask", torch.bool, self.device)
            if tuple(mask.shape) != (self.batch,):
                raise QtError(f"SequenceHistory.reset: mask must have shape [{self.batch}] (got {list(mask.shape)})")
            self.counts.masked_fill_(mask, 0)
        return self

    def _swap(self):
        """(read, write) buffers of the next call; the written ones become the current state"""
        r, w = self._cur, 1 - self._cur
        self._cur = w
        return self._frames[r], self._counts[r], self._frames[w], self._counts[w]


class SequencePoseFeatures:
    """mode: "zero" or "raw"; frame_size: (W, H) of every clip's frames, or None when each call brings `sizes`.  See the
    module text."""

    def __init__(self, mode="zero", frame_size=None):
        if mode not in _MODES:
            raise ValueError(f"SequencePoseFeatures: mode must be one of {sorted(_MODES)} (got {mode!r})")
        if frame_size is not None:
            w, h = (int(v) for v in frame_size)
            if w < 1 or h < 1:
                raise ValueError(f"SequencePoseFeatures: frame_size must be positive (got {frame_size})")
            frame_size = (w, h)
        self.mode, self.frame_size = mode, frame_size

    @staticmethod
    def history(batch, device):
        return SequenceHistory(batch, device)

    def from_landmarks(self, landmarks, detected=None, sizes=None, history=None):
        """landmarks: f32 [B,T,33,4] on the GPU, or [T,33,4] (one clip); detected: uint8 or bool [B,T] / [T], zero where no
        pose was found (None: found everywhere); sizes: int32 [B,2] = (W, H) per clip on the GPU (None: frame_size);
        history: a SequenceHistory of B clips, read and advanced by the call (None: every clip starts empty).  Returns f32
        [B,T,443] / [T,443]."""
        what = "SequencePoseFeatures.from_landmarks"
        landmarks = _device_tensor(landmarks, "landmarks", torch.float32)
        dev = landmarks.device
        if landmarks.dim() not in (3, 4) or tuple(landmarks.shape[-2:]) != (NUM_LANDMARKS, 4) or landmarks.numel() == 0:
            raise QtError(f"{what}: landmarks must be [B,T,33,4] or [T,33,4], no empty dimension (got {list(landmarks.shape)})")
        lead = tuple(landmarks.shape[:-2])
        B, T = (1, lead[0]) if len(lead) == 1 else lead
        if B * T > MAX_FRAMES:
            raise QtError(f"{what}: {B * T} frames; at most {MAX_FRAMES} are handled in one call")
        landmarks = landmarks.contiguous()
        if landmarks.data_ptr() % 16:
            landmarks = landmarks.clone()   # (a view that starts inside an allocation)
        if detected is not None:
            if isinstance(detected, torch.Tensor) and detected.dtype == torch.bool:
                detected = detected.to(torch.uint8)
            detected = _device_tensor(detected, "detected", torch.uint8, dev).contiguous()
            if tuple(detected.shape) != lead:
                raise QtError(f"{what}: detected must have shape {list(lead)} (got {list(detected.shape)})")
        if sizes is not None:
            sizes = _device_tensor(sizes, "sizes", torch.int32, dev).contiguous()
            if tuple(sizes.shape) != (B, 2):
                raise QtError(f"{what}: sizes must have shape [{B},2] (got {list(sizes.shape)})")
        elif self.frame_size is None:
            raise QtError(f"{what}: no frame size: give frame_size=(W, H) to the constructor or `sizes` to the call")
        if history is not None:
            if not isinstance(history, SequenceHistory) or history.batch != B or history.device != dev:
                raise QtError(f"{what}: history must be a SequenceHistory of {B} clips on {dev}")
            hist_in, count_in, hist_out, count_out = history._swap()
        else:
            hist_in = count_in = hist_out = count_out = None
        out = torch.empty(lead + (NUM_SEQUENCE_FEATURES,), dtype=torch.float32, device=dev)
        w, h = self.frame_size if self.frame_size is not None else (0, 0)
        desc = PoseSeqDesc(B, T, w, h, _MODES[self.mode])
        L = _lib.lib()
        with torch.cuda.device(dev):
            _lib.check(L.qt_pose_sequence_features(ctypes.byref(desc), _lib.ptr(landmarks), _lib.ptr(detected), _lib.ptr(sizes),
                                                   _lib.ptr(hist_in), _lib.ptr(count_in), _lib.ptr(hist_out),
                                                   _lib.ptr(count_out), _lib.ptr(out), _lib.stream_ptr()),
                       "qt_pose_sequence_features")
        return out
