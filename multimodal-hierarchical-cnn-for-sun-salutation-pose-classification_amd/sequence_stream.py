"""CnnLstm on a video stream: one row of logits per frame, every frame embedded once (csrc/lstm_stream.hip, csrc/plan.hip).

`CnnLstm.forward` classifies a WINDOW: to label every frame of a video from its last T frames a caller would materialise
stride-1 windows and pay the frozen ResNet-18 T times per frame.  The LSTM's input at a frame, [cnn(frame), mlp(pose)], does
not depend on the window, so here a frame goes through the backbone, the pose MLP and layer 0's input product once; the
T - 1 most recent products are carried from call to call and only the recurrence runs per window, for a tile of neighbouring
windows at a time.  It is the 2-D models' per-frame loop for the sequence model:

    stream = CnnLstmStream(model.eval(), streams=S)                     # window = model.sequence_length
    for frames, landmarks, detected in video:                           # chunks of any length n >= 1
        logits = stream.step(pre(frames), pose(landmarks, detected))    # [S,n,3,224,224], [S,n,47] -> [S,n,C]
        pred, confidence, stable, rows = timeline.update(logits.softmax(-1), smoothed=True)
        path, path_class = decoder.decode(rows)

The rule (include/qtcnn.h): frame g of a stream gets the model's eval() logits on the window of the min(T, g + 1) frames
ending at g -- the first T - 1 frames of a stream are classified from as many frames as have been seen.  Any split of a
stream into calls gives the bits of one call.  A step makes no host synchronisation.

Not built: training through the stream, image gradients, streams that advance by different n, strides other than 1, the
clip models (their temporal convolutions pad at window edges, so frames are not shareable), captured graphs of the live
step.  There is no torch fallback: CPU tensors raise QtError.
"""

import torch

from . import _lib
from ._abi import bind  # noqa: F401  (<module>.bind is _abi.bind)
from . import quadtree as _quadtree
from ._lib import QtError

TILE = 8                    # QT_LSTM_STREAM_TILE: consecutive windows of one stream a workgroup owns
MAX_WINDOW = 64
HIDDEN_SIZES = (256, 64)
IMAGE_HW = _quadtree.IMAGE_HW


class CnnLstmStream:
    """Per-frame logits of a CnnLstm over `streams` videos that advance together.  It runs on the model's own plan and
    weights; `window` defaults to model.sequence_length.  `seen` counts the frames of each stream so far; reset() starts
    new videos.  The carry holds products of layer 0's W_ih: when the model's weights change the stream starts over."""

    def __init__(self, model, streams=16, window=None):
        if not isinstance(model, _quadtree.CnnLstm):
            raise TypeError(f"CnnLstmStream needs a CnnLstm, got {type(model).__name__}: the 2-D models classify a frame "
                            "by itself (call the model), the clip models' frames are not shareable between windows")
        window = model.sequence_length if window is None else window
        if isinstance(window, bool) or not isinstance(window, int) or not 1 <= window <= MAX_WINDOW:
            raise ValueError(f"window must be an integer in 1 .. {MAX_WINDOW} (got {window!r})")
        if isinstance(streams, bool) or not isinstance(streams, int) or streams < 1:
            raise ValueError(f"streams must be a positive integer (got {streams!r})")
        self.model, self.streams, self.window = model, streams, window
        self.seen = 0
        self._carry = None       # [2][S][T-1][4H] f32: read [self._cur], written [1 - self._cur]
        self._cur = 0
        self._ws = None
        self._engine = None
        self._version = None

    def reset(self):
        """start new videos: the next frame is frame 0 of every stream"""
        self.seen = 0

    def _plan(self, frames, device):
        """the model's engine with room for `frames` frames, its weights bound and packed; starts over on new weights"""
        m = self.model
        if m._seq_len_bound is None:      # the plan is laid out for whole sequences; a stream does not care which length
            m._seq_len_bound = self.window
        if m._max_batch_hint and m._max_batch_hint % m._seq_len_bound:
            m._max_batch_hint = (m._max_batch_hint // m._seq_len_bound + 1) * m._seq_len_bound
        eng = m._ensure_engine(-(-frames // m._seq_len_bound) * m._seq_len_bound, device)
        version = m._bind(eng)
        same_engine = eng is self._engine
        if version != self._version or (same_engine and eng._weights_stale):
            self.seen = 0
        eng.pack_weights(version, False)
        self._engine, self._version = eng, version
        return eng

    def step(self, frames, poses):
        """frames [S,n,3,224,224] f32, poses [S,n,47] f32, both on the model's GPU -> logits [S,n,C] f32"""
        m, S, T = self.model, self.streams, self.window
        if m.training:
            raise QtError("CnnLstmStream.step: the model is in train(); a stream is eval arithmetic (call model.eval())")
        if not isinstance(frames, torch.Tensor) or not isinstance(poses, torch.Tensor):
            raise QtError("CnnLstmStream.step: frames and poses must be tensors")
        if frames.device.type != "cuda" or poses.device != frames.device:
            raise QtError("CnnLstmStream.step: frames and poses must be on the same AMD GPU (cuda:N); there is no CPU "
                          "fallback")
        if frames.dtype != torch.float32 or poses.dtype != torch.float32:
            raise QtError(f"CnnLstmStream.step: frames and poses must be float32 (got {frames.dtype}, {poses.dtype})")
        if frames.dim() != 5 or frames.shape[0] != S or frames.shape[1] < 1 or \
                tuple(frames.shape[2:]) != (3, IMAGE_HW, IMAGE_HW):
            raise ValueError(f"frames must be [{S},n,3,{IMAGE_HW},{IMAGE_HW}] with n >= 1, got {tuple(frames.shape)}")
        n = int(frames.shape[1])
        if tuple(poses.shape) != (S, n, m.numerical_feature_dim):
            raise ValueError(f"poses must be [{S},{n},{m.numerical_feature_dim}], got {tuple(poses.shape)}")
        m._check_hooks()
        device = frames.device
        H = m.lstm_hidden_size
        with torch.cuda.device(device):
            eng = self._plan(S * n, device)
            L = eng.L
            if T > 1 and (self._carry is None or self._carry.device != device):
                self._carry = torch.empty(2, S, T - 1, 4 * H, dtype=torch.float32, device=device)
                self.seen = 0
            need = L.qt_plan_stream_workspace_bytes(eng.handle, S, n, T)
            if self._ws is None or self._ws.device != device or self._ws.numel() < need:
                self._ws = torch.empty(max(need, 16), dtype=torch.uint8, device=device)
            images = frames.reshape(S * n, 3, IMAGE_HW, IMAGE_HW).contiguous()
            numerical = poses.reshape(S * n, m.numerical_feature_dim).contiguous()
            logits = torch.empty(S, n, m.num_classes, dtype=torch.float32, device=device)
            cin = self._carry[self._cur] if T > 1 else None
            cout = self._carry[1 - self._cur] if T > 1 else None
            _lib.check(L.qt_plan_stream_forward(eng.handle, eng.ws_ptr, eng._tensor_ptrs, _lib.ptr(images),
                                                _lib.ptr(numerical), _lib.ptr(logits), _lib.ptr(cin), _lib.ptr(cout),
                                                _lib.ptr(self._ws), self._ws.numel(), self.seen, S, n, T,
                                                _lib.stream_ptr()), "qt_plan_stream_forward")
            eng.fwd_counter += 1     # a backward() of an earlier forward finds its activations gone
            eng._handed_out = None
        self._cur = 1 - self._cur
        self.seen += n
        return logits
