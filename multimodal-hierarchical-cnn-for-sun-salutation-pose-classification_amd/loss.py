"""Loss head on the device: CrossEntropyLoss, FocalLoss and the epoch meter (csrc/loss.hip).

The reference's trainers compute `nn.CrossEntropyLoss()(outputs, labels)` and then read the device twice per step
(`loss.item()`, `(predicted == labels).sum().item()`: 3dcnn/train_3D_Quadtree_cnn_model.py:127-137).  Here the loss is one
launch forward and one backward, the argmax / correct count come out of the forward launch, and the running sums live in
device memory until the epoch ends:

    criterion = CrossEntropyLoss()                   # was nn.CrossEntropyLoss()
    meter = LossMeter(device)
    for images, features, labels in loader:
        loss = criterion(model(images, features), labels, meter=meter)
        loss.backward(); optimizer.step()
    stats = meter.result()                           # the one host sync: mean loss, accuracy, samples, skipped steps

`CrossEntropyLoss` follows torch.nn.functional.cross_entropy for class-index targets (weight, ignore_index, reduction,
label_smoothing); `FocalLoss` takes the constructor arguments of the reference class (3dcnn/models.py:8-47) and computes
what it computes.  Logits are f32 [rows, C] (any row stride, C <= 1024), labels int64 [rows].  There is no torch fallback:
CPU tensors, other dtypes and double backward raise QtError.  A label outside [0, C) that is not `ignore_index` makes the
loss NaN (the device is the only one that sees it; nothing is indexed with it).
"""
import ctypes

import torch

from . import _lib
from ._abi import LossDesc, bind  # noqa: F401  (<module>.bind is _abi.bind)
from ._lib import QtError

QT_LOSS_CROSS_ENTROPY, QT_LOSS_FOCAL = 0, 1
_REDUCTIONS = {"mean": 0, "sum": 1, "none": 2}
MAX_CLASSES = 1024


class LossMeter:
    """Epoch bookkeeping in device memory: {loss_sum, samples, correct, skipped_steps} as four doubles that the loss
    kernel updates by the trainers' rule (a step whose loss is not finite only counts as skipped).  `result()` is the one
    host sync."""

    def __init__(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise QtError("LossMeter lives on an AMD GPU (device must be cuda:N); no CPU fallback")
        self.state = torch.zeros(4, dtype=torch.float64, device=device)

    def reset(self):
        self.state.zero_()

    def result(self):
        loss_sum, samples, correct, skipped = self.state.tolist()
        n = max(samples, 1.0)
        return {"loss": loss_sum / n, "accuracy": correct / n, "samples": int(samples), "skipped_steps": int(skipped)}


def _check_inputs(logits, labels, what):
    if not isinstance(logits, torch.Tensor) or not isinstance(labels, torch.Tensor):
        raise QtError(f"{what}: logits and labels must be tensors")
    if logits.device.type != "cuda" or labels.device != logits.device:
        raise QtError(f"{what}: logits and labels must be on one AMD GPU (got {logits.device} / {labels.device}); "
                      "there is no CPU or torch fallback")
    if logits.dtype != torch.float32:
        raise QtError(f"{what}: f32 logits only (got {logits.dtype})")
    if labels.dtype != torch.int64:
        raise QtError(f"{what}: int64 labels only (got {labels.dtype})")
    if logits.dim() != 2 or labels.dim() != 1 or labels.shape[0] != logits.shape[0] or logits.shape[0] < 1:
        raise QtError(f"{what}: needs logits [rows, C] and labels [rows] with rows >= 1 (got {tuple(logits.shape)} / "
                      f"{tuple(labels.shape)})")
    if not 1 <= logits.shape[1] <= MAX_CLASSES:
        raise QtError(f"{what}: C = {logits.shape[1]} classes; 1 .. {MAX_CLASSES} are handled")


def _row_major(t):
    """the tensor itself when its rows are contiguous (any row stride >= C), else a contiguous copy"""
    if t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
        return t
    if t.shape[1] == 1 and t.stride(0) >= 1:
        return t
    return t.contiguous()


class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, weight, cfg, meter, predictions):
        kind, reduction, ignore_index, smoothing, gamma = cfg
        z = _row_major(logits.detach())
        y = labels.contiguous()
        rows, C = z.shape
        dev = z.device
        L = _lib.lib()
        desc = LossDesc(_lib.QT_F32, kind, reduction, ignore_index, smoothing, gamma, _lib.ptr(weight))
        keep = ctx.needs_input_grad[0]
        with torch.cuda.device(dev):
            loss = torch.empty(rows if reduction == 2 else (), dtype=torch.float32, device=dev)
            row_state = torch.empty(rows, 2, dtype=torch.float32, device=dev) if keep else None
            stats = torch.empty(3, dtype=torch.float64, device=dev)
            need = L.qt_loss_workspace_bytes(rows, C)
            ws = torch.empty(need // 8, dtype=torch.float64, device=dev) if need else None
            _lib.check(L.qt_loss_forward(ctypes.byref(desc), z.data_ptr(), z.stride(0), y.data_ptr(), rows, C, loss.data_ptr(),
                                         _lib.ptr(row_state), stats.data_ptr(), _lib.ptr(predictions),
                                         _lib.ptr(meter), _lib.ptr(ws), need, _lib.stream_ptr()), "qt_loss_forward")
        if keep:
            ctx.save_for_backward(z, y, row_state, stats, weight)
            ctx.cfg = cfg
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)   # no zeros launch for the gradient of `stats`
        return loss, stats

    @staticmethod
    def backward(ctx, grad_loss, _grad_stats):
        if torch.is_grad_enabled():   # backward(create_graph=True) / autograd.grad of a gradient
            raise QtError("the fused loss has no double backward (and no torch fallback for one)")
        if grad_loss is None:
            return None, None, None, None, None, None
        z, y, row_state, stats, weight = ctx.saved_tensors
        kind, reduction, ignore_index, smoothing, gamma = ctx.cfg
        rows, C = z.shape
        if grad_loss.device != z.device:
            raise QtError("loss backward: the upstream gradient must be on the logits' device")
        g = grad_loss.to(torch.float32).contiguous()
        L = _lib.lib()
        desc = LossDesc(_lib.QT_F32, kind, reduction, ignore_index, smoothing, gamma, _lib.ptr(weight))
        with torch.cuda.device(z.device):
            dz = torch.empty(rows, C, dtype=torch.float32, device=z.device)
            _lib.check(L.qt_loss_backward(ctypes.byref(desc), z.data_ptr(), z.stride(0), y.data_ptr(), rows, C,
                                          row_state.data_ptr(), stats.data_ptr(), g.data_ptr(), dz.data_ptr(), C,
                                          _lib.stream_ptr()), "qt_loss_backward")
        return dz, None, None, None, None, None


class _FusedLoss(torch.nn.Module):
    _kind = QT_LOSS_CROSS_ENTROPY

    def _cfg(self):
        raise NotImplementedError

    def _class_vector(self):
        raise NotImplementedError

    def forward(self, logits, labels, meter=None, predictions=None):
        """The loss (0-dim, or [rows] for reduction='none').  meter: a LossMeter to update in the same launch.
        predictions: an int64 [rows] tensor on the logits' device that receives torch.max(logits, 1)'s indices."""
        what = type(self).__name__
        _check_inputs(logits, labels, what)
        rows, C = logits.shape
        w = self._class_vector()
        if w is not None:
            if w.device != logits.device or w.dtype != torch.float32 or w.numel() != C:
                raise QtError(f"{what}: the per-class vector must be f32 [{C}] on {logits.device} (got {w.dtype} "
                              f"[{w.numel()}] on {w.device}); move the module with .to(device)")
            w = w.contiguous()
        state = None
        if meter is not None:
            if not isinstance(meter, LossMeter) or meter.state.device != logits.device:
                raise QtError(f"{what}: meter must be a LossMeter on the logits' device")
            state = meter.state
        if predictions is not None:
            if predictions.dtype != torch.int64 or predictions.device != logits.device or \
                    tuple(predictions.shape) != (rows,) or not predictions.is_contiguous():
                raise QtError(f"{what}: predictions must be a contiguous int64 [{rows}] tensor on the logits' device")
        loss, stats = _LossFn.apply(logits, labels, w, self._cfg(), state, predictions)
        self.last_stats = stats   # device doubles {sum of row losses, denominator, correct}
        return loss


class CrossEntropyLoss(_FusedLoss):
    """torch.nn.CrossEntropyLoss for class-index targets, one HIP launch per direction."""

    def __init__(self, weight=None, ignore_index=-100, reduction="mean", label_smoothing=0.0):
        super().__init__()
        if reduction not in _REDUCTIONS:
            raise ValueError(f"CrossEntropyLoss: reduction must be one of {sorted(_REDUCTIONS)} (got {reduction!r})")
        if not 0.0 <= float(label_smoothing) <= 1.0:
            raise ValueError(f"CrossEntropyLoss: label_smoothing must be in [0, 1] (got {label_smoothing})")
        if weight is not None:
            weight = torch.as_tensor(weight, dtype=torch.float32).detach().clone()
            if weight.dim() != 1:
                raise ValueError("CrossEntropyLoss: weight must be a vector with one entry per class")
        self.register_buffer("weight", weight)
        self.ignore_index = int(ignore_index)
        self.reduction = reduction
        self.label_smoothing = float(label_smoothing)
        self.last_stats = None

    def _cfg(self):
        return (QT_LOSS_CROSS_ENTROPY, _REDUCTIONS[self.reduction], self.ignore_index, self.label_smoothing, 0.0)

    def _class_vector(self):
        return self.weight


class FocalLoss(_FusedLoss):
    """The reference's FocalLoss (3dcnn/models.py:8-47), loss_i = -alpha[y_i] (1 - p_y)^gamma log p_y, on the device.

    Supported, as in the reference: `alpha` a list with one weight per class (len == num_classes), or a number with
    num_classes == 2 (alpha for class 0, 1 - alpha for class 1).  The reference class fails in forward() with an unbound
    `alpha_t` for every other combination; this one raises ValueError here.  gamma is 0 or >= 1 (in between the derivative
    at p = 1 is infinite).  With reduction='none' the result is always [rows] (the reference squeezes a one-row batch to
    0-dim)."""

    def __init__(self, alpha=0.25, gamma=2.0, reduction="mean", num_classes=None):
        super().__init__()
        if reduction not in _REDUCTIONS:
            raise ValueError(f"FocalLoss: reduction must be one of {sorted(_REDUCTIONS)} (got {reduction!r})")
        gamma = float(gamma)
        if not (gamma == 0.0 or (1.0 <= gamma < float("inf"))):
            raise ValueError(f"FocalLoss: gamma must be 0 or a finite number >= 1 (got {gamma})")
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float, list)):
            raise ValueError("FocalLoss: alpha must be a number or a list of per-class weights")
        if isinstance(alpha, (int, float)):
            if num_classes != 2:
                raise ValueError("FocalLoss: a scalar alpha means [alpha, 1 - alpha] and needs num_classes == 2; the "
                                 "reference leaves alpha_t unbound for any other class count")
            vec = torch.tensor([float(alpha), 1.0 - float(alpha)], dtype=torch.float32)
        else:
            vec = torch.tensor(alpha, dtype=torch.float32)
            if vec.dim() != 1 or num_classes is None or vec.numel() != int(num_classes):
                raise ValueError("FocalLoss: alpha must hold one weight per class (len == num_classes); the reference "
                                 "leaves alpha_t unbound otherwise")
        self.register_buffer("alpha", vec)
        self.gamma = gamma
        self.reduction = reduction
        self.num_classes = int(num_classes)
        self.last_stats = None

    def _cfg(self):
        return (QT_LOSS_FOCAL, _REDUCTIONS[self.reduction], -100, 0.0, self.gamma)

    def _class_vector(self):
        return self.alpha
