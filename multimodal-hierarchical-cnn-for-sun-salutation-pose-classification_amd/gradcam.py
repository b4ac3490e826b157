"""Grad-CAM on the device: class maps for a whole batch and uint8 overlays, two HIP kernels (csrc/gradcam.hip) behind the
recipe of the reference's scripts (resnet/grad_cam_analysis.py:237-343, grad_cam/5_grad_cam_visualizer.py:220-275,
Quadtree_from scratch/grad_cam.py:70-96):

    explainer = GradCAM(model)                                   # alpha 0.4, jet colours, cv2's channel order
    overlays, target, logits = explainer.explain(frames_u8.to(device), numerical.to(device))   # uint8 [B,H,W,3]

or step by step

    cam, target, logits = explainer.maps(images, numerical)      # f32 [B,7,7] ([B,t,h,w] for Quadtree3DCNN), int64 [B]
    overlays = explainer.overlay(frames_u8, cam)

The reference explains one image per call, pulls two [1,512,7,7] tensors to the host, loops over the channels in Python and
draws with cv2 on a CPU core.  Here the target class is the device's argmax, the map is one call on the two hook tensors
(w_c = mean_p grad, s_p = sum_c w_c act, ReLU, divided by its maximum; an all-zero map stays zero), and the overlay is one
launch (bilinear sample with half-pixel centres and clamped taps, idx = int(255 v), uint8(alpha lut[idx] + (1 - alpha)
frame)); include/qtcnn.h states both rules.  Nothing in `maps` or `overlay` reads the host.

Served: QuadtreeCNN (modes fusion and image_only, frozen or trainable backbone) and StandardResNetCNN through
`base_cnn.layer4`, Quadtree3DCNN through `conv3d_final_features`.  A numerical_only model has no image branch (ValueError;
the reference returns None); models without a served hook point raise TypeError, as the reference does.

The colour table is the usual piecewise-linear jet, written out in jet_lut below.  It is not taken from OpenCV's
COLORMAP_JET table and has not been compared with it (OpenCV is not a dependency here); pass `lut=` to use another table.
Not built: a one-hot backward that skips the weight gradients (the model's ordinary backward runs), temporal upsampling of
a clip's [t,h,w] map, other colour maps as built-ins, guided Grad-CAM.  There is no torch fallback.
"""

import torch

from . import _lib
from ._abi import bind  # noqa: F401  (<module>.bind is _abi.bind)
from ._lib import QtError
from .preprocess import FramePreprocessor
from .quadtree import QuadtreeCNN, StandardResNetCNN
from .video3d import Quadtree3DCNN

MAX_POSITIONS = 4096   # QT_GRADCAM_MAX_POSITIONS


def jet_lut(order="bgr"):
    """The jet colour table, CPU uint8 [256, 3] in the given channel order: for x = i / 255,
    red = clamp(1.5 - |4x - 3|), green = clamp(1.5 - |4x - 2|), blue = clamp(1.5 - |4x - 1|), clamp to [0, 1], times 255 and
    rounded to nearest.  Entry 0 is dark blue (0, 0, 128 as r, g, b), entry 255 dark red (128, 0, 0).  Written out here, not
    read from OpenCV's COLORMAP_JET, which it resembles but has not been compared with."""
    if order not in ("rgb", "bgr"):
        raise ValueError(f"jet_lut: order must be 'rgb' or 'bgr' (got {order!r})")
    x = torch.arange(256, dtype=torch.float64) / 255.0
    rgb = [(1.5 - (4.0 * x - c).abs()).clamp(0.0, 1.0) for c in (3.0, 2.0, 1.0)]
    if order == "bgr":
        rgb.reverse()
    return torch.floor(torch.stack(rgb, dim=1) * 255.0 + 0.5).to(torch.uint8).contiguous()


def _check_alpha(alpha):
    try:
        a = float(alpha)
    except (TypeError, ValueError):
        raise ValueError(f"GradCAM: alpha must be a number in [0, 1] (got {alpha!r})") from None
    if not 0.0 <= a <= 1.0:   # false for a NaN as well
        raise ValueError(f"GradCAM: alpha must be in [0, 1] (got {alpha!r})")
    return a


def _device_tensor(t, name, dtype, dev=None):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"GradCAM: {name} must be a tensor")
    if t.dtype != dtype:
        raise ValueError(f"GradCAM: {name} must be {dtype} (got {t.dtype})")
    if t.device.type != "cuda" or (dev is not None and t.device != dev):
        raise ValueError(f"GradCAM: {name} must be on {'an AMD GPU' if dev is None else dev} (got {t.device}); there is no "
                         "CPU or torch fallback")
    return t


def gradcam_map(act, grad):
    """qt_gradcam_map on two f32 [B,C,...] device tensors of one shape: (cam f32 [B,...], peak f32 [B])"""
    act = _device_tensor(act, "activations", torch.float32)
    grad = _device_tensor(grad, "gradients", torch.float32, act.device)
    if act.dim() < 3 or act.shape != grad.shape or min(act.shape) < 1:
        raise ValueError(f"GradCAM: activations and gradients must share one shape [B,C,...], no empty dimension (got "
                         f"{list(act.shape)} and {list(grad.shape)})")
    B, C = int(act.shape[0]), int(act.shape[1])
    P = act[0, 0].numel()
    act, grad = act.contiguous(), grad.contiguous()
    L = _lib.lib()
    with torch.cuda.device(act.device):
        cam = torch.empty((B,) + tuple(act.shape[2:]), dtype=torch.float32, device=act.device)
        peak = torch.empty(B, dtype=torch.float32, device=act.device)
        ws_bytes = L.qt_gradcam_workspace_bytes(B, C, min(P, MAX_POSITIONS))
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=act.device) if ws_bytes else None
        _lib.check(L.qt_gradcam_map(act.data_ptr(), grad.data_ptr(), B, C, P, cam.data_ptr(), peak.data_ptr(), _lib.ptr(ws),
                                    ws_bytes, _lib.stream_ptr()), "qt_gradcam_map")
    return cam, peak


class GradCAM:
    """Grad-CAM of `model` for whole batches; see the module text.  alpha: weight of the colour in the overlay, in [0, 1];
    lut: uint8 [256,3] colour table in the frames' channel order (default: jet_lut(channel_order)); channel_order: of the
    uint8 frames, 'bgr' (cv2's, the reference's) or 'rgb'."""

    def __init__(self, model, alpha=0.4, lut=None, channel_order="bgr"):
        if isinstance(model, QuadtreeCNN):
            if model.mode == "numerical_only":
                raise ValueError("GradCAM: a numerical_only model has no image branch to explain")
            self._hooked = model.base_cnn.layer4
        elif isinstance(model, StandardResNetCNN):
            self._hooked = model.base_cnn.layer4
        elif isinstance(model, Quadtree3DCNN):
            self._hooked = model.conv3d_final_features
        else:
            raise TypeError(f"GradCAM: unsupported model type {type(model).__name__}; served are QuadtreeCNN and "
                            "StandardResNetCNN (base_cnn.layer4) and Quadtree3DCNN (conv3d_final_features)")
        if channel_order not in ("rgb", "bgr"):
            raise ValueError(f"GradCAM: channel_order must be 'rgb' or 'bgr' (got {channel_order!r})")
        self.model = model
        self.alpha = _check_alpha(alpha)
        self.channel_order = channel_order
        if lut is None:
            lut = jet_lut(channel_order)
        if not isinstance(lut, torch.Tensor) or lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3):
            raise ValueError("GradCAM: lut must be a uint8 [256, 3] tensor")
        self.lut = lut.detach().contiguous()
        self._lut_on = {}          # device -> the table there
        self._preprocessor = None  # explain()'s default, built at first use

    def _lut(self, dev):
        t = self._lut_on.get(dev)
        if t is None:
            t = self._lut_on[dev] = self.lut.to(dev)
        return t

    def maps(self, image, numerical=None, target_class=None):
        """image: the model's image input on the GPU (f32 [B,3,224,224]; [B,T,3,h,w] for Quadtree3DCNN); numerical: its second
        input (None where the model does not read one); target_class: None (the arg-max of the logits, taken on the device), an
        int, or an int64 [B] tensor on the image's device, which is clamped to the class range there (the host cannot see it).
        Returns (cam f32 [B,h,w] or [B,t,h,w], target int64 [B], logits [B,classes] detached).  The model is left as it was:
        training flag, hooks, and every parameter's .grad (the same objects, the same values)."""
        image = _device_tensor(image, "image", torch.float32)
        dev = image.device
        if numerical is not None:
            numerical = _device_tensor(numerical, "numerical", torch.float32, dev)
        if isinstance(target_class, torch.Tensor):
            target_class = _device_tensor(target_class, "target_class", torch.int64, dev)
            if target_class.dim() != 1 or target_class.shape[0] != image.shape[0]:
                raise ValueError(f"GradCAM: target_class must have shape [{image.shape[0]}] (got {list(target_class.shape)})")
        elif target_class is not None:
            if isinstance(target_class, bool) or not isinstance(target_class, int):
                raise ValueError(f"GradCAM: target_class must be None, an int or an int64 tensor (got {target_class!r})")
            if not 0 <= target_class < self.model.num_classes:
                raise ValueError(f"GradCAM: target_class {target_class} is outside the model's {self.model.num_classes} classes")
        model = self.model
        taken = {}
        was_training = model.training
        params = list(model.parameters())
        kept = [p.grad for p in params]
        handles = [self._hooked.register_forward_hook(lambda m, i, o: taken.__setitem__("act", o)),
                   self._hooked.register_full_backward_hook(lambda m, gi, go: taken.__setitem__("grad", go[0]))]
        try:
            model.eval()
            for p in params:
                p.grad = None
            with torch.enable_grad():
                # A frozen StandardResNetCNN has no trainable parameter below its classifier, and its plan forms
                # d(loss)/d(pooled features), which the served backward hook reads, only on the way to the image: the
                # reference's recipe asks for the image gradient too (grad_cam_analysis.py:247), so does this call.
                x = image.detach()
                if isinstance(model, StandardResNetCNN):
                    x = x.requires_grad_(True)
                logits = model(x, numerical)
                classes = int(logits.shape[1])
                if target_class is None:
                    target = logits.detach().argmax(1)
                elif isinstance(target_class, int):
                    target = torch.full((logits.shape[0],), target_class, dtype=torch.int64, device=dev)
                else:
                    target = target_class.clamp(0, classes - 1)
                one_hot = torch.zeros_like(logits).scatter_(1, target.view(-1, 1), 1.0)
                logits.backward(gradient=one_hot)
        finally:
            for h in handles:
                h.remove()
            for p, g in zip(params, kept):
                p.grad = g
            model.train(was_training)
        if "act" not in taken or "grad" not in taken:
            raise QtError("GradCAM: the model did not serve its Grad-CAM hooks")
        cam, _ = gradcam_map(taken["act"].detach(), taken["grad"].detach())
        return cam, target, logits.detach()

    def overlay(self, frames_u8, cam, alpha=None, heat=None, index=None):
        """frames_u8: uint8 [B,H,W,3] on the GPU; cam: f32 [B,h,w] on the same device (a [B,t,h,w] map goes frame-wise, as
        [B*t,h,w] with the frames the caller picks: there is no temporal upsampling).  Returns uint8 [B,H,W,3].  heat (f32
        [B,H,W]) and index (uint8 [B,H,W]), when given, receive the sampled map and the colour index."""
        a = self.alpha if alpha is None else _check_alpha(alpha)
        frames_u8 = _device_tensor(frames_u8, "frames", torch.uint8)
        dev = frames_u8.device
        cam = _device_tensor(cam, "cam", torch.float32, dev)
        if frames_u8.dim() != 4 or frames_u8.shape[-1] != 3 or min(frames_u8.shape) < 1:
            raise ValueError(f"GradCAM: frames must be [B,H,W,3], no empty dimension (got {list(frames_u8.shape)})")
        B, H, W = (int(v) for v in frames_u8.shape[:3])
        if cam.dim() != 3 or cam.shape[0] != B or min(cam.shape) < 1:
            raise ValueError(f"GradCAM: cam must be [{B},h,w] (got {list(cam.shape)})")
        for t, name, dt in ((heat, "heat", torch.float32), (index, "index", torch.uint8)):
            if t is not None:
                _device_tensor(t, name, dt, dev)
                if tuple(t.shape) != (B, H, W) or not t.is_contiguous():
                    raise ValueError(f"GradCAM: {name} must be a contiguous [{B},{H},{W}] tensor")
        frames_u8, cam = frames_u8.contiguous(), cam.contiguous()
        L = _lib.lib()
        with torch.cuda.device(dev):
            out = torch.empty_like(frames_u8)
            _lib.check(L.qt_gradcam_overlay_u8(cam.data_ptr(), int(cam.shape[1]), int(cam.shape[2]), frames_u8.data_ptr(), B, H, W,
                                               self._lut(dev).data_ptr(), a, out.data_ptr(), _lib.ptr(heat), _lib.ptr(index),
                                               _lib.stream_ptr()), "qt_gradcam_overlay_u8")
        return out

    def explain(self, frames_u8, numerical=None, target_class=None, preprocessor=None):
        """frames_u8: uint8 [B,H,W,3] on the GPU ([B,T,H,W,3] clips for Quadtree3DCNN) -> (overlays, target, logits): the
        frames through `preprocessor` (default: FramePreprocessor() for this explainer's channel order), maps, overlay.
        Overlays are uint8 [B,H,W,3].  For clips they are [B,t,H,W,3]: slice j of the [t,h,w] map drawn over the centre frame
        of the T / t frames it covers, frame (2 j + 1) T // (2 t)."""
        pre = preprocessor
        if pre is None:
            if self._preprocessor is None:
                self._preprocessor = FramePreprocessor(channel_order=self.channel_order)
            pre = self._preprocessor
        frames_u8 = _device_tensor(frames_u8, "frames", torch.uint8)
        clips = isinstance(self.model, Quadtree3DCNN)
        if frames_u8.dim() != (5 if clips else 4):
            raise ValueError(f"GradCAM: frames must be {'[B,T,H,W,3]' if clips else '[B,H,W,3]'} for this model (got "
                             f"{list(frames_u8.shape)})")
        cam, target, logits = self.maps(pre(frames_u8), numerical, target_class)
        if not clips:
            return self.overlay(frames_u8, cam), target, logits
        B, T, H, W = (int(v) for v in frames_u8.shape[:4])
        t = int(cam.shape[1])
        centre = [(2 * j + 1) * T // (2 * t) for j in range(t)]
        picked = torch.stack([frames_u8[:, c] for c in centre], dim=1).view(B * t, H, W, 3)
        out = self.overlay(picked, cam.reshape(B * t, int(cam.shape[2]), int(cam.shape[3])))
        return out.view(B, t, H, W, 3), target, logits
