"""Training augmentations on the device: ColorJitter, RandomRotation, GaussianBlur and Normalize in one HIP call
(csrc/augment.hip), the part of the reference's training transform that follows the resized crop:

    RandomResizedCrop(224, scale=(0.8, 1.0)) -> RandomHorizontalFlip(0.5)                      FramePreprocessor
      -> ColorJitter(0.2, 0.2, 0.2, 0.1) -> RandomRotation(10) -> GaussianBlur((5, 9), (0.1, 0.5)) -> Normalize   FrameAugmenter

The training pipeline: the loader hands over uint8 frames, boxes, flips and parameter rows, the device does the rest:

    pre, aug = FramePreprocessor(mean=0, std=1), FrameAugmenter()          # [0, 1] planes, then the reference's defaults
    unit = pre(frames.to(device, non_blocking=True), boxes.to(device, non_blocking=True), flips.to(device, non_blocking=True))
    images = aug(unit, aug.sample(len(frames)).to(device, non_blocking=True))   # f32 [B,3,224,224], normalised

The rule is torchvision's float-tensor path (include/qtcnn.h states it): the reference's loaders run the same ops on PIL
images, which round to uint8 after every step, so a result is about a grey level apart per stage.  Rotation is nearest
neighbour with fill 0, the blur border is reflected.  The parameter rows are drawn on the host by the rule of torchvision's
get_params (not its random stream) and are read on the device only: a malformed row makes that image NaN.  There is no
torch fallback: CPU tensors and other dtypes raise QtError.
"""
import ctypes
import math

import torch

from . import _lib
from ._abi import AugmentDesc, bind  # noqa: F401  (<module>.bind is _abi.bind)
from ._lib import QtError
from .preprocess import IMAGENET_MEAN, IMAGENET_STD, _one_batch_dim, _triple

PARAMS = 12          # QT_AUGMENT_PARAMS
MAX_BLUR = 15        # largest blur kernel per axis (csrc/augment.hip)
OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE = 0, 1, 2, 3


def _amount(v, what, limit=None):
    """a jitter amount: None or 0 disables the component"""
    v = 0.0 if v is None else float(v)
    if not math.isfinite(v) or v < 0.0 or (limit is not None and v > limit):
        raise ValueError(f"FrameAugmenter: {what} must be a finite number >= 0{'' if limit is None else f' and <= {limit}'} (got {v})")
    return v


class FrameAugmenter:
    """f32 [B,3,h,w] images or [B,T,3,h,w] clips in [0, 1] on the GPU -> the same shape, jittered, rotated, blurred, normalised."""

    def __init__(self, brightness=0.2, contrast=0.2, saturation=0.2, hue=0.1, degrees=10, blur_kernel=(5, 9),
                 blur_sigma=(0.1, 0.5), mean=IMAGENET_MEAN, std=IMAGENET_STD):
        self.brightness = _amount(brightness, "brightness")
        self.contrast = _amount(contrast, "contrast")
        self.saturation = _amount(saturation, "saturation")
        self.hue = _amount(hue, "hue", 0.5)
        self.degrees = _amount(degrees, "degrees")
        if blur_kernel is None or blur_kernel == 0:
            blur_kernel = (1, 1)
        if isinstance(blur_kernel, int):
            blur_kernel = (blur_kernel, blur_kernel)
        kx, ky = (int(k) for k in blur_kernel)      # torchvision's order: (along a row, along a column)
        if not all(1 <= k <= MAX_BLUR and k % 2 == 1 for k in (kx, ky)):
            raise ValueError(f"FrameAugmenter: blur_kernel sizes must be odd and at most {MAX_BLUR} (got {blur_kernel!r})")
        self.blur_kernel = (kx, ky)
        if blur_sigma is None:
            blur_sigma = (1.0, 1.0)
        if isinstance(blur_sigma, (int, float)):
            blur_sigma = (float(blur_sigma), float(blur_sigma))
        lo, hi = (float(s) for s in blur_sigma)
        if not (0.0 < lo <= hi and math.isfinite(hi)):
            raise ValueError(f"FrameAugmenter: blur_sigma must be a positive increasing pair (got {blur_sigma!r})")
        self.blur_sigma = (lo, hi)
        self.mean = _triple(mean, "mean")
        std = _triple(std, "std")
        if any(s == 0.0 for s in std):
            raise ValueError("FrameAugmenter: std must not be zero")
        self.inv_std = tuple(1.0 / s for s in std)
        self._workspace = {}      # device -> f32 partial sums of the contrast mean

    @property
    def enabled_ops(self):
        amounts = (self.brightness, self.contrast, self.saturation, self.hue)
        return [op for op, a in enumerate(amounts) if a > 0.0]

    def sample(self, n, generator=None):
        """n parameter rows, CPU f32 [n, 12], by the rule of torchvision's get_params: brightness / contrast / saturation
        factors uniform in [max(0, 1 - x), 1 + x], the hue shift uniform in [-x, x], a random permutation of the enabled ops,
        the angle uniform in [-degrees, degrees], one sigma per image uniform in blur_sigma.  (The rule, not torchvision's
        random stream.)  A disabled component gives skip slots, (cos, sin) = (1, 0), sigma 1."""
        if n < 1:
            raise ValueError(f"FrameAugmenter.sample: needs n >= 1 (got {n})")
        u = torch.rand(n, 6, generator=generator, dtype=torch.float64)
        keys = torch.rand(n, 4, generator=generator, dtype=torch.float64)
        rows = torch.zeros(n, PARAMS, dtype=torch.float64)
        for op, x in ((OP_BRIGHTNESS, self.brightness), (OP_CONTRAST, self.contrast), (OP_SATURATION, self.saturation)):
            lo = max(0.0, 1.0 - x)
            rows[:, op] = lo + (1.0 + x - lo) * u[:, op]
        rows[:, OP_HUE] = -self.hue + 2.0 * self.hue * u[:, OP_HUE]
        # a uniform permutation of the four ids; the disabled ones drop out and the rest keeps its (uniform) order
        perm = torch.argsort(keys, dim=1)
        on = torch.zeros(4, dtype=torch.bool)
        on[self.enabled_ops] = True
        keep = on[perm]
        dest = torch.cumsum(keep.long(), dim=1) - 1
        slots = torch.full((n, 4), -1.0, dtype=torch.float64)
        r, c = torch.nonzero(keep, as_tuple=True)
        slots[r, dest[r, c]] = perm[r, c].double()
        rows[:, 4:8] = slots
        angle = (-self.degrees + 2.0 * self.degrees * u[:, 4]) * (math.pi / 180.0)
        rows[:, 8] = torch.cos(angle)
        rows[:, 9] = torch.sin(angle)
        if self.degrees == 0.0:
            rows[:, 8], rows[:, 9] = 1.0, 0.0
        lo, hi = self.blur_sigma
        rows[:, 10] = lo + (hi - lo) * u[:, 5] if self.blur_kernel != (1, 1) else 1.0
        return rows.to(torch.float32).contiguous()

    def __call__(self, images, params, out=None):
        """params: f32 [B(,T),12] rows on the images' device (sample()); out: an f32 tensor of the images' shape to write
        (dense planes, one stride between images) that shares no storage with `images`."""
        if not isinstance(images, torch.Tensor):
            raise QtError("FrameAugmenter: images must be a tensor")
        if images.device.type != "cuda":
            raise QtError(f"FrameAugmenter: images must be on an AMD GPU (got {images.device}); there is no CPU or torch "
                          "fallback")
        if images.dtype != torch.float32:
            raise QtError(f"FrameAugmenter: f32 images only (got {images.dtype})")
        if images.dim() not in (4, 5) or images.shape[-3] != 3 or min(images.shape) < 1:
            raise QtError(f"FrameAugmenter: images must be [B,3,h,w] or [B,T,3,h,w], no empty dimension (got "
                          f"{list(images.shape)})")
        lead = tuple(images.shape[:-3])
        h, w = int(images.shape[-2]), int(images.shape[-1])
        dev = images.device
        n = math.prod(lead)
        if not isinstance(params, torch.Tensor) or params.device != dev or params.dtype != torch.float32 or \
                tuple(params.shape) != lead + (PARAMS,):
            raise QtError(f"FrameAugmenter: params must be an f32 {list(lead + (PARAMS,))} tensor on {dev}")
        params = params.contiguous()
        kx, ky = self.blur_kernel
        if w <= kx // 2 or h <= ky // 2:
            raise QtError(f"FrameAugmenter: a {kx} x {ky} blur reflects further than a {h} x {w} image reaches")
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.float32 or \
                    tuple(out.shape) != tuple(images.shape):
                raise QtError(f"FrameAugmenter: out must be an f32 {list(images.shape)} tensor on {dev}")
            if out.untyped_storage().data_ptr() == images.untyped_storage().data_ptr():
                raise QtError("FrameAugmenter: out shares storage with images (rotation and blur gather: not in place)")
            o = out if len(lead) == 1 else _one_batch_dim(out)
            if o is None or o.stride()[1:] != (h * w, w, 1) or (n > 1 and o.stride(0) < 3 * h * w):
                raise QtError("FrameAugmenter: out must have dense [3,h,w] images one stride apart")
        # dense [3,h,w] images one stride apart go through as they are; everything else is copied once
        f = images if len(lead) == 1 else _one_batch_dim(images)
        if f is None or f.stride()[1:] != (h * w, w, 1) or (n > 1 and f.stride(0) < 3 * h * w):
            f = images.contiguous().view(n, 3, h, w)
        src_stride = f.stride(0) if n > 1 else 3 * h * w
        use_contrast = int(self.contrast > 0.0)
        L = _lib.lib()
        with torch.cuda.device(dev):
            ws, ws_bytes = None, 0
            if use_contrast:
                ws_bytes = L.qt_augment_workspace_bytes(n, 1)
                ws = self._workspace.get(dev)
                if ws is None or ws.numel() * 4 < ws_bytes:
                    ws = self._workspace[dev] = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev)
            if out is None:
                out = torch.empty(tuple(images.shape), dtype=torch.float32, device=dev)
                dst_stride = 3 * h * w
            else:
                dst_stride = o.stride(0) if n > 1 else 3 * h * w
            desc = AugmentDesc(n, h, w, src_stride, dst_stride, kx, ky, (ctypes.c_float * 3)(*self.mean),
                               (ctypes.c_float * 3)(*self.inv_std), use_contrast)
            _lib.check(L.qt_augment_f32(ctypes.byref(desc), f.data_ptr(), params.data_ptr(), out.data_ptr(), _lib.ptr(ws),
                                        ws_bytes, _lib.stream_ptr()), "qt_augment_f32")
        return out
