"""Frame preprocessing on the device: crop, flip, antialiased bilinear resize, /255 and mean/std in one HIP launch
(csrc/preprocess.hip).

The reference's loaders run `Resize -> ToTensor -> Normalize` per image on a CPU core and send f32 [B,3,224,224] over the
host link; the training loaders put `RandomResizedCrop(scale=(0.8, 1.0))` and `RandomHorizontalFlip` in front.  Here the
loader hands over the decoded uint8 frames (a quarter of the bytes), the boxes and the flips, and the device does the rest:

    pre = FramePreprocessor()                                   # 224 x 224, ImageNet mean / std
    boxes = random_resized_crop_boxes(len(frames), frames.shape[1:3]).to(device, non_blocking=True)
    flips = random_flips(len(frames)).to(device, non_blocking=True)
    images = pre(frames.to(device, non_blocking=True), boxes, flips)   # f32 [B,3,224,224], what every model here takes

The resize is torch's `interpolate(mode='bilinear', antialias=True)` of the crop, which is PIL's BILINEAR resize without
its uint8 rounding between the two passes (at most one grey level apart).  Decoding, file I/O and the photometric
augmentations stay with the loader.  There is no torch fallback: CPU tensors and other dtypes raise QtError.  A box that is
not inside its frame makes that image's output NaN (only the device sees it; nothing outside the frame is read).
"""
import ctypes
import math

import torch

from . import _lib
from ._abi import PreprocessDesc, bind  # noqa: F401  (<module>.bind is _abi.bind)
from ._lib import QtError

MAX_DOWNSCALE = 24   # per axis, frame size / output size (csrc/preprocess.hip)
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def _triple(v, what):
    try:
        t = tuple(float(x) for x in v)
    except TypeError:
        t = (float(v),) * 3
    if len(t) != 3 or not all(math.isfinite(x) for x in t):
        raise ValueError(f"FramePreprocessor: {what} must be three finite numbers (got {v!r})")
    return t


class FramePreprocessor:
    """uint8 frames [B,H,W,3] or clips [B,T,H,W,3] on the GPU -> f32 [B,3,h,w] / [B,T,3,h,w], normalised."""

    def __init__(self, size=(224, 224), mean=IMAGENET_MEAN, std=IMAGENET_STD, channel_order="rgb"):
        if isinstance(size, int):
            size = (size, size)
        if len(size) != 2 or int(size[0]) < 1 or int(size[1]) < 1:
            raise ValueError(f"FramePreprocessor: size must be (height, width) >= 1 (got {size!r})")
        if channel_order not in ("rgb", "bgr"):
            raise ValueError(f"FramePreprocessor: channel_order must be 'rgb' or 'bgr' (got {channel_order!r})")
        self.size = (int(size[0]), int(size[1]))
        self.mean = _triple(mean, "mean")
        std = _triple(std, "std")
        if any(s == 0.0 for s in std):
            raise ValueError("FramePreprocessor: std must not be zero")
        self.inv_std = tuple(1.0 / s for s in std)
        self.channel_order = channel_order

    def _side(self, t, name, lead, dev, dtypes, tail):
        if not isinstance(t, torch.Tensor):
            raise QtError(f"FramePreprocessor: {name} must be a tensor")
        if t.device != dev:
            raise QtError(f"FramePreprocessor: {name} must be on the frames' device {dev} (got {t.device})")
        if t.dtype not in dtypes:
            raise QtError(f"FramePreprocessor: {name} must be {' or '.join(str(d) for d in dtypes)} (got {t.dtype})")
        if tuple(t.shape) != lead + tail:
            raise QtError(f"FramePreprocessor: {name} must have shape {list(lead + tail)} (got {list(t.shape)})")
        return t.contiguous()

    def __call__(self, frames, boxes=None, flips=None, out=None):
        """boxes: int32 [B(,T),4] = top, left, height, width on the frames' device (None: whole frames); flips: uint8 or
        bool [B(,T)] (None: no flip); out: an f32 [B(,T),3,h,w] tensor to write (dense planes, one stride between images)."""
        if not isinstance(frames, torch.Tensor):
            raise QtError("FramePreprocessor: frames must be a tensor")
        if frames.device.type != "cuda":
            raise QtError(f"FramePreprocessor: frames must be on an AMD GPU (got {frames.device}); there is no CPU or torch "
                          "fallback")
        if frames.dtype != torch.uint8:
            raise QtError(f"FramePreprocessor: uint8 frames only (got {frames.dtype})")
        if frames.dim() not in (4, 5) or frames.shape[-1] != 3 or min(frames.shape) < 1:
            raise QtError(f"FramePreprocessor: frames must be [B,H,W,3] or [B,T,H,W,3], no empty dimension (got "
                          f"{list(frames.shape)})")
        lead = tuple(frames.shape[:-3])
        H, W = int(frames.shape[-3]), int(frames.shape[-2])
        h, w = self.size
        dev = frames.device
        n = math.prod(lead)
        if boxes is not None:
            boxes = self._side(boxes, "boxes", lead, dev, (torch.int32,), (4,))
        if flips is not None:
            flips = self._side(flips, "flips", lead, dev, (torch.uint8, torch.bool), ())
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.float32 or \
                    tuple(out.shape) != lead + (3, h, w):
                raise QtError(f"FramePreprocessor: out must be an f32 {list(lead + (3, h, w))} tensor on {dev}")
            o = out if len(lead) == 1 else _one_batch_dim(out)
            if o is None or o.stride()[1:] != (h * w, w, 1) or (n > 1 and o.stride(0) < 3 * h * w):
                raise QtError("FramePreprocessor: out must have dense [3,h,w] images one stride apart")
        # any row / image stride the descriptor can express goes through as it is; everything else is copied once
        f = frames if len(lead) == 1 else _one_batch_dim(frames)
        if f is None or f.stride(3) != 1 or f.stride(2) != 3 or f.stride(1) < 3 * W or (n > 1 and f.stride(0) < H * f.stride(1)):
            f = frames.contiguous().view(n, H, W, 3)
        row_stride = f.stride(1)
        image_stride = f.stride(0) if n > 1 else H * row_stride
        L = _lib.lib()
        desc = PreprocessDesc(n, H, W, row_stride, image_stride, h, w, int(self.channel_order == "bgr"),
                              (ctypes.c_float * 3)(*self.mean), (ctypes.c_float * 3)(*self.inv_std))
        with torch.cuda.device(dev):
            if out is None:
                out = torch.empty(lead + (3, h, w), dtype=torch.float32, device=dev)
                dst_stride = 3 * h * w
            else:
                dst_stride = o.stride(0) if n > 1 else 3 * h * w
            _lib.check(L.qt_preprocess_u8(ctypes.byref(desc), f.data_ptr(), _lib.ptr(boxes), _lib.ptr(flips), out.data_ptr(),
                                          dst_stride, _lib.stream_ptr()), "qt_preprocess_u8")
        return out


def _one_batch_dim(t):
    """[B,T,...] as a [B*T,...] view when one stride separates consecutive images, else None"""
    B, T = t.shape[:2]
    if T == 1 or B == 1 or t.stride(0) == T * t.stride(1):
        stride0 = t.stride(1) if T > 1 else t.stride(0)
        return t.as_strided((B * T,) + tuple(t.shape[2:]), (stride0,) + tuple(t.stride()[2:]), t.storage_offset())
    return None


def random_resized_crop_boxes(n, src_hw, scale=(0.8, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), generator=None):
    """n boxes (top, left, height, width) by the rule of torchvision's RandomResizedCrop.get_params, drawn on the host:
    area = H W u with u uniform in `scale`, aspect ratio exp(v) with v uniform in log(ratio), w = round(sqrt(area ratio)),
    h = round(sqrt(area / ratio)); the first of ten draws with 0 < w <= W and 0 < h <= H gets a uniform position, otherwise
    the centre crop of the whole frame clamped to the ratio range.  (The rule, not torchvision's random stream.)
    Returns a CPU int32 [n, 4] tensor."""
    H, W = int(src_hw[0]), int(src_hw[1])
    if n < 1 or H < 1 or W < 1:
        raise ValueError(f"random_resized_crop_boxes: needs n >= 1 and a frame of at least 1 x 1 (got {n}, {src_hw!r})")
    if not (0 < scale[0] <= scale[1]) or not (0 < ratio[0] <= ratio[1]):
        raise ValueError(f"random_resized_crop_boxes: scale and ratio must be increasing positive pairs (got {scale}, {ratio})")
    u = torch.rand(n, 10, generator=generator, dtype=torch.float64)
    v = torch.rand(n, 10, generator=generator, dtype=torch.float64)
    pos = torch.rand(n, 2, generator=generator, dtype=torch.float64)
    area = H * W * (scale[0] + (scale[1] - scale[0]) * u)
    r = torch.exp(math.log(ratio[0]) + (math.log(ratio[1]) - math.log(ratio[0])) * v)
    w = torch.round(torch.sqrt(area * r)).long()
    h = torch.round(torch.sqrt(area / r)).long()
    ok = (w > 0) & (w <= W) & (h > 0) & (h <= H)
    first = torch.argmax(ok.int(), dim=1)             # the first valid draw (0 when there is none)
    rows = torch.arange(n)
    found = ok[rows, first]
    _, _, fh, fw = fallback_box((H, W), ratio)
    bh = torch.where(found, h[rows, first], torch.full((n,), fh))
    bw = torch.where(found, w[rows, first], torch.full((n,), fw))
    top = torch.where(found, torch.floor(pos[:, 0] * (H - bh + 1).double()).long().clamp(max=H - 1), (H - bh) // 2)
    left = torch.where(found, torch.floor(pos[:, 1] * (W - bw + 1).double()).long().clamp(max=W - 1), (W - bw) // 2)
    top = torch.minimum(top, H - bh)
    left = torch.minimum(left, W - bw)
    return torch.stack([top, left, bh, bw], dim=1).to(torch.int32).contiguous()


def random_flips(n, p=0.5, generator=None):
    """n flags (uint8, 1 = mirror left-right) with probability p, drawn on the host (RandomHorizontalFlip's rule)."""
    if n < 1 or not 0.0 <= p <= 1.0:
        raise ValueError(f"random_flips: needs n >= 1 and p in [0, 1] (got {n}, {p})")
    return (torch.rand(n, generator=generator) < p).to(torch.uint8)


def fallback_box(src_hw, ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """the box random_resized_crop_boxes returns when none of its ten draws fits the frame"""
    H, W = int(src_hw[0]), int(src_hw[1])
    in_ratio = W / H
    if in_ratio < ratio[0]:
        fw, fh = W, int(round(W / ratio[0]))
    elif in_ratio > ratio[1]:
        fh, fw = H, int(round(H * ratio[1]))
    else:
        fw, fh = W, H
    fh, fw = min(max(fh, 1), H), min(max(fw, 1), W)
    return ((H - fh) // 2, (W - fw) // 2, fh, fw)
