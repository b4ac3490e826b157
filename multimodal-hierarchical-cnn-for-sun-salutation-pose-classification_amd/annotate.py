"""Annotated frames on the device: the pose skeleton and the prediction caption drawn into uint8 frames by one HIP kernel
(csrc/annotate.hip), the last step of the reference's video loop (experiment/test_on_video_cnn.py:280-295) and the drawing
step of sqn process/processing_image_sequence.py:250-318, resnet/grad_cam_analysis.py:437 and grad_cam/5_grad_cam_visualizer.py:

    annotator = FrameAnnotator(class_names)                            # renders the caption atlas once, on the host (PIL)
    probs, confidence, pred = predict(model(images, numerical))       # all on the device
    shown = annotator.draw(frames, landmarks, detected, pred, confidence)     # uint8 [N,H,W,3] in, the same out
    writer.write(shown.cpu().numpy())                                  # the one host copy

`frames` is uint8 [N,H,W,3] (or [B,T,H,W,3]) on the GPU, `landmarks` f32 [N,33,4] = MediaPipe's x, y, z, visibility, the
tensor PoseFeatures.from_landmarks takes; `pred` and `confidence` are what predict / EvalMeter.update(probs=True) return.
draw() reads nothing back.  The skeleton is draw_enhanced_skeleton's: the 35 POSE_CONNECTIONS, the twelve MAJOR_SEGMENTS
5 pixels thick and the others 2, purple lines between two landmarks whose visibility is above min_visibility and orange
ones otherwise, then an orange disc of radius 3 on every visible landmark and a red one of radius 2 on the others.  The
caption is "<prefix><class> (<confidence with two decimals>)" from pre-rendered glyph tiles.  include/qtcnn.h states the
rule pixel by pixel, in integers.

Against the reference: a pixel belongs to a line when its centre is within half the thickness of the segment (exact
Euclidean distance), where cv2.line fills a fixed-point polygon with round caps; landmark positions are int(x * W) with the
product in f32, not float64; the confidence is rounded from f32 confidence * 100.  MediaPipe's default drawing style
(test_on_video_cnn.py) is not reproduced, and text is the caller's atlas, not cv2's Hershey font.  Not built: anti-aliased
lines, video encoding.  There is no torch fallback: CPU tensors and other dtypes raise QtError.
"""
import ctypes

import torch

from . import _lib
from ._abi import AnnotateDesc, bind  # noqa: F401  (<module>.bind is _abi.bind)
from ._lib import QtError

NUM_LANDMARKS = 33             # QT_POSE_LANDMARKS
MAX_SEGMENTS = 64              # QT_ANNOTATE_MAX_SEGMENTS
EXTRA_GLYPHS = "0123456789.() "    # the atlas tiles behind the class captions, in this order

# mp.solutions.pose.POSE_CONNECTIONS
POSE_CONNECTIONS = ((0, 1), (1, 2), (2, 3), (3, 7), (0, 4), (4, 5), (5, 6), (6, 8), (9, 10), (11, 12), (11, 13), (13, 15),
                    (15, 17), (15, 19), (15, 21), (17, 19), (12, 14), (14, 16), (16, 18), (16, 20), (16, 22), (18, 20),
                    (11, 23), (12, 24), (23, 24), (23, 25), (24, 26), (25, 27), (26, 28), (27, 29), (28, 30), (29, 31),
                    (30, 32), (27, 31), (28, 32))
# processing_image_sequence.py:271-284: shoulders, hips, the torso's sides, upper arms, forearms, thighs, shins
MAJOR_SEGMENTS = ((11, 12), (23, 24), (11, 23), (12, 24), (11, 13), (12, 14), (13, 15), (14, 16), (23, 25), (24, 26),
                  (25, 27), (26, 28))

_U8x3 = ctypes.c_ubyte * 3


def caption_atlas(class_names, prefix="Pose: ", height=24, font=None):
    """The caption tiles of qt_annotate_u8, rendered once on the host with PIL: (atlas uint8 [C + 14, height, width], widths
    int32 [C + 14]) as CPU tensors.  Tile g < C is `prefix + class_names[g]`, then come the fourteen EXTRA_GLYPHS; each tile
    is a coverage mask (0 .. 255) whose first widths[g] columns are in use, width is the widest of them.  font: a
    PIL.ImageFont of your own; by default PIL's built-in font, at `height` pixels where this PIL can scale it."""
    try:
        from PIL import Image, ImageDraw, ImageFont
    except ImportError as e:
        raise QtError("caption_atlas renders its tiles with PIL (pip package 'pillow'), which is not installed; build a "
                      "uint8 atlas [C + 14, h, w] with int32 widths [C + 14] by other means and pass atlas=(atlas, widths)") from e
    names = [str(c) for c in class_names]
    if not names:
        raise ValueError("caption_atlas: no class names")
    if height < 1:
        raise ValueError("caption_atlas: height must be positive")
    if font is None:
        try:
            font = ImageFont.load_default(size=max(1.0, 0.75 * height))   # (leaves room for descenders)
        except TypeError:                                                  # an older PIL: its one bitmap size
            font = ImageFont.load_default()
    strings = [prefix + n for n in names] + list(EXTRA_GLYPHS)
    probe = ImageDraw.Draw(Image.new("L", (1, 1)))
    widths = [max(0, int(-(-probe.textlength(s, font=font) // 1))) for s in strings]
    width = max(1, max(widths))
    atlas = torch.zeros(len(strings), height, width, dtype=torch.uint8)
    for g, s in enumerate(strings):
        tile = Image.new("L", (width, height), 0)
        ImageDraw.Draw(tile).text((0, 0), s, fill=255, font=font)
        atlas[g] = torch.frombuffer(bytearray(tile.tobytes()), dtype=torch.uint8).view(height, width)
    return atlas, torch.tensor(widths, dtype=torch.int32)


def _colour(c, name, reverse):
    c = tuple(int(v) for v in c)
    if len(c) != 3 or not all(0 <= v <= 255 for v in c):
        raise ValueError(f"FrameAnnotator: {name} must be three bytes (got {c})")
    return _U8x3(*(c[::-1] if reverse else c))


def _device_tensor(t, name, dtype, dev=None):
    if not isinstance(t, torch.Tensor):
        raise QtError(f"FrameAnnotator.draw: {name} must be a tensor")
    if t.dtype != dtype:
        raise QtError(f"FrameAnnotator.draw: {name} must be {dtype} (got {t.dtype})")
    if t.device.type != "cuda" or (dev is not None and t.device != dev):
        raise QtError(f"FrameAnnotator.draw: {name} must be on {'an AMD GPU' if dev is None else dev} (got {t.device}); there is "
                      "no CPU or torch fallback")
    return t


class FrameAnnotator:
    """class_names: the classes of `pred`, rendered by caption_atlas(class_names, prefix, glyph_height); or atlas=(atlas,
    widths), any uint8 [C + 14, h, w] / int32 [C + 14] pair in caption_atlas's layout; neither: no caption is drawn.
    channel_order: "bgr" (cv2 frames) or "rgb".  Colours are given as the reference writes them, for BGR frames, and are
    reversed for "rgb".  connections / major_segments: landmark pairs; a connection that is in major_segments (in either
    orientation) is thick_major wide.  caption_origin: (x, y) of the caption's top-left corner.  The defaults are
    draw_enhanced_skeleton's constants with the visibility threshold of its call, and putText's green."""

    def __init__(self, class_names=None, atlas=None, channel_order="bgr", connections=POSE_CONNECTIONS,
                 major_segments=MAJOR_SEGMENTS, min_visibility=0.65, thick_major=5, thick_minor=2, radius_hi=3, radius_lo=2,
                 line_hi=(245, 66, 230), line_lo=(0, 165, 255), point_hi=(245, 117, 66), point_lo=(0, 0, 255),
                 prefix="Pose: ", glyph_height=24, caption_origin=(10, 10), caption_colour=(0, 255, 0)):
        if channel_order not in ("bgr", "rgb"):
            raise ValueError(f"FrameAnnotator: channel_order must be 'bgr' or 'rgb' (got {channel_order!r})")
        rev = channel_order == "rgb"
        self.channel_order = channel_order
        connections = [(int(a), int(b)) for a, b in connections]
        if len(connections) > MAX_SEGMENTS:
            raise ValueError(f"FrameAnnotator: {len(connections)} connections; at most {MAX_SEGMENTS} are drawn")
        if any(not 0 <= v <= 255 for pair in connections for v in pair):
            raise ValueError("FrameAnnotator: a landmark index must fit a byte")
        major = {frozenset((int(a), int(b))) for a, b in major_segments}
        self.segments = torch.zeros(max(1, len(connections)), 3, dtype=torch.uint8)   # (never an empty allocation)
        for k, (a, b) in enumerate(connections):
            self.segments[k] = torch.tensor([a, b, int(frozenset((a, b)) in major)], dtype=torch.uint8)
        for name, v in (("thick_major", thick_major), ("thick_minor", thick_minor), ("radius_hi", radius_hi),
                        ("radius_lo", radius_lo)):
            if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= 15:
                raise ValueError(f"FrameAnnotator: {name} must be an integer in 1 .. 15 (got {v!r})")
        if not float(min_visibility) == float(min_visibility):
            raise ValueError("FrameAnnotator: min_visibility is NaN")
        if atlas is not None and class_names is not None:
            raise ValueError("FrameAnnotator: give class_names or a ready atlas, not both")
        if class_names is not None:
            atlas = caption_atlas(class_names, prefix, glyph_height)
        if atlas is not None:
            tiles, widths = atlas
            if (not isinstance(tiles, torch.Tensor) or tiles.dtype != torch.uint8 or tiles.dim() != 3
                    or tiles.shape[0] <= len(EXTRA_GLYPHS) or tiles.shape[1] < 1 or tiles.shape[2] < 1):
                raise ValueError("FrameAnnotator: the atlas must be a uint8 [C + 14, h, w] tensor with C >= 1")
            if not isinstance(widths, torch.Tensor) or widths.dtype != torch.int32 or tuple(widths.shape) != (tiles.shape[0],):
                raise ValueError(f"FrameAnnotator: the atlas widths must be an int32 [{tiles.shape[0]}] tensor")
            atlas = (tiles.detach().contiguous(), widths.detach().contiguous())
        self.atlas = atlas
        self.num_classes = 0 if atlas is None else int(atlas[0].shape[0]) - len(EXTRA_GLYPHS)
        self._desc = AnnotateDesc(
            0, 0, 0, len(connections), float(min_visibility), thick_major, thick_minor, radius_hi, radius_lo,
            _colour(line_hi, "line_hi", rev), _colour(line_lo, "line_lo", rev), _colour(point_hi, "point_hi", rev),
            _colour(point_lo, "point_lo", rev), self.num_classes, 0 if atlas is None else int(atlas[0].shape[1]),
            0 if atlas is None else int(atlas[0].shape[2]), int(caption_origin[0]), int(caption_origin[1]),
            _colour(caption_colour, "caption_colour", rev))
        self._on = {}   # device -> (segments, atlas, widths) there

    def _tables(self, dev):
        t = self._on.get(dev)
        if t is None:
            t = (self.segments.to(dev), None if self.atlas is None else self.atlas[0].to(dev),
                 None if self.atlas is None else self.atlas[1].to(dev))
            self._on[dev] = t
        return t

    def draw(self, frames, landmarks=None, detected=None, pred=None, confidence=None, out=None):
        """frames: uint8 [N,H,W,3] or [B,T,H,W,3] on the GPU, in the annotator's channel order.  With N the leading shape:
        landmarks f32 [N,33,4] draws the skeleton (detected: uint8 or bool [N], zero where no pose was found; None: found
        everywhere); pred int64 [N] draws the class caption (none where pred is outside [0, C)), confidence f32 [N] appends
        " (0.87)".  out: None (a new tensor), or a contiguous uint8 tensor of frames' shape, which may be frames itself
        (in place; pixels nothing is drawn on are then not touched).  Returns out.  One launch, no host read."""
        what = "FrameAnnotator.draw"
        frames = _device_tensor(frames, "frames", torch.uint8)
        dev = frames.device
        if frames.dim() not in (4, 5) or frames.shape[-1] != 3 or frames.numel() == 0:
            raise QtError(f"{what}: frames must be [N,H,W,3] or [B,T,H,W,3], no empty dimension (got {list(frames.shape)})")
        lead = tuple(frames.shape[:-3])
        H, W = int(frames.shape[-3]), int(frames.shape[-2])
        batch = frames.numel() // (3 * H * W)
        if landmarks is None and pred is None:
            raise QtError(f"{what}: nothing to draw: give landmarks, pred or both")
        if out is not None:
            _device_tensor(out, "out", torch.uint8, dev)
            if out.shape != frames.shape or not out.is_contiguous():
                raise QtError(f"{what}: out must be a contiguous tensor of frames' shape {list(frames.shape)}")
        if not frames.is_contiguous():
            if out is frames:
                raise QtError(f"{what}: frames that are drawn on in place must be contiguous")
            frames = frames.contiguous()
        if out is None:
            out = torch.empty_like(frames)
        segments, atlas, widths = self._tables(dev)
        if landmarks is not None:
            landmarks = _device_tensor(landmarks, "landmarks", torch.float32, dev)
            if tuple(landmarks.shape) != lead + (NUM_LANDMARKS, 4):
                raise QtError(f"{what}: landmarks must have shape {list(lead + (NUM_LANDMARKS, 4))} (got {list(landmarks.shape)})")
            landmarks = landmarks.contiguous()
            if landmarks.data_ptr() % 16:
                landmarks = landmarks.clone()   # (a view that starts inside an allocation)
            if detected is not None:
                if isinstance(detected, torch.Tensor) and detected.dtype == torch.bool:
                    detected = detected.to(torch.uint8)
                detected = _device_tensor(detected, "detected", torch.uint8, dev).contiguous()
                if tuple(detected.shape) != lead:
                    raise QtError(f"{what}: detected must have shape {list(lead)} (got {list(detected.shape)})")
        elif detected is not None:
            raise QtError(f"{what}: detected belongs to landmarks")
        if pred is not None:
            if atlas is None:
                raise QtError(f"{what}: this annotator has no caption atlas (give class_names or atlas= to FrameAnnotator)")
            pred = _device_tensor(pred, "pred", torch.int64, dev).contiguous()
            if tuple(pred.shape) != lead:
                raise QtError(f"{what}: pred must have shape {list(lead)} (got {list(pred.shape)})")
            if confidence is not None:
                confidence = _device_tensor(confidence, "confidence", torch.float32, dev).contiguous()
                if tuple(confidence.shape) != lead:
                    raise QtError(f"{what}: confidence must have shape {list(lead)} (got {list(confidence.shape)})")
        elif confidence is not None:
            raise QtError(f"{what}: confidence belongs to pred")
        desc = AnnotateDesc.from_buffer_copy(self._desc)
        desc.batch, desc.H, desc.W = batch, H, W
        L = _lib.lib()
        with torch.cuda.device(dev):
            _lib.check(L.qt_annotate_u8(ctypes.byref(desc), _lib.ptr(frames), _lib.ptr(landmarks), _lib.ptr(detected),
                                        _lib.ptr(segments if landmarks is not None else None), _lib.ptr(pred),
                                        _lib.ptr(confidence), _lib.ptr(atlas if pred is not None else None),
                                        _lib.ptr(widths if pred is not None else None), _lib.ptr(out), _lib.stream_ptr()),
                       "qt_annotate_u8")
        return out
