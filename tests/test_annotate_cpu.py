"""Annotated frames, the parts that need no GPU: the integer rule of tests/_annotate_ref.py against a float64 Euclidean
distance and on hand-made cases, the kernel's walk restated in Python against that rule, the C ABI's declarations and its
host-side refusals, the Python surface."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import _annotate_ref as R
from _util import PKG, ROOT, pkg

QT_OK, QT_ERR_INVALID_ARG, QT_ERR_UNSUPPORTED = 0, -1, -3


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    declared = set(re.findall(r"\b(qt_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(os.path.join(ROOT, PKG, "libqtcnn_hip.so"))
    assert "qt_annotate_u8" in declared and hasattr(lib, "qt_annotate_u8")
    assert "} qt_annotate_desc;" in header and "#define QT_ANNOTATE_MAX_SEGMENTS 64" in header
    M = pkg("annotate")
    assert M.MAX_SEGMENTS == R.MAX_SEGMENTS == 64 and M.NUM_LANDMARKS == 33
    # the ctypes mirror has the header's fields in the header's order
    body = header[header.index("typedef struct qt_annotate_desc {"):header.index("} qt_annotate_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split("{", 1)[1].split(";"):
        names = re.sub(r"^\s*(unsigned char|int|float)\s+", "", decl.strip())
        fields += [n.split("[")[0].strip() for n in names.split(",") if n.strip()]
    assert fields == [f[0] for f in M.AnnotateDesc._fields_]
    assert ctypes.sizeof(M.AnnotateDesc) == 72


def test_exports_and_tables():
    P, M = pkg(), pkg("annotate")
    names = {"FrameAnnotator", "caption_atlas", "POSE_CONNECTIONS", "MAJOR_SEGMENTS"}
    assert names <= set(P.__all__)
    for n in names:
        assert getattr(P, n) is getattr(M, n)
    assert tuple(M.POSE_CONNECTIONS) == R.POSE_CONNECTIONS and tuple(M.MAJOR_SEGMENTS) == R.MAJOR_SEGMENTS
    pairs = {frozenset(p) for p in M.POSE_CONNECTIONS}
    assert len(M.POSE_CONNECTIONS) == 35 and len(pairs) == 35 and all(len(p) == 2 for p in pairs)
    assert all(0 <= v <= 32 for p in M.POSE_CONNECTIONS for v in p)
    assert len(M.MAJOR_SEGMENTS) == 12 and {frozenset(p) for p in M.MAJOR_SEGMENTS} <= pairs
    seg = M.FrameAnnotator().segments.numpy()
    assert np.array_equal(seg, R.default_segments()) and int(seg[:, 2].sum()) == 12


def _desc(M, **kw):
    d = M.AnnotateDesc(batch=2, H=48, W=64, n_segments=35, min_visibility=0.65, thick_major=5, thick_minor=2, radius_hi=3,
                       radius_lo=2, num_classes=12, glyph_h=24, glyph_w=100, ox=10, oy=10)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_host_side_argument_checks_need_no_device():
    """every refusal below comes before the first device call: the pointers are never dereferenced"""
    M = pkg("annotate")
    L = pkg("_lib").lib()
    fr, lm, det, seg, pr, cf, at, wd, out = (0x100000 * k for k in range(1, 10))

    def call(desc, frames=fr, landmarks=lm, detected=None, segments=seg, pred=pr, confidence=cf, atlas=at, widths=wd, dst=out):
        return L.qt_annotate_u8(ctypes.byref(desc), frames, landmarks, detected, segments, pred, confidence, atlas, widths,
                                dst, None)

    bad = QT_ERR_INVALID_ARG
    assert L.qt_annotate_u8(None, fr, lm, None, seg, pr, cf, at, wd, out, None) == bad
    for field in ("batch", "H", "W"):
        for v in (0, -3):
            assert call(_desc(M, **{field: v})) == bad and b"positive" in L.qt_last_error(), field
    assert call(_desc(M), frames=None) == bad and call(_desc(M), dst=None) == bad
    assert call(_desc(M, n_segments=65)) == bad and b"n_segments" in L.qt_last_error()
    assert call(_desc(M, n_segments=-1)) == bad
    for field in ("thick_major", "thick_minor", "radius_hi", "radius_lo"):
        for v in (0, 16, -1):
            assert call(_desc(M, **{field: v})) == bad and b"[1, 15]" in L.qt_last_error(), field
    assert call(_desc(M, min_visibility=float("nan"))) == bad and b"NaN" in L.qt_last_error()
    # half-given groups, and neither group
    assert call(_desc(M), segments=None) == bad and b"skeleton group" in L.qt_last_error()
    assert call(_desc(M), landmarks=None) == bad
    assert call(_desc(M), landmarks=None, segments=None, detected=det) == bad
    assert call(_desc(M), atlas=None) == bad and b"caption group" in L.qt_last_error()
    assert call(_desc(M), widths=None) == bad
    assert call(_desc(M), pred=None) == bad
    assert call(_desc(M), pred=None, atlas=None, widths=None) == bad        # confidence without them
    assert call(_desc(M), landmarks=None, segments=None, pred=None, confidence=None, atlas=None, widths=None) == bad
    assert b"nothing to draw" in L.qt_last_error()
    # alignment
    assert call(_desc(M), landmarks=lm + 4) == bad and b"16-byte" in L.qt_last_error()
    assert call(_desc(M), pred=pr + 4) == bad and call(_desc(M), confidence=cf + 2) == bad and call(_desc(M), widths=wd + 1) == bad
    for field in ("num_classes", "glyph_h", "glyph_w"):
        assert call(_desc(M, **{field: 0})) == bad, field
    # out overlaps frames without being frames
    assert call(_desc(M), dst=fr + 3) == bad and b"overlaps" in L.qt_last_error()
    assert call(_desc(M), dst=fr - 2 * 48 * 64 * 3 + 1) == bad
    # sizes that are not handled
    unsup = QT_ERR_UNSUPPORTED
    assert call(_desc(M, H=8193)) == unsup and call(_desc(M, W=8193)) == unsup and b"8192" in L.qt_last_error()
    assert call(_desc(M, batch=11, H=8192, W=8192)) == unsup                # 11 * 3 * 2^26 > 2^31
    assert call(_desc(M, glyph_w=8193)) == unsup and call(_desc(M, glyph_h=8193)) == unsup
    assert call(_desc(M, ox=(1 << 20) + 1)) == unsup and call(_desc(M, oy=-(1 << 20) - 1)) == unsup
    # a caption alone does not read the skeleton's style
    assert call(_desc(M, thick_major=0, H=8193), landmarks=None, segments=None) == unsup


def _dist2(xs, ys, ax, ay, bx, by):
    """float64 squared Euclidean distance from the pixel grids to segment AB"""
    dx, dy = float(bx - ax), float(by - ay)
    L = dx * dx + dy * dy
    ex, ey = xs - float(ax), ys - float(ay)
    t = np.clip((ex * dx + ey * dy) / L, 0.0, 1.0) if L > 0 else np.zeros_like(ex)
    return (ex - t * dx) ** 2 + (ey - t * dy) ** 2


def test_integer_rule_is_the_euclidean_distance():
    rng = np.random.default_rng(2024)
    H, W = 48, 64
    ys, xs = np.mgrid[0:H, 0:W]
    xf, yf = xs.astype(np.float64), ys.astype(np.float64)
    xi, yi = xs.astype(np.int64), ys.astype(np.int64)
    excluded = total = covered = 0
    for T in (2, 5):
        for k in range(400):
            ax, ay, bx, by = (int(v) for v in rng.integers(-10, 70, 4))
            if k % 10 == 0:
                bx, by = ax, ay
            got = R.segment_covers(xi, yi, ax, ay, bx, by, T)
            margin = 4.0 * _dist2(xf, yf, ax, ay, bx, by) - T * T
            sure = np.abs(margin) >= 1e-6
            assert np.array_equal(got[sure], (margin <= 0)[sure]), (T, k, ax, ay, bx, by)
            excluded += int((~sure).sum())
            total += sure.size
            covered += int(got.sum())
    print(f"excluded {excluded} of {total} pixels ({100.0 * excluded / total:.3f} %), {covered} covered")
    assert excluded / total < 0.01 and covered > 10000
    # a disc is the segment of length zero with T = 2 r
    for r in (1, 2, 3, 15):
        assert np.array_equal(R.disc_covers(xi, yi, 20, 17, r), R.segment_covers(xi, yi, 20, 17, 20, 17, 2 * r))


def test_painters_order_and_visibility():
    H, W = 40, 40
    lm = np.zeros((33, 4), np.float32)
    lm[:, :2] = -1.0                                  # everything else far outside (usable, nothing reaches the frame)
    lm[:, 3] = 0.9
    at = lambda j, x, y, vis=0.9: lm.__setitem__(j, ((x + 0.5) / W, (y + 0.5) / H, 0, vis))
    at(0, 5, 20), at(1, 35, 20), at(2, 20, 5, 0.65), at(3, 20, 35)
    style = R.Style()
    seg = np.array([[0, 1, 1], [2, 3, 0]], np.uint8)
    out = R.annotate(np.zeros((1, H, W, 3), np.uint8), lm[None], None, seg, style=style)[0]
    assert tuple(out[20, 12]) == style.line_hi        # the thick horizontal line, both ends visible
    assert tuple(out[18, 12]) == style.line_hi and tuple(out[17, 12]) == (0, 0, 0)      # 4 * 2^2 <= 25 < 4 * 3^2
    assert tuple(out[12, 20]) == style.line_lo        # the vertical one: visibility 0.65 is not > 0.65
    assert tuple(out[12, 21]) == style.line_lo and tuple(out[12, 22]) == (0, 0, 0) and tuple(out[12, 19]) == style.line_lo
    assert tuple(out[20, 20]) == style.line_lo        # the later segment wins the crossing ...
    assert tuple(out[20, 22]) == style.line_hi
    assert tuple(out[20, 5]) == style.point_hi and tuple(out[20, 8]) == style.point_hi  # ... and a disc beats both lines
    assert tuple(out[20, 9]) == style.line_hi
    assert tuple(out[5, 20]) == style.point_lo and tuple(out[7, 20]) == style.point_lo and tuple(out[8, 20]) == style.line_lo
    swapped = R.annotate(np.zeros((1, H, W, 3), np.uint8), lm[None], None, seg[::-1], style=style)[0]
    assert tuple(swapped[20, 20]) == style.line_hi and tuple(swapped[20, 22]) == style.line_hi
    # detected == 0: nothing; a segment index above 32: that segment only
    assert not R.annotate(np.zeros((1, H, W, 3), np.uint8), lm[None], np.array([0], np.uint8), seg).any()
    skipped = R.annotate(np.zeros((1, H, W, 3), np.uint8), lm[None], None, np.array([[0, 200, 1], [2, 3, 0]], np.uint8))[0]
    assert tuple(skipped[20, 12]) == (0, 0, 0) and tuple(skipped[12, 20]) == style.line_lo


def test_digit_rule():
    assert R.confidence_digits(0.0) == (0, 0, 0) and R.confidence_digits(1.0) == (1, 0, 0)
    assert R.confidence_digits(0.05) == (0, 0, 5) and R.confidence_digits(0.99) == (0, 9, 9)
    assert R.confidence_digits(np.float32(0.005)) == (0, 0, 0)        # f32: 0.005 * 100 = 0.49999997
    # f32(0.995) * 100 = 99.5000005 exactly, within half an f32 step (3.8e-6) of 99.5: the f32 product IS 99.5, a tie, and
    # rintf takes it to the even 100 (f"{c:.2f}" of that f32 says 1.00 as well; at 0.985 it says 0.99 where this says 0.98).
    exact = Fraction(float(np.float32(0.995))) * 100
    assert abs(exact - Fraction(199, 2)) < Fraction(1, 2 ** 18) and np.float32(0.995) * np.float32(100) == np.float32(99.5)
    assert R.confidence_digits(np.float32(0.995)) == (1, 0, 0)
    assert R.confidence_digits(np.float32(0.985)) == (0, 9, 8)        # likewise a tie at 98.5: to the even 98
    assert R.confidence_digits(0.996) == (1, 0, 0) and R.confidence_digits(0.125) == (0, 1, 2)      # 12.5 rounds to even
    assert R.confidence_digits(-3.0) == (0, 0, 0) and R.confidence_digits(7.0) == (1, 0, 0)
    assert R.confidence_digits(np.inf) == (1, 0, 0) and R.confidence_digits(-np.inf) == (0, 0, 0)
    assert R.confidence_digits(np.nan) is None
    C = 5
    assert R.glyph_sequence(3, 0.05, C) == [3, C + 13, C + 11, C + 0, C + 10, C + 0, C + 5, C + 12]
    assert R.glyph_sequence(3, np.nan, C) == [3] and R.glyph_sequence(3, None, C) == [3]
    assert R.glyph_sequence(-1, 0.5, C) == [] and R.glyph_sequence(C, 0.5, C) == []


def test_caption_blend_and_clipping():
    C, gh, gw = 2, 4, 3
    atlas = np.zeros((C + 14, gh, gw), np.uint8)
    widths = np.full(C + 14, gw, np.int32)
    atlas[0] = 255
    atlas[1, :, 0], atlas[1, :, 1], atlas[1, :, 2] = 0, 128, 255
    widths[1] = 2
    style = R.Style(origin=(6, 5), caption_colour=(10, 200, 255))
    frames = np.full((1, 8, 8, 3), 100, np.uint8)
    out = R.annotate(frames, pred=np.array([0]), atlas=atlas, widths=widths, style=style)[0]
    assert (out[5:8, 6:8] == style.caption_colour).all()              # clipped on the right and at the bottom
    changed = (out != 100).any(axis=-1)
    assert changed.sum() == 6 and changed[5:8, 6:8].all()
    out = R.annotate(frames, pred=np.array([1]), atlas=atlas, widths=widths, style=R.Style(origin=(-1, -2), caption_colour=(10, 200, 255)))[0]
    assert (out[0:2, 0] == [(128 * 10 + 127 * 100 + 127) // 255, (128 * 200 + 127 * 100 + 127) // 255,
                            (128 * 255 + 127 * 100 + 127) // 255]).all()
    assert ((out != 100).any(axis=-1).sum()) == 2                     # column -1 (mask 0) is off the frame, column 2 is past the width
    # a width outside [0, glyph_w] counts as 0: the glyph draws nothing and the pen stays
    widths[0] = gw + 1
    out = R.annotate(frames, pred=np.array([0]), confidence=np.array([0.5], np.float32), atlas=atlas, widths=widths, style=style)[0]
    assert (out == 100).all()                                         # every following tile is an empty mask
    assert (R.annotate(frames, pred=np.array([C]), atlas=atlas, widths=widths) == frames).all()


CASES = [dict(B=1, H=37, W=53, mod=0), dict(B=2, H=37, W=53, mod=7), dict(B=2, H=64, W=80, mod=0), dict(B=1, H=3, W=5, mod=9),
         dict(B=1, H=1, W=16, mod=3), dict(B=1, H=72, W=120, mod=5)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "{B}x{H}x{W}+{mod}".format(**c))
def test_kernel_walk_restated_matches_the_rule(case):
    """heads, groups, tails, tiles, bounding-box culls and the narrowed tests of csrc/annotate.hip leave no pixel out and
    change no bit (72 x 120 is three tiles per frame)"""
    B, H, W = case["B"], case["H"], case["W"]
    atlas, widths = R.make_atlas()
    frames = R.make_frames(B, H, W, seed=H)
    lm = R.make_landmarks(B, seed=W)
    seg = R.default_segments()
    if min(H, W) >= 16:                              # (the hand-placed cases need room)
        lm[0], edge_seg = R.edge_landmarks(H, W)
        seg = np.concatenate([edge_seg, seg])
    pred = np.array([0, 3][:B])
    conf = np.array([0.995, 0.5][:B], np.float32)
    style = R.Style(origin=(W - 30, H - 6), thick_major=15, radius_hi=7)
    args = dict(landmarks=lm, segments=seg, pred=pred, confidence=conf, atlas=atlas, widths=widths, style=style)
    want = R.annotate(frames, **args)
    assert (want != frames).any()
    for in_place in (False, True):
        got = R.restated(frames, out_mod16=case["mod"], in_place=in_place, **args)
        assert np.array_equal(got, want), in_place
    only = dict(pred=pred, atlas=atlas, widths=widths, style=R.Style(origin=(2, 1)))
    assert np.array_equal(R.restated(frames, out_mod16=case["mod"], in_place=True, **only), R.annotate(frames, **only))


def test_caption_atlas_shapes():
    pytest.importorskip("PIL")
    M = pkg("annotate")
    names = ["Tadasana", "Bhujangasana", "Adho Mukha"]
    atlas, widths = M.caption_atlas(names, prefix="Pose: ", height=20)
    assert atlas.dtype == torch.uint8 and widths.dtype == torch.int32 and atlas.device.type == "cpu"
    assert tuple(atlas.shape[:2]) == (3 + 14, 20) and tuple(widths.shape) == (17,)
    assert int(widths.max()) == atlas.shape[2] and int(widths.min()) >= 0
    assert int(widths[1]) > int(widths[0]) > int(widths[3 + 1]) > 0            # longer strings are wider; a digit is narrow
    assert int(atlas[0].max()) == 255 and not bool(atlas[3 + 13].any())        # ' ' has a width and no ink
    assert int(widths[3 + 13]) > 0
    for g in range(17):
        assert not bool(atlas[g, :, int(widths[g]):].any()), g                  # no ink behind a tile's width
    a = M.FrameAnnotator(class_names=names, glyph_height=20)
    assert a.num_classes == 3 and torch.equal(a.atlas[0], atlas)
    b = M.FrameAnnotator(atlas=(atlas, widths))
    assert b.num_classes == 3


def test_constructor_and_device_checks():
    P, M = pkg(), pkg("annotate")
    for bad in (dict(channel_order="gbr"), dict(thick_major=16), dict(radius_lo=0), dict(min_visibility=float("nan")),
                dict(line_hi=(1, 2)), dict(point_lo=(0, 0, 256)), dict(connections=[(0, 1)] * 65),
                dict(atlas=(torch.zeros(14, 4, 4, dtype=torch.uint8), torch.zeros(14, dtype=torch.int32))),
                dict(atlas=(torch.zeros(15, 4, 4, dtype=torch.uint8), torch.zeros(15, dtype=torch.int64)))):
        with pytest.raises(ValueError):
            P.FrameAnnotator(**bad)
    rgb, bgr = P.FrameAnnotator(channel_order="rgb"), P.FrameAnnotator()
    assert tuple(bgr._desc.line_hi) == (245, 66, 230) and tuple(rgb._desc.line_hi) == (230, 66, 245)
    assert tuple(bgr._desc.point_lo) == (0, 0, 255) and tuple(rgb._desc.point_lo) == (255, 0, 0)
    assert (bgr._desc.thick_major, bgr._desc.thick_minor, bgr._desc.radius_hi, bgr._desc.radius_lo) == (5, 2, 3, 2)
    assert abs(bgr._desc.min_visibility - 0.65) < 1e-7 and bgr._desc.n_segments == 35
    # no torch fallback
    frames, lm = torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.zeros(2, 33, 4)
    with pytest.raises(P.QtError, match="AMD GPU"):
        bgr.draw(frames, lm)
    with pytest.raises(P.QtError, match="uint8"):
        bgr.draw(frames.float(), lm)
    with pytest.raises(P.QtError, match="tensor"):
        bgr.draw(frames.numpy(), lm)
