"""Frame preprocessing without a GPU: the float64 reference of tests/_preprocess_ref.py against torch and PIL, a torch-f32
restatement of the kernel's operation order against the derived bound (and two wrong versions that must miss it), the
exact-integer tap windows, descriptor validation before any device call, and the host-side box / flip draws."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import _preprocess_ref as R
from _util import pkg

ALL_CASES = R.CASES + [R.IDENTITY]
IDS = [c[0] for c in ALL_CASES]


def _boxes_of(case):
    _, H, W, boxes, _, _ = case
    return [(0, 0, H, W)] if boxes is None else boxes


@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_reference_equals_torch_float64_antialias(case):
    frames, boxes, hw = R.case_inputs(case)
    _, _, grey = R.reference(frames, boxes, None, hw)
    worst = 0.0
    for b, (t, l, bh, bw) in enumerate(_boxes_of(case)):
        crop = frames[b, t:t + bh, l:l + bw, :].double().permute(2, 0, 1).unsqueeze(0)
        want = F.interpolate(crop, size=hw, mode="bilinear", antialias=True, align_corners=False)[0]
        worst = max(worst, float((grey[b] - want).abs().max()))
    print(f"{case[0]}: max |restatement - torch float64| = {worst:.3e} grey levels")
    assert worst <= 1e-10      # 255 * taps * 2^-53 is 1e-12; the issue measured 6e-14 on [0, 1] data


@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_pil_bilinear_within_one_grey_level(case):
    """the one difference from the reference's transform: PIL rounds to uint8 after each pass (two roundings of at most 0.5,
    the second pass a convex combination of the first)"""
    Image = pytest.importorskip("PIL.Image")
    frames, boxes, hw = R.case_inputs(case)
    _, _, grey = R.reference(frames, boxes, None, hw)
    worst = 0.0
    for b, (t, l, bh, bw) in enumerate(_boxes_of(case)):
        crop = frames[b, t:t + bh, l:l + bw, :].contiguous().numpy()
        pil = Image.fromarray(crop, "RGB").resize((hw[1], hw[0]), Image.BILINEAR)
        got = torch.from_numpy(__import__("numpy").asarray(pil).copy()).double().permute(2, 0, 1)
        worst = max(worst, float((got - grey[b]).abs().max()))
    print(f"{case[0]}: max |PIL - restatement| = {worst:.4f} grey levels")
    assert worst <= 1.01


@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_f32_restatement_passes_the_derived_bound(case):
    frames, boxes, hw = R.case_inputs(case)
    n = frames.shape[0]
    flips = [i % 2 for i in range(n)]
    for bgr in (False, True):
        ref, bound, _ = R.reference(frames, boxes, flips, hw, bgr=bgr)
        got = R.kernel_f32(frames, boxes, flips, hw, bgr=bgr)
        r = R.ratio(got, ref, bound)
        print(f"{case[0]} bgr={bgr}: error / bound = {r:.3f}")
        assert r <= 1.0


@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_wrong_versions_miss_the_bound(case):
    """the bound is not loose: a tap window shifted by one and border weights that are not renormalised both miss it"""
    frames, boxes, hw = R.case_inputs(case)
    ref, bound, _ = R.reference(frames, boxes, None, hw)
    shifted = R.ratio(R.kernel_f32(frames, boxes, None, hw, shift=1), ref, bound)
    raw = R.ratio(R.kernel_f32(frames, boxes, None, hw, renormalise=False), ref, bound)
    print(f"{case[0]}: error / bound: window shifted {shifted:.3g}, border not renormalised {raw:.3g}")
    if case is R.IDENTITY:
        assert shifted > 1.0      # weights {1, 0}: no window is clipped, so only the shift can show
        return
    assert shifted > 1.0 and raw > 1.0


def test_black_frame_is_the_rounded_constant():
    """A = 0: the bound is its mean term alone, and -mean * inv_std rounded once passes it"""
    frames = torch.zeros(1, 9, 11, 3, dtype=torch.uint8)
    ref, bound, _ = R.reference(frames, None, None, (4, 5))
    assert R.ratio(R.kernel_f32(frames, None, None, (4, 5)), ref, bound) <= 1.0
    assert float(bound.max()) <= 2 * R.U * 2.2


@pytest.mark.parametrize("n_in,n_out", [(113, 24), (85, 24), (28, 64), (240, 24), (30, 30), (1, 8), (50, 23), (1560, 65),
                                        (480, 224), (270, 224), (7, 7), (3, 10), (1000, 41)])
def test_integer_window_equals_float64_window(n_in, n_out):
    for i in range(n_out):
        lo_f, w_f = R.window_f64(i, n_in, n_out)
        lo_i, m = R.window_int(i, n_in, n_out)
        M = sum(m)
        assert M > 0
        wf = {lo_f + k: v for k, v in enumerate(w_f)}
        wi = {lo_i + k: v / M for k, v in enumerate(m)}
        for j in set(wf) | set(wi):
            if j in wf and j in wi:
                assert abs(wf[j] - wi[j]) <= 1e-12, (i, j)
            else:                                  # a tap only one of them has sits at a window's end with next to no weight
                assert wf.get(j, 0.0) < 1e-12 and wi.get(j, 0.0) < 1e-12, (i, j)
        assert 0 <= lo_i and lo_i + len(m) <= n_in
        assert len(m) <= 2 * math.ceil(max(n_in, n_out) / n_out) + 1      # the launcher's tap bound


def _desc(M, **kw):
    d = dict(batch=2, src_h=48, src_w=64, src_row_stride=192, src_image_stride=48 * 192, out_h=24, out_w=24, bgr=0)
    d.update(kw)
    return M.PreprocessDesc(d["batch"], d["src_h"], d["src_w"], d["src_row_stride"], d["src_image_stride"], d["out_h"],
                            d["out_w"], d["bgr"], (ctypes.c_float * 3)(*R.MEAN32), (ctypes.c_float * 3)(*R.INV_STD32))


def test_descriptor_validation_needs_no_device():
    """every refusal comes with a message and before any HIP call: the pointers are never dereferenced"""
    M, Lm = pkg("preprocess"), pkg("_lib")
    L = Lm.lib()
    fake = ctypes.c_void_p(4096)
    stride = 3 * 24 * 24

    def call(desc, src=fake, dst=fake, dst_stride=stride):
        return L.qt_preprocess_u8(ctypes.byref(desc) if desc is not None else None, src, None, None, dst, dst_stride, None)

    invalid = [("batch", 0), ("src_h", 0), ("src_w", -1), ("out_h", 0), ("out_w", -3), ("src_row_stride", 191),
               ("src_image_stride", 48 * 192 - 1), ("bgr", 2)]
    for field, bad in invalid:
        assert call(_desc(M, **{field: bad})) == -1, field                 # QT_ERR_INVALID_ARG
        assert b"qt_preprocess_u8" in L.qt_last_error(), field
    assert call(None) == -1
    assert call(_desc(M), src=None) == -1 and b"null" in L.qt_last_error()
    assert call(_desc(M), dst=None) == -1 and b"null" in L.qt_last_error()
    assert call(_desc(M), dst=ctypes.c_void_p(4098)) == -1 and b"aligned" in L.qt_last_error()
    assert call(_desc(M), dst_stride=stride - 1) == -1 and b"destination image stride" in L.qt_last_error()
    # beyond the downscale limit: QT_ERR_UNSUPPORTED, naming the limit, still without a device
    rs = 3 * (M.MAX_DOWNSCALE * 24 + 1)
    assert call(_desc(M, src_w=M.MAX_DOWNSCALE * 24 + 1, src_row_stride=rs, src_image_stride=48 * rs)) == -3
    assert b"downscale limit" in L.qt_last_error()
    assert call(_desc(M, src_h=M.MAX_DOWNSCALE * 24 + 1, src_image_stride=(M.MAX_DOWNSCALE * 24 + 1) * 192)) == -3
    assert b"downscale limit" in L.qt_last_error()


def test_frame_preprocessor_refuses_before_device_work():
    P = pkg()
    pre = P.FramePreprocessor()
    with pytest.raises(P.QtError, match="AMD GPU"):
        pre(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(P.QtError):
        pre("frames")
    with pytest.raises(ValueError):
        P.FramePreprocessor(channel_order="gbr")
    with pytest.raises(ValueError):
        P.FramePreprocessor(std=(0.2, 0.0, 0.2))


@pytest.mark.parametrize("H,W", [(480, 600), (600, 480), (64, 64), (270, 480), (17, 200)])
def test_random_boxes_follow_the_rule(H, W):
    M = pkg("preprocess")
    scale, ratio = (0.8, 1.0), (3.0 / 4.0, 4.0 / 3.0)
    g = torch.Generator().manual_seed(5)
    boxes = M.random_resized_crop_boxes(4096, (H, W), scale, ratio, generator=g)
    assert boxes.dtype == torch.int32 and tuple(boxes.shape) == (4096, 4) and boxes.device.type == "cpu"
    fb = M.fallback_box((H, W), ratio)
    drawn = 0
    for t, l, h, w in boxes.tolist():
        assert t >= 0 and l >= 0 and h >= 1 and w >= 1 and t + h <= H and l + w <= W
        if (t, l, h, w) == fb:
            continue
        drawn += 1
        # h = round(hr), w = round(wr) with hr wr = area in [0.8, 1] H W and wr / hr in the ratio range: each side is
        # within 0.5 of its real value
        lo_area = max(h - 0.5, 0.0) * max(w - 0.5, 0.0)
        hi_area = (h + 0.5) * (w + 0.5)
        assert lo_area <= scale[1] * H * W and hi_area >= scale[0] * H * W, (t, l, h, w)
        assert (w - 0.5) / (h + 0.5) <= ratio[1] and (w + 0.5) / max(h - 0.5, 1e-9) >= ratio[0], (t, l, h, w)
    if W / H > ratio[1]:
        # a box with at least 0.8 of the area and a ratio of at most 4/3 is higher than sqrt(0.8 * 3/4 * H * W) > H when
        # W / H > 5/3, so it never fits a 16:9 frame: always the fallback, the centre crop clamped to the ratio range
        assert math.sqrt(scale[0] / ratio[1] * H * W) > H + 0.5
        assert drawn == 0 and fb == {(270, 480): (0, 60, 270, 360), (17, 200): (0, 88, 17, 23)}[(H, W)]
    else:
        assert drawn > 2048
        tops = boxes[:, 0].double()
        assert float(tops.min()) == 0.0      # positions cover their range from its first value on


def test_random_flips_are_flags():
    M = pkg("preprocess")
    g = torch.Generator().manual_seed(9)
    f = M.random_flips(4096, generator=g)
    assert f.dtype == torch.uint8 and tuple(f.shape) == (4096,) and set(f.tolist()) == {0, 1}
    share = float(f.double().mean())
    assert abs(share - 0.5) <= 5 * math.sqrt(0.25 / 4096)
    assert int(M.random_flips(64, p=0.0).sum()) == 0 and int(M.random_flips(64, p=1.0).sum()) == 64
    g1, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    assert torch.equal(M.random_flips(100, generator=g1), M.random_flips(100, generator=g2))
    assert torch.equal(M.random_resized_crop_boxes(100, (270, 480), generator=g1),
                       M.random_resized_crop_boxes(100, (270, 480), generator=g2))
