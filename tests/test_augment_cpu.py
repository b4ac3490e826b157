"""Frame augmentation without a GPU: the float64 reference of tests/_augment_ref.py against torch's own ops, a torch-f32
restatement of the kernel's operation order against the derived bound (and a wrong version that must miss it), the tie
conditions the GPU tests rely on, FrameAugmenter.sample, and the refusals that need no device."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import _augment_ref as R
from _util import pkg


def test_blur_equals_conv2d_on_a_reflect_padded_image():
    for (h, w), (kx, ky), sigma in [((18, 21), (5, 9), 0.1), ((18, 21), (5, 9), 0.5), ((33, 130), (15, 15), 3.0), ((5, 3), (5, 9), 0.4)]:
        img = R.make_images(1, h, w, 3)[0].double()
        wx, wy = R.taps(kx, sigma)[0], R.taps(ky, sigma)[0]
        assert abs(float(wx.sum()) - 1.0) < 1e-15 and float(wx[kx // 2]) == float(wx.max())
        pad = F.pad(img.unsqueeze(0), (kx // 2, kx // 2, ky // 2, ky // 2), mode="reflect")
        k2 = (wy.view(ky, 1) * wx.view(1, kx)).expand(3, 1, ky, kx)
        want = F.conv2d(pad, k2, groups=3)[0]
        assert float((R.blur(img, kx, ky, sigma) - want).abs().max()) <= 1e-14


@pytest.mark.parametrize("deg", R.ANGLES)
@pytest.mark.parametrize("h,w", R.SHAPES + [(224, 224)])
def test_rotation_equals_grid_sample_nearest_and_few_pixels_are_undecided(h, w, deg):
    cs, sn = R.f32(math.cos(math.radians(deg))), R.f32(math.sin(math.radians(deg)))
    und = R.undecided_mask(h, w, cs, sn)
    share = float(und.double().mean())
    print(f"{deg} deg at {h} x {w}: {100 * share:.2f} % undecided")
    assert share <= 0.01                                   # the condition of the GPU test 'rotation alone is a copy'
    img = R.make_images(1, h, w, 5)[0].double() + 0.5      # no zero pixel: the fill is recognisable
    xf, yf = R.rotation_map(h, w, cs, sn)
    grid = torch.stack([(2.0 * xf + 1.0) / w - 1.0, (2.0 * yf + 1.0) / h - 1.0], dim=-1).unsqueeze(0)
    want = F.grid_sample(img.unsqueeze(0), grid, mode="nearest", padding_mode="zeros", align_corners=False)[0]
    got = R.rotate(img, cs, sn)
    keep = ~und
    assert torch.equal(got[:, keep], want[:, keep])
    assert bool((got[:, keep] == 0).any()) == (deg not in (180.0,))     # the corners are filled unless the image maps onto itself


def test_blend_ops_equal_their_one_line_forms():
    img = R.make_images(1, 18, 21, 7)[0].double()
    for f in (0.8, 1.2, 0.0, 1.0):
        f = R.f32(f)                                        # what the row carries
        p = R.rows([R.row(b=f, order=(0,)), R.row(c=f, order=(1,)), R.row(s=f, order=(2,))])
        ref, _, _ = R.reference(img.expand(3, 3, 18, 21), p)
        g = (0.2989 * img[0] + 0.587 * img[1] + 0.114 * img[2])
        assert torch.equal(ref[0], (f * img).clamp(0, 1))
        assert float((ref[1] - (f * img + (1 - f) * g.mean()).clamp(0, 1)).abs().max()) <= 1e-15
        assert float((ref[2] - (f * img + (1 - f) * g).clamp(0, 1)).abs().max()) <= 1e-15


def test_hue_round_trip_with_shift_zero_returns_the_input():
    img = R.make_images(2, 18, 21, 9).double()
    for b in range(2):
        assert float((R.hue(img[b], 0.0) - img[b]).abs().max()) <= 1e-14
        full = R.hue(R.hue(img[b], 0.3), 0.7)              # a whole turn in two steps
        assert float((full - img[b]).abs().max()) <= 1e-13
    red = torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64).view(3, 1, 1)
    assert float((R.hue(red, 1.0 / 3.0) - torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64).view(3, 1, 1)).abs().max()) <= 1e-14


def test_hue_is_seven_lipschitz_near_grey():
    """the constant the bound rests on, tried where h is ill-conditioned"""
    g = torch.Generator().manual_seed(1)
    base = torch.rand(1, 1, 4000, generator=g, dtype=torch.float64).expand(3, 1, 4000)
    for scale in (1e-3, 1e-6, 1e-9):
        a = (base + scale * torch.rand(3, 1, 4000, generator=g, dtype=torch.float64)).clamp(0, 1)
        d = 1e-3 * scale * (2 * torch.rand(3, 1, 4000, generator=g, dtype=torch.float64) - 1)
        for shift in (0.1, -0.1, 0.37):
            moved = (R.hue((a + d).clamp(0, 1), shift) - R.hue(a, shift)).abs().max(dim=0).values
            assert bool((moved <= R.HUE_LIP * d.abs().max(dim=0).values + 1e-15).all())


# ---------------------------------------------------------------------------------------------------------------------
# the f32 restatement against the bound, on the cases of the GPU test
# ---------------------------------------------------------------------------------------------------------------------
def _within(got, ref, bound, what, skip=None):
    r = R.ratio(got, ref, bound, skip)
    print(f"{what}: error / bound = {r:.3f}")
    assert r <= 1.0, (what, r)
    assert R.same_nan_pattern(got, ref)


@pytest.mark.parametrize("h,w", R.SHAPES)
def test_f32_restatement_of_the_jitter_stage(h, w):
    img, p = R.make_images(24, h, w, 11), R.jitter_rows()
    ref, bound, _ = R.reference(img, p)
    _within(R.kernel_f32(img, p), ref, bound, f"jitter {h} x {w}")
    wrong = R.ratio(R.kernel_f32(img, p, hue_sector_bug=True), ref, bound)
    assert wrong > 1.0                                                   # the bound is not loose


@pytest.mark.parametrize("h,w", R.SHAPES)
def test_f32_restatement_of_the_rotation_stage(h, w):
    img = R.make_images(len(R.ANGLES), h, w, 13)
    p = R.rows([R.row(deg=a) for a in R.ANGLES])
    ref, bound, und = R.reference(img, p)
    got = R.kernel_f32(img, p)
    keep = ~und.unsqueeze(1).expand_as(ref)
    assert torch.equal(got[keep].double(), ref[keep])                    # a copy: no rounding anywhere


@pytest.mark.parametrize("h,w,kx,ky,sigma", [(18, 21, 5, 9, 0.1), (18, 21, 5, 9, 0.5), (33, 130, 5, 9, 0.1), (33, 130, 5, 9, 0.5),
                                             (33, 130, 15, 15, 3.0), (5, 3, 5, 9, 0.3)])
def test_f32_restatement_of_the_blur_stage(h, w, kx, ky, sigma):
    img = R.make_images(2, h, w, 17)
    p = R.rows([R.row(sigma=sigma)] * 2)
    ref, bound, _ = R.reference(img, p, kx, ky)
    _within(R.kernel_f32(img, p, kx, ky), ref, bound, f"blur {kx} x {ky} sigma {sigma} at {h} x {w}")
    assert float((bound / ref.abs().clamp_min(1e-3)).max()) < 1e-4      # and stays a rounding-level bound


@pytest.mark.parametrize("h,w", R.CHAIN_SHAPES)
def test_f32_restatement_of_the_whole_chain(h, w):
    p = R.chain_rows(h, w)
    img = R.make_images(p.shape[0], h, w, 19)
    ref, bound, und = R.reference(img, p, 5, 9, (R.MEAN32, R.INV_STD32))
    assert not bool(und.any())                                           # the searched angles leave nothing undecided
    for cs, sn in R.decided_angles(h, w):
        assert 1.0 < abs(math.degrees(math.atan2(sn, cs))) <= 10.0
    _within(R.kernel_f32(img, p, 5, 9, (R.MEAN32, R.INV_STD32)), ref, bound, f"chain {h} x {w}")
    print(f"largest bound {float(bound.max()):.3e}")
    assert float(bound.max()) < 1e-3


def test_malformed_rows_and_nan_images_in_the_reference():
    img = R.make_images(3, 18, 21, 23)
    for bad in _malformed_rows():
        p = R.rows([R.row(order=(0, 1), b=1.1), bad, R.row(order=(3,), hue=0.05)])
        ref, _, _ = R.reference(img, p, 5, 9)
        assert bool(torch.isnan(ref[1]).all()) and bool(torch.isfinite(ref[0]).all()) and bool(torch.isfinite(ref[2]).all())
    ref, _, _ = R.reference(img, R.rows([R.row(order=(1,), c=0.9)] * 3), use_contrast=False)
    assert bool(torch.isnan(ref).all())
    img, p = R.nan_case()
    ref, _, und = R.reference(img, p, 5, 9)
    assert not bool(und.any())
    nan = torch.isnan(ref[1])
    assert bool(nan.any()) and not bool(nan.all())                       # the fill away from the blur's reach stays 0
    assert torch.equal(R.kernel_f32(img, p, 5, 9).isnan(), ref.isnan())


def _malformed_rows():
    inf, nan = float("inf"), float("nan")
    out = [R.row(b=nan, order=(0,)), R.row(hue=inf), R.row(order=(0, 0)), R.row(order=(2, 1, 2)), R.row(sigma=0.0), R.row(sigma=-1.0),
           R.row(cs=nan)]
    for slot in (4.0, 0.5, -2.0):
        r = R.row()
        r[5] = slot
        out.append(r)
    r = R.row()
    r[11] = nan
    out.append(r)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# FrameAugmenter.sample
# ---------------------------------------------------------------------------------------------------------------------
def test_sample_follows_the_rule():
    P = pkg()
    aug = P.FrameAugmenter()
    g = torch.Generator().manual_seed(5)
    p = aug.sample(4096, generator=g)
    assert p.dtype == torch.float32 and tuple(p.shape) == (4096, 12) and p.device.type == "cpu" and p.is_contiguous()
    for col, (lo, hi) in enumerate([(0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.1, 0.1)]):
        assert lo - 1e-6 <= float(p[:, col].min()) < lo + 0.01 and hi - 0.01 < float(p[:, col].max()) <= hi + 1e-6
    slots = p[:, 4:8]
    assert torch.equal(slots.sort(dim=1).values, torch.tensor([0.0, 1.0, 2.0, 3.0]).expand(4096, 4))
    seen = {tuple(int(x) for x in r) for r in slots.tolist()}
    assert len(seen) == 24                                               # every order occurs
    first = torch.bincount(slots[:, 0].long(), minlength=4).double() / 4096
    assert float((first - 0.25).abs().max()) <= 5 * math.sqrt(0.25 * 0.75 / 4096)
    ang = torch.atan2(p[:, 9].double(), p[:, 8].double()) * 180.0 / math.pi
    assert -10.0 - 1e-4 <= float(ang.min()) < -9.9 and 9.9 < float(ang.max()) <= 10.0 + 1e-4
    assert float((p[:, 8].double() ** 2 + p[:, 9].double() ** 2 - 1).abs().max()) < 1e-6
    assert 0.1 - 1e-6 <= float(p[:, 10].min()) < 0.11 and 0.49 < float(p[:, 10].max()) <= 0.5 + 1e-6
    assert bool((p[:, 11] == 0).all())
    assert all(R.row_valid(r, True) for r in p[:64].tolist())
    g1, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    assert torch.equal(aug.sample(100, generator=g1), aug.sample(100, generator=g2))


def test_sample_with_disabled_components():
    P = pkg()
    aug = P.FrameAugmenter(brightness=0, contrast=None, hue=0.05, degrees=0, blur_kernel=None)
    assert aug.blur_kernel == (1, 1) and aug.enabled_ops == [2, 3]
    p = aug.sample(512, generator=torch.Generator().manual_seed(2))
    assert torch.equal(p[:, 4:6].sort(dim=1).values, torch.tensor([2.0, 3.0]).expand(512, 2))
    assert bool((p[:, 6:8] == -1).all())
    assert 0.3 < float((p[:, 4] == 2).double().mean()) < 0.7
    assert bool((p[:, 8] == 1).all()) and bool((p[:, 9] == 0).all()) and bool((p[:, 10] > 0).all())
    off = P.FrameAugmenter(0, 0, 0, 0, 0, (1, 1)).sample(8)
    assert bool((off[:, 4:8] == -1).all()) and bool((off[:, 8] == 1).all()) and bool((off[:, 9] == 0).all())
    for bad in (dict(hue=0.6), dict(brightness=-0.1), dict(blur_kernel=(4, 9)), dict(blur_kernel=17), dict(blur_sigma=(0.5, 0.1)),
                dict(blur_sigma=(0.0, 0.1)), dict(std=(0.2, 0.0, 0.2))):
        with pytest.raises(ValueError):
            P.FrameAugmenter(**bad)


# ---------------------------------------------------------------------------------------------------------------------
# refusals before any device call
# ---------------------------------------------------------------------------------------------------------------------
def _desc(M, **kw):
    d = dict(batch=2, h=24, w=40, src_image_stride=3 * 24 * 40, dst_image_stride=3 * 24 * 40, blur_kx=5, blur_ky=9, use_contrast=1)
    d.update(kw)
    return M.AugmentDesc(d["batch"], d["h"], d["w"], d["src_image_stride"], d["dst_image_stride"], d["blur_kx"], d["blur_ky"],
                         (ctypes.c_float * 3)(*R.MEAN32), (ctypes.c_float * 3)(*R.INV_STD32), d["use_contrast"])


def test_descriptor_validation_needs_no_device():
    """every refusal comes with a message and before any HIP call: the pointers are never dereferenced"""
    M, Lm = pkg("augment"), pkg("_lib")
    L = Lm.lib()
    src, par, dst, ws = (ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20), ctypes.c_void_p(3 << 20), ctypes.c_void_p(4 << 20))
    need = L.qt_augment_workspace_bytes(2, 1)
    assert need == 2 * 16 * 4 and L.qt_augment_workspace_bytes(2, 0) == 0

    def call(desc, src=src, par=par, dst=dst, ws=ws, ws_bytes=need):
        return L.qt_augment_f32(ctypes.byref(desc) if desc is not None else None, src, par, dst, ws, ws_bytes, None)

    image = 3 * 24 * 40
    invalid = [("batch", 0), ("h", 0), ("w", -1), ("blur_kx", 4), ("blur_ky", 17), ("blur_kx", 0), ("blur_ky", -3),
               ("src_image_stride", image - 1), ("dst_image_stride", image - 1), ("use_contrast", 2)]
    for field, bad in invalid:
        assert call(_desc(M, **{field: bad})) == -1, field                 # QT_ERR_INVALID_ARG
        assert b"qt_augment_f32" in L.qt_last_error(), field
    assert call(None) == -1
    for name in ("src", "par", "dst"):
        assert call(_desc(M), **{name: None}) == -1 and b"null" in L.qt_last_error()
        assert call(_desc(M), **{name: ctypes.c_void_p((1 << 20) + 2)}) == -1 and b"aligned" in L.qt_last_error()
    assert call(_desc(M), ws=None) == -1 and b"workspace" in L.qt_last_error()
    assert call(_desc(M), ws_bytes=need - 1) == -1 and b"workspace" in L.qt_last_error()
    # the blur must not reflect beyond the image: 5 x 3 is the least a (5, 9) kernel takes
    assert call(_desc(M, h=4, w=3, src_image_stride=36, dst_image_stride=36)) == -1 and b"reflects" in L.qt_last_error()
    assert call(_desc(M, h=5, w=2, src_image_stride=30, dst_image_stride=30)) == -1 and b"reflects" in L.qt_last_error()
    # source and destination that overlap: the same pointer, and a destination that starts inside the last source image
    assert call(_desc(M), dst=src) == -1 and b"overlap" in L.qt_last_error()
    assert call(_desc(M), dst=ctypes.c_void_p((1 << 20) + 4 * (2 * image - 1))) == -1 and b"overlap" in L.qt_last_error()
    assert call(_desc(M), src=ctypes.c_void_p((3 << 20) + 4 * image), dst=dst) == -1 and b"overlap" in L.qt_last_error()
    # sizes above 2^22: QT_ERR_UNSUPPORTED
    big = (1 << 22) + 1
    assert call(_desc(M, w=big, src_image_stride=3 * 24 * big, dst_image_stride=3 * 24 * big)) == -3
    assert b"at most" in L.qt_last_error()
    assert call(_desc(M, h=big, src_image_stride=3 * 40 * big, dst_image_stride=3 * 40 * big)) == -3


def test_frame_augmenter_refuses_before_device_work():
    P = pkg()
    aug = P.FrameAugmenter()
    with pytest.raises(P.QtError, match="AMD GPU"):
        aug(torch.zeros(1, 3, 8, 8), aug.sample(1))
    with pytest.raises(P.QtError):
        aug("images", aug.sample(1))
    assert "FrameAugmenter" in P.__all__ and P.FrameAugmenter is pkg("augment").FrameAugmenter
