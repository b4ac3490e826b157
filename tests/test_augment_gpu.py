"""Frame augmentation on the GPU (csrc/augment.hip, <pkg>/augment.py): the C ABI against the float64 reference and the
derived bound of tests/_augment_ref.py, stage by stage and as a whole, then FrameAugmenter's surface."""
import ctypes
import functools

import pytest
import torch

import _augment_ref as R
from _util import pkg

pytestmark = pytest.mark.gpu
POISON = 12345.0


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def run(dev, images, params, kx=1, ky=1, norm=R.NO_NORM, use_contrast=1, src_pad=0, dst_pad=0, check=True, spare_ws=None):
    """qt_augment_f32 through ctypes; the source has src_pad and the destination dst_pad poisoned floats after every image
    (and one poisoned image after the last).  spare_ws: a poisoned workspace handed over although use_contrast is 0.
    Returns the CPU result and the status."""
    M, Lm = pkg("augment"), pkg("_lib")
    L = Lm.lib()
    N, _, h, w = images.shape
    image = 3 * h * w
    src = torch.full((N, image + src_pad), POISON, device=dev)
    src[:, :image] = images.reshape(N, image).to(dev)
    src0 = src.clone()
    par = params.to(dev)
    dst = torch.full((N + 1, image + dst_pad), POISON, device=dev)
    ws_bytes = L.qt_augment_workspace_bytes(N, use_contrast)
    ws = torch.full((ws_bytes // 4 + 4,), POISON, device=dev) if ws_bytes else spare_ws
    desc = M.AugmentDesc(N, h, w, image + src_pad, image + dst_pad, kx, ky, (ctypes.c_float * 3)(*norm[0]),
                         (ctypes.c_float * 3)(*norm[1]), use_contrast)
    st = L.qt_augment_f32(ctypes.byref(desc), src.data_ptr(), par.data_ptr(), dst.data_ptr(), Lm.ptr(ws), ws_bytes, Lm.stream_ptr())
    if check:
        Lm.check(st, "qt_augment_f32")
    torch.cuda.synchronize()
    out = dst.cpu()
    assert bool((out[:N, image:] == POISON).all()) and bool((out[N] == POISON).all()), "destination padding was written"
    assert torch.equal(src.view(torch.int32), src0.view(torch.int32)), "the source was written"      # bits: a NaN source equals itself
    if ws is not None:
        assert bool((ws[ws_bytes // 4:] == POISON).all()), "the workspace was overrun"
    return out[:N, :image].reshape(N, 3, h, w), st


def _within(got, ref, bound, what, skip=None):
    r = R.ratio(got, ref, bound, skip)
    print(f"{what}: error / bound = {r:.3f}")
    assert r <= 1.0, (what, r)
    assert R.same_nan_pattern(got, ref), what


@functools.lru_cache(maxsize=None)
def _jitter_case(h, w):
    img, p = R.make_images(24, h, w, 11), R.jitter_rows()
    return img, p, R.reference(img, p)


@functools.lru_cache(maxsize=None)
def _chain_case(h, w):
    p = R.chain_rows(h, w)
    img = R.make_images(p.shape[0], h, w, 19)
    return img, p, R.reference(img, p, 5, 9, (R.MEAN32, R.INV_STD32))


@pytest.mark.parametrize("h,w", R.SHAPES)
def test_jitter_alone_all_24_orders(h, w):
    dev = _dev()
    img, p, (ref, bound, _) = _jitter_case(h, w)
    got, _ = run(dev, img, p)
    _within(got, ref, bound, f"jitter {h} x {w}")


@pytest.mark.parametrize("h,w", R.SHAPES)
def test_rotation_alone_is_a_copy(h, w):
    dev = _dev()
    img = R.make_images(len(R.ANGLES) + 1, h, w, 13) + 0.5          # no zero pixel: the fill is recognisable
    p = R.rows([R.row(deg=a) for a in R.ANGLES] + [R.row()])          # the last row: (cos, sin) = (1, 0)
    got, _ = run(dev, img, p, use_contrast=0)
    for n in range(len(R.ANGLES)):
        cs, sn = float(p[n, 8]), float(p[n, 9])
        und = R.undecided_mask(h, w, cs, sn)
        assert float(und.double().mean()) <= 0.01
        want = R.rotate(img[n].double(), cs, sn).float()
        keep = ~und
        assert torch.equal(got[n][:, keep], want[:, keep]), R.ANGLES[n]           # bit-equal to the pixel the reference names
        cands = [c.float() for c in R.rotation_candidates(img[n].double(), cs, sn)]
        hit = torch.stack([(got[n] == c).all(dim=0) for c in cands]).any(dim=0)
        assert bool(hit[und].all()), R.ANGLES[n]                                   # an undecided pixel equals a candidate
    assert torch.equal(got[-1], img[-1])                              # rotation off: bit-identical to the input


@pytest.mark.parametrize("h,w,kx,ky,sigma", [(18, 21, 5, 9, 0.1), (18, 21, 5, 9, 0.5), (33, 130, 5, 9, 0.1), (33, 130, 5, 9, 0.5),
                                             (33, 130, 15, 15, 3.0), (5, 3, 5, 9, 0.3)])
def test_blur_alone(h, w, kx, ky, sigma):
    dev = _dev()
    img = R.make_images(2, h, w, 17)
    p = R.rows([R.row(sigma=sigma)] * 2)
    ref, bound, _ = R.reference(img, p, kx, ky)
    got, _ = run(dev, img, p, kx, ky, use_contrast=0)
    _within(got, ref, bound, f"blur {kx} x {ky} sigma {sigma} at {h} x {w}")


def test_image_the_blur_reflects_beyond_is_refused_before_launching():
    dev = _dev()
    out, st = run(dev, R.make_images(1, 4, 3, 1), R.rows([R.row(sigma=0.3)]), 5, 9, check=False)
    assert st == -1 and b"reflects" in pkg("_lib").lib().qt_last_error()
    assert bool((out == POISON).all())                                 # nothing was launched


@pytest.mark.parametrize("h,w", R.CHAIN_SHAPES)
def test_whole_chain_with_the_reference_configuration(h, w):
    dev = _dev()
    img, p, (ref, bound, und) = _chain_case(h, w)
    assert not bool(und.any())
    got, _ = run(dev, img, p, 5, 9, (R.MEAN32, R.INV_STD32))
    _within(got, ref, bound, f"chain {h} x {w}")


def test_padded_strides_are_untouched_and_without_influence():
    dev = _dev()
    img, p, (ref, bound, _) = _chain_case(24, 40)
    a, _ = run(dev, img, p, 5, 9, (R.MEAN32, R.INV_STD32), src_pad=5, dst_pad=3)     # run() checks both paddings
    b, _ = run(dev, img, p, 5, 9, (R.MEAN32, R.INV_STD32))
    assert torch.equal(a, b)
    _within(a, ref, bound, "padded strides")


def test_two_runs_are_bit_identical():
    dev = _dev()
    img, p, _ = _chain_case(33, 130)
    a, _ = run(dev, img, p, 5, 9, (R.MEAN32, R.INV_STD32))
    b, _ = run(dev, img, p, 5, 9, (R.MEAN32, R.INV_STD32))
    assert torch.equal(a, b)


def _malformed_rows():
    inf, nan = float("inf"), float("nan")
    out = [R.row(b=nan, order=(0,)), R.row(hue=inf), R.row(order=(0, 0)), R.row(sigma=0.0), R.row(sigma=-1.0)]
    for slot in (4.0, 0.5):
        r = R.row()
        r[5] = slot
        out.append(r)
    return out


def test_malformed_rows_are_nan_and_neighbours_are_unaffected():
    dev = _dev()
    img = R.make_images(3, 18, 70, 29)
    good = [R.row(order=(0, 1), b=1.1, c=0.9, sigma=0.4), R.row(order=(3,), hue=0.05, sigma=0.2)]
    for bad in _malformed_rows():
        p = R.rows([good[0], bad, good[1]])
        ref, bound, _ = R.reference(img, p, 5, 9)
        got, _ = run(dev, img, p, 5, 9)
        assert bool(torch.isnan(got[1]).all()) and bool(torch.isnan(ref[1]).all()), bad
        _within(got, ref, bound, f"neighbours of {bad}")


def test_nan_image_is_nan_wherever_the_reference_is():
    dev = _dev()
    img, p = R.nan_case()
    ref, bound, _ = R.reference(img, p, 5, 9)
    nan = torch.isnan(ref[1])
    assert bool(nan.any()) and not bool(nan.all())
    got, _ = run(dev, img, p, 5, 9, use_contrast=0)
    _within(got, ref, bound, "NaN image")                              # _within compares the NaN pattern


def test_without_contrast_one_kernel_is_launched():
    dev = _dev()
    img = R.make_images(3, 18, 70, 31)
    p = R.rows([R.row(order=(0, 2, 3), b=1.2, s=0.8, hue=-0.1, sigma=0.3), R.row(order=(3, 0), b=0.8, hue=0.1, sigma=0.5),
                R.row(order=(2, 1), c=0.9, s=1.1, sigma=0.2)])          # the last row names contrast anyway: NaN
    ref, bound, _ = R.reference(img, p, 5, 9, use_contrast=False)
    assert bool(torch.isnan(ref[2]).all()) and bool(torch.isfinite(ref[:2]).all())
    # the contrast-mean launch writes all 16 partial sums of every image and nothing else does: a workspace handed over with
    # use_contrast = 0 stays as it was, so the one launch left is the main kernel
    spare = torch.full((3 * R.PARTS,), POISON, device=dev)
    got, _ = run(dev, img, p, 5, 9, use_contrast=0, spare_ws=spare)
    assert bool((spare == POISON).all())
    _within(got, ref, bound, "use_contrast = 0")
    M, Lm = pkg("augment"), pkg("_lib")
    L = Lm.lib()
    desc = M.AugmentDesc(3, 18, 70, 3 * 18 * 70, 3 * 18 * 70, 5, 9, (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1), 1)
    src, par, dst = img.to(dev), p.to(dev), torch.empty(3, 3, 18, 70, device=dev)
    Lm.check(L.qt_augment_f32(ctypes.byref(desc), src.data_ptr(), par.data_ptr(), dst.data_ptr(), spare.data_ptr(), 4 * 3 * R.PARTS,
                              Lm.stream_ptr()), "qt_augment_f32")
    torch.cuda.synchronize()
    assert bool((spare != POISON).all())                               # with use_contrast = 1 the first launch runs
    assert torch.equal(dst[:2].cpu(), got[:2]) and bool(torch.isfinite(dst[2]).all())


def test_frame_augmenter_surface_and_no_host_synchronisation():
    dev = _dev()
    P = pkg()
    aug = P.FrameAugmenter()
    img, p, (ref, bound, _) = _chain_case(24, 40)
    x, par = img.to(dev), p.to(dev)
    got = aug(x, par)
    assert got.dtype == torch.float32 and tuple(got.shape) == (4, 3, 24, 40) and got.is_contiguous() and got.device == x.device
    _within(got.cpu(), ref, bound, "FrameAugmenter")
    out = torch.empty_like(x)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        aug(x, par, out=out)
        fresh = aug(x, par)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert torch.equal(out, got) and torch.equal(fresh, got)
    clip = aug(x.view(2, 2, 3, 24, 40), par.view(2, 2, 12))          # 5-D clips equal the flattened batch
    assert tuple(clip.shape) == (2, 2, 3, 24, 40) and torch.equal(clip.view(4, 3, 24, 40), got)
    wide = torch.full((4, 3 * 24 * 40 + 8), POISON, device=dev)       # images one (padded) stride apart go through as they are
    view = wide[:, :3 * 24 * 40].view(4, 3, 24, 40)
    view.copy_(x)
    assert torch.equal(aug(view, par), got)
    assert torch.equal(aug(x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), par), got)      # anything else is copied once
    drawn = aug(x, aug.sample(4, generator=torch.Generator().manual_seed(1)).to(dev))
    assert bool(torch.isfinite(drawn).all())
    for bad in (lambda: aug(x.double(), par), lambda: aug(x[:, :2], par), lambda: aug(x, par.cpu()), lambda: aug(x, par[:3]),
                lambda: aug(x, par.double()), lambda: aug(x, par, out=x), lambda: aug(x, par, out=x.view(-1).view(4, 3, 24, 40)),
                lambda: aug(x, par, out=torch.empty(4, 3, 24, 41, device=dev)), lambda: aug(x[:, :, :4, :2], par)):
        with pytest.raises(P.QtError):
            bad()


def test_frames_to_logits_and_all_disabled_equals_the_preprocessor():
    dev = _dev()
    P = pkg()
    synth = pkg("synth")
    models = pkg("quadtree_from_scratch.models")
    import _preprocess_ref as PR
    frames, _ = PR.make_frames(2, 270, 480, 19)
    f = frames.to(dev)
    boxes = P.random_resized_crop_boxes(2, (270, 480), generator=torch.Generator().manual_seed(1)).to(dev)
    flips = P.random_flips(2, generator=torch.Generator().manual_seed(1)).to(dev)
    unit = P.FramePreprocessor(mean=0, std=1)(f, boxes, flips)
    assert float(unit.min()) >= 0.0 and float(unit.max()) <= 1.0 + 1e-6
    aug = P.FrameAugmenter()
    images = aug(unit, aug.sample(2, generator=torch.Generator().manual_seed(4)).to(dev))
    assert tuple(images.shape) == (2, 3, 224, 224) and bool(torch.isfinite(images).all())
    model = models.get_model("quadtree", 12, dev, print_num_params=False)
    model.load_state_dict({k: v.to(dev) for k, v in synth.synth_state_dict(model).items()})
    model = model.train()
    logits = model(images, synth.synth_pose_features(2, salt=3).to(dev))
    assert tuple(logits.shape) == (2, 12) and bool(torch.isfinite(logits).all())
    # every component disabled: the normalisation alone.  With X = unit * inv_std and C = |mean inv_std| the two paths differ
    # by the roundings of 1/255 and of unit (on X), of inv_std / 255 (on X) and of the two final fmas (on |X - C| each):
    # at most u (3 X + 2 |X - C|), which for ImageNet's statistics (X <= 4.5 < 6 C) is within two f32 roundings (2^-23 each)
    # of the magnitudes in play, 2 * 2^-23 (X + C)
    off = P.FrameAugmenter(0, 0, 0, 0, 0, None)
    plain = off(unit, off.sample(2).to(dev)).double().cpu()
    want = P.FramePreprocessor()(f, boxes, flips).double().cpu()
    s = torch.tensor(R.INV_STD32, dtype=torch.float64).view(1, 3, 1, 1)
    c = (torch.tensor(R.MEAN32, dtype=torch.float64).view(1, 3, 1, 1) * s).abs()
    tol = 2.0 * 2.0 ** -23 * (unit.double().cpu() * s + c)
    worst = float(((plain - want).abs() / tol).max())
    print(f"all disabled against FramePreprocessor(): error / (two roundings) = {worst:.3f}")
    assert worst <= 1.0
