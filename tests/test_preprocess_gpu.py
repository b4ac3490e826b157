"""Frame preprocessing on the GPU (csrc/preprocess.hip, <pkg>/preprocess.py): the C ABI against the float64 reference and
the derived bound of tests/_preprocess_ref.py, then FramePreprocessor's surface."""
import ctypes
import functools

import pytest
import torch

import _preprocess_ref as R
from _util import pkg

pytestmark = pytest.mark.gpu
POISON = 12345.0
ALL_CASES = R.CASES + [R.IDENTITY]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def run(dev, frames, boxes, flips, hw, bgr=False, dst_pad=0, check=True):
    """qt_preprocess_u8 through ctypes on `frames` (a uint8 [N,H,W,3] CPU view with any row / image stride, copied to the
    device with its padding); the destination has dst_pad poisoned floats after every image.  Returns the CPU result."""
    M, Lm = pkg("preprocess"), pkg("_lib")
    L = Lm.lib()
    N, H, W, _ = frames.shape
    h, w = hw
    ims, rs = frames.stride(0), frames.stride(1)
    span = (N - 1) * ims + (H - 1) * rs + 3 * W
    host = frames.as_strided((span,), (1,), frames.storage_offset())
    src = host.to(dev)
    bx = None if boxes is None else torch.tensor(boxes, dtype=torch.int32, device=dev)
    fl = None if flips is None else torch.tensor(flips, dtype=torch.uint8, device=dev)
    ds = 3 * h * w + dst_pad
    dst = torch.full((N + 1, ds), POISON, device=dev)
    desc = M.PreprocessDesc(N, H, W, rs, ims, h, w, int(bgr), (ctypes.c_float * 3)(*R.MEAN32), (ctypes.c_float * 3)(*R.INV_STD32))
    st = L.qt_preprocess_u8(ctypes.byref(desc), src.data_ptr(), Lm.ptr(bx), Lm.ptr(fl), dst.data_ptr(), ds, Lm.stream_ptr())
    if check:
        Lm.check(st, "qt_preprocess_u8")
    torch.cuda.synchronize()
    out = dst.cpu()
    assert bool((out[:N, 3 * h * w:] == POISON).all()) and bool((out[N] == POISON).all()), "destination padding was written"
    assert torch.equal(src.cpu(), host), "the source was written"
    return out[:N, :3 * h * w].reshape(N, 3, h, w), st


@functools.lru_cache(maxsize=None)
def _case(i):
    """inputs and reference of one case, computed once and shared"""
    case = ALL_CASES[i]
    frames, boxes, hw = R.case_inputs(case, seed=i)
    return frames, boxes, hw, R.reference(frames, boxes, None, hw)


def _within(got, ref, bound, what):
    r = R.ratio(got, ref, bound)
    print(f"{what}: error / bound = {r:.3f}")
    assert r <= 1.0, (what, r)


@pytest.mark.parametrize("i", range(len(ALL_CASES)), ids=[c[0] for c in ALL_CASES])
def test_kernel_within_derived_bound(i):
    dev = _dev()
    frames, boxes, hw, (ref, bound, _) = _case(i)
    got, _ = run(dev, frames, boxes, None, hw)
    _within(got, ref, bound, ALL_CASES[i][0])


def test_box_equal_to_output_is_one_rounding():
    """weights are exactly {1, 0}: the value is the pixel itself and the output its normalisation rounded once"""
    dev = _dev()
    i = len(ALL_CASES) - 1
    frames, boxes, hw, _ = _case(i)
    got, _ = run(dev, frames, boxes, None, hw)
    t, l, bh, bw = boxes[0]
    px = frames[0, t:t + bh, l:l + bw, :].double().permute(2, 0, 1)
    m = torch.tensor(R.MEAN32, dtype=torch.float64).view(3, 1, 1)
    s = torch.tensor(R.INV_STD32, dtype=torch.float64).view(3, 1, 1)
    want = (px / 255.0 - m) * s
    # one rounding of scale = inv_std / 255, one of shift = -mean inv_std, one of the fused multiply-add
    tol = R.U * (2 * (px / 255.0 * s) + 2 * (m * s).abs())
    assert bool(((got[0].double() - want).abs() <= tol).all())


def test_batch_of_five_boxes_and_mixed_flips():
    dev = _dev()
    frames, _ = R.make_frames(5, 61, 83, 41)
    boxes = [(0, 0, 61, 83), (3, 9, 50, 70), (11, 2, 20, 81), (30, 40, 31, 43), (7, 7, 9, 11)]
    flips = [1, 0, 1, 1, 0]
    got, _ = run(dev, frames, boxes, flips, (18, 21))
    ref, bound, _ = R.reference(frames, boxes, flips, (18, 21))
    _within(got, ref, bound, "five boxes, mixed flips")
    unflipped, _ = run(dev, frames, boxes, None, (18, 21))
    for b, f in enumerate(flips):
        assert torch.equal(got[b], unflipped[b].flip(-1) if f else unflipped[b])      # a flip only reverses the columns


def test_bgr_source_against_channel_swapped_reference():
    dev = _dev()
    frames, boxes, hw, _ = _case(0)
    got, _ = run(dev, frames, boxes, None, hw, bgr=True)
    ref, bound, _ = R.reference(frames.flip(-1), boxes, None, hw)       # the same frames with their channels swapped, as RGB
    _within(got, ref, bound, "bgr")


def test_padded_strides_are_untouched_and_without_influence():
    dev = _dev()
    H, W, hw = 37, 53, (16, 23)
    boxes = [(1, 1, 33, 50), (0, 3, 37, 50), (4, 0, 30, 53)]
    padded, buf = R.make_frames(3, H, W, 77, row_pad=5, image_pad=7)     # odd strides: every row starts at another alignment
    assert int((buf == 255).sum()) >= 3 * (H * 5 + 7)
    dense = padded.contiguous()
    a, _ = run(dev, padded, boxes, [0, 1, 0], hw, dst_pad=3)             # run() checks both paddings
    b, _ = run(dev, dense, boxes, [0, 1, 0], hw)
    assert torch.equal(a, b)
    ref, bound, _ = R.reference(dense, boxes, [0, 1, 0], hw)
    _within(a, ref, bound, "padded strides")


def test_invalid_box_is_nan_and_neighbours_are_unaffected():
    dev = _dev()
    frames, _ = R.make_frames(3, 30, 40, 7)
    for bad in [(5, 5, 30, 30), (-1, 0, 10, 10), (0, 0, 0, 10), (0, 39, 10, 2), (0, 0, 10, -4), (2 ** 31 - 1, 0, 2 ** 31 - 1, 1)]:
        boxes = [(1, 2, 20, 30), bad, (0, 0, 30, 40)]
        got, _ = run(dev, frames, boxes, [1, 0, 1], (9, 70))
        ref, bound, _ = R.reference(frames, boxes, [1, 0, 1], (9, 70))
        assert bool(torch.isnan(got[1]).all()), bad
        assert bool(torch.isnan(ref[1]).all())
        _within(got, ref, bound, f"neighbours of {bad}")


def test_two_runs_are_bit_identical():
    dev = _dev()
    frames, boxes, hw, _ = _case(ALL_CASES.index(next(c for c in ALL_CASES if c[0] == "realistic")))
    a, _ = run(dev, frames, boxes, [0, 1], hw)
    b, _ = run(dev, frames, boxes, [0, 1], hw)
    assert torch.equal(a, b)


def test_downscale_beyond_the_limit_raises_before_launching():
    dev = _dev()
    P, M = pkg(), pkg("preprocess")
    lim = M.MAX_DOWNSCALE
    frames = torch.ones(1, lim * 2 + 1, 8, 3, dtype=torch.uint8)
    out, st = run(dev, frames, None, None, (2, 8), check=False)
    assert st == -3 and b"downscale limit" in pkg("_lib").lib().qt_last_error()
    assert bool((out == POISON).all())                                   # nothing was launched
    with pytest.raises(P.QtError, match="downscale limit"):
        P.FramePreprocessor(size=(2, 8))(frames.to(dev))
    ok, st = run(dev, torch.ones(1, lim * 2, 8, 3, dtype=torch.uint8), None, None, (2, 8))      # at the limit it runs
    assert st == 0 and bool(torch.isfinite(ok).all())


def test_no_host_synchronisation_during_the_call():
    dev = _dev()
    P = pkg()
    pre = P.FramePreprocessor(size=(24, 24))
    frames, _ = R.make_frames(4, 48, 64, 3)
    f = frames.to(dev)
    boxes = torch.tensor([(0, 0, 48, 64)] * 4, dtype=torch.int32, device=dev)
    flips = torch.tensor([0, 1, 0, 1], dtype=torch.uint8, device=dev)
    out = torch.empty(4, 3, 24, 24, device=dev)
    pre(f, boxes, flips, out=out)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pre(f, boxes, flips, out=out)
        fresh = pre(f, boxes, flips)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert torch.equal(out, fresh)


def test_frame_preprocessor_shapes_dtypes_and_views():
    dev = _dev()
    P = pkg()
    pre = P.FramePreprocessor(size=(20, 27))
    frames, _ = R.make_frames(6, 64, 80, 11)
    boxes = [(0, 0, 40, 50), (24, 30, 40, 50), (0, 30, 64, 50), (10, 0, 54, 80), (0, 0, 64, 80), (5, 6, 7, 8)]
    flips = [0, 1, 1, 0, 1, 0]
    ref, bound, _ = R.reference(frames, boxes, flips, (20, 27))
    f = frames.to(dev)
    bx = torch.tensor(boxes, dtype=torch.int32, device=dev)
    fl = torch.tensor(flips, dtype=torch.bool, device=dev)
    img = pre(f, bx, fl)
    assert img.dtype == torch.float32 and tuple(img.shape) == (6, 3, 20, 27) and img.is_contiguous() and img.device == f.device
    _within(img.cpu(), ref, bound, "images")
    clip = pre(f.view(2, 3, 64, 80, 3), bx.view(2, 3, 4), fl.view(2, 3))
    assert tuple(clip.shape) == (2, 3, 3, 20, 27) and clip.is_contiguous()
    assert torch.equal(clip.view(6, 3, 20, 27), img)
    # a view the descriptor can express (a column window of wider frames) goes through without a copy, one it cannot
    # (channels first in memory) is copied once: both give the dense result
    wide = torch.full((6, 64, 90, 3), 255, dtype=torch.uint8, device=dev)
    wide[:, :, 4:84] = f
    assert torch.equal(pre(wide[:, :, 4:84], bx, fl), img)
    chw = f.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    assert torch.equal(pre(chw, bx, fl), img)
    bgr = P.FramePreprocessor(size=(20, 27), channel_order="bgr")(f.flip(-1), bx, fl)
    assert torch.equal(bgr, img)
    whole = pre(f)
    assert tuple(whole.shape) == (6, 3, 20, 27) and bool(torch.isfinite(whole).all())
    for bad in (lambda: pre(f.float()), lambda: pre(f[..., :2]), lambda: pre(f, bx.long(), fl), lambda: pre(f, bx[:5], fl),
                lambda: pre(f, bx.cpu(), fl), lambda: pre(f, bx, fl.float()), lambda: pre(f, bx, fl, out=torch.empty(6, 3, 20, 28, device=dev))):
        with pytest.raises(P.QtError):
            bad()


def test_output_feeds_the_quadtree_model():
    dev = _dev()
    P = pkg()
    synth = pkg("synth")
    models = pkg("quadtree_from_scratch.models")
    model = models.get_model("quadtree", 12, dev, print_num_params=False)
    model.load_state_dict({k: v.to(dev) for k, v in synth.synth_state_dict(model).items()})
    model = model.eval()
    frames, _ = R.make_frames(2, 270, 480, 19)
    boxes = P.random_resized_crop_boxes(2, (270, 480), generator=torch.Generator().manual_seed(1)).to(dev)
    flips = P.random_flips(2, generator=torch.Generator().manual_seed(1)).to(dev)
    images = P.FramePreprocessor()(frames.to(dev), boxes, flips)
    assert tuple(images.shape) == (2, 3, 224, 224)
    with torch.no_grad():
        logits = model(images, synth.synth_pose_features(2, salt=3).to(dev))
    assert tuple(logits.shape) == (2, 12) and bool(torch.isfinite(logits).all())
