"""Grad-CAM on the GPU (csrc/gradcam.hip, <pkg>/gradcam.py): the two kernels through the C ABI against the float64 rules and
the derived bounds of tests/_gradcam_ref.py, every pixel checked, then the GradCAM class on every served model."""
import functools

import numpy as np
import pytest
import torch

import _gradcam_ref as R
from _util import pkg

pytestmark = pytest.mark.gpu
POISON = 12345.0
POISON_U8 = 0xA5


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def run_map(dev, act, grad):
    """qt_gradcam_map through ctypes.  The map, the peaks and the workspace are followed by poisoned floats that must stay
    as they are, and the inputs must not be written.  Returns (cam [B,P], peak [B]) as f32 numpy."""
    G, Lm = pkg("gradcam"), pkg("_lib")
    L = Lm.lib()
    B, C, P = act.shape
    a, g = torch.from_numpy(act).to(dev), torch.from_numpy(grad).to(dev)
    a0, g0 = a.clone(), g.clone()
    cam = torch.full((B * P + 64,), POISON, device=dev)
    peak = torch.full((B + 64,), POISON, device=dev)
    ws_bytes = L.qt_gradcam_workspace_bytes(B, C, P)
    ws = torch.full((ws_bytes // 4 + 64,), POISON, device=dev)
    Lm.check(L.qt_gradcam_map(a.data_ptr(), g.data_ptr(), B, C, P, cam.data_ptr(), peak.data_ptr(),
                              Lm.ptr(ws) if ws_bytes else None, ws_bytes, Lm.stream_ptr()), "qt_gradcam_map")
    torch.cuda.synchronize()
    assert bool((cam[B * P:] == POISON).all()) and bool((peak[B:] == POISON).all()), "written behind the outputs"
    assert bool((ws[ws_bytes // 4:] == POISON).all()), "the workspace was overrun"
    assert torch.equal(a.view(torch.int32), a0.view(torch.int32)) and torch.equal(g.view(torch.int32), g0.view(torch.int32))
    return cam[:B * P].view(B, P).cpu().numpy(), peak[:B].cpu().numpy()


def _check_map(got, act, grad, what):
    cam, peak = got
    ref, ref_peak = R.cam_ref(act, grad)
    bound, peak_bound = R.cam_bound(act, grad)
    assert np.isfinite(bound).all() and bound.max() <= R.CAM_BOUND_CAP, what
    r = float((np.abs(cam - ref) / bound).max())
    rp = float((np.abs(peak - ref_peak) / peak_bound).max())
    print(f"{what}: map error / bound = {r:.3f} (bound {bound.max():.2e}), peak error / bound = {rp:.3f}")
    assert r <= 1.0 and rp <= 1.0, (what, r, rp)


@pytest.mark.parametrize("form", R.GRAD_FORMS)
@pytest.mark.parametrize("shape", R.MAP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_map_within_bound(shape, form):
    dev = _dev()
    act, grad = R.make_inputs(*shape, form, seed=0)
    _check_map(run_map(dev, act, grad), act, grad, f"{shape} {form}")
    for k in (-40, 40):   # the map is scale-free
        sa, sg = np.ldexp(act, k), np.ldexp(grad, k)
        _check_map(run_map(dev, sa, sg), sa, sg, f"{shape} {form} x 2^{k}")


@pytest.mark.parametrize("C", [32, 33])
def test_map_at_the_one_launch_threshold(C):
    """32 channels are one workgroup per image in one launch, 33 are two chunks and a finalize"""
    dev = _dev()
    for form in R.GRAD_FORMS:
        act, grad = R.make_inputs(2, C, 49, form, seed=0)
        _check_map(run_map(dev, act, grad), act, grad, f"C = {C} {form}")


def test_map_edge_cases():
    dev = _dev()
    act, grad = R.make_inputs(3, 70, 15, "noisy", seed=1)
    # an image whose s_p <= 0 everywhere (activations >= 0, every pooled weight <= 0): zeros and peak 0
    grad[1] = -np.abs(grad[1])
    cam, peak = run_map(dev, act, grad)
    assert peak[1] == 0.0 and not cam[1].any() and not np.signbit(cam[1]).any()
    again = run_map(dev, act, grad)
    assert cam.tobytes() == again[0].tobytes() and peak.tobytes() == again[1].tobytes()   # the same bits
    # one NaN element: that image all NaN, the others inside the bound (and the very bits of the run without it)
    for where in ("act", "grad"):
        a, g = R.make_inputs(3, 70, 15, "noisy", seed=2)
        clean = run_map(dev, a, g)
        (a if where == "act" else g)[1, 66, 7] = np.nan
        cam, peak = run_map(dev, a, g)
        assert np.isnan(cam[1]).all() and np.isnan(peak[1]), where
        keep = [0, 2]
        _check_map((cam[keep], peak[keep]), a[keep], g[keep], f"NaN in {where}, other images")
        assert np.array_equal(cam[keep], clean[0][keep]) and np.array_equal(peak[keep], clean[1][keep])


@pytest.mark.parametrize("shape", [(3, 512, 49), (3, 70, 15), (3, 5, 300)], ids=lambda s: "x".join(map(str, s)))
def test_map_of_a_batch_is_the_map_of_each_image(shape):
    dev = _dev()
    act, grad = R.make_inputs(*shape, "noisy", seed=4)
    cam, peak = run_map(dev, act, grad)
    for b in range(shape[0]):
        one, one_peak = run_map(dev, act[b:b + 1], grad[b:b + 1])
        assert np.array_equal(one[0], cam[b]) and one_peak[0] == peak[b], b


# ---- overlay ----------------------------------------------------------------------------------------------------------------
FRAME_SHAPES = ((1, 7, 9), (2, 37, 61), (1, 224, 224), (1, 1080, 1920))
MAP_HW = ((7, 7), (5, 3), (1, 1))


@functools.lru_cache(maxsize=None)
def _lut():
    return pkg("gradcam").jet_lut().numpy()


def run_overlay(dev, cam, frames, alpha, planes=False, off_out=0, off_src=0, off_planes=0, lut=None):
    """qt_gradcam_overlay_u8 through ctypes.  Frames, output, heat and index start `off_*` bytes (floats for heat) into a
    poisoned allocation and are followed by poison, which must stay; with planes=False the two planes are handed over as
    NULL and a poisoned stand-in shows that nothing else was written either.  Returns (out, heat, index) as numpy."""
    G, Lm = pkg("gradcam"), pkg("_lib")
    L = Lm.lib()
    B, H, W, _ = frames.shape
    n = B * H * W
    c = torch.from_numpy(cam).to(dev)
    table = torch.from_numpy(_lut() if lut is None else lut).to(dev)
    src = torch.full((off_src + 3 * n + 64,), POISON_U8, dtype=torch.uint8, device=dev)
    src[off_src:off_src + 3 * n] = torch.from_numpy(frames).to(dev).view(-1)
    src0 = src.clone()
    out = torch.full((off_out + 3 * n + 3 * W + 64,), POISON_U8, dtype=torch.uint8, device=dev)   # a row and more behind
    heat = torch.full((off_planes + n + 64,), POISON, device=dev)
    index = torch.full((off_planes + n + 64,), POISON_U8, dtype=torch.uint8, device=dev)
    Lm.check(L.qt_gradcam_overlay_u8(c.data_ptr(), cam.shape[1], cam.shape[2], src.data_ptr() + off_src, B, H, W, table.data_ptr(),
                                     alpha, out.data_ptr() + off_out, heat.data_ptr() + 4 * off_planes if planes else None,
                                     index.data_ptr() + off_planes if planes else None, Lm.stream_ptr()), "qt_gradcam_overlay_u8")
    torch.cuda.synchronize()
    assert torch.equal(src, src0), "the frames were written"
    assert bool((out[:off_out] == POISON_U8).all()) and bool((out[off_out + 3 * n:] == POISON_U8).all()), "written outside out"
    lo, hi = (off_planes, off_planes + n) if planes else (0, 0)
    assert bool((heat[:lo] == POISON).all()) and bool((heat[hi:] == POISON).all()), "written outside heat"
    assert bool((index[:lo] == POISON_U8).all()) and bool((index[hi:] == POISON_U8).all()), "written outside index"
    o = out[off_out:off_out + 3 * n].view(B, H, W, 3).cpu().numpy()
    if not planes:
        return o, None, None
    return o, heat[lo:hi].view(B, H, W).cpu().numpy(), index[lo:hi].view(B, H, W).cpu().numpy()


def _check_heat(heat, cam, what):
    ref, eps = R.heat_ref(cam, *heat.shape[1:]), R.heat_bound(cam)
    r = float((np.abs(heat - ref) / eps).max())
    print(f"{what}: heat error / bound = {r:.3f} (bound {float(eps.max()):.2e})")
    assert r <= 1.0, (what, r)


@pytest.mark.parametrize("hw", MAP_HW, ids=lambda s: "map%dx%d" % s)
@pytest.mark.parametrize("shape", FRAME_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_overlay(shape, hw):
    dev = _dev()
    B, H, W = shape
    cam, frames, lut = R.make_cam(B, *hw, seed=H + hw[1]), R.make_frames(B, H, W, seed=W), _lut()
    lohi = R.admissible(cam, H, W)
    # alpha 0.4 with both planes, 0.5 without
    out, heat, index = run_overlay(dev, cam, frames, 0.4, planes=True)
    _check_heat(heat, cam, f"{shape} {hw}")
    span = R.check_overlay(out, lohi, frames, lut, 0.4, index)
    print(f"{shape} {hw}: at most {span} admissible indices per pixel")
    again = run_overlay(dev, cam, frames, 0.4, planes=True)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip((out, heat, index), again))   # same bits
    half, _, _ = run_overlay(dev, cam, frames, 0.5)
    R.check_overlay(half, lohi, frames, lut, 0.5)
    # the exact cases
    same, _, _ = run_overlay(dev, cam, frames, 0.0)
    assert np.array_equal(same, frames)
    full, _, index1 = run_overlay(dev, cam, frames, 1.0, planes=True)
    assert np.array_equal(index1, index) and np.array_equal(full, lut[index1.astype(np.int64)])
    assert ((index1 >= lohi[0]) & (index1 <= lohi[1])).all()
    if hw == (1, 1):
        assert (index == index[:, :1, :1]).all() and (index[:, 0, 0] == 255).all()   # make_cam: the only value is the maximum


@pytest.mark.parametrize("off_out,off_src", [(1, 1), (7, 7), (13, 2), (0, 5), (16, 32)])
def test_overlay_at_any_alignment(off_out, off_src):
    """out's address decides where the 16-byte groups start; frames with another address modulo 16 are read bytewise"""
    dev = _dev()
    B, H, W = 2, 37, 61
    cam, frames, lut = R.make_cam(B, 5, 3, seed=9), R.make_frames(B, H, W, seed=10), _lut()
    lohi = R.admissible(cam, H, W)
    want = run_overlay(dev, cam, frames, 0.4, planes=True)
    got = run_overlay(dev, cam, frames, 0.4, planes=True, off_out=off_out, off_src=off_src, off_planes=off_out % 4 + 1)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(want, got))
    R.check_overlay(got[0], lohi, frames, lut, 0.4, got[2])


def test_overlay_small_and_nan():
    dev = _dev()
    lut = _lut()
    # fewer pixels than one 16-pixel group, and exactly the head
    for (B, H, W) in ((1, 1, 1), (1, 3, 5), (1, 1, 16)):
        cam, frames = R.make_cam(B, 5, 3, seed=H), R.make_frames(B, H, W, seed=W)
        out, heat, index = run_overlay(dev, cam, frames, 0.4, planes=True, off_out=3)
        R.check_overlay(out, R.admissible(cam, H, W), frames, lut, 0.4, index)
    # a NaN map (what qt_gradcam_map leaves for an image with a NaN): index 0 and NaN in heat, the other image unaffected
    cam, frames = R.make_cam(2, 7, 7, seed=5), R.make_frames(2, 37, 61, seed=6)
    clean = run_overlay(dev, cam, frames, 0.4, planes=True)
    cam[0] = np.nan
    out, heat, index = run_overlay(dev, cam, frames, 0.4, planes=True)
    assert np.isnan(heat[0]).all() and not index[0].any()
    assert all(np.array_equal(x[1], y[1]) for x, y in zip((out, heat, index), clean))
    R.check_overlay(out, R.admissible(cam, 37, 61), frames, lut, 0.4, index)


# ---- the class on the served models --------------------------------------------------------------------------------------
MODELS = ("resnet_fusion", "resnet_image_only", "from_scratch", "standard", "clip")


def _model(kind):
    """(model on the CPU with synthetic weights, image input, numerical input, uint8 frames, preprocessor or None)"""
    P, synth = pkg(), pkg("synth")
    if kind == "clip":
        m = P.Quadtree3DCNN(12, sequence_length=4, dropout_rate=0.5)
        B, T, HW = 2, 4, 64
        x = synth.synth_images(B * T, salt=51, size=HW).view(B, T, 3, HW, HW)
        f = synth.synth_pose_features(B * T, salt=51, realistic=True).view(B, T, 47)
        frames = torch.from_numpy(R.make_frames(B * T, 48, 80, seed=52)).view(B, T, 48, 80, 3)
        pre = P.FramePreprocessor(size=(HW, HW), channel_order="bgr")
    else:
        if kind == "standard":
            m = P.StandardResNetCNN(12)
        elif kind == "from_scratch":
            m = P.QuadtreeCNN(12, freeze_backbone=False)
        else:
            m = P.QuadtreeCNN(12, mode=kind[len("resnet_"):], freeze_backbone=True)
        x, f = synth.synth_images(3, salt=53), synth.synth_pose_features(3, salt=53)
        frames = torch.from_numpy(R.make_frames(3, 120, 90, seed=54))
        pre = None
        if kind in ("standard", "resnet_image_only"):
            f = None
    m.load_state_dict(synth.synth_state_dict(m))
    return m, x, f, frames, pre


@pytest.mark.parametrize("kind", MODELS)
def test_gradcam_on_model(kind):
    dev = _dev()
    P = pkg()
    m, x, f, frames, pre = _model(kind)
    m = m.to(dev).train()
    x, frames = x.to(dev), frames.to(dev)
    f = None if f is None else f.to(dev)
    hooked = m.conv3d_final_features if kind == "clip" else m.base_cnn.layer4
    params = list(m.parameters())
    marks = []
    for i, p in enumerate(params):     # every other parameter carries a gradient that must survive, the rest None
        p.grad = torch.full_like(p, float(i)) if i % 2 == 0 else None
        marks.append(p.grad)
    explainer = P.GradCAM(m)

    # a second, independent pair of hooks sees the tensors of the same call
    seen = {}
    h1 = hooked.register_forward_hook(lambda mod, i, o: seen.__setitem__("act", o.detach().clone()))
    h2 = hooked.register_full_backward_hook(lambda mod, gi, go: seen.__setitem__("grad", go[0].detach().clone()))
    cam, target, logits = explainer.maps(x, f)
    h1.remove()
    h2.remove()
    torch.cuda.synchronize()
    B = x.shape[0]
    act, grad = seen["act"].cpu().numpy(), seen["grad"].cpu().numpy()
    assert act.dtype == np.float32 and act.shape == grad.shape and act.shape[0] == B
    assert tuple(cam.shape) == (B,) + act.shape[2:] and cam.dtype == torch.float32 and cam.dim() == (4 if kind == "clip" else 3)
    C = act.shape[1]
    a3, g3 = act.reshape(B, C, -1), grad.reshape(B, C, -1)
    ref, _ = R.cam_ref(a3, g3)
    bound, _ = R.cam_bound(a3, g3)
    err = np.abs(cam.cpu().numpy().reshape(B, -1) - ref)
    print(f"{kind}: hook tensors {act.shape}, map error / bound = {float((err / bound).max()):.3f}, bound {bound.max():.2e}, "
          f"peaks {ref.max(axis=1)}")
    assert (err <= bound).all()
    assert target.dtype == torch.int64 and torch.equal(target, logits.argmax(1)) and not logits.requires_grad

    # the model is as it was
    assert m.training and not hooked._forward_hooks and not hooked._backward_hooks
    for p, g, i in zip(params, marks, range(len(params))):
        assert p.grad is g
        assert g is None or bool((g == float(i)).all())

    # a given class is honoured, as a tensor and as an int: the hooked gradient is that class's (another one than the
    # arg-max's; the normalised maps may coincide where one hidden unit carries every class), the map follows the rule
    other = (target + 1) % 12
    h2 = hooked.register_full_backward_hook(lambda mod, gi, go: seen.__setitem__("grad_other", go[0].detach().clone()))
    cam_t, target_t, logits_t = explainer.maps(x, f, target_class=other)
    h2.remove()
    assert torch.equal(target_t, other) and torch.equal(logits_t, logits)
    g_other = seen["grad_other"].cpu().numpy().reshape(B, C, -1)
    assert all(not np.array_equal(g_other[b], g3[b]) for b in range(B))
    ref_t, _ = R.cam_ref(a3, g_other)
    assert (np.abs(cam_t.cpu().numpy().reshape(B, -1) - ref_t) <= R.cam_bound(a3, g_other)[0]).all()
    k = int(other[0])
    cam_k, target_k, _ = explainer.maps(x, f, target_class=k)
    assert bool((target_k == k).all()) and torch.allclose(cam_k[0], cam_t[0], rtol=0.0, atol=1e-5)
    again, _, _ = explainer.maps(x, f)
    assert torch.equal(again, cam)

    # explain = preprocess, maps, overlay, bit for bit
    overlays, target_e, logits_e = explainer.explain(frames, f, preprocessor=pre)
    images = (pre or P.FramePreprocessor(channel_order="bgr"))(frames)
    cam_e, target_m, logits_m = explainer.maps(images, f)
    assert torch.equal(target_e, target_m) and torch.equal(logits_e, logits_m)
    if kind == "clip":
        t = cam_e.shape[1]
        assert tuple(overlays.shape) == (2, t, 48, 80, 3) and t == 1
        want = explainer.overlay(frames[:, 2], cam_e[:, 0])          # the centre frame of the four
        assert torch.equal(overlays[:, 0], want)
    else:
        assert tuple(overlays.shape) == tuple(frames.shape) and overlays.dtype == torch.uint8
        assert torch.equal(overlays, explainer.overlay(frames, cam_e))
    assert m.training and not hooked._forward_hooks


def test_maps_and_overlay_do_not_read_the_host():
    dev = _dev()
    P = pkg()
    m, x, f, frames, _ = _model("resnet_fusion")
    m = m.to(dev).eval()
    x, f, frames = x.to(dev), f.to(dev), frames.to(dev)
    explainer = P.GradCAM(m)
    other = torch.tensor([3, 1, 4], device=dev)
    cam, _, _ = explainer.maps(x, f)          # first launches outside the guarded region (code-object load, workspaces)
    explainer.overlay(frames, cam)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        cam2, target, _ = explainer.maps(x, f)
        cam3, _, _ = explainer.maps(x, f, target_class=other)
        cam4, _, _ = explainer.maps(x, f, target_class=5)
        out = explainer.overlay(frames, cam2)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert torch.equal(cam2, cam) and tuple(out.shape) == tuple(frames.shape)


def test_errors_on_the_device():
    dev = _dev()
    P = pkg()
    m, x, f, frames, _ = _model("resnet_fusion")
    m = m.to(dev)
    explainer = P.GradCAM(m)
    x, f, frames = x.to(dev), f.to(dev), frames.to(dev)
    with pytest.raises(ValueError, match="target_class"):
        explainer.maps(x, f, target_class=12)
    with pytest.raises(ValueError, match="target_class"):
        explainer.maps(x, f, target_class=torch.zeros(3, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="target_class"):
        explainer.maps(x, f, target_class=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="cam"):
        explainer.overlay(frames, torch.zeros(2, 7, 7, device=dev))
    with pytest.raises(ValueError, match="frames"):
        explainer.overlay(frames.float(), torch.zeros(3, 7, 7, device=dev))
    with pytest.raises(P.QtError, match="positions"):
        pkg("gradcam").gradcam_map(torch.zeros(1, 2, 4097, device=dev), torch.zeros(1, 2, 4097, device=dev))
    assert not m.base_cnn.layer4._forward_hooks and m.training
