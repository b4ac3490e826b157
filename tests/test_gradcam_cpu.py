"""Grad-CAM without a GPU: the float64 reference of tests/_gradcam_ref.py against the reference's recipe, the conditions
that keep the GPU bound tests meaningful, the colour table, argument errors and the exports."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import _gradcam_ref as R
from _util import PKG, ROOT, pkg


def test_float64_reference_is_the_reference_recipe():
    for (B, C, P) in ((3, 70, 15), (2, 64, 1), (1, 8, 65)):
        for form in R.GRAD_FORMS:
            act, grad = R.make_inputs(B, C, P, form, seed=3)
            cam, peak = R.cam_ref(act, grad)
            assert np.abs(cam - R.cam_ref_torch(act, grad)).max() <= 1e-12
            assert cam.max(axis=1).tolist() == [1.0] * B and (peak > 0).all()
    # an image without a positive score: zeros, not the NaN of a division by a zero peak
    act, grad = R.make_inputs(2, 8, 9, "noisy", seed=1)
    grad[1] = -np.abs(grad[1])
    cam, peak = R.cam_ref(act, grad)
    assert peak[1] == 0.0 and not cam[1].any() and cam[0].max() == 1.0
    again = R.cam_ref_torch(act, grad)
    assert np.abs(cam - again).max() <= 1e-12 and not again[1].any()
    # the channel mean of Quadtree_from scratch/grad_cam.py:84 gives the same normalised map
    a, g = act[:1].astype(np.float64), grad[:1].astype(np.float64)
    mean_map = np.maximum((g.mean(axis=2)[:, :, None] * a).mean(axis=1), 0.0)
    assert np.abs(mean_map / mean_map.max() - cam[:1]).max() <= 1e-12


def test_reference_carries_nan_per_image():
    act, grad = R.make_inputs(3, 8, 9, "noisy", seed=2)
    act[1, 3, 4] = np.nan
    grad[2, 0, 0] = np.nan
    cam, peak = R.cam_ref(act, grad)
    assert np.isnan(cam[1]).all() and np.isnan(cam[2]).all() and np.isnan(peak[1:]).all()
    clean, _ = R.cam_ref(act[:1], grad[:1])
    assert np.array_equal(cam[0], clean[0]) and peak[0] > 0


@pytest.mark.parametrize("shape", R.MAP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_map_bound_is_below_one_colour_index(shape):
    """Non-vacuity of the GPU bound test: on every input set it uses (both gradient forms, seeds 0-7, also scaled by
    2^-40 and 2^40) the derived bound stays below 2^-10, less than one colour index."""
    B, C, P = shape
    worst = 0.0
    for form in R.GRAD_FORMS:
        for seed in range(8):
            act, grad = R.make_inputs(B, C, P, form, seed)
            bound, _ = R.cam_bound(act, grad)
            worst = max(worst, float(bound.max()))
            if seed == 0:
                for k in (-40, 40):
                    scaled, _ = R.cam_bound(np.ldexp(act, k), np.ldexp(grad, k))
                    assert np.allclose(scaled, bound, rtol=1e-9, atol=0.0)
    print(f"{shape}: largest bound {worst:.3e}")
    assert worst <= R.CAM_BOUND_CAP


def test_zero_mean_gradients_are_ill_conditioned():
    """why the bound test does not feed them: the pooled weights cancel and the bound exceeds the cap"""
    rng = np.random.default_rng(5)
    act = np.maximum(rng.standard_normal((1, 512, 49)), 0.0).astype(np.float32)
    grad = rng.standard_normal((1, 512, 49))
    grad = (grad - grad.mean(axis=2, keepdims=True) + 1e-7).astype(np.float32)
    bound, _ = R.cam_bound(act, grad)
    assert bound.max() > R.CAM_BOUND_CAP


def test_overlay_reference_and_admissible_indices():
    cam = R.make_cam(2, 5, 3, seed=1)
    # same size: the sample is the map itself; 1 x 1: one value everywhere
    assert np.array_equal(R.heat_ref(cam, 5, 3), cam.astype(np.float64))
    one = R.heat_ref(cam[:, :1, :1], 4, 6)
    assert (one == cam[:, :1, :1].astype(np.float64)).all()
    # against torch's bilinear interpolation with half-pixel centres (align_corners=False), in double
    want = torch.nn.functional.interpolate(torch.from_numpy(cam).double()[:, None], size=(37, 61), mode="bilinear",
                                           align_corners=False)[:, 0].numpy()
    assert np.abs(R.heat_ref(cam, 37, 61) - want).max() <= 1e-12
    for (H, W) in ((7, 9), (37, 61), (224, 224)):
        for hw in ((7, 7), (5, 3), (1, 1)):
            c = R.make_cam(2, *hw, seed=H + hw[0])
            lo, hi = R.admissible(c, H, W)
            assert (hi - lo).max() <= 1 and (lo >= 0).all() and (hi <= 255).all()
            assert float(R.heat_bound(c).max()) < 1e-5
    c = R.make_cam(2, 7, 7, seed=3)
    c[1] = np.nan
    lo, hi = R.admissible(c, 9, 9)
    assert not lo[1].any() and not hi[1].any() and np.isnan(R.heat_ref(c, 9, 9)[1]).all()
    # the checker refuses a wrong overlay
    frames, lut = R.make_frames(2, 9, 9, 4), pkg("gradcam").jet_lut().numpy()
    c = R.make_cam(2, 7, 7, seed=3)
    good = R.blend_ref(lut, lo * 0 + R.admissible(c, 9, 9)[0], frames, 0.4).astype(np.uint8)
    assert R.check_overlay(good, R.admissible(c, 9, 9), frames, lut, 0.4) <= 2
    bad = good.copy()
    bad[1, 4, 4, 2] ^= 0x40
    with pytest.raises(AssertionError):
        R.check_overlay(bad, R.admissible(c, 9, 9), frames, lut, 0.4)


def test_jet_lut():
    G = pkg("gradcam")
    rgb, bgr = G.jet_lut("rgb"), G.jet_lut()
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (256, 3) and rgb.device.type == "cpu"
    assert torch.equal(bgr, rgb.flip(1))
    assert rgb[0].tolist() == [0, 0, 128] and rgb[255].tolist() == [128, 0, 0]      # the documented ends
    r, g, b = (rgb[:, k].long() for k in range(3))
    d = lambda v: v[1:] - v[:-1]
    # each channel rises to a plateau of 255 and falls again: red over entries 160-223, green 96-159, blue 32-95
    for v, first, last in ((r, 160, 223), (g, 96, 159), (b, 32, 95)):
        assert (d(v)[:first] >= 0).all() and (v[first:last + 1] == 255).all() and (d(v)[last:] <= 0).all()
        assert v[first - 1] < 255 and v[last + 1] < 255
    assert r[:96].max() == 0 and g[:32].max() == 0 and g[224:].max() == 0 and b[160:].max() == 0
    with pytest.raises(ValueError):
        G.jet_lut("hsv")


def test_argument_errors_without_a_gpu():
    P, G = pkg(), pkg("gradcam")
    m = P.QuadtreeCNN(12)
    for alpha in (-0.1, 1.5, float("nan"), "x"):
        with pytest.raises(ValueError, match="alpha"):
            P.GradCAM(m, alpha=alpha)
    with pytest.raises(ValueError, match="lut"):
        P.GradCAM(m, lut=torch.zeros(256, 3))
    with pytest.raises(ValueError, match="numerical_only"):
        P.GradCAM(P.QuadtreeCNN(12, mode="numerical_only"))
    for unserved in (P.AttentionHierarchicalCNN(12), P.CnnLstm(12), P.Ji3DCNN(12), torch.nn.Linear(2, 2)):
        with pytest.raises(TypeError, match="unsupported model"):
            P.GradCAM(unserved)
    for served in (m, P.QuadtreeCNN(12, mode="image_only"), P.StandardResNetCNN(12), P.Quadtree3DCNN(12, sequence_length=4)):
        P.GradCAM(served)
    cam = P.GradCAM(m)
    hooks = lambda: (len(m.base_cnn.layer4._forward_hooks), len(m.base_cnn.layer4._backward_hooks))
    with pytest.raises(ValueError, match="AMD GPU"):
        cam.maps(torch.zeros(1, 3, 224, 224), torch.zeros(1, 47))
    with pytest.raises(ValueError, match="float32"):
        cam.maps(torch.zeros(1, 3, 224, 224, dtype=torch.float64))
    with pytest.raises(ValueError, match="AMD GPU"):
        cam.overlay(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 7, 7))
    with pytest.raises(ValueError, match="AMD GPU"):
        cam.explain(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="alpha"):
        cam.overlay(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 7, 7), alpha=2.0)
    with pytest.raises(ValueError, match="AMD GPU"):
        G.gradcam_map(torch.zeros(1, 4, 9), torch.zeros(1, 4, 9))
    assert hooks() == (0, 0) and m.training


def test_c_abi_refuses_before_any_launch():
    """every refusal below comes before the first device call: the pointers are not device memory"""
    G, Lm = pkg("gradcam"), pkg("_lib")
    L = Lm.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    limit = G.MAX_POSITIONS
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    assert f"#define QT_GRADCAM_MAX_POSITIONS {limit}" in header and limit >= 2048
    assert L.qt_gradcam_map(p, p, 1, 4, limit + 1, p, p, None, 0, None) == -3          # QT_ERR_UNSUPPORTED
    assert b"positions" in L.qt_last_error()
    assert L.qt_gradcam_workspace_bytes(1, 4, limit + 1) == 0
    assert L.qt_gradcam_map(p, p, 0, 4, 9, p, p, None, 0, None) == -1
    assert L.qt_gradcam_map(p, None, 1, 4, 9, p, p, None, 0, None) == -1
    assert L.qt_gradcam_map(p, p + 2, 1, 4, 9, p, p, None, 0, None) == -1
    need = L.qt_gradcam_workspace_bytes(2, 512, 49)
    assert need == 2 * 16 * 49 * 4 and L.qt_gradcam_workspace_bytes(2, 32, 49) == 0       # 32-channel chunks; one chunk: none
    assert L.qt_gradcam_map(p, p, 2, 512, 49, p, p, p, need - 4, None) == -1
    assert b"workspace" in L.qt_last_error()
    for alpha in (-0.5, 1.25, float("nan")):
        assert L.qt_gradcam_overlay_u8(p, 7, 7, p, 1, 8, 8, p, alpha, p, None, None, None) == -1
        assert b"alpha" in L.qt_last_error()
    assert L.qt_gradcam_overlay_u8(p, 7, 7, p, 1, 8, 0, p, 0.4, p, None, None, None) == -1
    assert L.qt_gradcam_overlay_u8(p, 7, 7, None, 1, 8, 8, p, 0.4, p, None, None, None) == -1
    assert L.qt_gradcam_overlay_u8(p, 7, 7, p, 1, 8, (1 << 22) + 1, p, 0.4, p, None, None, None) == -3


def test_exports():
    P = pkg()
    assert {"GradCAM", "jet_lut"} <= set(P.__all__)
    assert P.GradCAM is pkg("gradcam").GradCAM and P.jet_lut is pkg("gradcam").jet_lut
    for sub in ("resnet", "quadtree_from_scratch", "threed_cnn"):
        spec = importlib.util.spec_from_file_location(f"_dropin_{sub}_models", os.path.join(ROOT, PKG, sub, "models.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        assert mod.GradCAM is P.GradCAM and mod.jet_lut is P.jet_lut, sub
