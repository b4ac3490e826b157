"""d(loss)/d(clip) of the clip models and the Grad-CAM hooks of Quadtree3DCNN: qt_conv3d_first_dgrad (conv3d_block1's data
gradient down to the f32 clip, csrc/conv3d_first_dgrad.hip) behind `image_sequence.grad`, and the forward / full backward
hooks on `conv3d_final_features` (/root/reference/3dcnn/models.py:178-182), against torch autograd on the CPU
(oracle/quadtree_oracle.py).

Tolerances.  The kernel alone: 2e-4 of max|ref| for bf16 dy (the reference multiplies the same bf16-rounded operands in f32:
the products are exact, only the summation order differs -- the bound tests/test_clip3d_gpu.py holds the first layer's weight
gradient to), 1e-5 for f32.  The clip gradient of a whole model passes through every ReLU / max-pool decision of the conv
blocks, so it is held to the bars tests/test_input_grad_gpu.py applies to the 2-D image gradient: f32 build cosine >= 0.999
and max error <= 6e-2 of max|ref|; bf16 build cosine >= 0.85."""
import functools
import sys

import pytest
import torch
import torch.nn.functional as F

from _util import ROOT, pkg, rel_err

pytestmark = pytest.mark.gpu
LOGIT_TOL = {torch.float32: 1e-3, torch.bfloat16: 1e-2}   # tests/test_clip3d_gpu.py


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _oracle():
    sys.path.insert(0, ROOT)
    import oracle.quadtree_oracle as o
    return o


def _cos(a, b):
    a = a.double().ravel()
    b = b.double().ravel()
    return float(a @ b / max(float(a.norm() * b.norm()), 1e-300))


# ---- 1, 2. the kernel alone --------------------------------------------------------------------------------------------
def _run_kernel(dt, B, T, H, W):
    dev = _dev()
    L = pkg("_lib")
    lib = L.lib()
    g = torch.Generator().manual_seed(1000 * T + H + W)
    dy = torch.randn(B, 32, T, H, W, generator=g).to(dt).float()             # d(loss)/d(conv output), rounded to dt
    w = torch.randn(32, 3, 3, 3, 3, generator=g) * (2.0 / 81) ** 0.5
    x = torch.zeros(B, 3, T, H, W, requires_grad=True)
    (ref,) = torch.autograd.grad(F.conv3d(x, w.to(dt).float(), None, 1, 1), x, dy)
    ref = ref.permute(0, 2, 1, 3, 4).contiguous()                             # the clip's layout [B][T][3][H][W]
    dyd = dy.permute(2, 0, 3, 4, 1).contiguous().to(dev, dt)                  # [T][B][H][W][32]
    wd = w.to(dev)
    outs = []
    for _ in range(2):
        dx = torch.full((B, T, 3, H, W), float("nan"), device=dev)
        st = lib.qt_conv3d_first_dgrad(L.qt_dtype(dt), dyd.data_ptr(), wd.data_ptr(), dx.data_ptr(), B, T, H, W, L.stream_ptr())
        assert st == 0, lib.qt_last_error()
        torch.cuda.synchronize()
        outs.append(dx.cpu())
    assert not bool(torch.isnan(outs[0]).any())          # every element written, none from a neighbour's NaN
    assert torch.equal(outs[0], outs[1])                 # the same bits on every run
    err = rel_err(outs[0], ref)
    print(f"qt_conv3d_first_dgrad {dt} {(B, T, H, W)}: rel err {err:.2e}")
    return err


@pytest.mark.parametrize("shape", [(1, 1, 4, 16), (2, 3, 8, 32), (1, 5, 12, 64), (1, 2, 8, 256)])
def test_kernel_fast_form(shape):
    """bf16 MFMA form: T = 1 (both neighbour frames outside, one slab, one 16-pixel block), several clips and slabs, odd T,
    the widest row (three column tiles, the last one short)."""
    assert _run_kernel(torch.bfloat16, *shape) <= 2e-4


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(1, 2, 6, 20), (1, 1, 3, 5)])
def test_kernel_general_form(dt, shape):
    """the direct kernel: H no multiple of 4, W no multiple of 16; f32 dy for the f32 parity build"""
    assert _run_kernel(dt, *shape) <= (1e-5 if dt == torch.float32 else 2e-4)


# ---- 3. clip.grad of the whole models -----------------------------------------------------------------------------------
# the shapes of tests/test_clip3d_gpu.py::CASES at 64 x 64
CASES = [("q3_t8", 2, 8, 64, "quadtree_3d_fusion", 31), ("q3_t5", 2, 5, 64, "quadtree_3d_fusion", 31),
         ("q3_img_t8", 2, 8, 64, "quadtree_3d_image_only", 31), ("ji_t4", 2, 4, 64, None, 32)]


def _inputs(B, T, HW, salt):
    synth = pkg("synth")
    return (synth.synth_images(B * T, salt=salt, size=HW).view(B, T, 3, HW, HW),
            synth.synth_pose_features(B * T, salt=salt, realistic=True).view(B, T, 47), synth.synth_labels(B, 12, salt=salt))


def _build(mode, T, dt, dropout=0.0):
    P, synth = pkg(), pkg("synth")
    m = P.Ji3DCNN(12, sequence_length=T, dropout_rate=dropout, compute_dtype=dt) if mode is None else \
        P.Quadtree3DCNN(12, sequence_length=T, mode=mode, dropout_rate=dropout, compute_dtype=dt)
    m.load_state_dict(synth.synth_state_dict(m))
    return m


def _oracle_forward(mode, sd, x, f, train, taps=None):
    o = _oracle()
    if mode is None:
        return o.ji3d_forward(sd, x, f, train=train, dropout_p=0.0, taps=taps)
    return o.quadtree3d_forward(sd, x, f, mode=mode, train=train, dropout_p=0.0, taps=taps)


@functools.lru_cache(maxsize=None)
def _oracle_clip_grad(tag, train):
    """(logits, d(cross entropy)/d(clip)) of the CPU oracle: computed once per case, shared by both dtypes, never modified"""
    _, B, T, HW, mode, salt = next(c for c in CASES if c[0] == tag)
    x, f, y = _inputs(B, T, HW, salt)
    sd = _oracle().clip_params(_build(mode, T, torch.float32).state_dict())
    xr = x.clone().requires_grad_(True)
    ref = _oracle_forward(mode, sd, xr, f, train)
    F.cross_entropy(ref, y).backward()
    return ref.detach(), xr.grad.detach()


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("tag,B,T,HW,mode,salt", CASES)
def test_clip_grad_matches_oracle(tag, B, T, HW, mode, salt, dt, train):
    dev = _dev()
    x, f, y = _inputs(B, T, HW, salt)
    m = _build(mode, T, dt).to(dev).train(train)
    clip = x.to(dev).requires_grad_(True)
    logits = m(clip, f.to(dev))
    F.cross_entropy(logits, y.to(dev)).backward()
    torch.cuda.synchronize()
    assert clip.grad is not None
    assert clip.grad.shape == x.shape and clip.grad.dtype == torch.float32
    ref, gref = _oracle_clip_grad(tag, train)
    assert rel_err(logits.detach().cpu(), ref) <= LOGIT_TOL[dt]
    got = clip.grad.cpu()
    assert bool(torch.isfinite(got).all())
    # measured: f32 cosine >= 0.99991, max error <= 4.3e-2 (the cases where a ReLU / max-pool decision flips; 4e-6 where none
    # does); bf16 cosine 0.963 .. 0.991
    cos, err = _cos(got, gref), rel_err(got, gref)
    print(f"{tag} {dt} train={train}: clip gradient cosine {cos:.5f}, rel err {err:.2e}")
    if dt == torch.float32:
        assert cos >= 0.999 and err <= 6e-2, (cos, err)
    else:
        assert cos >= 0.85, (cos, err)


# ---- 4. parameter gradients are not disturbed ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", ["quadtree_3d_fusion", None], ids=["quadtree3d", "ji3d"])
def test_parameter_grads_bit_identical_with_clip_grad(dt, mode):
    """Parameter gradients with and without `requires_grad` on the clip are torch.equal.  The one exception is not the clip
    gradient's doing: the f32 build sums Conv3d weight gradients with float atomics (qt_conv2d_wgrad without a workspace), so
    those differ between two IDENTICAL runs too (measured: conv3d_block1 / 2 / 3.0.weight and visual_stream.0 / 2 / 4.0.weight
    differ between two runs without the clip gradient; the test prints the list).  A Conv3d weight gradient of the f32 build that is not bit-equal is therefore held
    to 1e-5 of its maximum (the order of f32 additions) -- the rule of tests/test_input_grad_gpu.py for the 2-D backbone;
    every other gradient, and every gradient of the bf16 build (fixed-order sums throughout), must be bit-identical."""
    dev = _dev()
    B, T, HW = 2, 4, 64
    x, f, y = (t.to(dev) for t in _inputs(B, T, HW, 35))
    m = _build(mode, T, dt)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.to(dev).train()
    runs = []
    for want_dx in (False, True, False):
        m.load_state_dict(sd0)
        m.zero_grad(set_to_none=True)
        clip = x.clone().requires_grad_(want_dx)
        logits = m(clip, f)
        F.cross_entropy(logits, y).backward()
        torch.cuda.synchronize()
        assert (clip.grad is not None) == want_dx
        runs.append((logits.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()}))
    (l0, g0), (l1, g1), (l2, g2) = runs
    assert torch.equal(l0, l1) and torch.equal(l0, l2)
    assert sorted(g0) == sorted(g1)
    unrepeatable = [n for n in g0 if not torch.equal(g0[n], g2[n])]
    print(f"{dt}: gradients that differ between two runs without the clip gradient: {unrepeatable}")
    for n in g0:
        if torch.equal(g0[n], g1[n]):
            continue
        assert dt == torch.float32 and g0[n].dim() == 5 and n.endswith(".0.weight"), n
        assert rel_err(g1[n].cpu(), g0[n].cpu()) <= 1e-5, n


# ---- 5. autograd.grad == .backward --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["quadtree_3d_fusion", None], ids=["quadtree3d", "ji3d"])
def test_autograd_grad_equals_backward_form(mode):
    dev = _dev()
    B, T, HW = 2, 4, 64
    x, f, _ = (t.to(dev) for t in _inputs(B, T, HW, 36))
    m = _build(mode, T, torch.bfloat16).to(dev).eval()
    one_hot = torch.zeros(B, 12, device=dev)
    one_hot[:, 3] = 1.0
    c1 = x.clone().requires_grad_(True)
    (g1,) = torch.autograd.grad(m(c1, f), c1, one_hot)
    c2 = x.clone().requires_grad_(True)
    m(c2, f).backward(one_hot)
    torch.cuda.synchronize()
    assert g1.shape == x.shape and torch.equal(g1, c2.grad)


# ---- 6. the Grad-CAM recipe ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_gradcam_hooks_on_conv3d_final_features(dt):
    dev = _dev()
    B, T, HW, mode = 2, 8, 64, "quadtree_3d_fusion"
    x, f, _ = _inputs(B, T, HW, 37)
    m = _build(mode, T, dt)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(dev).eval()
    h1 = m.conv3d_final_features.register_forward_hook(m.save_activation_hook)
    h2 = m.conv3d_final_features.register_full_backward_hook(m.save_gradient_hook)
    clip = x.to(dev).requires_grad_(True)
    logits = m(clip, f.to(dev))
    one_hot = torch.zeros_like(logits)
    one_hot[:, 3] = 1.0
    logits.backward(gradient=one_hot)
    torch.cuda.synchronize()
    h1.remove()
    h2.remove()
    taps = {}
    xr = x.clone().requires_grad_(True)
    ref = _oracle_forward(mode, sd, xr, f, False, taps)
    tap = taps["conv3d_final_features"]
    tap.retain_grad()
    ref.backward(gradient=one_hot.cpu())
    t, hw = T // 4, HW // 16                                   # pools (1,2,2) (2,2,2) (2,2,2) (1,2,2)
    assert tuple(tap.shape) == (B, m.cnn_3d_feature_dim, t, hw, hw)
    assert tuple(m.activations.shape) == tuple(tap.shape) and tuple(m.gradients.shape) == tuple(tap.shape)
    assert m.activations.dtype == torch.float32 and m.gradients.dtype == torch.float32
    ea, eg = rel_err(m.activations.cpu(), tap.detach()), rel_err(m.gradients.cpu(), tap.grad)
    print(f"Grad-CAM {dt}: activations rel err {ea:.2e}, gradients rel err {eg:.2e}")
    assert ea <= LOGIT_TOL[dt] and eg <= LOGIT_TOL[dt], (ea, eg)
    # the clip gradient is still produced in the same call
    assert clip.grad is not None and clip.grad.shape == x.shape
    cos = _cos(clip.grad.cpu(), xr.grad)
    assert cos >= (0.999 if dt == torch.float32 else 0.85), cos


# ---- 7. hooks elsewhere stay refused ------------------------------------------------------------------------------------
def test_hooks_on_other_submodules_still_raise():
    dev = _dev()
    QtError = pkg("_lib").QtError
    B, T, HW = 2, 4, 32
    x, f, _ = (t.to(dev) for t in _inputs(B, T, HW, 38))
    m = _build("quadtree_3d_fusion", T, torch.bfloat16).to(dev).eval()
    h = m.conv3d_block2.register_forward_hook(m.save_activation_hook)
    with pytest.raises(QtError):
        m(x, f)
    h.remove()
    h = m.conv3d_final_features[0].register_forward_hook(m.save_activation_hook)   # the conv inside the served block
    with pytest.raises(QtError):
        m(x, f)
    h.remove()
    ji = _build(None, T, torch.bfloat16).to(dev).eval()
    for mod in (ji.visual_stream, ji.visual_stream[4], ji.classifier):
        h = mod.register_forward_hook(lambda *a: None)
        with pytest.raises(QtError):
            ji(x, f)
        h.remove()
        h = mod.register_full_backward_hook(lambda *a: None)
        with pytest.raises(QtError):
            ji(x, f)
        h.remove()
    with torch.no_grad():
        assert torch.isfinite(ji(x, f)).all() and torch.isfinite(m(x, f)).all()   # with the hooks gone both run again
