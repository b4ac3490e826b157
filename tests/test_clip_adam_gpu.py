"""Global-norm gradient clipping inside FusedAdam (csrc/grad_norm.hip, the *_scaled Adam entry points,
qt_plan_adam_step_clipped, FusedAdam(max_grad_norm=...)).

* the norm kernel against a float64 norm on the CPU, its coefficient against torch's formula bit for bit, two runs
  bit for bit;
* the multi-tensor Adam kernel with the coefficient read from device memory against torch.optim.Adam on pre-scaled
  gradients; a null pointer gives the bits of qt_adam_multi;
* whole optimizer steps: a coefficient of exactly 1 changes nothing, an active one matches
  torch.nn.utils.clip_grad_norm_ + the unclipped FusedAdam on a twin model (plan path, clip-model path), frozen
  parameters stay out of the norm.

Bounds.  Norm: 1e-5 relative.  An f32 tree sum of n <= 2^25 non-negative terms errs by at most about
log2(n) * 2^-24 = 1.5e-6 relative, the square root halves that, and the rest is room for the 32-term serial part of
every thread.  Adam arithmetic: the 2e-6 of test_model_gpu.py::test_adam_multi_kernel_*.  Twin models: 2e-6 * max|p|
per tensor, logits 1e-5 (tests/_util.rel_err, the project's parity metric).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from _util import pkg, rel_err

pytestmark = pytest.mark.gpu

NORM_TOL = 1e-5
ADAM_TOL = 2e-6


def _dev():
    return torch.device("cuda:0")


def _api():
    L = pkg("_lib")
    lib = L.lib()
    return L, lib, pkg("engine")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- tensor lists: (name, [(numel, storage offset in elements)]) -------------------------------------------------------
_MIXED49 = [((7 * i) % 61 + 1, 0) for i in range(46)] + [(5000, 0), (8192, 0), (8193, 0)]
LISTS = {
    "one": [(1, 0)],
    "three": [(3, 0)],
    "around_256": [(255, 0), (256, 0), (257, 0)],
    "chunks": [(4097, 0), (1, 0), ((1 << 20) + 3, 0)],
    "mixed49": _MIXED49,                                   # crosses the 48-tensors-per-launch boundary
    "unaligned": [(20001, 1), (2, 3), (1, 2), (8192 + 3, 1), (8192 + 4, 1)],   # pointers 4-, not 16-byte aligned
}
_cache = {}


def _tensors(name):
    """The list's tensors on the host (made once, never modified): randn times per-tensor scales from 1e-3 to 1e3."""
    if name not in _cache:
        g = torch.Generator().manual_seed(len(name) * 131 + 7)
        spec = LISTS[name]
        out = []
        for j, (n, _) in enumerate(spec):
            scale = 10.0 ** (-3.0 + 6.0 * j / max(len(spec) - 1, 1))
            out.append(torch.randn(n, generator=g) * scale)
        ref = torch.sqrt(sum((t.double() ** 2).sum() for t in out))
        _cache[name] = (out, float(ref))
    return _cache[name]


def _on_device(name):
    """Device copies honouring the storage offsets (the caching allocator hands out 512-byte aligned blocks)."""
    host, _ = _tensors(name)
    out = []
    for t, (n, off) in zip(host, LISTS[name]):
        buf = torch.empty(n + off, device=_dev())
        view = buf[off:]
        view.copy_(t)
        assert view.data_ptr() % 16 == (off * 4) % 16
        out.append(view)
    return out


def _norm(lib, L, eng, tensors, max_norm):
    items = (eng.AdamItem * len(tensors))(*[eng.AdamItem(None, t.data_ptr(), None, None, t.numel()) for t in tensors])
    need = lib.qt_grad_norm_workspace_bytes(items, len(tensors))
    assert need > 0 and need % 4 == 0
    ws = torch.full((need // 4,), float("nan"), device=_dev())      # nothing needs zeroing: every slot is written
    out = torch.full((2,), float("nan"), device=_dev())
    L.check(lib.qt_grad_norm_multi(items, len(tensors), max_norm, ws.data_ptr(), need, out.data_ptr(), L.stream_ptr()),
            "qt_grad_norm_multi")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("max_norm", [1.0, 1e30])
@pytest.mark.parametrize("name", list(LISTS))
def test_norm_kernel_against_float64(name, max_norm):
    L, lib, eng = _api()
    tensors = _on_device(name)
    _, ref = _tensors(name)
    a = _norm(lib, L, eng, tensors, max_norm)
    b = _norm(lib, L, eng, tensors, max_norm)
    err = abs(float(a[0]) - ref) / ref
    print(f"{name}: norm {float(a[0]):.9g}, float64 {ref:.9g}, rel err {err:.2e}, coef {float(a[1]):.9g}")
    assert err <= NORM_TOL
    # torch.nn.utils.clip_grad_norm_'s own lines, in f32, on the kernel's norm
    expect = torch.clamp(max_norm / (a[0] + 1e-6), max=1.0)
    assert expect.dtype == torch.float32
    assert torch.equal(_bits(a[1]), _bits(expect)), (float(a[1]), float(expect))
    if max_norm == 1e30:
        assert float(a[1]) == 1.0
    assert torch.equal(_bits(a), _bits(b))


def test_grad_norm_function_skips_parameters_without_gradient():
    P = pkg()
    ps = [torch.nn.Parameter(torch.zeros(n, device=_dev())) for n in (5, 300, 9000)]
    g = torch.Generator().manual_seed(3)
    ps[0].grad = torch.randn(5, generator=g).to(_dev())
    ps[2].grad = torch.randn(9000, generator=g).to(_dev())
    n = P.grad_norm(ps)
    assert n.dim() == 0 and n.dtype == torch.float32 and n.device.type == "cuda"
    ref = float(torch.sqrt((ps[0].grad.double() ** 2).sum() + (ps[2].grad.double() ** 2).sum()))
    assert abs(float(n) - ref) / ref <= NORM_TOL
    assert abs(float(P.grad_norm(ps[2])) - float(ps[2].grad.double().norm())) / ref <= NORM_TOL


# ---- multi-tensor Adam with the device coefficient -------------------------------------------------------------------
HYPER = dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.02)


def _adam_items(eng, ps, gs, ms, vs):
    return (eng.AdamItem * len(ps))(*[eng.AdamItem(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel())
                                      for p, g, m, v in zip(ps, gs, ms, vs)])


@pytest.mark.parametrize("name", list(LISTS))
def test_adam_multi_with_device_coefficient(name):
    L, lib, eng = _api()
    dev = _dev()
    host, _ = _tensors(name)
    g = torch.Generator().manual_seed(61)
    ps = [torch.randn(t.numel(), generator=g) for t in host]
    ref = [torch.nn.Parameter(p.clone()) for p in ps]
    opt = torch.optim.Adam(ref, foreach=False, **HYPER)
    mine = [p.clone().to(dev) for p in ps]
    ms, vs = [torch.zeros_like(p) for p in mine], [torch.zeros_like(p) for p in mine]
    plain = [p.clone() for p in mine]
    pm, pv = [torch.zeros_like(p) for p in mine], [torch.zeros_like(p) for p in mine]
    null = [p.clone() for p in mine]
    nm, nv = [torch.zeros_like(p) for p in mine], [torch.zeros_like(p) for p in mine]
    for step in range(1, 4):
        grads = [t * torch.randn(t.numel(), generator=g).sign() for t in host]      # the list's magnitudes, fresh signs
        gd = _on_device(name)
        for d, gr in zip(gd, grads):
            d.copy_(gr)
        total = float(torch.sqrt(sum((x.double() ** 2).sum() for x in grads)))
        out = torch.empty(2, device=dev)
        items_n = _adam_items(eng, mine, gd, ms, vs)
        need = lib.qt_grad_norm_workspace_bytes(items_n, len(mine))
        ws = torch.empty(need // 4, device=dev)
        L.check(lib.qt_grad_norm_multi(items_n, len(mine), 0.25 * total, ws.data_ptr(), need, out.data_ptr(),
                                       L.stream_ptr()), "qt_grad_norm_multi")
        desc = eng.AdamDesc(HYPER["lr"], *HYPER["betas"], HYPER["eps"], HYPER["weight_decay"], 1.0, step)
        L.check(lib.qt_adam_multi_scaled(items_n, len(mine), ctypes.byref(desc), out.data_ptr() + 4, L.stream_ptr()),
                "qt_adam_multi_scaled")
        L.check(lib.qt_adam_multi_scaled(_adam_items(eng, null, gd, nm, nv), len(mine), ctypes.byref(desc), None,
                                         L.stream_ptr()), "qt_adam_multi_scaled(null)")
        L.check(lib.qt_adam_multi(_adam_items(eng, plain, gd, pm, pv), len(mine), ctypes.byref(desc), L.stream_ptr()),
                "qt_adam_multi")
        torch.cuda.synchronize()
        coef = out.cpu()[1]
        assert 0.2 < float(coef) < 0.3
        for r, gr in zip(ref, grads):
            r.grad = gr * coef          # f32 product, the rounding the kernel makes
        opt.step()
    for r, p, m, v in zip(ref, mine, ms, vs):
        assert rel_err(p.cpu(), r.detach()) <= ADAM_TOL
        assert rel_err(m.cpu(), opt.state[r]["exp_avg"]) <= ADAM_TOL
        assert rel_err(v.cpu(), opt.state[r]["exp_avg_sq"]) <= ADAM_TOL
    for a, b in zip(null + nm + nv, plain + pm + pv):
        assert torch.equal(a, b)


# ---- whole optimizer steps ---------------------------------------------------------------------------------------------
def _quadtree(dt, B, frozen=False):
    P = pkg()
    m = P.QuadtreeCNN(12, dropout_rate=0.0, compute_dtype=dt, max_batch=B, freeze_backbone=frozen)
    m.load_state_dict(pkg("synth").synth_state_dict(m))
    return m.to(_dev()).train()


def _batch(B, salt=5):
    synth = pkg("synth")
    return (synth.synth_images(B, salt=salt).to(_dev()), synth.synth_pose_features(B, salt=salt).to(_dev()),
            synth.synth_labels(B, 12, salt=salt).to(_dev()))


def _backward(model, opt, data):
    x, f, y = data
    opt.zero_grad(set_to_none=True)
    F.cross_entropy(model(x, f), y).backward()


def _eval_logits(model, data):
    model.eval()
    with torch.no_grad():
        out = model(data[0], data[1]).float().cpu()
    model.train()
    return out


def _float64_norm(params):
    return float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params if p.grad is not None)))


def _step_state(m, opt, data):
    state = {n: p.detach().cpu().clone() for n, p in m.named_parameters()}
    for n, p in m.named_parameters():
        if p in opt.state:
            state["m/" + n] = opt.state[p]["exp_avg"].cpu().clone()
            state["v/" + n] = opt.state[p]["exp_avg_sq"].cpu().clone()
    state["logits"] = _eval_logits(m, data)     # read from the packed copies the step rewrote
    return state


def _assert_same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_inactive_clipping_is_free():
    """max_grad_norm=1e30: the coefficient is exactly 1.0, so parameters, moments and the packed copies (eval logits)
    carry the bits of the unclipped step.  f32, B = 2, one train step.  The f32 build's backward is not bit-reproducible
    from run to run (conv1 / layer1 / layer2 weight gradients differ in the last bit between two identical models, with or
    without clipping), so both optimizers step the SAME gradients: backward once, step unclipped, put the parameters
    back, step with max_grad_norm=1e30."""
    P = pkg()
    data = _batch(2)
    m = _quadtree(torch.float32, 2)
    params = list(m.parameters())
    opt = P.FusedAdam(params, lr=1e-3, weight_decay=1e-4, model=m)
    _backward(m, opt, data)
    start = [p.detach().clone() for p in params]
    grads = [None if p.grad is None else p.grad.clone() for p in params]
    opt.step()
    assert opt.last_grad_norm is None and opt.last_clip_coef is None
    plain = _step_state(m, opt, data)
    with torch.no_grad():
        for p, s in zip(params, start):
            p.copy_(s)
    clipped_opt = P.FusedAdam(params, lr=1e-3, weight_decay=1e-4, model=m, max_grad_norm=1e30)
    clipped_opt.step()
    assert float(clipped_opt.last_clip_coef) == 1.0
    assert abs(float(clipped_opt.last_grad_norm) - _float64_norm(params)) <= NORM_TOL * float(clipped_opt.last_grad_norm)
    for p, g in zip(params, grads):
        assert (p.grad is None) == (g is None) and (g is None or torch.equal(p.grad, g))
    assert any(not torch.equal(p.detach(), s) for p, s in zip(params, start))
    _assert_same_bits(plain, _step_state(m, clipped_opt, data))


def test_inactive_clipping_is_free_two_models_bf16():
    """The same on the bf16 build, whose backward is bit-reproducible: two models, two steps each, one with
    max_grad_norm=1e30 and one without, every bit equal."""
    P = pkg()
    data = _batch(2)
    got = []
    for max_norm in (None, 1e30):
        m = _quadtree(torch.bfloat16, 2)
        opt = P.FusedAdam(m.parameters(), lr=1e-3, weight_decay=1e-4, model=m, max_grad_norm=max_norm)
        for _ in range(2):
            _backward(m, opt, data)
            opt.step()
        got.append(_step_state(m, opt, data))
    _assert_same_bits(got[0], got[1])


def test_default_still_overlaps_and_clipped_step_is_serial():
    """bf16, the build that has the side-stream order: without max_grad_norm the second step still runs beside the stem
    backward (tests/test_adam_overlap_gpu.py); with it every step is serial."""
    P = pkg()
    data = _batch(4)
    for max_norm, want in ((None, [False, True]), (1.0, [False, False])):
        m = _quadtree(torch.bfloat16, 4)
        opt = P.FusedAdam(m.parameters(), lr=1e-3, weight_decay=1e-4, model=m, max_grad_norm=max_norm)
        took = []
        for _ in range(2):
            _backward(m, opt, data)
            opt.step()
            took.append(m._engine.last_adam_overlapped)
        torch.cuda.synchronize()
        assert took == want, (max_norm, took)


def _compare_twins(make_model, make_opt, data, max_norm, steps=2, share_grads=False):
    """Twin A: FusedAdam(max_grad_norm=max_norm).  Twin B: torch.nn.utils.clip_grad_norm_ + the unclipped FusedAdam.
    share_grads: twin B steps twin A's gradients (copied into its own .grad tensors after its backward).  The f32
    build's backward is not bit-reproducible from run to run, and Adam turns a last-bit difference of a near-zero gradient
    into a visible difference of the update: two twins that BOTH use torch's clipping + the unclipped FusedAdam end
    up to 11 x (2e-6 * max|p|) apart after one step (measured, base_cnn.layer2.0.conv2.weight), so without sharing the
    bound would test the backward, not the clipping.  The bf16 build is reproducible and is compared without sharing."""
    a, b = make_model(), make_model()
    oa, ob = make_opt(a, max_norm), make_opt(b, None)
    coefs = []
    for s in range(steps):
        _backward(a, oa, data)
        _backward(b, ob, data)
        if share_grads:
            for p, q in zip(a.parameters(), b.parameters()):
                assert (p.grad is None) == (q.grad is None)
                if p.grad is not None:
                    q.grad.copy_(p.grad)
        torch_norm = torch.nn.utils.clip_grad_norm_(b.parameters(), max_norm)
        ob.step()
        before = {n: p.grad.clone() for n, p in a.named_parameters() if p.grad is not None}
        oa.step()
        for n, p in a.named_parameters():
            if p.grad is not None:
                assert torch.equal(p.grad, before[n]), f"step() changed {n}.grad"
        err = abs(float(oa.last_grad_norm) - float(torch_norm)) / float(torch_norm)
        print(f"step {s}: norm {float(oa.last_grad_norm):.8g} torch {float(torch_norm):.8g} rel {err:.2e} "
              f"coef {float(oa.last_clip_coef):.6f}")
        assert oa.last_grad_norm.dim() == 0 and oa.last_grad_norm.dtype == torch.float32 and oa.last_grad_norm.is_cuda
        assert err <= NORM_TOL
        coefs.append(float(oa.last_clip_coef))
    worst = 0.0
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        d = float((p.detach() - q.detach()).abs().max())
        bound = ADAM_TOL * float(q.detach().abs().max())
        worst = max(worst, d / max(bound, 1e-30))
        print(f"  {n}: max|diff| {d:.3e}, bound {bound:.3e}")
    la, lb = _eval_logits(a, data), _eval_logits(b, data)
    lerr = rel_err(la, lb)
    print(f"worst parameter diff / bound {worst:.3f}; eval logits rel err {lerr:.2e}")
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert float((p.detach() - q.detach()).abs().max()) <= ADAM_TOL * float(q.detach().abs().max()), n
    assert lerr <= 1e-5
    return a, oa, coefs


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_active_clipping_plan_path(dt):
    P = pkg()
    data = _batch(2)
    probe = _quadtree(dt, 2)
    _backward(probe, torch.optim.SGD(probe.parameters(), lr=0.0), data)
    norm0 = float(P.grad_norm(probe.parameters()))
    assert abs(norm0 - _float64_norm(probe.parameters())) <= NORM_TOL * norm0
    del probe

    def make_opt(m, max_norm):
        return P.FusedAdam(m.parameters(), lr=1e-4, weight_decay=1e-4, model=m, max_grad_norm=max_norm)
    a, oa, coefs = _compare_twins(lambda: _quadtree(dt, 2), make_opt, data, 0.5 * norm0,
                                  share_grads=(dt == torch.float32))
    assert a._engine.last_adam_overlapped is False
    assert 0.49 < coefs[0] < 0.51      # (the second step's norm is whatever the first step left: it may not clip)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_clip_model_path(dt):
    """Quadtree3DCNN has no plan: the multi-tensor path.  The 3dcnn trainer's loop body (zero_grad, forward,
    cross-entropy, backward, clip to 1.0, step: 3dcnn/train_3D_Quadtree_cnn_model.py:111-125)."""
    P, synth, optim = pkg(), pkg("synth"), pkg("optim")
    B, T, HW = 2, 5, 64
    x = synth.synth_images(B * T, salt=31, size=HW).view(B, T, 3, HW, HW).to(_dev())
    f = synth.synth_pose_features(B * T, salt=31, realistic=True).view(B, T, 47).to(_dev())
    y = synth.synth_labels(B, 12, salt=31).to(_dev())

    def make_model():
        m = P.Quadtree3DCNN(12, sequence_length=T, mode="quadtree_3d_fusion", dropout_rate=0.0,
                            compute_dtype=dt)
        m.load_state_dict(synth.synth_state_dict(m))
        return m.to(_dev()).train()

    def make_opt(m, max_norm):
        return P.FusedAdam(m.parameters(), lr=1e-4, weight_decay=1e-4, max_grad_norm=max_norm)
    count = optim.raw_update_count()
    _, _, coefs = _compare_twins(make_model, make_opt, (x, f, y), 1.0, share_grads=(dt == torch.float32))
    assert coefs[0] < 1.0, "the first step must clip"
    assert optim.raw_update_count() >= count + 4      # two steps of two optimizers: the next forward re-packs


def test_frozen_parameters_stay_out_of_the_norm():
    """resnet/ variant: frozen backbone (and base_cnn.fc, which nothing uses): the norm covers exactly the tensors that
    have a gradient."""
    P = pkg()
    data = _batch(2)
    m = _quadtree(torch.float32, 2, frozen=True)
    opt = P.FusedAdam(m.parameters(), lr=1e-4, weight_decay=1e-4, model=m, max_grad_norm=1e-3)
    _backward(m, opt, data)
    with_grad = [n for n, p in m.named_parameters() if p.grad is not None]
    assert with_grad and not any(n.startswith("base_cnn.") for n in with_grad)
    assert m.base_cnn.fc.weight.grad is None and m.base_cnn.conv1.weight.grad is None
    ref = _float64_norm(m.parameters())
    frozen = dict(m.named_parameters())["base_cnn.layer4.1.conv2.weight"]
    frozen_before = frozen.detach().clone()
    opt.step()
    assert abs(float(opt.last_grad_norm) - ref) <= NORM_TOL * ref
    assert abs(float(P.grad_norm(m.parameters())) - ref) <= NORM_TOL * ref
    expect = torch.clamp(1e-3 / (opt.last_grad_norm.cpu() + 1e-6), max=1.0)
    assert torch.equal(_bits(opt.last_clip_coef), _bits(expect))
    assert torch.equal(frozen.detach(), frozen_before)
