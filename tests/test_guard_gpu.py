"""Guard-band cases for the entry points the launch helpers of the convolution tests do not reach (tests/_guard.py): the size
queries, the multi-tensor optimizer kernels, the weight packers and the plan workspace.

Every case is ONE function of an allocator, run twice: on `Plain` (ordinary torch tensors) and on a `Guard` (outputs NaN,
workspaces of exactly the queried size, inputs with NaN around them, all between 0xFF bands).  Guard.check() asserts the
memory properties; the guarded results must equal the plain ones -- bit for bit where the existing test of the entry point
shows the bits are reproducible, inside that test's documented bound where the kernel uses atomics.  Shapes are the existing
tests' smallest per dispatch branch.  Byte outputs run with payload fills 0xFF and 0x00 and must agree.

The guards observe memory after ordinary calls.  A store farther out than a band stays invisible; an internal buffer of the plan
workspace running into the next one is the business of tests/test_plan_gaps_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _augment_ref as AR
import _gradcam_ref as GR
import _loss_ref as LR
import _stem_bounds as Sb
from _guard import POISON, Guard
from _plan_gaps import compare_twins, plan_run, rehome
from _util import pkg, rel_err
from test_clip_adam_gpu import ADAM_TOL, HYPER, LISTS, _tensors

pytestmark = pytest.mark.gpu

F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class Plain:
    """the allocator interface of Guard on ordinary tensors"""

    def __init__(self, dev):
        self.dev = dev

    def output(self, name, shape, dt, fill=POISON, offset=0, written=None):
        shape = shape if isinstance(shape, tuple) else (shape,)
        n = int(np.prod(shape))
        whole = torch.empty(n + offset, dtype=dt, device=self.dev)
        whole.view(U8).fill_(fill)
        return whole[offset:].view(shape)

    def workspace(self, name, nbytes):
        return torch.empty(int(nbytes), dtype=U8, device=self.dev)

    def input(self, name, t, offset=0):
        if t is None:
            return None
        whole = torch.empty(t.numel() + offset, dtype=t.dtype, device=self.dev)
        whole[offset:].copy_(t.reshape(-1))
        return whole[offset:].view(t.shape)

    def check(self):
        torch.cuda.synchronize()


def _both(case, *args, **kw):
    """(plain results, guarded results) of case(allocator, ...); the guarded run is checked"""
    dev = _dev()
    plain = case(Plain(dev), *args, **kw)
    torch.cuda.synchronize()
    g = Guard(dev)
    got = case(g, *args, **kw)
    g.check()
    return plain, got


def _bits_equal(a, b, what=""):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(a.contiguous().view(U8), b.contiguous().view(U8)), what


def _L():
    L = pkg("_lib")
    return L, L.lib()


# ======================================================================================================================
# a. size-query contracts
# ======================================================================================================================
@pytest.mark.parametrize("dt,rows,cols,ld", [(BF16, 300, 1, 1),            # 3 chunks of 128 rows, the last one short
                                             (F32, 12544, 64, 80),         # 98 chunks, ld > cols
                                             (BF16, 200704, 128, 128)])    # 1568 chunks: capped at 1024
def test_col_sum(dt, rows, cols, ld):
    """qt_col_sum_ws (both stages, write and accumulate) bit for bit; the atomic qt_col_sum inside the 1e-5 that
    tests/test_conv_gpu.py::test_col_sum_ws_is_deterministic holds it to"""
    L, lib = _L()
    nws = lib.qt_col_sum_workspace_bytes(rows, cols)
    assert nws == min(-(-rows // 128), 1024) * cols * 4
    x = torch.randn(rows, ld, generator=torch.Generator().manual_seed(5)).to(dt)
    ref = x[:, :cols].double().sum(0)

    def case(A):
        xd = A.input("x", x)
        outs = []
        for acc in (0, 1):
            ws = A.workspace(f"ws{acc}", nws)
            out = A.output(f"out{acc}", (cols,), F32, fill=0) if acc else A.output(f"out{acc}", (cols,), F32)
            L.check(lib.qt_col_sum_ws(L.qt_dtype(dt), L.ptr(xd), rows, cols, ld, L.ptr(out), acc, L.ptr(ws),
                                      nws, L.stream_ptr()), "qt_col_sum_ws")
            outs.append(out)
        atomic = A.output("atomic", (cols,), F32)
        L.check(lib.qt_col_sum(L.qt_dtype(dt), L.ptr(xd), rows, cols, ld, L.ptr(atomic), 0, L.stream_ptr()),
                "qt_col_sum")
        return outs + [atomic]

    plain, got = _both(case)
    _bits_equal(plain[0], got[0], "write")
    _bits_equal(plain[1], got[1], "accumulate into zeros")
    _bits_equal(got[0], got[1])
    assert rel_err(got[0].cpu(), ref) <= 1e-5
    assert rel_err(got[2].cpu(), plain[2].cpu()) <= 1e-5 and rel_err(got[2].cpu(), ref) <= 1e-5


@pytest.mark.parametrize("M,N,K,with_bias,relu", [(5, 64, 64, True, 0),          # one tile, one K-step: no split
                                                  (200, 192, 448, False, 1),     # seven K-steps in ragged slices
                                                  (37, 2688, 5376, True, 1)])    # classifier.0, ragged batch: split K
def test_linear_workspace(M, N, K, with_bias, relu):
    """qt_linear_bf16 on exactly qt_linear_workspace_bytes: partial products are added in a fixed order, bit for bit"""
    L, lib = _L()
    g = torch.Generator().manual_seed(41)
    x = torch.randn(M, K, generator=g).to(BF16)
    w = (torch.randn(N, K, generator=g) * 0.05).to(BF16)
    b = torch.randn(N, generator=g) if with_bias else None
    nbytes = lib.qt_linear_workspace_bytes(M, N, K)
    assert nbytes >= M * N * 4

    def case(A):
        xd, wd, bd = A.input("x", x), A.input("w", w), A.input("bias", b)
        ws, y = A.workspace("ws", nbytes), A.output("y", (M, N), BF16)
        L.check(lib.qt_linear_bf16(L.ptr(xd), L.ptr(wd), L.ptr(bd), relu, L.ptr(y), M, N, K, L.ptr(ws), nbytes,
                                   L.stream_ptr()), "qt_linear_bf16")
        return y

    plain, got = _both(case)
    _bits_equal(plain, got)
    ref = F.linear(x.float(), w.float(), b)
    assert rel_err(got.float().cpu(), torch.relu(ref) if relu else ref) <= 4e-3


class _LossCase:
    def __init__(self, kind, rows, C, red):
        self.M, self.lib = pkg("loss"), pkg("_lib")
        self.L = self.lib.lib()
        self.kind, self.rows, self.C, self.red = kind, rows, C, red
        seed = 7 + rows + C
        self.z = LR.make_logits(rows, C, "x1", seed=seed)
        self.y = LR.make_labels(rows, C, "some" if kind == LR.CE else "no", seed=seed)
        self.w = LR.make_weights(C, seed)
        self.g = LR.make_grad_out(rows, red, seed)
        self.eps, self.gamma = (0.1, 0.0) if kind == LR.CE else (0.0, 2.0)

    def __call__(self, A):
        rows, C, L, lib = self.rows, self.C, self.L, self.lib
        zd, yd, wd, gd = A.input("logits", self.z), A.input("labels", self.y), A.input("weights", self.w), A.input("grad_out", self.g)
        desc = self.M.LossDesc(0, self.kind, self.red, LR.IGNORE, self.eps, self.gamma, lib.ptr(wd))
        loss = A.output("loss", (rows if self.red == LR.NONE else 1,), F32)
        state = A.output("row_state", (rows, 2), F32)
        stats = A.output("stats", (3,), torch.float64)
        pred = A.output("pred", (rows,), torch.int64)
        need = L.qt_loss_workspace_bytes(rows, C)
        ws = A.workspace("ws", need) if need else None
        lib.check(L.qt_loss_forward(ctypes.byref(desc), zd.data_ptr(), C, yd.data_ptr(), rows, C, loss.data_ptr(), state.data_ptr(),
                                    stats.data_ptr(), pred.data_ptr(), None, lib.ptr(ws), need, lib.stream_ptr()), "qt_loss_forward")
        dz = A.output("dlogits", (rows, C), F32)
        lib.check(L.qt_loss_backward(ctypes.byref(desc), zd.data_ptr(), C, yd.data_ptr(), rows, C, state.data_ptr(),
                                     stats.data_ptr(), gd.data_ptr(), dz.data_ptr(), C, lib.stream_ptr()), "qt_loss_backward")
        return {"loss": loss, "dz": dz, "pred": pred, "stats": stats, "row_state": state, "need": need}


@pytest.mark.parametrize("kind", [LR.CE, LR.FOCAL], ids=["ce", "focal"])
@pytest.mark.parametrize("rows,C", [(256, 12), (257, 12), (16, 17), (17, 17), (5, 65)])   # each side of the three thresholds
def test_loss_workspace(kind, rows, C):
    """qt_loss_forward / qt_loss_backward, with and without the partial-sum workspace (tests/test_loss_cpu.py pins the three
    thresholds of qt_loss_workspace_bytes): the bits of the run on plain buffers (tests/test_loss_gpu.py::
    test_two_runs_are_bit_identical: both entry points are reproducible), inside the derived bounds of tests/_loss_ref.py,
    bookkeeping exact"""
    _dev()
    needs = set()
    for red in (LR.MEAN, LR.NONE):
        c = _LossCase(kind, rows, C, red)
        plain, got = _both(c)
        needs.add(got["need"])
        # (row_state of the focal form is not among what that test pins)
        for k in ("loss", "dz", "stats", "pred") + (("row_state",) if kind == LR.CE else ()):
            _bits_equal(plain[k], got[k], (red, k))
        ref = LR.ce_ref(c.z, c.y, c.w, c.eps, red, c.g) if kind == LR.CE else LR.focal_ref(c.z, c.y, c.w, c.gamma, red, c.g)
        for out in (plain, got):
            assert torch.equal(out["pred"].cpu(), torch.max(c.z, 1).indices)
            assert float(out["stats"][2]) == float((torch.max(c.z, 1).indices == c.y).sum())
            rl = LR.ratio(out["loss"].cpu().reshape(-1), ref["loss"].reshape(-1), ref["loss_bound"].reshape(-1))
            rg = LR.ratio(out["dz"].cpu(), ref["dz"], ref["dz_bound"])
            assert rl <= 1.0 and rg <= 1.0, (red, rl, rg)
    assert needs == {0} or needs == {48}


@pytest.mark.parametrize("name", ["jitter", "chain", "rotation"])
def test_augment_workspace(name):
    """qt_augment_f32 with the contrast workspace (jitter in all 24 orders; the whole chain) and without one (rotation alone):
    the bits of the run on plain buffers (tests/test_augment_gpu.py::test_two_runs_are_bit_identical) and inside the derived
    bound of tests/_augment_ref.py"""
    _dev()
    M, Lm = pkg("augment"), pkg("_lib")
    L = Lm.lib()
    if name == "jitter":
        h, w = AR.SHAPES[0]
        img, p = AR.make_images(24, h, w, 11), AR.jitter_rows()
        kx, ky, norm, contrast = 1, 1, AR.NO_NORM, 1
    elif name == "chain":
        h, w = AR.CHAIN_SHAPES[0]
        p = AR.chain_rows(h, w)
        img = AR.make_images(p.shape[0], h, w, 19)
        kx, ky, norm, contrast = 5, 9, (AR.MEAN32, AR.INV_STD32), 1
    else:
        h, w = AR.SHAPES[0]
        img = AR.make_images(len(AR.ANGLES) + 1, h, w, 13) + 0.5
        p = AR.rows([AR.row(deg=a) for a in AR.ANGLES] + [AR.row()])
        kx, ky, norm, contrast = 1, 1, AR.NO_NORM, 0
    N, image = img.shape[0], 3 * h * w
    need = L.qt_augment_workspace_bytes(N, contrast)
    assert (need > 0) == bool(contrast)

    def case(A):
        src, par = A.input("images", img.reshape(N, image).float()), A.input("params", p)
        dst = A.output("out", (N, image), F32)
        ws = A.workspace("ws", need) if need else None
        desc = M.AugmentDesc(N, h, w, image, image, kx, ky, (ctypes.c_float * 3)(*norm[0]), (ctypes.c_float * 3)(*norm[1]), contrast)
        Lm.check(L.qt_augment_f32(ctypes.byref(desc), src.data_ptr(), par.data_ptr(), dst.data_ptr(), Lm.ptr(ws), need,
                                  Lm.stream_ptr()), "qt_augment_f32")
        return dst

    plain, got = _both(case)
    _bits_equal(plain, got)
    if name == "rotation":     # a copy of source pixels, held to the float64 rule by tests/test_augment_gpu.py
        return
    ref, bound, _ = AR.reference(img, p, kx, ky, norm)
    for out in (plain, got):
        o = out.cpu().reshape(N, 3, h, w)
        assert AR.ratio(o, ref, bound) <= 1.0 and AR.same_nan_pattern(o, ref)


@pytest.mark.parametrize("B,C,P", [(2, 32, 49), (2, 33, 49), (3, 70, 15)])   # one launch, no workspace; two and three chunks
def test_gradcam_map_workspace(B, C, P):
    """qt_gradcam_map: the same bits as on plain buffers (tests/test_gradcam_gpu.py::test_map_edge_cases: reproducible)"""
    _dev()
    G, Lm = pkg("gradcam"), pkg("_lib")
    L = Lm.lib()
    act, grad = GR.make_inputs(B, C, P, "noisy", seed=0)
    need = L.qt_gradcam_workspace_bytes(B, C, P)
    assert (need > 0) == (C > 32)

    def case(A):
        a, g = A.input("act", torch.from_numpy(act)), A.input("grad", torch.from_numpy(grad))
        cam, peak = A.output("cam", (B, P), F32), A.output("peak", (B,), F32)
        ws = A.workspace("ws", need) if need else None
        Lm.check(L.qt_gradcam_map(a.data_ptr(), g.data_ptr(), B, C, P, cam.data_ptr(), peak.data_ptr(), Lm.ptr(ws), need,
                                  Lm.stream_ptr()), "qt_gradcam_map")
        return cam, peak

    plain, got = _both(case)
    _bits_equal(plain[0], got[0], "map")
    _bits_equal(plain[1], got[1], "peak")
    ref, ref_peak = GR.cam_ref(act, grad)
    bound, peak_bound = GR.cam_bound(act, grad)
    assert float((np.abs(got[0].cpu().numpy() - ref) / bound).max()) <= 1.0
    assert float((np.abs(got[1].cpu().numpy() - ref_peak) / peak_bound).max()) <= 1.0


def test_gradcam_overlay_byte_outputs():
    """qt_gradcam_overlay_u8 writes bytes, which may be 0xFF: payload fills 0xFF and 0x00 give the same overlay and index"""
    _dev()
    G, Lm = pkg("gradcam"), pkg("_lib")
    L = Lm.lib()
    B, H, W = 2, 37, 61
    cam, frames, lut = GR.make_cam(B, 5, 3, seed=9), GR.make_frames(B, H, W, seed=10), G.jet_lut().numpy()

    def case(A, fill):
        c, table = A.input("cam", torch.from_numpy(cam)), A.input("lut", torch.from_numpy(lut))
        src = A.input("frames", torch.from_numpy(frames))
        out = A.output("out", (B, H, W, 3), U8, fill=fill)
        heat = A.output("heat", (B, H, W), F32)
        index = A.output("index", (B, H, W), U8, fill=fill)
        Lm.check(L.qt_gradcam_overlay_u8(c.data_ptr(), 5, 3, src.data_ptr(), B, H, W, table.data_ptr(), 0.4, out.data_ptr(),
                                         heat.data_ptr(), index.data_ptr(), Lm.stream_ptr()), "qt_gradcam_overlay_u8")
        return out, heat, index

    plain, ff = _both(case, 0xFF)
    _, zero = _both(case, 0x00)
    for a, b, c in zip(plain, ff, zero):
        _bits_equal(a, b)
        _bits_equal(b, c)
    GR.check_overlay(ff[0].cpu().numpy(), GR.admissible(cam, H, W), frames, lut, 0.4, ff[2].cpu().numpy())


@pytest.mark.parametrize("B", [1, 11])    # 56 workgroups; 616 tiles on the capped grid of 256
def test_stem_bn_bwd_wgrad_workspace(B):
    """qt_stem_bn_bwd_wgrad_ws on the sparse probe of tests/_stem_bounds.py: an exactly known filter, the same bits"""
    L, lib = _L()
    c = Sb.case("grid", B)
    d, coef, image, dw_ref, _ = Sb.sparse_probe(B)
    nws = lib.qt_stem_bn_bwd_wgrad_workspace_bytes(B)
    assert nws == min(B * 56, 256) * 64 * 7 * 32 * 4
    f = lambda t: t.float().contiguous()

    def case(A):
        t = dict(d=A.input("dpooled", d.to(BF16)), code=A.input("argmax", c["code"]), y=A.input("y", c["y"].to(BF16)),
                 scale=A.input("scale", f(c["scale"])), shift=A.input("shift", f(c["shift"])), mean=A.input("mean", f(c["mean"])),
                 invstd=A.input("invstd", f(c["invstd"])), coef=A.input("coef", f(coef)))
        xpad = A.input("xpad", Sb.pack_image(image, BF16))
        ws = A.workspace("ws", nws)
        dw = A.output("dw", (64, 7, 8, 4), F32, fill=0)    # zeros: include/qtcnn.h has the caller zero dw (dw += ...)
        rc = lib.qt_stem_bn_bwd_wgrad_ws(L.qt_dtype(BF16), L.ptr(t["d"]), L.ptr(t["code"]), L.ptr(t["y"]), L.ptr(t["scale"]),
                                         L.ptr(t["shift"]), L.ptr(t["mean"]), L.ptr(t["invstd"]), L.ptr(t["coef"]), L.ptr(xpad),
                                         L.ptr(dw), L.ptr(ws), nws, B, L.stream_ptr())
        assert rc == 0, lib.qt_last_error()
        return dw

    try:
        plain, got = _both(case)
    finally:
        Sb.clear_caches()
    _bits_equal(plain, got)
    want = Sb.pack_wgrad(dw_ref)[:, :, :7, :3]
    assert torch.equal(got.cpu()[:, :, :7, :3].double(), want)


# ======================================================================================================================
# b. optimizer and packers
# ======================================================================================================================
ADAM_LISTS = {k: LISTS[k] for k in ("one", "around_256", "mixed49", "unaligned")}
ADAM_LISTS["chunks"] = [(4097, 0), (1, 0), (8192 * 2 + 3, 0)]       # (the 1 Mi tensor of test_clip_adam_gpu.py cut to three chunks)


def _list_tensors(name):
    if name != "chunks":
        return _tensors(name)[0]
    g = torch.Generator().manual_seed(len(name) * 131 + 7)
    return [torch.randn(n, generator=g) * 10.0 ** (-3.0 + 3.0 * j) for j, (n, _) in enumerate(ADAM_LISTS[name])]


def _engine_api():
    L, lib = _L()
    eng = pkg("engine")
    return L, lib, eng


@pytest.mark.parametrize("scaled", [False, True], ids=["adam_multi", "adam_multi_scaled"])
@pytest.mark.parametrize("name", list(ADAM_LISTS))
def test_adam_multi(name, scaled):
    """p, g, m, v of every tensor in a guarded buffer of its own, at element offsets 0..3 (the entry points accept 4-byte
    alignment): p / m / v bit-equal to the run on plain tensors after two steps, g untouched (Guard.check), and p against
    torch.optim.Adam inside the 2e-6 of tests/test_clip_adam_gpu.py"""
    L, lib, eng = _engine_api()
    grads = _list_tensors(name)
    g = torch.Generator().manual_seed(61)
    params = [torch.randn(t.numel(), generator=g) for t in grads]
    coef = torch.tensor([0.375])

    def case(A):
        ps, gs, ms, vs = [], [], [], []
        for j, (p, gr) in enumerate(zip(params, grads)):
            off = ADAM_LISTS[name][j][1] + j
            ps.append(A.input(f"p{j}", p, offset=off % 4))
            gs.append(A.input(f"g{j}", gr, offset=(off + 1) % 4))
            ms.append(A.output(f"m{j}", (p.numel(),), F32, fill=0, offset=(off + 2) % 4))
            vs.append(A.output(f"v{j}", (p.numel(),), F32, fill=0, offset=(off + 3) % 4))
        cd = A.input("coef", coef)
        items = (eng.AdamItem * len(ps))(*[eng.AdamItem(p.data_ptr(), q.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel())
                                           for p, q, m, v in zip(ps, gs, ms, vs)])
        for step in (1, 2):
            desc = eng.AdamDesc(HYPER["lr"], *HYPER["betas"], HYPER["eps"], HYPER["weight_decay"], 1.0, step)
            if scaled:
                L.check(lib.qt_adam_multi_scaled(items, len(ps), ctypes.byref(desc), cd.data_ptr(), L.stream_ptr()),
                        "qt_adam_multi_scaled")
            else:
                L.check(lib.qt_adam_multi(items, len(ps), ctypes.byref(desc), L.stream_ptr()), "qt_adam_multi")
        return ps, ms, vs

    dev = _dev()
    plain = case(Plain(dev))
    torch.cuda.synchronize()
    gd = Guard(dev)
    got = case(gd)
    # p is updated in place: it is an input only as far as the bands go
    for b in gd.bufs:
        if b.name.startswith("p"):
            b.snapshot = b.payload.clone()
    gd.check()
    for a, b in zip(plain, got):
        for x, y in zip(a, b):
            _bits_equal(x, y)
    ref = [torch.nn.Parameter(p.clone()) for p in params]
    opt = torch.optim.Adam(ref, foreach=False, **HYPER)
    for _ in range(2):
        for r, gr in zip(ref, grads):
            r.grad = gr * coef[0] if scaled else gr.clone()
        opt.step()
    for r, p in zip(ref, got[0]):
        assert rel_err(p.cpu(), r.detach()) <= ADAM_TOL


@pytest.mark.parametrize("name", list(ADAM_LISTS))
def test_grad_norm_multi(name):
    """the exact-size workspace and the 2-float output guarded, gradients at the offsets of the list; bits of the plain run
    (two deterministic stages) and the float64 norm inside 1e-5"""
    L, lib, eng = _engine_api()
    grads = _list_tensors(name)
    ref = float(torch.sqrt(sum((t.double() ** 2).sum() for t in grads)))

    def case(A):
        gs = [A.input(f"g{j}", t, offset=(ADAM_LISTS[name][j][1] + j) % 4) for j, t in enumerate(grads)]
        items = (eng.AdamItem * len(gs))(*[eng.AdamItem(None, t.data_ptr(), None, None, t.numel()) for t in gs])
        need = lib.qt_grad_norm_workspace_bytes(items, len(gs))
        assert need > 0 and need % 4 == 0
        ws, out = A.workspace("ws", need), A.output("out2", (2,), F32)
        L.check(lib.qt_grad_norm_multi(items, len(gs), 1.0, ws.data_ptr(), need, out.data_ptr(), L.stream_ptr()),
                "qt_grad_norm_multi")
        return out

    plain, got = _both(case)
    _bits_equal(plain, got)
    assert abs(float(got[0]) - ref) <= 1e-5 * ref


def state_view(gd, name):
    return next(b.t for b in gd.bufs if b.name == name)


_PackItem = pkg("_abi").PackItem   # qt_pack_item


# (O, I, k, stride2_dgrad): a 3x3 stride 1, a 3x3 stride 2 in the 4-slot merged form, a 3x3 stride 2 in the 5-slot form with its
# 1x1 downsample partner (slot 4 of the SAME operand), a 1x1 and a linear layer; sizes of tests/test_conv_gpu.py and
# tests/test_adam_overlap_gpu.py
PACK_SHAPES = [(64, 64, 3, 0), (128, 64, 3, 2), (256, 128, 3, 3), (256, 128, 1, 4), (128, 192, 1, 0), (2688, 5376, 1, 0)]


def _pack_reference(dt, ws):
    """the per-tensor packers on plain tensors: [(fwd, dgrad or None)] per item; item 2's dgrad is the five-slot operand
    assembled from qt_pack_dgrad_s2_merged's four slots and the downsample's [I][O] transpose in slot 4 of class (0,0)"""
    L, lib = _L()
    dev, qdt, st = _dev(), L.qt_dtype(dt), L.stream_ptr()
    out = []
    for (O, I, k, s2), w in zip(PACK_SHAPES, ws):
        wd = w.to(dev)
        fwd = torch.zeros(O * k * k * I, dtype=dt, device=dev)
        if s2 == 0:
            dg = torch.zeros(k * k * O * I, dtype=dt, device=dev)
            L.check(lib.qt_pack_conv_weight(qdt, L.ptr(wd), L.ptr(fwd), L.ptr(dg), O, I, k, k, st), "qt_pack_conv_weight")
        elif s2 == 4:      # the 1x1 partner: its [I][O] transpose goes into slot 4 below
            dg = torch.zeros(O * I, dtype=dt, device=dev)
            L.check(lib.qt_pack_conv_weight(qdt, L.ptr(wd), L.ptr(fwd), L.ptr(dg), O, I, 1, 1, st), "qt_pack_conv_weight")
        else:
            L.check(lib.qt_pack_conv_weight(qdt, L.ptr(wd), L.ptr(fwd), None, O, I, k, k, st), "qt_pack_conv_weight")
            dg = torch.zeros(16 * O * I, dtype=dt, device=dev)
            L.check(lib.qt_pack_dgrad_s2_merged(qdt, L.ptr(wd), L.ptr(dg), O, I, st), "qt_pack_dgrad_s2_merged")
        out.append((fwd, dg))
    torch.cuda.synchronize()
    O, I = PACK_SHAPES[2][:2]
    five = torch.zeros(4 * I, 5, O, dtype=dt, device=dev)
    five[:, :4] = out[2][1].view(4 * I, 4, O)
    five[:I, 4] = out[3][1].view(I, O)                       # element ((i*5 + 4)*O + o) = w[o][i], class (0,0) rows
    out[2] = (out[2][0], five.view(-1))
    out[3] = (out[3][0], None)                               # (checked as part of item 2's operand)
    return out


@pytest.mark.parametrize("entry", ["pack", "adam_pack", "adam_pack_scaled"])
@pytest.mark.parametrize("dt", [BF16, F32])
def test_batched_packers(entry, dt):
    """qt_pack_weights_batched / qt_adam_pack_weights_batched(_scaled): forward and data-gradient operands guarded (zeros
    where the merged layouts keep their zero slots, NaN elsewhere), masters / gradients / moments guarded too; the operands
    equal the per-tensor packers' bit for bit -- on the masters as they are, or on the masters qt_adam_multi(_scaled) leaves"""
    L, lib, eng = _engine_api()
    dev, qdt, st = _dev(), L.qt_dtype(dt), L.stream_ptr()
    g = torch.Generator().manual_seed(11)
    ws = [(torch.randn(O, I, k, k, generator=g) * 0.05) for (O, I, k, _) in PACK_SHAPES]
    grs = [(torch.randn(O, I, k, k, generator=g) * 0.01) for (O, I, k, _) in PACK_SHAPES]
    coef = torch.tensor([0.375])
    n = len(PACK_SHAPES)
    desc = eng.AdamDesc(1e-3, 0.9, 0.999, 1e-8, 1e-4, 1.0, 1)
    gd = Guard(dev)
    items, state, keep = (_PackItem * n)(), (eng.AdamItem * n)(), []
    five = None
    for j, (O, I, k, s2) in enumerate(PACK_SHAPES):
        w, gr = gd.input(f"w{j}", ws[j]), gd.input(f"grad{j}", grs[j])
        m, v = gd.output(f"m{j}", (O * I * k * k,), F32, fill=0), gd.output(f"v{j}", (O * I * k * k,), F32, fill=0)
        fwd = gd.output(f"fwd{j}", (O * k * k * I,), dt)
        if s2 == 0:
            dg = gd.output(f"dgrad{j}", (k * k * O * I,), dt)
        elif s2 == 2:
            dg = gd.output(f"dgrad{j}", (16 * O * I,), dt, fill=0)     # only the nine real taps are written
        elif s2 == 3:
            dg = five = gd.output(f"dgrad{j}", (20 * O * I,), dt, fill=0)
        else:
            dg = five                                                  # the downsample fills slot 4 of conv1's operand
        items[j] = _PackItem(w.data_ptr(), fwd.data_ptr(), dg.data_ptr(), O, I, k, s2)
        state[j] = eng.AdamItem(w.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), w.numel())
        keep.append((w, fwd, dg))
    cd = gd.input("coef", coef)
    masters = ws
    if entry == "pack":
        L.check(lib.qt_pack_weights_batched(qdt, items, n, st), "qt_pack_weights_batched")
    else:
        # the same update by qt_adam_multi(_scaled) on plain tensors gives the masters the operands are packed from
        pw = [w.clone().to(dev) for w in ws]
        pg = [x.to(dev) for x in grs]
        pm, pv = [torch.zeros_like(x) for x in pw], [torch.zeros_like(x) for x in pw]
        pit = (eng.AdamItem * n)(*[eng.AdamItem(a.data_ptr(), b.data_ptr(), c.data_ptr(), d.data_ptr(), a.numel())
                                   for a, b, c, d in zip(pw, pg, pm, pv)])
        pc = coef.to(dev)
        if entry == "adam_pack":
            L.check(lib.qt_adam_pack_weights_batched(qdt, items, state, ctypes.byref(desc), n, st), "qt_adam_pack_weights_batched")
            L.check(lib.qt_adam_multi(pit, n, ctypes.byref(desc), st), "qt_adam_multi")
        else:
            L.check(lib.qt_adam_pack_weights_batched_scaled(qdt, items, state, ctypes.byref(desc), cd.data_ptr(), n, st),
                    "qt_adam_pack_weights_batched_scaled")
            L.check(lib.qt_adam_multi_scaled(pit, n, ctypes.byref(desc), pc.data_ptr(), st), "qt_adam_multi_scaled")
        torch.cuda.synchronize()
        masters = [x.cpu() for x in pw]
        for j, b in enumerate(x for x in gd.bufs if x.name.startswith("w")):   # the masters are updated in place
            _bits_equal(b.t, pw[j], ("master", j))
            b.snapshot = b.payload.clone()
        for j in range(n):
            _bits_equal(state_view(gd, f"m{j}"), pm[j].view(-1), ("exp_avg", j))
            _bits_equal(state_view(gd, f"v{j}"), pv[j].view(-1), ("exp_avg_sq", j))
    gd.check()
    want = _pack_reference(dt, masters)
    for j, ((w, fwd, dg), (rf, rd)) in enumerate(zip(keep, want)):
        _bits_equal(fwd, rf, ("fwd", PACK_SHAPES[j]))
        if rd is not None:
            _bits_equal(dg, rd, ("dgrad", PACK_SHAPES[j]))


def _pack_desc():
    L, lib = _L()
    return L, lib, _dev(), L.stream_ptr()


@pytest.mark.parametrize("dt", [BF16, F32])
def test_standalone_weight_packers(dt):
    """qt_pack_conv_weight (both operands), qt_pack_dgrad_s2 (k = 3 and k = 1), qt_pack_dgrad_s2_merged and qt_pack_stem_weight
    (7 and 8 taps) into NaN destinations: every element written, the same bits as on plain tensors"""
    L, lib, dev, st = _pack_desc()
    qdt = L.qt_dtype(dt)
    g = torch.Generator().manual_seed(31)
    O, I = 128, 64
    w3, w1, ws = torch.randn(O, I, 3, 3, generator=g), torch.randn(O, I, 1, 1, generator=g), torch.randn(64, 3, 7, 7, generator=g)

    def case(A):
        a3, a1, as_ = A.input("w3", w3), A.input("w1", w1), A.input("w_stem", ws)
        fwd, dg = A.output("fwd", (O * 9 * I,), dt), A.output("dgrad", (O * 9 * I,), dt)
        L.check(lib.qt_pack_conv_weight(qdt, L.ptr(a3), L.ptr(fwd), L.ptr(dg), O, I, 3, 3, st), "qt_pack_conv_weight")
        c3, c1 = A.output("classes3", (O * I * 9,), dt), A.output("classes1", (O * I,), dt)
        L.check(lib.qt_pack_dgrad_s2(qdt, L.ptr(a3), L.ptr(c3), O, I, 3, None, None, None, st), "qt_pack_dgrad_s2")
        L.check(lib.qt_pack_dgrad_s2(qdt, L.ptr(a1), L.ptr(c1), O, I, 1, None, None, None, st), "qt_pack_dgrad_s2")
        mg = A.output("merged", (16 * O * I,), dt)            # NaN: this packer zeroes its unused slots itself
        L.check(lib.qt_pack_dgrad_s2_merged(qdt, L.ptr(a3), L.ptr(mg), O, I, st), "qt_pack_dgrad_s2_merged")
        s7, s8 = A.output("stem7", (64, 7, 32), dt), A.output("stem8", (64, 8, 32), dt)
        L.check(lib.qt_pack_stem_weight(qdt, L.ptr(as_), L.ptr(s7), 7, st), "qt_pack_stem_weight")
        L.check(lib.qt_pack_stem_weight(qdt, L.ptr(as_), L.ptr(s8), 8, st), "qt_pack_stem_weight")
        return fwd, dg, c3, c1, mg, s7, s8

    plain, got = _both(case)
    for a, b in zip(plain, got):
        _bits_equal(a, b)
    assert torch.equal(got[0].view(O, 3, 3, I).cpu(), w3.permute(0, 2, 3, 1).to(dt))
    assert torch.equal(got[1].view(I, 3, 3, O).cpu(), w3.permute(1, 2, 3, 0).to(dt))


@pytest.mark.parametrize("dt", [BF16, F32])
def test_pack_stem_input(dt):
    """qt_pack_stem_input at B = 1: every element of the padded destination written (zero borders, zero fourth channel)"""
    L, lib, dev, st = _pack_desc()
    image = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(22))

    def case(A):
        im = A.input("image", image)
        xpad = A.output("xpad", (1, 230, 232, 4), dt)
        L.check(lib.qt_pack_stem_input(L.qt_dtype(dt), L.ptr(im), L.ptr(xpad), 1, st), "qt_pack_stem_input")
        return xpad

    plain, got = _both(case)
    _bits_equal(plain, got)
    assert torch.equal(got.cpu(), Sb.pack_image(image, dt))


def test_unpack_weight_gradients():
    """qt_unpack_conv_wgrad and qt_unpack_stem_wgrad, writing (NaN destination) and accumulating (onto ones): exact copies"""
    L, lib, dev, st = _pack_desc()
    g = torch.Generator().manual_seed(33)
    O, I = 64, 64
    dw = torch.randn(O, 3, 3, I, generator=g)
    dws = torch.randn(64, 7, 8, 4, generator=g)
    ones, ones_s = torch.ones(O, I, 3, 3), torch.ones(64, 3, 7, 7)

    def case(A):
        a, s = A.input("dw", dw), A.input("dw_stem", dws)
        out = [A.output("grad", (O, I, 3, 3), F32), A.input("grad_acc", ones), A.output("grad_stem", (64, 3, 7, 7), F32),
               A.input("grad_stem_acc", ones_s)]
        L.check(lib.qt_unpack_conv_wgrad(L.ptr(a), L.ptr(out[0]), O, I, 3, 3, 0, st), "qt_unpack_conv_wgrad")
        L.check(lib.qt_unpack_conv_wgrad(L.ptr(a), L.ptr(out[1]), O, I, 3, 3, 1, st), "qt_unpack_conv_wgrad")
        L.check(lib.qt_unpack_stem_wgrad(L.ptr(s), L.ptr(out[2]), 0, st), "qt_unpack_stem_wgrad")
        L.check(lib.qt_unpack_stem_wgrad(L.ptr(s), L.ptr(out[3]), 1, st), "qt_unpack_stem_wgrad")
        return out

    dev = _dev()
    plain = case(Plain(dev))
    gd = Guard(dev)
    got = case(gd)
    for b in gd.bufs:
        if b.name.endswith("_acc"):      # accumulated in place: inputs only as far as the bands go
            torch.cuda.synchronize()
            b.snapshot = b.payload.clone()
    gd.check()
    for a, b in zip(plain, got):
        _bits_equal(a, b)
    want, want_s = dw.permute(0, 3, 1, 2), dws[:, :, :7, :3].permute(0, 3, 1, 2)
    assert torch.equal(got[0].cpu(), want) and torch.equal(got[1].cpu(), want + 1)
    assert torch.equal(got[2].cpu(), want_s) and torch.equal(got[3].cpu(), want_s + 1)


# ======================================================================================================================
# c. the plan workspace
# ======================================================================================================================
def _quadtree(dt, guard):
    """QuadtreeCNN at max_batch = 2 with its engine built; guard: the workspace is exactly qt_plan_workspace_bytes of NaN
    between two bands (tests/_plan_gaps.py::rehome)."""
    P, synth = pkg(), pkg("synth")
    dev = _dev()
    m = P.QuadtreeCNN(12, dropout_rate=0.0, compute_dtype=dt, max_batch=2)
    m.load_state_dict(synth.synth_state_dict(m))
    m = m.to(dev).train()
    eng = m._ensure_engine(2, dev)
    if guard is not None:
        rehome(eng, guard)
    return m


def _plan_run(models, checks, share_grads):
    """tests/_plan_gaps.py::plan_run at B = 2 and B = 1"""
    synth = pkg("synth")
    dev = _dev()
    data = (synth.synth_images(2, salt=5).to(dev), synth.synth_pose_features(2, salt=5).to(dev),
            synth.synth_labels(2, 12, salt=5).to(dev))
    return plan_run(models, checks, share_grads, data, small=1)


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
def test_plan_on_a_guarded_workspace(dt):
    dev = _dev()
    guard = Guard(dev)
    models = [_quadtree(dt, None), _quadtree(dt, guard)]
    ws = guard.bufs[0].t
    want, got = _plan_run(models, [torch.cuda.synchronize, guard.check], share_grads=(dt == F32))
    # the engine was not rebuilt on the way: every call above ran on the guarded workspace
    eng = models[1]._engine
    assert eng.workspace is ws and eng.ws_ptr.value == ws.data_ptr() and ws.numel() == eng.workspace_bytes
    # bf16: bit for bit; f32: ADAM_TOL for the stepped parameters, 1e-3 for the gradients, 1e-5 for the rest
    compare_twins(want, got, dt)
