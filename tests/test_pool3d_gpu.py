"""The kernels between the clip models' convolutions through the C ABI -- qt_pool3d_max, qt_pool3d_max_bwd, qt_pool3d_bn_relu_max,
qt_pool3d_bn_bwd_apply (general and resident-grid kernel), qt_pack_conv3d_block (element-per-thread and LDS-tile kernel),
qt_unpack_conv3d_wgrad, qt_pack_clip27 (csrc/video3d.hip) -- against the hand-written float64 reference of tests/_pool3d_bounds.py:
bit for bit wherever the result is a selection or the input class makes it exact (pooled map, argmax codes, y at the maximum, dx,
g; dy of the grid class, its bf16 rounding included; every packed operand), inside bounds DERIVED from the kernel's own
arithmetic elsewhere (dy of the random class, dgamma / dbeta through qt_bn_bwd_reduce on the pooled side + qt_bn_bwd_finalize).
tests/test_pool3d_bounds_cpu.py shows that correct f32 arithmetic passes the same comparisons and that a subtly wrong kernel
does not.  Every backward kernel gets the REFERENCE's pooled map and codes, so one kernel's error cannot hide another's.  Output
buffers are pre-filled with NaN / 0xFF and carry a guard row that must stay as it was; tests print max(|err| / bound).

Not reached here (see _pool3d_bounds.py): the 65 536-block cap of the pool kernels and of qt_pack_clip27 (more than 16.7 M groups:
tests/test_grid_caps_gpu.py, on a slab of images repeated along the batch); QTCNN_PACK3D_TILED=0 and QTCNN_POOL3D_APPLY_LIGHT=0,
which are read once per process and have no setter.

Reference behaviour: BatchNorm3d -> ReLU -> MaxPool3d of a conv block of the reference's Quadtree3DCNN (3dcnn/models.py) and
their autograd; nn.Conv3d's weight layout."""
import math

import pytest
import torch

import _pool3d_bounds as Pb
from _util import pkg

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")
QT_ERR_INVALID_ARG = -1
KINDS = ["grid", "random"]
POOL_RUNS = [("c1", 1, "f32"), ("c1", 1, "bf16"), ("c1", 2, "f32"), ("c1", 2, "bf16"), ("c2", 1, "bf16"), ("c2", 2, "f32"),
             ("c3", 1, "f32"), ("c3", 2, "bf16")]


@pytest.fixture(scope="module", autouse=True)
def _drop_references():
    yield
    Pb.clear_caches()


def _env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    L = pkg("_lib")
    return torch.device("cuda:0"), L, L.lib()


class _Out:
    """an output buffer pre-filled with NaN (0xFF for bytes) + one guard row behind it"""

    def __init__(self, shape, dt, dev):
        self.n = math.prod(shape)
        self.fill = 0xFF if dt == torch.uint8 else NAN
        self.whole = torch.full((self.n + max(shape[-1], 64),), self.fill, dtype=dt, device=dev)
        self.t = self.whole[:self.n].view(shape)

    def cpu(self):
        """the result, after checking that nothing was written behind it"""
        tail = self.whole[self.n:]
        assert bool((tail == 0xFF).all() if self.fill == 0xFF else torch.isnan(tail).all()), "guard row overwritten"
        return self.t.cpu()

    def untouched(self):
        return bool((self.whole == 0xFF).all() if self.fill == 0xFF else torch.isnan(self.whole).all())


def _report(name, r):
    print(f"  err/bound {name}: {r:.3f}")
    assert r <= 1.0, (name, r)


def _dev_inputs(c, dev):
    """the case's tensors on the device: maps in the activation type, per-channel vectors in f32, the reference's codes"""
    dt = c["dt"]
    f = lambda t: t.float().to(dev).contiguous()
    return dict(y=c["y"].to(dt).to(dev), x=c["x"].to(dt).to(dev), d=c["d"].to(dt).to(dev), code=c["code"].to(dev),
                xcode=c["xcode"].to(dev), pooled=c["pooled"].to(dt).to(dev), ymax=c["ymax"].to(dt).to(dev), scale=f(c["scale"]),
                shift=f(c["shift"]), mean=f(c["mean"]), invstd=f(c["invstd"]), coef=f(c["coef"]))


def _apply(L, lib, t, c, dev, Cy=None, Cd=None, light_min=None):
    """qt_pool3d_bn_bwd_apply on the reference's pooled map and codes; light_min: the resident-grid threshold for this call"""
    T, B, H, W, C = c["shape"]
    Cy, Cd = C if Cy is None else Cy, C if Cd is None else Cd
    dy = _Out((T, B, H, W, Cd), c["dt"], dev)
    if light_min is not None:
        lib.qt_set_pool3d_apply_light_min(light_min)
    try:
        L.check(lib.qt_pool3d_bn_bwd_apply(L.qt_dtype(c["dt"]), L.ptr(t["d"]), L.ptr(t["code"]), L.ptr(t["pooled"]), L.ptr(t["y"]),
                                           L.ptr(t["mean"]), L.ptr(t["invstd"]), L.ptr(t["coef"]), L.ptr(dy.t), T, B, H, W, C, Cy, Cd,
                                           c["pt"], L.stream_ptr()), "qt_pool3d_bn_bwd_apply")
        torch.cuda.synchronize()
    finally:
        if light_min is not None:
            lib.qt_set_pool3d_apply_light_min(0)
    return dy.cpu()


# ----------------------------------------------------------------------------------------------------------------------
# MaxPool3d and its backward
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pt,dtn", POOL_RUNS)
@pytest.mark.parametrize("kind", KINDS)
def test_pool3d_max_and_backward_bit_exact(kind, name, pt, dtn):
    dev, L, lib = _env()
    c = Pb.case(kind, name, pt, dtn)
    t = _dev_inputs(c, dev)
    dt, (T, B, H, W, C) = c["dt"], c["shape"]
    q, st = L.qt_dtype(dt), L.stream_ptr()
    ps = Pb.pooled_shape(T, B, H, W, C, pt)
    out, arg, only = _Out(ps, dt, dev), _Out(ps, torch.uint8, dev), _Out(ps, dt, dev)
    L.check(lib.qt_pool3d_max(q, L.ptr(t["x"]), L.ptr(out.t), L.ptr(arg.t), T, B, H, W, C, pt, st), "qt_pool3d_max")
    L.check(lib.qt_pool3d_max(q, L.ptr(t["x"]), L.ptr(only.t), None, T, B, H, W, C, pt, st), "qt_pool3d_max (no argmax)")
    dx = _Out((T, B, H, W, C), dt, dev)
    L.check(lib.qt_pool3d_max_bwd(q, L.ptr(t["d"]), L.ptr(t["xcode"]), L.ptr(dx.t), T, B, H, W, C, pt, st), "qt_pool3d_max_bwd")
    torch.cuda.synchronize()
    assert Pb.pool_failures(c, out.cpu(), arg.cpu()) == []
    assert Pb.same(only.cpu(), c["xpooled"])
    assert Pb.same(dx.cpu(), c["dx"]), "dx"


# ----------------------------------------------------------------------------------------------------------------------
# BatchNorm3d + ReLU + MaxPool3d in one pass: pooled, argmax, y at the maximum -- bit for bit
# ----------------------------------------------------------------------------------------------------------------------
def _fused(L, lib, t, c, dev, Cy=None, train=True):
    T, B, H, W, C = c["shape"]
    ps = Pb.pooled_shape(T, B, H, W, C, c["pt"])
    y = t["y"] if Cy is None else t["y"][..., :Cy].contiguous()
    out = _Out(ps, c["dt"], dev)
    arg, ymax = (_Out(ps, torch.uint8, dev), _Out(ps, c["dt"], dev)) if train else (None, None)
    L.check(lib.qt_pool3d_bn_relu_max(L.qt_dtype(c["dt"]), L.ptr(y), L.ptr(t["scale"]), L.ptr(t["shift"]), L.ptr(out.t),
                                      L.ptr(arg.t) if train else None, L.ptr(ymax.t) if train else None, T, B, H, W, C,
                                      C if Cy is None else Cy, c["pt"], L.stream_ptr()), "qt_pool3d_bn_relu_max")
    torch.cuda.synchronize()
    return out.cpu(), arg.cpu() if train else None, ymax.cpu() if train else None


@pytest.mark.parametrize("name,pt,dtn", POOL_RUNS)
@pytest.mark.parametrize("kind", KINDS)
def test_fused_forward_bit_exact(kind, name, pt, dtn):
    dev, L, lib = _env()
    c = Pb.case(kind, name, pt, dtn)
    t = _dev_inputs(c, dev)
    pooled, arg, ymax = _fused(L, lib, t, c, dev)
    assert Pb.forward_failures(c, pooled, arg, ymax) == []
    assert Pb.forward_failures(c, _fused(L, lib, t, c, dev, train=False)[0], None, None) == []      # the eval form


# ----------------------------------------------------------------------------------------------------------------------
# max-pool backward + ReLU mask + BatchNorm backward in one pass
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pt,dtn", POOL_RUNS)
@pytest.mark.parametrize("kind", KINDS)
def test_fused_backward_vs_float64(kind, name, pt, dtn):
    dev, L, lib = _env()
    c = Pb.case(kind, name, pt, dtn)
    t = _dev_inputs(c, dev)
    T, B, H, W, C = c["shape"]
    n = Pb.apply_groups(T, B, H, W, C)
    assert not Pb.light_taken(c["dt"], C, C, C, n)                                  # the general kernel
    bad, r = Pb.dy_check(c, _apply(L, lib, t, c, dev))
    assert bad == [], bad
    if r is not None:
        _report(f"pool3d_bn_bwd_apply {kind} {name} pool_t={pt} {dtn}", r)
    if name == "c3" and dtn == "bf16":   # 3 groups per row do not divide the resident grid: still the general kernel, still right
        assert not Pb.light_taken(c["dt"], C, C, C, n, 1)
        assert Pb.dy_check(c, _apply(L, lib, t, c, dev, light_min=1))[0] == []


@pytest.mark.parametrize("pt", [1, 2])
@pytest.mark.parametrize("dtn", ["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_narrow_rows(kind, dtn, pt):
    """y rows of 32 channels feeding 64-channel pooled rows, dy rows of 32 or 64: the first 32 channels as in the full-width run,
    zeros above; what lies in the padding channels of the inputs (here: never zero) is not read"""
    dev, L, lib = _env()
    c = Pb.case(kind, "c1", pt, dtn)
    t = _dev_inputs(c, dev)
    C, Cy = c["shape"][4], 32
    for k in ("scale", "shift"):
        t[k] = t[k].clone()
        t[k][Cy:] = 3.0
    pooled, arg, ymax = _fused(L, lib, t, c, dev, Cy=Cy)
    assert Pb.forward_failures(c, pooled, arg, ymax, Cy=Cy) == []
    t["y"] = t["y"][..., :Cy].contiguous()
    for k, v in (("d", 3.0), ("pooled", 7.0), ("code", 5)):
        t[k] = t[k].clone()
        t[k][..., Cy:] = v
    for k in ("mean", "invstd", "coef"):
        t[k] = t[k].clone()
        t[k][..., Cy:] = 3.0
    for Cd in (Cy, C):
        bad, r = Pb.dy_check(c, _apply(L, lib, t, c, dev, Cy=Cy, Cd=Cd, light_min=1), Cy=Cy, Cd=Cd)
        assert bad == [], (Cd, bad)
        if r is not None:
            _report(f"pool3d_bn_bwd_apply {kind} c1 pool_t={pt} {dtn} y_channels={Cy} dy_channels={Cd}", r)


@pytest.mark.parametrize("dtn", ["f32", "bf16"])
@pytest.mark.parametrize("name,pt", [("c1", 1), ("c1", 2), ("c2", 2)])
def test_bn_backward_sums_from_the_pooled_side_vs_float64(name, pt, dtn):
    """the chain the model runs: qt_bn_bwd_reduce over the pooled cells (dout, pooled as the ReLU mask, y at the maximum), then
    qt_bn_bwd_finalize -- against the float64 sums over every position of the full-size map"""
    dev, L, lib = _env()
    c = Pb.case("random", name, pt, dtn)
    t = _dev_inputs(c, dev)
    T, B, H, W, C = c["shape"]
    q, st = L.qt_dtype(c["dt"]), L.stream_ptr()
    cells, M = c["d"].numel() // C, T * B * H * W
    rows = lib.qt_bn_bwd_partial_rows(cells, C)
    assert rows > 0
    part = _Out((lib.qt_stats_capacity_rows(rows), 2, C), F32, dev)
    L.check(lib.qt_bn_bwd_reduce(q, L.ptr(t["d"]), L.ptr(t["pooled"]), L.ptr(t["ymax"]), L.ptr(t["mean"]), L.ptr(t["invstd"]),
                                 L.ptr(part.t), cells, C, st), "qt_bn_bwd_reduce (pooled side)")
    gamma = c["gamma"].float().to(dev)
    dgamma, dbeta, coef = _Out((C,), F32, dev), _Out((C,), F32, dev), _Out((3, C), F32, dev)
    L.check(lib.qt_bn_bwd_finalize(L.ptr(part.t), rows, C, M, L.ptr(gamma), L.ptr(t["invstd"]), L.ptr(dgamma.t), L.ptr(dbeta.t),
                                   0, L.ptr(coef.t), st), "qt_bn_bwd_finalize")
    torch.cuda.synchronize()
    p = part.cpu()
    assert bool(torch.isfinite(p[:rows]).all()) and bool(torch.isnan(p[rows:]).all())
    r = Pb.bn_sums_ratios(c, p[:rows], cells, dgamma.cpu(), dbeta.cpu(), coef.cpu())
    for k, v in r.items():
        _report(f"bn backward from the pooled side {name} pool_t={pt} {dtn} {k}", v)


# ----------------------------------------------------------------------------------------------------------------------
# the resident-grid apply kernel: idle threads, a second row live for part of the grid, a second trip
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pt", Pb.LIGHT_CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_resident_grid_apply_vs_float64(kind, name, pt):
    dev, L, lib = _env()
    T, B, H, W, C = Pb.shape(name, pt)
    n, S = Pb.apply_groups(T, B, H, W, C), Pb.LIGHT_THREADS
    lo, hi = {"L1": (0, S), "L2": (S, 2 * S), "L3": (2 * S, 3 * S)}[name]
    assert lo < n < hi and C // 8 == 32 and S % (C // 8) == 0
    assert Pb.light_taken(BF16, C, C, C, n, 1) and not Pb.light_taken(BF16, C, C, C, n, n + 1)
    c = Pb.build(kind, name, pt, "bf16")
    t = _dev_inputs(c, dev)
    light = _apply(L, lib, t, c, dev, light_min=1)
    general = _apply(L, lib, t, c, dev, light_min=n + 1)
    bad, r = Pb.dy_check(c, light)
    assert bad == [], ("resident grid", bad)
    bad, _ = Pb.dy_check(c, general)
    assert bad == [], ("general kernel", bad)
    assert torch.equal(light.view(torch.int16), general.view(torch.int16))           # the same arithmetic: the same bits
    if r is not None:
        _report(f"pool3d_bn_bwd_apply (resident grid) {kind} {name} pool_t={pt} bf16", r)


# ----------------------------------------------------------------------------------------------------------------------
# the packers
# ----------------------------------------------------------------------------------------------------------------------
PACK_RUNS = [s + (0,) for s in Pb.PACK_TILE + Pb.PACK_ELEMENT] + [(O, Op, I, 0, 1) for O, Op, I in Pb.PACK_FIRST]


def _weight_on_device(w, dev, offset):
    """the weight at a 16-byte aligned address, or at a view 4 bytes behind one"""
    flat = torch.empty(w.numel() + 4, dtype=F32, device=dev)
    assert flat.data_ptr() % 16 == 0
    view = flat[1:1 + w.numel()] if offset else flat[:w.numel()]
    view.copy_(w.flatten())
    assert view.data_ptr() % 16 == (4 if offset else 0)
    return flat, view


def _pack(L, lib, dev, dt, wv, O, I, Op, Ip, first, vecs, with_wd):
    nf = Op * 128 if first else Op * 27 * Ip
    keep = [None if v is None else v.to(dev) for v in vecs]
    table = torch.tensor([0 if v is None else v.data_ptr() for v in keep], dtype=torch.int64).to(dev)
    wf, vec = _Out((nf,), dt, dev), _Out((5, Op), F32, dev)
    wd = _Out((nf,), dt, dev) if with_wd else None
    L.check(lib.qt_pack_conv3d_block(L.qt_dtype(dt), L.ptr(wv), L.ptr(wf.t), L.ptr(wd.t) if with_wd else None, O, I, Op, Ip, first,
                                     L.ptr(table), L.ptr(vec.t), L.stream_ptr()), "qt_pack_conv3d_block")
    torch.cuda.synchronize()
    return wf.cpu(), wd.cpu() if with_wd else None, vec.cpu()


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", PACK_RUNS, ids=lambda s: "O{}p{}_I{}p{}_first{}".format(*s))
def test_pack_conv3d_block_equals_the_layout(shape, dt):
    dev, L, lib = _env()
    O, Op, I, Ip, first = shape
    w, vecs = Pb.pack_weights(O, I, O + I), Pb.pack_vectors(O, O)
    assert Pb.bf16_tie_share(w) >= 0.01 and vecs[0] is None
    rf, rd, rv = Pb.pack_ref(w, Op, Ip, first, vecs)
    tile = Pb.pack_kernel(O, Op, I, Ip, first) == "tile"
    for offset in ((0, 1) if tile else (0,)):       # 4 bytes off a 16-byte boundary: the launcher takes the element kernel
        assert Pb.pack_kernel(O, Op, I, Ip, first, aligned=not offset) == ("tile" if tile and not offset else "element")
        _, wv = _weight_on_device(w, dev, offset)
        for with_wd in (True, False):
            wf, wd, vec = _pack(L, lib, dev, dt, wv, O, I, Op, Ip, first, vecs, with_wd)
            tag = (shape, dt, "offset" if offset else "aligned", "w_dgrad" if with_wd else "no w_dgrad")
            assert Pb.same(wf, rf.to(dt).flatten()), ("w_fwd",) + tag        # f32: the values; bf16: round-to-nearest-even
            if with_wd and first:                                             # the first layer has no data-gradient operand
                assert bool(torch.isnan(wd).all()), ("w_dgrad written",) + tag
            elif with_wd:
                assert Pb.same(wd, rd.to(dt).flatten()), ("w_dgrad",) + tag
            assert Pb.same(vec, rv), ("vec",) + tag
            assert bool((vec[0] == 0).all())                                  # no bias: the whole row is the pad value


@pytest.mark.parametrize("shape", PACK_RUNS, ids=lambda s: "O{}p{}_I{}p{}_first{}".format(*s))
def test_unpack_conv3d_wgrad_and_round_trip(shape):
    dev, L, lib = _env()
    O, Op, I, Ip, first = shape
    st = L.stream_ptr()
    n = Op * 128 if first else 3 * Op * 9 * Ip
    assert n < 2 ** 24
    dw = torch.arange(n, dtype=F32)                   # distinct integers, the padding slots included
    out = _Out((O, I, 27), F32, dev)
    L.check(lib.qt_unpack_conv3d_wgrad(L.ptr(dw.to(dev)), L.ptr(out.t), O, I, Op, Ip, first, st), "qt_unpack_conv3d_wgrad")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), Pb.unpack_ref(dw, O, I, Op, Ip, first))
    # round trip: pack an integer weight in f32, regroup the forward operand as the weight gradient is laid out, unpack
    w = Pb.pack_weights(O, I, 3 * O + I, integer=True)
    _, wv = _weight_on_device(w, dev, 0)
    wf, _, _ = _pack(L, lib, dev, F32, wv, O, I, Op, Ip, first, [None] * 5, False)
    back = _Out((O, I, 27), F32, dev)
    as_dw = Pb.forward_operand_as_wgrad(wf, Op, Ip, first).to(dev)
    L.check(lib.qt_unpack_conv3d_wgrad(L.ptr(as_dw), L.ptr(back.t), O, I, Op, Ip, first, st), "qt_unpack_conv3d_wgrad")
    torch.cuda.synchronize()
    assert torch.equal(back.cpu(), w)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", Pb.CLIP_SHAPES, ids=lambda s: "B{}_T{}_H{}_W{}".format(*s))
def test_pack_clip27_equals_the_27_taps(shape, dt):
    dev, L, lib = _env()
    B, T, H, W = shape
    clips = torch.randint(-8, 9, (B, T, 3, H, W), generator=torch.Generator().manual_seed(B * 7 + T)).float()
    dst = _Out((T, B, H, W, 128), dt, dev)
    L.check(lib.qt_pack_clip27(L.qt_dtype(dt), L.ptr(clips.to(dev)), L.ptr(dst.t), B, T, H, W, L.stream_ptr()), "qt_pack_clip27")
    torch.cuda.synchronize()
    got = dst.cpu()
    assert torch.equal(got.float(), Pb.clip27_ref(clips)) and bool((got[..., 81:] == 0).all())


# ----------------------------------------------------------------------------------------------------------------------
# refusals: QT_ERR_INVALID_ARG, nothing written
# ----------------------------------------------------------------------------------------------------------------------
BAD_POOL = [dict(pt=3), dict(T=1, pt=2), dict(H=1), dict(C=12), dict(Cy=24), dict(C=0), dict(C=-8)]


@pytest.mark.parametrize("bad", BAD_POOL, ids=lambda b: "_".join(f"{k}{v}" for k, v in b.items()))
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_pool_entry_points_refuse(dt, bad):
    dev, L, lib = _env()
    a = dict(T=2, B=1, H=2, W=2, C=16, Cy=16, pt=2)
    a.update(bad)
    if "C" in bad:
        a["Cy"] = 8 if bad["C"] == 12 else bad["C"]       # (the channel count itself is what must be refused)
    T, B, H, W, C, Cy, pt = (a[k] for k in ("T", "B", "H", "W", "C", "Cy", "pt"))
    q, st = L.qt_dtype(dt), L.stream_ptr()
    full, cell = (2, 1, 2, 2, 16), (1, 1, 1, 1, 16)
    src = torch.ones(full, dtype=dt, device=dev)
    vec = torch.ones(3, 16, device=dev)
    code = torch.zeros(cell, dtype=torch.uint8, device=dev)
    small = torch.ones(cell, dtype=dt, device=dev)
    outs = [_Out(full, dt, dev), _Out(cell, dt, dev), _Out(cell, torch.uint8, dev), _Out(cell, dt, dev)]
    big, o1, o2, o3 = outs
    status = []
    if "Cy" not in bad:   # (the plain pool has no y_channels)
        status.append(lib.qt_pool3d_max(q, L.ptr(src), L.ptr(o1.t), L.ptr(o2.t), T, B, H, W, C, pt, st))
        status.append(lib.qt_pool3d_max_bwd(q, L.ptr(small), L.ptr(code), L.ptr(big.t), T, B, H, W, C, pt, st))
    status.append(lib.qt_pool3d_bn_relu_max(q, L.ptr(src), L.ptr(vec[0]), L.ptr(vec[1]), L.ptr(o1.t), L.ptr(o2.t), L.ptr(o3.t), T, B, H, W,
                                            C, Cy, pt, st))
    status.append(lib.qt_pool3d_bn_bwd_apply(q, L.ptr(small), L.ptr(code), L.ptr(small), L.ptr(src), L.ptr(vec[0]), L.ptr(vec[1]),
                                             L.ptr(vec), L.ptr(big.t), T, B, H, W, C, Cy, max(Cy, 8), pt, st))
    torch.cuda.synchronize()
    assert status == [QT_ERR_INVALID_ARG] * len(status), (a, status, lib.qt_last_error())
    assert all(o.untouched() for o in outs)


@pytest.mark.parametrize("first", [0, 1])
def test_packers_refuse(first):
    dev, L, lib = _env()
    st = L.stream_ptr()
    w = torch.ones(16 * 16 * 27 + 4, device=dev)
    table = torch.zeros(5, dtype=torch.int64, device=dev)
    outs = [_Out((64 * 27 * 64,), F32, dev), _Out((64 * 27 * 64,), F32, dev), _Out((5, 64), F32, dev), _Out((16, 16, 27), F32, dev)]
    wf, wd, vec, dW = outs
    bad = [(16, 16, 8, 64), (16, 16, 64, 8)] if not first else [(16, 4, 8, 0), (32, 5, 64, 0)]    # (O, I, O_pad, I_pad)
    for O, I, Op, Ip in bad:
        assert Op < O or (not first and Ip < I) or (first and 27 * I > 128)
        rc = lib.qt_pack_conv3d_block(0, L.ptr(w), L.ptr(wf.t), None if first else L.ptr(wd.t), O, I, Op, Ip, first, L.ptr(table),
                                      L.ptr(vec.t), st)
        assert rc == QT_ERR_INVALID_ARG, (O, I, Op, Ip, first)
        if 27 * I <= 128 or not first:
            rc = lib.qt_unpack_conv3d_wgrad(L.ptr(w), L.ptr(dW.t), O, I, Op, Ip, first, st)
            assert rc == QT_ERR_INVALID_ARG, (O, I, Op, Ip, first)
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)
