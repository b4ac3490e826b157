"""The stem tail through the C ABI -- qt_stem_pool, qt_stem_pool_bwd, qt_stem_bn_bwd_reduce / _sums / _apply
(csrc/elementwise.hip) and the one-launch stem backward qt_stem_bn_bwd_wgrad_ws (csrc/conv_wgrad.hip) -- against the hand-written
float64 reference of tests/_stem_bounds.py: bit for bit wherever the input class makes the result exact (the whole forward, g and
the BatchNorm-backward sums of the grid class, the sparse probe of the one-launch backward), inside bounds DERIVED from the kernel's
own arithmetic elsewhere (tests/test_stem_bounds_cpu.py shows that correct f32 arithmetic meets them).  Batches 1, 3 and 11: at 11
the one-launch backward walks up to three tiles per workgroup through both LDS buffers, across an image boundary and into a
last-row tile in a reused buffer, the reduce / sums grids are capped and the light sums kernel takes its tail.  Every kernel
gets the REFERENCE's inputs (argmax codes, y at the maximum), so one kernel's error cannot hide another's.  Output buffers are
pre-filled with NaN / 0xFF; every test prints max(|err| / bound).

Not reached here (see _stem_bounds.py): the 16384-block cap of the pool / pool-backward / apply kernels (B >= 42 / 168), which
tests/test_grid_caps_gpu.py reaches on repeated images, and the bf16 instantiation of the general sums kernel (a process-wide
switch).

Reference behaviour: bn1 -> relu -> maxpool of torchvision's ResNet-18 stem and their autograd, as the reference's QuadtreeCNN
runs them (Quadtree_from scratch/models.py:224-226)."""
import ctypes

import pytest
import torch

import _bounds as Bd
import _stem_bounds as Sb
from _util import pkg

pytestmark = pytest.mark.gpu

H, W, P, C = Sb.H, Sb.W, Sb.P, Sb.C
F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")
KINDS = ["grid", "random"]


@pytest.fixture(scope="module", autouse=True)
def _drop_references():
    yield
    Sb.clear_caches()


def _env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    L = pkg("_lib")
    return torch.device("cuda:0"), L, L.lib()


def _report(name, r):
    print(f"  err/bound {name}: {r:.3f}")
    assert r <= 1.0, (name, r)


def _nan(shape, dt, dev):
    return torch.full(shape, NAN, dtype=dt, device=dev)


def _dev_inputs(c, dt, dev, coef=None, d=None):
    """the case's tensors on the device: activations in dt, per-channel vectors in f32, the reference's argmax codes"""
    f = lambda t: t.float().to(dev).contiguous()
    return dict(y=c["y"].to(dt).to(dev), d=(c["d"] if d is None else d).to(dt).to(dev), code=c["code"].to(dev),
                ymax=c["ymax"].to(dt).to(dev), scale=f(c["scale"]), shift=f(c["shift"]), mean=f(c["mean"]), invstd=f(c["invstd"]),
                coef=f(c["coef"] if coef is None else coef))


# ----------------------------------------------------------------------------------------------------------------------
# forward: pooled, argmax, y at the maximum -- bit for bit
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("B", Sb.BATCHES)
@pytest.mark.parametrize("kind", KINDS)
def test_stem_pool_forward_bit_exact(kind, B, dt):
    dev, L, lib = _env()
    c = Sb.case(kind, B)
    t = _dev_inputs(c, dt, dev)
    qdt, st = L.qt_dtype(dt), L.stream_ptr()
    pooled, ymax = _nan((B, P, P, C), dt, dev), _nan((B, P, P, C), dt, dev)
    code = torch.full((B, P, P, C), 0xFF, dtype=torch.uint8, device=dev)
    L.check(lib.qt_stem_pool(qdt, L.ptr(t["y"]), L.ptr(t["scale"]), L.ptr(t["shift"]), L.ptr(pooled), L.ptr(code), L.ptr(ymax),
                             B, st), "qt_stem_pool")
    only = _nan((B, P, P, C), dt, dev)      # the eval form: no argmax, no y at the maximum
    L.check(lib.qt_stem_pool(qdt, L.ptr(t["y"]), L.ptr(t["scale"]), L.ptr(t["shift"]), L.ptr(only), None, None, B, st),
            "qt_stem_pool (eval)")
    torch.cuda.synchronize()
    # the activation is exact in f32 (and in bf16 on the grid class): the stored maximum is ONE rounding of a known value
    want = c["pooled"].to(dt)
    if dt == F32 or c["exact_bf16"]:
        assert torch.equal(want.double(), c["pooled"])
    assert torch.equal(pooled.cpu(), want), "pooled"
    assert torch.equal(only.cpu(), want), "pooled (eval form)"
    assert bool((pooled.view(torch.int16 if dt == BF16 else torch.int32) >= 0).all())      # +0, never -0
    wrong = code.cpu() != c["code"]
    assert not bool(wrong.any()), ("argmax", int(wrong.sum()), torch.nonzero(wrong)[:4].tolist())
    assert torch.equal(ymax.cpu().double(), c["ymax"]), "y_at_max"


# ----------------------------------------------------------------------------------------------------------------------
# g = max-pool backward + ReLU mask
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("B", Sb.BATCHES)
@pytest.mark.parametrize("kind", KINDS)
def test_stem_pool_bwd_vs_float64(kind, B, dt):
    dev, L, lib = _env()
    c = Sb.case(kind, B)
    t = _dev_inputs(c, dt, dev)
    g = _nan((B, H, W, C), dt, dev)
    L.check(lib.qt_stem_pool_bwd(L.qt_dtype(dt), L.ptr(t["d"]), L.ptr(t["code"]), L.ptr(t["y"]), L.ptr(t["scale"]),
                                 L.ptr(t["shift"]), L.ptr(g), B, L.stream_ptr()), "qt_stem_pool_bwd")
    torch.cuda.synchronize()
    got = g.cpu()
    _report(f"stem_pool_bwd {kind} B={B} {dt}", Bd.ratio(got, c["g"], Sb.g_bound(c["g"], c["gabs"], dt)))
    if kind == "grid":
        assert torch.equal(got.double(), c["g"])


# ----------------------------------------------------------------------------------------------------------------------
# BatchNorm-backward sums: from the positions (reduce) and from the pooled side (sums: general kernel in f32, light in bf16)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("B", Sb.BATCHES)
@pytest.mark.parametrize("kind", KINDS)
def test_stem_bn_bwd_sums_vs_float64(kind, B, dt):
    dev, L, lib = _env()
    c = Sb.case(kind, B)
    t = _dev_inputs(c, dt, dev)
    qdt, st = L.qt_dtype(dt), L.stream_ptr()
    S = c["S"]
    rows_r, rows_s = lib.qt_stem_bn_bwd_rows(B), lib.qt_stem_bn_bwd_sums_rows(B)
    assert (rows_r, rows_s) == (Sb.reduce_rows(B), Sb.sums_rows(B))
    part_r = _nan((lib.qt_stats_capacity_rows(rows_r), 2, C), F32, dev)
    part_s = _nan((lib.qt_stats_capacity_rows(rows_s), 2, C), F32, dev)
    L.check(lib.qt_stem_bn_bwd_reduce(qdt, L.ptr(t["d"]), L.ptr(t["code"]), L.ptr(t["y"]), L.ptr(t["scale"]), L.ptr(t["shift"]),
                                      L.ptr(t["mean"]), L.ptr(t["invstd"]), L.ptr(part_r), B, st), "qt_stem_bn_bwd_reduce")
    L.check(lib.qt_stem_bn_bwd_sums(qdt, L.ptr(t["d"]), L.ptr(t["ymax"]), L.ptr(t["scale"]), L.ptr(t["shift"]), L.ptr(t["mean"]),
                                    L.ptr(t["invstd"]), L.ptr(part_s), B, st), "qt_stem_bn_bwd_sums")
    torch.cuda.synchronize()
    light = dt == BF16
    bounds = {"reduce": Sb.sums_bound(S, Sb.chain_reduce(B)),
              "sums": Sb.light_bound(S, Sb.chain_light(B), c["mean"], c["invstd"]) if light else Sb.sums_bound(S, Sb.chain_sums(B))}
    for name, part, rows in (("reduce", part_r, rows_r), ("sums", part_s, rows_s)):
        p = part[:rows].cpu()
        assert bool(torch.isfinite(p).all()), name                     # every row written,
        assert bool(torch.isnan(part[rows:]).all()), name              # and none beyond
        s1, s2 = p[:, 0].double().sum(0), p[:, 1].double().sum(0)      # the partial rows, added in float64 by the test
        if kind == "grid":                                             # every row sum is exact: a dropped or doubled element shows
            assert torch.equal(s1, S["s1"]), (name, "sum g", float((s1 - S["s1"]).abs().max()))
            assert torch.equal(s2, S["s2"]), (name, "sum g xhat", float((s2 - S["s2"]).abs().max()))
            print(f"  {name}{' (light)' if light and name == 'sums' else ''} {kind} B={B} {dt}: equal")
        else:
            b1, b2 = bounds[name]
            tag = f"stem_bn_bwd_{name}{' (light)' if light and name == 'sums' else ''} {kind} B={B} {dt}"
            _report(tag + " sum g", Bd.ratio(s1, S["s1"], b1))
            _report(tag + " sum g xhat", Bd.ratio(s2, S["s2"], b2))


# ----------------------------------------------------------------------------------------------------------------------
# dy = a (g - b - xhat c), gathered
# ----------------------------------------------------------------------------------------------------------------------
def _apply(L, lib, t, dt, B, dev):
    dy = _nan((B, H, W, C), dt, dev)
    L.check(lib.qt_stem_bn_bwd_apply(L.qt_dtype(dt), L.ptr(t["d"]), L.ptr(t["code"]), L.ptr(t["y"]), L.ptr(t["scale"]),
                                     L.ptr(t["shift"]), L.ptr(t["mean"]), L.ptr(t["invstd"]), L.ptr(t["coef"]), L.ptr(dy), B,
                                     L.stream_ptr()), "qt_stem_bn_bwd_apply")
    return dy


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("B", Sb.BATCHES)
@pytest.mark.parametrize("kind", KINDS)
def test_stem_bn_bwd_apply_vs_float64(kind, B, dt):
    dev, L, lib = _env()
    c = Sb.case(kind, B)
    dy = _apply(L, lib, _dev_inputs(c, dt, dev), dt, B, dev)
    torch.cuda.synchronize()
    bound = Sb.dy_bound(c["dy"], c["g"], c["y"], c["mean"], c["invstd"], c["coef"], dt)
    _report(f"stem_bn_bwd_apply {kind} B={B} {dt}", Bd.ratio(dy.cpu(), c["dy"], bound))


# ----------------------------------------------------------------------------------------------------------------------
# the one-launch stem backward (bf16)
# ----------------------------------------------------------------------------------------------------------------------
def _fused(L, lib, t, xpad, B, dev, short=0, dt=BF16):
    nws = lib.qt_stem_bn_bwd_wgrad_workspace_bytes(B)
    assert nws == min(B * 56, 256) * 64 * 7 * 32 * 4
    ws = _nan((nws // 4,), F32, dev)
    dw = torch.zeros(C, 7, 8, 4, dtype=F32, device=dev)
    rc = lib.qt_stem_bn_bwd_wgrad_ws(L.qt_dtype(dt), L.ptr(t["d"]), L.ptr(t["code"]), L.ptr(t["y"]), L.ptr(t["scale"]),
                                     L.ptr(t["shift"]), L.ptr(t["mean"]), L.ptr(t["invstd"]), L.ptr(t["coef"]), L.ptr(xpad),
                                     L.ptr(dw), L.ptr(ws), nws - short, B, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, dw.cpu()


def _filter(dw):
    """the 64 x 7 x 7 x 3 filter entries of the packed [64][7][8][4] gradient; channel 3 of the packed image is zero, so its
    column receives nothing (kw == 7 lies outside the 7 x 7 window: it holds the products with the next pixel and is dropped
    by qt_unpack_stem_wgrad)"""
    assert float(dw[..., 3].abs().max()) == 0.0
    return dw[:, :, :7, :3]


@pytest.mark.parametrize("B", Sb.BATCHES)
def test_stem_fused_backward_dense_vs_float64(B):
    dev, L, lib = _env()
    c = Sb.case("random", B)
    image, dw, bound = Sb.dense_wgrad(B)
    want, bound = _filter(Sb.pack_wgrad(dw)), _filter(Sb.pack_wgrad(bound))
    t = _dev_inputs(c, BF16, dev)
    xpad = Sb.pack_image(image, BF16).to(dev)
    rc, got = _fused(L, lib, t, xpad, B, dev)
    assert rc == 0, lib.qt_last_error()
    _report(f"stem_bn_bwd_wgrad_ws random B={B}", Bd.ratio(_filter(got), want, bound))
    if B == max(Sb.BATCHES):   # the two-kernel form, held to the same float64 bound
        dy = _apply(L, lib, t, BF16, B, dev)
        d = L.ConvDesc()
        d.dtype, d.mode, d.batch = L.qt_dtype(BF16), L.QT_CONV_FWD, B
        d.in_h, d.in_w, d.out_h, d.out_w = 230, 232, 112, 112
        d.k_per_tap, d.n_out, d.kh, d.kw, d.stride, d.pad = 32, 64, 7, 1, 2, 0
        d.src_pix_stride, d.src_row_stride, d.src_img_stride = 4, 232 * 4, 230 * 232 * 4
        dw2 = torch.zeros(C, 7, 8, 4, dtype=F32, device=dev)
        L.check(lib.qt_conv2d_wgrad(ctypes.byref(d), L.ptr(dy), L.ptr(xpad), L.ptr(dw2), L.stream_ptr()), "qt_conv2d_wgrad")
        torch.cuda.synchronize()
        _report(f"stem_bn_bwd_apply + conv2d_wgrad random B={B}", Bd.ratio(_filter(dw2.cpu()), want, bound))


@pytest.mark.parametrize("B", Sb.BATCHES)
def test_stem_fused_backward_sparse_probe_bit_exact(B):
    """one pooled cell per tile, dy = g: a tile that is skipped, counted twice, read from the other LDS buffer or fed a stale
    pooled row changes an exactly known filter"""
    dev, L, lib = _env()
    c = Sb.case("grid", B)
    d, coef, image, dw, _ = Sb.sparse_probe(B)
    want = _filter(Sb.pack_wgrad(dw))
    t = _dev_inputs(c, BF16, dev, coef=coef, d=d)
    xpad = Sb.pack_image(image, BF16).to(dev)
    assert torch.equal(xpad[:, 3:227, 3:227, :3].cpu().double().permute(0, 3, 1, 2), image)
    rc, got = _fused(L, lib, t, xpad, B, dev)
    assert rc == 0, lib.qt_last_error()
    diff = _filter(got).double() != want
    assert not bool(diff.any()), (int(diff.sum()), float((_filter(got).double() - want).abs().max()))
    rc2, again = _fused(L, lib, t, xpad, B, dev)
    assert rc2 == 0 and torch.equal(got, again)                         # fixed summation order: the same bits on every run
    assert _fused(L, lib, t, xpad, B, dev, short=4)[0] != 0             # a workspace 4 bytes too small is refused
    assert _fused(L, lib, t, xpad, B, dev, dt=F32)[0] != 0              # f32 keeps the two-kernel form
