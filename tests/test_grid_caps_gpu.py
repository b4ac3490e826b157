"""Every capped grid-stride launch at the smallest shape at which some of its threads (or workgroups) take one trip more than
the others: the table of tests/_grid_caps.py, one test per row that no other test reaches (tests/test_grid_caps_cpu.py shows that
the shapes do what the rows claim).  What a kernel keeps across the back edge of its loop is wrong only here: the channel group a
thread folds once, the hash keyed on the flat index, the (image, row, column) recomputed from the index, the partial a workgroup
adds once.

Nothing in a comparison comes from the code under test, and no tolerance is introduced: every test uses the float64 reference and
the DERIVED bound of the kernel's own test (_bounds.py, _stem_bounds.py, _head_bounds.py, _pool3d_bounds.py, _metrics_ref.py,
_scores_ref.py), on the integer-grid input classes of those modules wherever they make the result exact, and then compares bit
for bit.  The WHOLE output is compared; outputs start as NaN (0xFF for bytes), so an element no trip wrote fails.

Periodic cases (the stem tail, the quadrant pool, the clip kernels: up to 134 M output elements): the input is a slab of P images
repeated along the image axis and the expected output is the slab's float64 reference repeated.  An image shares no pooling
window with its neighbours, so the repetition is exact.  A trip that started from a wrong offset would go unseen only if the
offset it should have used -- the stride, or a multiple of it below the total -- were a multiple of the period; the periods are
4099 or 211 images (primes) and 3 images of 49 * 2^k items against strides that are powers of two
(test_grid_caps_cpu.test_a_period_cannot_hide_a_wrong_trip_offset).

Every test prints the trip pattern it reached and max(|err| / bound) or `bit-exact`.  No case holds more than 4 GiB of device
memory; the references of the large float cases are evaluated in chunks of rows for that reason."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _bounds as Bd
import _grid_caps as G
import _metrics_ref as MR
import _pool3d_bounds as Pb
import _scores_ref as SR
import _stem_bounds as Sb
from _util import pkg

pytestmark = pytest.mark.gpu

NAN = float("nan")
F32, BF16 = torch.float32, torch.bfloat16
DTS = pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])


@pytest.fixture(scope="module", autouse=True)
def _drop_references():
    yield
    _pool_slab.cache_clear()
    Sb.clear_caches()
    torch.cuda.empty_cache()


def _env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    L = pkg("_lib")
    return torch.device("cuda:0"), L, L.lib()


def _nan(shape, dt, dev):
    return torch.full(shape, 0xFF if dt == torch.uint8 else NAN, dtype=dt, device=dev)


def _all_nan(t):
    return bool(torch.isnan(t.float()).all())


def _say(test, i=0, r=None):
    case, line = G.describe(test, i)
    print(f"  {line}: " + ("bit-exact" if r is None else f"max |err| / bound {r:.3f}"))
    assert r is None or r <= 1.0, (test, r)
    return case


def _shape(test, i=0):
    return G.find(test)["cases"][i]["shape"]


def _tile(slab, n, dim=0):
    """`slab` repeated along `dim` to n units (unit u holds slab unit u % P)"""
    idx = torch.arange(n, device=slab.device) % slab.shape[dim]
    return slab.index_select(dim, idx).contiguous()


def _same_as_slab(got, want, dim=0):
    """got == the slab `want` repeated along dim, compared slab by slab (values: -0.0 == +0.0, a NaN equals nothing)"""
    P, n = want.shape[dim], got.shape[dim]
    for u0 in range(0, n, P):
        m = min(P, n - u0)
        if not torch.equal(got.narrow(dim, u0, m), want.narrow(dim, 0, m)):
            return False
    return True


# ----------------------------------------------------------------------------------------------------------------------
# qt_bn_bwd_apply: the general kernel and the light one (two items in flight + a tail)
# ----------------------------------------------------------------------------------------------------------------------
def _apply_ratio(L, lib, dev, dt, M, C, with_mask, with_gout, seed):
    g, mask, y, mean, invstd, gamma = Bd.bwd_inputs(M, C, dt, with_mask, seed, dev)
    coef = Bd.bwd_coef(g, mask, y, mean, invstd, gamma)
    dy = _nan((M + 1, C), dt, dev)
    gout = _nan((M + 1, C), dt, dev) if with_gout else None
    L.check(lib.qt_bn_bwd_apply(L.qt_dtype(dt), L.ptr(g), L.ptr(mask), L.ptr(y), L.ptr(mean), L.ptr(invstd), L.ptr(coef), L.ptr(dy),
                                L.ptr(gout), M, C, L.stream_ptr()), "qt_bn_bwd_apply")
    torch.cuda.synchronize()
    light = Bd.light_route(M, C, dt, mask, gout)
    assert _all_nan(dy[M]) and (gout is None or _all_nan(gout[M]))
    worst = 0.0
    for r0 in range(0, M, 1 << 17):      # the float64 reference, 131072 rows at a time
        s = slice(r0, min(M, r0 + (1 << 17)))
        ref, bound, gm = Bd.bwd_apply_ref(g[s], None if mask is None else mask[s], y[s], mean, invstd, coef, dt, light)
        worst = max(worst, Bd.ratio(dy[s], ref, bound))
        if with_gout:
            assert torch.equal(gout[s].double(), gm), "g_out"
    return worst, light


@pytest.mark.parametrize("dt,with_mask,with_gout", [(F32, False, False), (F32, True, True), (BF16, True, False), (BF16, False, True)],
                         ids=["f32", "f32-mask-gout", "bf16-mask", "bf16-gout"])
def test_bn_bwd_apply_general(dt, with_mask, with_gout):
    dev, L, lib = _env()
    s = _shape("test_bn_bwd_apply_general")
    r, light = _apply_ratio(L, lib, dev, dt, s["M"], s["C"], with_mask, with_gout, 301)
    assert not light
    _say("test_bn_bwd_apply_general", 0, r)


@pytest.mark.parametrize("i", [0, 1, 2], ids=["pair-body-for-some", "tail-for-some", "back-edge-for-some"])
def test_bn_bwd_apply_light(i):
    """a thread folds P, Q, R of ITS four channels once: every later trip must land on the same channel group"""
    dev, L, lib = _env()
    s = _shape("test_bn_bwd_apply_light", i)
    r, light = _apply_ratio(L, lib, dev, BF16, s["M"], s["C"], False, False, 310 + i)
    assert light
    _say("test_bn_bwd_apply_light", i, r)


# ----------------------------------------------------------------------------------------------------------------------
# the stem tail: (image, row, column) recomputed from the flat index on every trip.  Periodic: _stem_bounds.case(.., 3) repeated
# ----------------------------------------------------------------------------------------------------------------------
def _stem(kind, dt, dev, B):
    c = Sb.case(kind, G.STEM_SLAB)
    f = lambda t: t.float().to(dev).contiguous()
    slab = dict(y=c["y"].to(dt).to(dev), d=c["d"].to(dt).to(dev), code=c["code"].to(dev), scale=f(c["scale"]), shift=f(c["shift"]),
                mean=f(c["mean"]), invstd=f(c["invstd"]), coef=f(c["coef"]))
    t = dict(slab)
    for k in ("y", "d", "code"):
        t[k] = _tile(slab[k], B)
    return c, t


@DTS
def test_stem_pool_forward(dt):
    dev, L, lib = _env()
    B = _shape("test_stem_pool_forward")["B"]
    c, t = _stem("grid", dt, dev, B)
    P, C = Sb.P, Sb.C
    pooled, ymax = _nan((B, P, P, C), dt, dev), _nan((B, P, P, C), dt, dev)
    code = _nan((B, P, P, C), torch.uint8, dev)
    L.check(lib.qt_stem_pool(L.qt_dtype(dt), L.ptr(t["y"]), L.ptr(t["scale"]), L.ptr(t["shift"]), L.ptr(pooled), L.ptr(code),
                             L.ptr(ymax), B, L.stream_ptr()), "qt_stem_pool")
    torch.cuda.synchronize()
    assert torch.equal(c["pooled"].to(dt).double(), c["pooled"])           # the grid class: exact in f32 and in bf16
    assert _same_as_slab(pooled, c["pooled"].to(dt).to(dev)), "pooled"
    assert _same_as_slab(code, c["code"].to(dev)), "argmax"
    assert _same_as_slab(ymax, c["ymax"].to(dt).to(dev)), "y_at_max"
    _say("test_stem_pool_forward")


@DTS
def test_stem_pool_bwd(dt):
    dev, L, lib = _env()
    B = _shape("test_stem_pool_bwd")["B"]
    c, t = _stem("grid", dt, dev, B)
    g = _nan((B, Sb.H, Sb.W, Sb.C), dt, dev)
    L.check(lib.qt_stem_pool_bwd(L.qt_dtype(dt), L.ptr(t["d"]), L.ptr(t["code"]), L.ptr(t["y"]), L.ptr(t["scale"]), L.ptr(t["shift"]),
                                 L.ptr(g), B, L.stream_ptr()), "qt_stem_pool_bwd")
    torch.cuda.synchronize()
    assert torch.equal(c["g"].to(dt).double(), c["g"])
    assert _same_as_slab(g, c["g"].to(dt).to(dev)), "g"
    _say("test_stem_pool_bwd")


@DTS
@pytest.mark.parametrize("kind", ["grid", "random"])
def test_stem_bn_bwd_apply(kind, dt):
    dev, L, lib = _env()
    B = _shape("test_stem_bn_bwd_apply")["B"]
    c, t = _stem(kind, dt, dev, B)
    dy = _nan((B, Sb.H, Sb.W, Sb.C), dt, dev)
    L.check(lib.qt_stem_bn_bwd_apply(L.qt_dtype(dt), L.ptr(t["d"]), L.ptr(t["code"]), L.ptr(t["y"]), L.ptr(t["scale"]), L.ptr(t["shift"]),
                                     L.ptr(t["mean"]), L.ptr(t["invstd"]), L.ptr(t["coef"]), L.ptr(dy), B, L.stream_ptr()),
            "qt_stem_bn_bwd_apply")
    torch.cuda.synchronize()
    ref = c["dy"].to(dev)
    bound = Sb.dy_bound(c["dy"], c["g"], c["y"], c["mean"], c["invstd"], c["coef"], dt).to(dev)
    P = G.STEM_SLAB
    r = max(Bd.ratio(dy[b0:b0 + P], ref[:min(P, B - b0)], bound[:min(P, B - b0)]) for b0 in range(0, B, P))
    _say("test_stem_bn_bwd_apply", 0, r)


def test_stem_bn_bwd_sums_light(i=0):
    """3.06 strides: the pair loop's back edge for some threads.  The grid class: every workgroup's partial row is exact in f32, so the float64 sum of the rows equals the reference's"""
    dev, L, lib = _env()
    B = _shape("test_stem_bn_bwd_sums_light", i)["B"]
    c = Sb.case("grid", G.STEM_SLAB)
    f = lambda t: t.float().to(dev).contiguous()
    d, ymax = _tile(c["d"].to(BF16).to(dev), B), _tile(c["ymax"].to(BF16).to(dev), B)
    rows = lib.qt_stem_bn_bwd_sums_rows(B)
    assert rows == Sb.sums_rows(B) == 1024
    part = _nan((rows + 2, 2, Sb.C), F32, dev)
    scale, shift, mean, invstd = (f(c[k]) for k in ("scale", "shift", "mean", "invstd"))
    L.check(lib.qt_stem_bn_bwd_sums(L.qt_dtype(BF16), L.ptr(d), L.ptr(ymax), L.ptr(scale), L.ptr(shift), L.ptr(mean), L.ptr(invstd),
                                    L.ptr(part), B, L.stream_ptr()), "qt_stem_bn_bwd_sums")
    torch.cuda.synchronize()
    p = part.cpu()
    assert bool(torch.isfinite(p[:rows]).all()) and bool(torch.isnan(p[rows:]).all())
    times = torch.tensor([len(range(j, B, G.STEM_SLAB)) for j in range(G.STEM_SLAB)], dtype=torch.float64).view(-1, 1)
    xhat = (c["y"] - c["mean"]) * c["invstd"]
    s1 = (c["g"].sum((1, 2)) * times).sum(0)                      # per image of the slab, times the images that repeat it
    s2 = ((c["g"] * xhat).sum((1, 2)) * times).sum(0)
    assert torch.equal(p[:rows, 0].double().sum(0), s1), "sum g"
    assert torch.equal(p[:rows, 1].double().sum(0), s2), "sum g xhat"
    _say("test_stem_bn_bwd_sums_light", i)


# ----------------------------------------------------------------------------------------------------------------------
# average pools
# ----------------------------------------------------------------------------------------------------------------------
@DTS
def test_avgpool(dt):
    dev, L, lib = _env()
    s = _shape("test_avgpool")
    batch, hw, C = s["batch"], s["hw"], s["C"]
    x, _ = Bd.pool_inputs(batch, hw, C, dt, 41, dev)
    dst = _nan((batch + 1, C), dt, dev)
    L.check(lib.qt_avgpool(L.qt_dtype(dt), L.ptr(x), L.ptr(dst), batch, hw, C, C, 0, L.stream_ptr()), "qt_avgpool")
    torch.cuda.synchronize()
    assert _all_nan(dst[batch])
    _say("test_avgpool", 0, Bd.ratio(dst[:batch], *Bd.avgpool_ref(x, dt)))


@DTS
def test_avgpool_bwd(dt):
    dev, L, lib = _env()
    s = _shape("test_avgpool_bwd")
    batch, hw, C = s["batch"], s["hw"], s["C"]
    x, d = Bd.pool_inputs(batch, hw, C, dt, 42, dev)
    gx = _nan((batch * hw + 1, C), dt, dev)
    L.check(lib.qt_avgpool_bwd(L.qt_dtype(dt), L.ptr(d), L.ptr(x), L.ptr(gx), batch, hw, C, C, 0, L.stream_ptr()), "qt_avgpool_bwd")
    torch.cuda.synchronize()
    assert _all_nan(gx[batch * hw])
    got = gx[:batch * hw].view(batch, hw, C)
    assert bool((got[x.float() <= 0] == 0).all())
    _say("test_avgpool_bwd", 0, Bd.ratio(got, *Bd.avgpool_bwd_ref(d, x, dt)))


@DTS
def test_avgpool_tb_bwd(dt):
    """T * HW = 128 and gradients on the bf16 grid: d / 128 is exact in f32 and in bf16, every element is compared bit for bit"""
    dev, L, lib = _env()
    s = _shape("test_avgpool_tb_bwd")
    T, B, HW, C = s["T"], s["B"], s["HW"], s["C"]
    ld, col0 = C + 36, 20
    d = torch.randn(B, ld, generator=torch.Generator().manual_seed(43)).to(BF16).float().to(dev)
    g = _nan((T * B * HW + 1, C), dt, dev)
    L.check(lib.qt_avgpool_tb_bwd(L.qt_dtype(dt), L.ptr(d), L.ptr(g), T, B, HW, C, ld, col0, L.stream_ptr()), "qt_avgpool_tb_bwd")
    torch.cuda.synchronize()
    want = (d[:, col0:col0 + C].double() / (T * HW))
    assert torch.equal(want.to(dt).double(), want)
    want = want.to(dt).view(1, B, 1, C)
    got = g[:T * B * HW].view(T, B, HW, C)
    assert _all_nan(g[T * B * HW]) and all(torch.equal(got[t, :, p], want[0, :, 0]) for t in range(T) for p in range(HW))
    _say("test_avgpool_tb_bwd")


# ----------------------------------------------------------------------------------------------------------------------
# the quadrant pool (periodic: 211 images)
# ----------------------------------------------------------------------------------------------------------------------
def _quad(dt, dev, B):
    P = G.QUAD_SLAB
    q, d = Bd.quad_inputs(P, dt)
    d = d[:, :4608].contiguous()
    assert Bd.quad_tie_share(q) >= 0.05
    pooled, dq = Bd.quad_pool_ref(q, d, P, 4608, 0)
    qt = _tile(q.view(P, 4, 7, 7, 128).to(dev), B).view(B * 4, 7, 7, 128)
    return qt, _tile(d.to(dev), B), pooled.to(dt).to(dev), dq.view(P, 4, 7, 7, 128).to(dt).to(dev)


@DTS
def test_quad_pool(dt):
    dev, L, lib = _env()
    B = _shape("test_quad_pool")["batch"]
    q, _, pooled, _ = _quad(dt, dev, B)
    dst = _nan((B + 1, 4608), dt, dev)
    L.check(lib.qt_quad_pool(L.qt_dtype(dt), L.ptr(q), L.ptr(dst), B, 4608, 0, L.stream_ptr()), "qt_quad_pool")
    torch.cuda.synchronize()
    assert _all_nan(dst[B]) and _same_as_slab(dst[:B], pooled)
    _say("test_quad_pool")


@DTS
def test_quad_pool_bwd(dt):
    dev, L, lib = _env()
    B = _shape("test_quad_pool_bwd")["batch"]
    q, d, _, dq_ref = _quad(dt, dev, B)
    dq = _nan((B * 4 * 49 + 1, 128), dt, dev)
    L.check(lib.qt_quad_pool_bwd(L.qt_dtype(dt), L.ptr(d), L.ptr(q), L.ptr(dq), B, 4608, 0, L.stream_ptr()), "qt_quad_pool_bwd")
    torch.cuda.synchronize()
    assert _all_nan(dq[B * 4 * 49]) and _same_as_slab(dq[:B * 4 * 49].view(B, 4, 7, 7, 128), dq_ref)
    _say("test_quad_pool_bwd")


# ----------------------------------------------------------------------------------------------------------------------
# dropout: the hash of (seed, flat element index), restated on the host
# ----------------------------------------------------------------------------------------------------------------------
def _hash_u32(seed, n):
    """hash_u32 of csrc/elementwise.hip (a splitmix64 round of seed + i * golden ratio, high word) for i = 0 .. n - 1"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return (z >> np.uint64(32)).astype(np.int64)


@DTS
@pytest.mark.parametrize("p", [0.5, 0.1])
def test_dropout(p, dt):
    """the mask is a function of the flat index r * cols + c alone: a trip that hashed another index keeps other elements"""
    dev, L, lib = _env()
    s = _shape("test_dropout")
    rows, cols, pad, seed = s["rows"], s["cols"], 24, 0x1234567887654321
    x0 = (torch.randn(rows, cols + pad, generator=torch.Generator().manual_seed(44)) + 3.0).to(dt)    # (no zeros among the inputs)
    x = x0.to(dev)
    L.check(lib.qt_dropout(L.qt_dtype(dt), L.ptr(x), rows, cols, cols + pad, seed, p, L.stream_ptr()),
            "qt_dropout")
    torch.cuda.synchronize()
    pf = np.float32(p)
    keep = torch.from_numpy(_hash_u32(seed, rows * cols) >= int(float(pf) * 4294967296.0)).view(rows, cols)
    inv = torch.ones((), dtype=F32) / (torch.ones((), dtype=F32) - torch.tensor(float(pf), dtype=F32))
    want = x0.clone()
    want[:, :cols] = torch.where(keep, x0[:, :cols].float() * inv, torch.zeros(())).to(dt)          # one f32 product, one store
    share = float(keep.double().mean())
    assert abs(share - (1 - float(pf))) <= 5 * (float(pf) * (1 - float(pf)) / keep.numel()) ** 0.5      # the binomial law, as in _bounds
    assert torch.equal(x.cpu(), want)
    _say("test_dropout")


# ----------------------------------------------------------------------------------------------------------------------
# one-liners
# ----------------------------------------------------------------------------------------------------------------------
def _act_and_grad(n, dt, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    act = torch.randn(n + 3, generator=gen, device=dev)
    act[::5] = 0.0
    act[1::7] = -0.0
    return act.to(dt), torch.randn(n + 3, generator=gen, device=dev).to(dt)


@DTS
def test_relu_mask_scale(dt):
    dev, L, lib = _env()
    n = _shape("test_relu_mask_scale")["n"]
    act, g = _act_and_grad(n, dt, dev, 45)
    g0 = g.clone()
    L.check(lib.qt_relu_mask_scale(L.qt_dtype(dt), L.ptr(g), L.ptr(act), n, 1.25, L.stream_ptr()), "qt_relu_mask_scale")
    torch.cuda.synchronize()
    want = torch.where(act[:n].float() > 0, g0[:n].float() * 1.25, torch.zeros((), device=dev)).to(dt)
    assert torch.equal(g[:n], want) and torch.equal(g[n:], g0[n:])
    _say("test_relu_mask_scale")


@DTS
def test_cast_f32(dt):
    dev, L, lib = _env()
    n = _shape("test_cast_f32")["n"]
    _, g = _act_and_grad(n, dt, dev, 46)
    out = _nan((n + 3,), F32, dev)
    L.check(lib.qt_cast_f32(L.qt_dtype(dt), L.ptr(g), L.ptr(out), n, L.stream_ptr()), "qt_cast_f32")
    torch.cuda.synchronize()
    assert torch.equal(out[:n], g[:n].float()) and _all_nan(out[n:])
    _say("test_cast_f32")


def test_scale_by_nonzero():
    dev, L, lib = _env()
    n = _shape("test_scale_by_nonzero")["n"]
    x, g = _act_and_grad(n, F32, dev, 47)
    g0 = g.clone()
    L.check(lib.qt_scale_by_nonzero(L.ptr(g), L.ptr(x), n, 2.0 / 3.0, L.stream_ptr()), "qt_scale_by_nonzero")
    torch.cuda.synchronize()
    mul = torch.tensor(2.0 / 3.0, dtype=F32, device=dev)
    want = torch.where(x[:n] != 0, g0[:n] * mul, torch.zeros((), device=dev))
    assert torch.equal(g[:n], want) and torch.equal(g[n:], g0[n:])
    _say("test_scale_by_nonzero")


@DTS
def test_relu_mask_cols(dt):
    dev, L, lib = _env()
    s = _shape("test_relu_mask_cols")
    rows, cols, ld, col0 = s["rows"], s["cols"], s["ld"], s["col0"]
    gen = torch.Generator(device=dev).manual_seed(48)
    act = torch.randn(rows, ld, generator=gen, device=dev)
    act[:, ::4] = 0.0
    act, d = act.to(dt), torch.randn(rows, ld, generator=gen, device=dev).to(dt)
    out = _nan((rows * cols + 3,), F32, dev)
    L.check(lib.qt_relu_mask_cols(L.qt_dtype(dt), L.ptr(d), L.ptr(act), L.ptr(out), rows, cols, ld, col0, 1.5, L.stream_ptr()),
            "qt_relu_mask_cols")
    torch.cuda.synchronize()
    sl = slice(col0, col0 + cols)
    want = torch.where(act[:, sl].float() > 0, d[:, sl].float() * 1.5, torch.zeros((), device=dev))
    assert torch.equal(out[:rows * cols].view(rows, cols), want) and _all_nan(out[rows * cols:])
    _say("test_relu_mask_cols")


# ----------------------------------------------------------------------------------------------------------------------
# packers and un-packers: plain indexing of the layouts in the kernels' comments
# ----------------------------------------------------------------------------------------------------------------------
@DTS
def test_pack_stem_input(dt):
    dev, L, lib = _env()
    B = _shape("test_pack_stem_input")["B"]
    image = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(49))
    xpad = _nan((B + 1, 230, 232, 4), dt, dev)
    L.check(lib.qt_pack_stem_input(L.qt_dtype(dt), L.ptr(image.to(dev)), L.ptr(xpad), B, L.stream_ptr()), "qt_pack_stem_input")
    torch.cuda.synchronize()
    assert _all_nan(xpad[B]) and torch.equal(xpad[:B].cpu(), Sb.pack_image(image, dt))
    _say("test_pack_stem_input")


def _weights(O, I, k, dev, seed):
    return torch.randn(O, I, k, k, generator=torch.Generator().manual_seed(seed)).to(dev)


@DTS
def test_pack_conv_weight(dt):
    dev, L, lib = _env()
    s = _shape("test_pack_conv_weight")
    O, I, k = s["O"], s["I"], s["k"]
    w = _weights(O, I, k, dev, 50)
    n = O * I * k * k
    fwd, dg, only = _nan((n + 8,), dt, dev), _nan((n + 8,), dt, dev), _nan((n + 8,), dt, dev)
    L.check(lib.qt_pack_conv_weight(L.qt_dtype(dt), L.ptr(w), L.ptr(fwd), L.ptr(dg), O, I, k, k, L.stream_ptr()), "qt_pack_conv_weight")
    L.check(lib.qt_pack_conv_weight(L.qt_dtype(dt), L.ptr(w), L.ptr(only), None, O, I, k, k, L.stream_ptr()), "qt_pack_conv_weight")
    torch.cuda.synchronize()
    assert torch.equal(fwd[:n].view(O, k, k, I), w.permute(0, 2, 3, 1).to(dt)) and torch.equal(only[:n], fwd[:n])      # [o][kh][kw][i]
    assert torch.equal(dg[:n].view(I, k, k, O), w.permute(1, 2, 3, 0).to(dt))                                   # [i][kh][kw][o]
    assert _all_nan(fwd[n:]) and _all_nan(dg[n:]) and _all_nan(only[n:])
    _say("test_pack_conv_weight")


def _s2_taps(parity):
    """filter taps of a stride-2 3 x 3 data gradient on even (the centre) and odd (2, then 0) output rows / columns"""
    return [2, 0] if parity else [1]


@DTS
def test_pack_dgrad_s2(dt):
    """dst[class][i][tap'][o], class = row parity * 2 + column parity; class 3 (I * 2 * 2 * O elements) is the loop that outgrows
    the stride"""
    dev, L, lib = _env()
    s = _shape("test_pack_dgrad_s2")
    O, I, k = s["O"], s["I"], s["k"]
    w = _weights(O, I, k, dev, 51)
    n = O * I * 9
    dst = _nan((n + 8,), dt, dev)
    offs, khs, kws = (ctypes.c_longlong * 4)(), (ctypes.c_int * 4)(), (ctypes.c_int * 4)()
    L.check(lib.qt_pack_dgrad_s2(L.qt_dtype(dt), L.ptr(w), L.ptr(dst), O, I, k, offs, khs, kws, L.stream_ptr()), "qt_pack_dgrad_s2")
    torch.cuda.synchronize()
    base = 0
    for cls in range(4):
        th, tw = _s2_taps(cls >> 1), _s2_taps(cls & 1)
        assert (offs[cls], khs[cls], kws[cls]) == (base, len(th), len(tw))
        want = torch.stack([w[:, :, a, b] for a in th for b in tw], 0).permute(2, 0, 1).to(dt)                  # [i][tap'][o]
        m = want.numel()
        assert torch.equal(dst[base:base + m].view(I, len(th) * len(tw), O), want), cls
        base += m
    assert base == n and _all_nan(dst[n:]) and I * 4 * O > 8192 * 256
    _say("test_pack_dgrad_s2")


@DTS
def test_pack_dgrad_s2_merged(dt):
    """dst[class * I + i][th * 2 + tw][o]; th / tw = 0: the tap on the row / column itself (1 on even, 2 on odd pixels), 1: the
    tap on the next one (0, odd pixels only); the slots no tap maps to are zero"""
    dev, L, lib = _env()
    s = _shape("test_pack_dgrad_s2_merged")
    O, I = s["O"], s["I"]
    w = _weights(O, I, 3, dev, 52)
    n = 16 * O * I
    dst = _nan((n + 8,), dt, dev)
    L.check(lib.qt_pack_dgrad_s2_merged(L.qt_dtype(dt), L.ptr(w), L.ptr(dst), O, I, L.stream_ptr()), "qt_pack_dgrad_s2_merged")
    torch.cuda.synchronize()
    want = torch.zeros(4, I, 2, 2, O, dtype=dt, device=dev)
    for cls in range(4):
        for a, kh in enumerate(_s2_taps(cls >> 1)):
            for b, kw in enumerate(_s2_taps(cls & 1)):
                want[cls, :, a, b, :] = w[:, :, kh, kw].t().to(dt)
    assert torch.equal(dst[:n].view(4, I, 2, 2, O), want) and _all_nan(dst[n:])
    _say("test_pack_dgrad_s2_merged")


def test_unpack_conv_wgrad():
    dev, L, lib = _env()
    s = _shape("test_unpack_conv_wgrad")
    O, I, k = s["O"], s["I"], s["k"]
    n = O * I * k * k
    dw = torch.randint(-2 ** 20, 2 ** 20, (O, k, k, I), generator=torch.Generator().manual_seed(53)).float().to(dev)
    grad, acc = _nan((n + 8,), F32, dev), _nan((n + 8,), F32, dev)
    acc[:n] = 1.0
    L.check(lib.qt_unpack_conv_wgrad(L.ptr(dw), L.ptr(grad), O, I, k, k, 0, L.stream_ptr()), "qt_unpack_conv_wgrad")
    L.check(lib.qt_unpack_conv_wgrad(L.ptr(dw), L.ptr(acc), O, I, k, k, 1, L.stream_ptr()), "qt_unpack_conv_wgrad")
    torch.cuda.synchronize()
    want = dw.permute(0, 3, 1, 2).contiguous()                                 # OIHW; integers below 2^21: + 1 is exact
    assert torch.equal(grad[:n].view(O, I, k, k), want) and torch.equal(acc[:n].view(O, I, k, k), want + 1.0)
    assert _all_nan(grad[n:]) and _all_nan(acc[n:])
    _say("test_unpack_conv_wgrad")


def test_lstm_stream_stage():
    dev, L, lib = _env()
    s = _shape("test_lstm_stream_stage")
    S, n, T, H = s["S"], s["n"], s["T"], s["H"]
    gen = torch.Generator(device=dev).manual_seed(54)
    carry = torch.randn(S, T - 1, 4 * H, generator=gen, device=dev)
    xnew = torch.randn(S, n, 4 * H, generator=gen, device=dev)
    out = _nan((S * (T - 1 + n) + 1, 4 * H), F32, dev)
    L.check(lib.qt_lstm_stream_stage(L.ptr(carry), L.ptr(xnew), L.ptr(out), S, n, T, H, L.stream_ptr()), "qt_lstm_stream_stage")
    torch.cuda.synchronize()
    assert torch.equal(out[:-1].view(S, T - 1 + n, 4 * H), torch.cat([carry, xnew], dim=1)) and _all_nan(out[-1])
    _say("test_lstm_stream_stage")


@DTS
def test_pack_clip27(dt):
    """periodic in the batch: clip b holds slab clip b % 4099; integers in [-8, 8] are exact in bf16"""
    dev, L, lib = _env()
    s = _shape("test_pack_clip27")
    B, T, H, W = s["B"], s["T"], s["H"], s["W"]
    slab = torch.randint(-8, 9, (G.PRIME, T, 3, H, W), generator=torch.Generator().manual_seed(55)).float()
    ref = Pb.clip27_ref(slab)                                                   # [T][P][H][W][128]
    clips = _tile(slab.to(dev), B)
    dst = _nan((T * B * H * W + 1, 128), dt, dev)
    L.check(lib.qt_pack_clip27(L.qt_dtype(dt), L.ptr(clips), L.ptr(dst), B, T, H, W, L.stream_ptr()), "qt_pack_clip27")
    torch.cuda.synchronize()
    assert _all_nan(dst[-1]) and _same_as_slab(dst[:-1].view(T, B, H, W, 128), ref.to(dt).to(dev), dim=1)
    _say("test_pack_clip27")


# ----------------------------------------------------------------------------------------------------------------------
# the clip models' pool kernels (periodic in the batch: 4099 images per frame; pool_t = 1; the grid class of _pool3d_bounds)
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pool_slab(dtn):
    d = G.POOL3D
    return Pb.build("grid", "c1", 1, dtn, dims=(d["T"], G.PRIME, d["H"], d["W"], d["C"]))


def _pool_case(test, dtn):
    s = _shape(test)
    c = _pool_slab(dtn)
    assert c["shape"] == (s["T"], G.PRIME, s["H"], s["W"], s["C"]) and c["pt"] == s["pt"] == 1
    return s, c, (s["T"], s["B"], s["H"], s["W"], s["C"]), (s["T"], s["B"], s["H"] // 2, s["W"] // 2, s["C"])


def _rep(c, key, dt, dev, B):
    t = c[key]
    return _tile((t if t.dtype == torch.uint8 else t.to(dt)).to(dev), B, dim=1)


def test_pool3d_max():
    dev, L, lib = _env()
    s, c, full, ps = _pool_case("test_pool3d_max", "bf16")
    T, B, H, W, C = full
    x = _rep(c, "x", BF16, dev, B)
    out, arg = _nan(ps, BF16, dev), _nan(ps, torch.uint8, dev)
    L.check(lib.qt_pool3d_max(L.qt_dtype(BF16), L.ptr(x), L.ptr(out), L.ptr(arg), T, B, H, W, C, 1, L.stream_ptr()), "qt_pool3d_max")
    torch.cuda.synchronize()
    assert _same_as_slab(out, c["xpooled"].to(BF16).to(dev), dim=1), "pooled"
    assert _same_as_slab(arg, c["xcode"].to(dev), dim=1), "argmax"
    _say("test_pool3d_max")


def test_pool3d_max_bwd():
    dev, L, lib = _env()
    s, c, full, ps = _pool_case("test_pool3d_max_bwd", "bf16")
    T, B, H, W, C = full
    d, code = _rep(c, "d", BF16, dev, B), _rep(c, "xcode", BF16, dev, B)
    dx = _nan(full, BF16, dev)
    L.check(lib.qt_pool3d_max_bwd(L.qt_dtype(BF16), L.ptr(d), L.ptr(code), L.ptr(dx), T, B, H, W, C, 1, L.stream_ptr()),
            "qt_pool3d_max_bwd")
    torch.cuda.synchronize()
    assert _same_as_slab(dx, c["dx"].to(BF16).to(dev), dim=1), "dx"
    _say("test_pool3d_max_bwd")


def test_pool3d_bn_relu_max():
    dev, L, lib = _env()
    s, c, full, ps = _pool_case("test_pool3d_bn_relu_max", "bf16")
    T, B, H, W, C = full
    y = _rep(c, "y", BF16, dev, B)
    out, arg, ymax = _nan(ps, BF16, dev), _nan(ps, torch.uint8, dev), _nan(ps, BF16, dev)
    scale, shift = c["scale"].float().to(dev), c["shift"].float().to(dev)
    L.check(lib.qt_pool3d_bn_relu_max(L.qt_dtype(BF16), L.ptr(y), L.ptr(scale), L.ptr(shift), L.ptr(out), L.ptr(arg), L.ptr(ymax),
                                      T, B, H, W, C, C, 1, L.stream_ptr()), "qt_pool3d_bn_relu_max")
    torch.cuda.synchronize()
    assert Pb.same(c["pooled"].to(BF16), c["pooled"])
    assert _same_as_slab(out, c["pooled"].to(BF16).to(dev), dim=1), "pooled"
    assert _same_as_slab(arg, c["code"].to(dev), dim=1), "argmax"
    assert _same_as_slab(ymax, c["ymax"].to(BF16).to(dev), dim=1), "y_at_max"
    _say("test_pool3d_bn_relu_max")


def test_pool3d_bn_bwd_apply():
    """f32: the general kernel (a bf16 launch of this size takes the resident-grid kernel, which tests/test_pool3d_gpu.py walks
    through its trips); the grid class: every operation of dy is exact in f32, compared bit for bit"""
    dev, L, lib = _env()
    s, c, full, ps = _pool_case("test_pool3d_bn_bwd_apply", "f32")
    T, B, H, W, C = full
    assert not Pb.light_taken(F32, C, C, C, Pb.apply_groups(*full)) and c["kind"] == "grid"
    d, code, pooled, y = (_rep(c, k, F32, dev, B) for k in ("d", "code", "pooled", "y"))
    mean, invstd, coef = (c[k].float().to(dev).contiguous() for k in ("mean", "invstd", "coef"))
    dy = _nan(full, F32, dev)
    L.check(lib.qt_pool3d_bn_bwd_apply(L.qt_dtype(F32), L.ptr(d), L.ptr(code), L.ptr(pooled), L.ptr(y), L.ptr(mean), L.ptr(invstd),
                                       L.ptr(coef), L.ptr(dy), T, B, H, W, C, C, C, 1, L.stream_ptr()), "qt_pool3d_bn_bwd_apply")
    torch.cuda.synchronize()
    assert torch.equal(c["dy"].float().double(), c["dy"])
    assert _same_as_slab(dy, c["dy"].float().to(dev), dim=1), "dy"
    _say("test_pool3d_bn_bwd_apply")


# ----------------------------------------------------------------------------------------------------------------------
# the meters: a workgroup adds its counters ONCE, behind its loop over tiles
# ----------------------------------------------------------------------------------------------------------------------
def _edge_rows(rows, rpb, cap=2048):
    """rows on both sides of the first trip's last tile (cap * rpb), and the first and last rows"""
    edge = cap * rpb
    assert 0 < edge - 8 and edge + 2 < rows
    return [0, 1, edge - 8, edge - 1, edge, edge + 1, rows - 2, rows - 1]


def _metrics_call(dev, C, z=None, pred_in=None, y=None, state=None, outputs=False):
    M, lib = pkg("metrics"), pkg("_lib")
    L = lib.lib()
    rows = len(y)
    yt = torch.from_numpy(y).to(dev)
    zt = pt = probs = conf = pred = None
    ldp = C + 5
    if z is not None:
        zt = torch.full((rows, C + 3), NAN, device=dev)
        zt[:, :C] = torch.from_numpy(z).to(dev)
        if outputs:
            probs, conf = _nan((rows + 1, ldp), F32, dev), _nan((rows + 1,), F32, dev)
            pred = torch.full((rows + 1,), -7, dtype=torch.int64, device=dev)
    else:
        pt = torch.from_numpy(pred_in).to(dev)
    if state is None:
        state = torch.zeros(C * C + 4, dtype=torch.int64, device=dev)
    desc = M.MetricsDesc(0, MR.IGNORE)
    lib.check(L.qt_metrics_update(ctypes.byref(desc), lib.ptr(zt), C + 3 if zt is not None else 0, lib.ptr(pt), lib.ptr(yt), rows, C,
                                  lib.ptr(state), lib.ptr(probs), ldp, lib.ptr(conf), lib.ptr(pred), lib.stream_ptr()),
              "qt_metrics_update")
    torch.cuda.synchronize()
    return state, probs, conf, pred


@pytest.mark.parametrize("i", [0, 1, 2], ids=["wave-rows", "16-lane-rows", "thread-rows"])
def test_metrics_logits(i):
    dev, _, _ = _env()
    s = _shape("test_metrics_logits", i)
    rows, C, rpb = s["rows"], s["C"], 256 // s["lanes"]
    z = MR.make_logits(rows, C, seed=60 + i)
    y = MR.make_labels(rows, C, seed=70 + i)
    edge = _edge_rows(rows, rpb)
    for j, r in enumerate(edge):                       # NaN rows, ignored rows and labels outside [0, C) on both sides of the boundary
        if j % 2 == 0:
            z[r, (3 * j) % C] = np.nan
        else:
            y[r] = MR.IGNORE
    y[edge[2] + 1], y[edge[5] + 1] = C, -1
    state, probs, conf, pred = _metrics_call(dev, C, z=z, y=y, outputs=True)
    want_pred = MR.argmax_ref(z)
    want = MR.count(y, want_pred, C)
    assert want[C * C + 1] == 4 and want[C * C + 2] == 2
    assert np.array_equal(state.cpu().numpy(), want), "state"
    assert int(pred[rows]) == -7 and np.array_equal(pred[:rows].cpu().numpy(), want_pred)
    # the same rows in two calls below the cap: the same integer state (one more update call)
    half = rows // 2
    assert -(-half // rpb) <= 2048 and -(-(rows - half) // rpb) <= 2048
    st2, _, _, _ = _metrics_call(dev, C, z=z[:half], y=y[:half])
    st2, _, _, _ = _metrics_call(dev, C, z=z[half:], y=y[half:], state=st2)
    two = st2.cpu().numpy()
    assert two[C * C + 3] == 2 and np.array_equal(two[:C * C + 3], want[:C * C + 3]), "two calls"
    # the float outputs inside the bound of their own test; NaN rows as torch has them; nothing behind the last row
    got_p, got_c = probs[:rows, :C].cpu().numpy(), conf[:rows].cpu().numpy()
    nanp = MR.nan_pattern(z)
    assert np.array_equal(np.isnan(got_p), nanp) and np.array_equal(np.isnan(got_c), nanp.all(1))
    fin = ~nanp.all(1)
    p, bound = MR.softmax_ref(z[fin])
    r = MR.ratio(got_p[fin], p, bound)
    assert np.array_equal(got_c[fin].view(np.uint32), got_p[fin][np.arange(int(fin.sum())), want_pred[fin]].view(np.uint32))
    assert _all_nan(probs[rows]) and _all_nan(conf[rows:]) and bool(torch.isnan(probs[:rows, C:]).all())
    _say("test_metrics_logits", i, r)


@pytest.mark.parametrize("i", [0, 1], ids=["lds-histogram", "global-atomics"])
def test_metrics_pred_in(i):
    dev, _, _ = _env()
    s = _shape("test_metrics_pred_in", i)
    rows, C = s["rows"], s["C"]
    y = MR.make_labels(rows, C, seed=80 + i)
    p = MR.make_labels(rows, C, seed=90 + i)
    edge = _edge_rows(rows, 256)
    for j, r in enumerate(edge):
        if j % 2 == 0:
            y[r] = MR.IGNORE
        else:
            p[r] = C + j                                # an invalid prediction
    state, _, _, _ = _metrics_call(dev, C, pred_in=p, y=y)
    want = MR.count(y, p, C)
    assert want[C * C + 1] == 4 and want[C * C + 2] == 4
    assert np.array_equal(state.cpu().numpy(), want), "state"
    half = rows // 2
    st2, _, _, _ = _metrics_call(dev, C, pred_in=p[:half], y=y[:half])
    st2, _, _, _ = _metrics_call(dev, C, pred_in=p[half:], y=y[half:], state=st2)
    two = st2.cpu().numpy()
    assert two[C * C + 3] == 2 and np.array_equal(two[:C * C + 3], want[:C * C + 3]), "two calls"
    _say("test_metrics_pred_in", i)


def _scores_call(dev, s, y, C, bits, M, state=None):
    S, lib = pkg("scores"), pkg("_lib")
    L = lib.lib()
    rows = len(y)
    st = torch.full((rows, C + 3), NAN, device=dev)
    st[:, :C] = torch.from_numpy(s).to(dev)
    yt = torch.from_numpy(y).to(dev)
    if state is None:
        state = torch.zeros(SR.cells(C, bits, M), dtype=torch.int64, device=dev)
    desc = S.ScoresDesc(0, SR.PROBS, bits, M, 1, SR.IGNORE)                    # route 1: the direct kernel, as the descriptor asks
    lib.check(L.qt_scores_update(ctypes.byref(desc), lib.ptr(st), C + 3, lib.ptr(yt), rows, C, lib.ptr(state), lib.stream_ptr()),
              "qt_scores_update")
    torch.cuda.synchronize()
    return state


@pytest.mark.parametrize("i", [0, 1], ids=["16-lane-rows", "thread-rows"])
def test_scores_direct(i):
    """probabilities as given (the rows themselves are p: no expf enters), every histogram, rank, calibration cell and counter
    equal to the numpy restatement"""
    dev, _, _ = _env()
    sh = _shape("test_scores_direct", i)
    rows, C, rpb, bits, M = sh["rows"], sh["C"], 256 // sh["lanes"], 8, 15
    z, y = SR.make_logits(rows, C, seed=100 + i)
    s, y = SR.mix_in(SR.softmax_f32(z), y, C, SR.PROBS)
    edge = _edge_rows(rows, rpb)
    for j, r in enumerate(edge[2:], 2):                # (rows 0 .. 10 hold mix_in's cases already)
        if j % 2 == 0:
            s[r, (3 * j) % C] = np.nan
        else:
            y[r] = SR.IGNORE
    want = SR.update(None, s, s, y, C, bits, M, SR.PROBS)
    assert min(want[-5:-1]) >= 2                     # counted, ignored, invalid and NaN rows all occur
    got = _scores_call(dev, s, y, C, bits, M).cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    half = rows // 2
    assert -(-half // rpb) <= 2048 and -(-(rows - half) // rpb) <= 2048
    st2 = _scores_call(dev, s[:half], y[:half], C, bits, M)
    two = _scores_call(dev, s[half:], y[half:], C, bits, M, state=st2).cpu().numpy()
    assert two[-1] == 2 and np.array_equal(two[:-1], want[:-1]), "two calls"
    _say("test_scores_direct", i)
