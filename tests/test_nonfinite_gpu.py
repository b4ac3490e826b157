"""NaN, +inf and -inf through the forward kernels and the models (tests/_nonfinite.py; its CPU twin is
tests/test_nonfinite_cpu.py).  Op level: activations of the integer-grid rows with planted non-finite values; the positions
of NaN / +inf / -inf in every output must equal those of torch's float64 result on the same operands, every finite element
equals it under the E.same rule (bit-exact; mode B rounds to bf16), statistics rows are added in float64 and compared per
channel.  Output buffers start at a finite sentinel no result can hold (a NaN prefill could not be told from a NaN result).
Max pools follow ATen for NaN: value and argmax are read off F.max_pool*d(..., return_indices=True) on the CPU.
Model level: a NaN or +inf pixel, a NaN conv weight, and one train step with a NaN pixel, against oracle/quadtree_oracle.py
on the CPU: the NaN / inf pattern of the logits (loss, running buffers, gradients) equals the oracle's, untouched rows stay
inside the models' own LOGIT_TOL."""
import ctypes
import sys

import pytest
import torch
import torch.nn.functional as F

import _exact as E
import _nonfinite as N
from _exact import BF, F32
from _util import ROOT, pkg, rel_err
from test_conv_exact_gpu import _check_path, _desc, _nchw, _ncthw, _tb, _walks
from test_conv_gpu import nhwc
from test_gemm_small_gpu import GemmSmallDesc

pytestmark = pytest.mark.gpu

SENTINEL = -1.5e38          # representable in bf16; no raw sum and no ReLU output comes near it
LOGIT_TOL = {F32: 1e-3, BF: 4e-2}


def _env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L = pkg("_lib")
    return torch.device("cuda:0"), L, L.lib()


def _out(shape, dt, dev):
    return torch.full(tuple(shape), SENTINEL, dtype=dt, device=dev)


def _agree(got, exp, dt, what):
    """positions of NaN, +inf and -inf equal; finite elements equal exp.to(dt) bit for bit"""
    got = got.cpu()
    assert got.shape == exp.shape and got.dtype == dt, (what, got.shape, exp.shape, got.dtype)
    g = got.double()
    for name, gm, em in (("NaN", torch.isnan(g), torch.isnan(exp)), ("+inf", g == N.INF, exp == N.INF),
                         ("-inf", g == -N.INF, exp == -N.INF)):
        if not torch.equal(gm, em):
            bad = (gm != em).nonzero()
            i = tuple(int(v) for v in bad[0])
            assert False, (what, name, "positions differ: got", int(gm.sum()), "expected", int(em.sum()), "first at", i,
                           "got", float(g[i]), "expected", float(exp[i]), "differing", len(bad))
    fin = torch.isfinite(exp)
    zero = torch.zeros((), dtype=torch.float64)
    if not E.same(torch.where(fin, got, torch.zeros((), dtype=dt)), torch.where(fin, exp, zero), dt):
        bad = E.first_mismatch(torch.where(fin, got, torch.zeros((), dtype=dt)), torch.where(fin, exp, zero), dt)
        assert False, (what, "finite elements: first mismatch (index, got, want, count)", bad)


def _stats_agree(partial, raw, what):
    """the partial rows [rows][2][C] added in float64: per channel the class of torch's float64 sums, finite channels exactly"""
    got = partial.double().sum(0).cpu()
    ref = N.stats_ref(raw)
    assert torch.equal(N.classes(got), N.classes(ref)), (what, N.classes(got).tolist(), N.classes(ref).tolist())
    fin = torch.isfinite(ref)
    assert torch.equal(got[fin], ref[fin]), what


# ----------------------------------------------------------------------------------------------------------------------
# 2-D convolutions: generic tile, ring, patch-resident, 27 taps
# ----------------------------------------------------------------------------------------------------------------------
CONV = [(n, dt) for n in ("generic_3x3", "generic_1x1_s2", "generic_3x3_rounded", "ring_b1", "pt_7_ragged", "pt_14_rounded",
                          "taps27") for dt in N.row_of(n)["dts"]]


def _conv(L, lib, dev, d, x, w, shape, dt, scale=None, shift=None, residual=None, stats_rows=0):
    y = _out(shape, dt, dev)
    st = _out((stats_rows, 2, shape[1]), torch.float32, dev) if stats_rows else None
    io = L.ConvIO(L.ptr(x), L.ptr(w), L.ptr(y), L.ptr(scale), L.ptr(shift), L.ptr(residual), None, L.ptr(st))
    L.check(lib.qt_conv2d_igemm(ctypes.byref(d), ctypes.byref(io), L.stream_ptr()), "qt_conv2d_igemm")
    torch.cuda.synchronize()
    return y, st


@pytest.mark.parametrize("name,dt", CONV, ids=[f"{n}-{'bf16' if dt == BF else 'f32'}" for n, dt in CONV])
def test_conv_forward_nonfinite(name, dt):
    dev, L, lib = _env()
    c = N.fwd_case(name)
    row = c["row"]
    N.conditions(c["raw_c"], c["pre_c"], c["act"], c["images"])
    B, Cin, Cout, H, k, s, p = row["cfg"]
    sc, sh = c["scale"].float().to(dev), c["shift"].float().to(dev)
    if row.get("frames"):
        T = row["frames"]
        xd = c["x"].permute(2, 0, 3, 4, 1).contiguous().to(dev, dt)
        wd = c["w"].permute(0, 2, 3, 4, 1).contiguous().to(dev, dt)
        resd = c["res"].permute(2, 0, 3, 4, 1).contiguous().to(dev, dt).view(-1, Cout)
        d = _desc(L, dt, L.QT_CONV_FWD, T * B, (H, H), (H, H), Cin, Cout, 3, 1, 1)
        d.kt, d.frames = 3, T
        M = T * B * H * H
        back = lambda t: t.cpu().view(T, B, H, H, Cout).permute(1, 4, 0, 2, 3)
        ctxs = [None]
    else:
        Ho = (H + 2 * p - k) // s + 1
        xd = nhwc(c["x"]).to(dev, dt)
        wd = c["w"].permute(0, 2, 3, 1).contiguous().to(dev, dt)
        resd = nhwc(c["res"]).to(dev, dt).view(-1, Cout)
        d = _desc(L, dt, L.QT_CONV_FWD, B, (H, H), (Ho, Ho), Cin, Cout, k, s, p)
        M = B * Ho * Ho
        _check_path(L, row, d, B, H, M)
        back = lambda t: _nchw(t, B, Ho, Ho, Cout)
        ctxs = _walks(L, row)
    for ctx in ctxs:
        def run():
            d.relu = 0
            y, st = _conv(L, lib, dev, d, xd, wd, (M, Cout), dt, stats_rows=lib.qt_conv2d_stats_rows(ctypes.byref(d)))
            d.relu = 1
            ya, _ = _conv(L, lib, dev, d, xd, wd, (M, Cout), dt, sc, sh, resd)
            d.relu = 0
            return y, st, ya
        if ctx is None:
            y, st, ya = run()
        else:
            with ctx:
                y, st, ya = run()
        _agree(back(y), c["raw"], dt, (name, "raw output"))
        _agree(back(ya), c["act"], dt, (name, "scale / shift / residual / ReLU"))
        _stats_agree(st, c["raw"], (name, "statistics rows"))


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
def test_stride2_pair_nonfinite(dt):
    dev, L, lib = _env()
    c = N.s2_case("s2_56")
    clean = c["clean"]
    N.conditions(c["raw_c"], c["pre_c"], c["act"], c["images"])
    N.conditions(c["rawd_c"], c["pred_c"], F.relu(c["pred"]), c["images"])
    B, Cin, Cout, H, _ = c["row"]["cfg"]
    OH = H // 2
    xd = nhwc(c["x"]).to(dev, dt)
    wc = clean["w"].permute(0, 2, 3, 1).contiguous().to(dev, dt)
    wdd = clean["wd"].view(Cout, Cin).contiguous().to(dev, dt)
    f = [clean[n].float().to(dev) for n in ("sc", "sh", "sd", "shd")]

    def pair(relu, affine, want_stats):
        d = L.ConvS2Desc(L.qt_dtype(dt), B, H, H, Cin, Cout, relu, 0)
        assert lib.qt_conv_s2_pair_supported(ctypes.byref(d)) == 1
        y, yd = _out((B * OH * OH, Cout), dt, dev), _out((B * OH * OH, Cout), dt, dev)
        rows = lib.qt_conv_s2_pair_stats_rows(ctypes.byref(d))
        st, std = (_out((rows, 2, Cout), torch.float32, dev) for _ in range(2)) if want_stats else (None, None)
        a = [L.ptr(t) for t in f] if affine else [None] * 4
        io = L.ConvS2IO(L.ptr(xd), L.ptr(wc), L.ptr(wdd), L.ptr(y), L.ptr(yd), a[0], a[1], a[2], a[3], L.ptr(st), L.ptr(std))
        L.check(lib.qt_conv_s2_pair(ctypes.byref(d), ctypes.byref(io), L.stream_ptr()), "qt_conv_s2_pair")
        torch.cuda.synchronize()
        return y, yd, st, std
    y0, yd0, st, std = pair(0, False, True)
    y1, yd1, _, _ = pair(1, True, False)
    _agree(_nchw(y0, B, OH, OH, Cout), c["raw"], dt, "conv1 raw")
    _agree(_nchw(yd0, B, OH, OH, Cout), c["rawd"], dt, "downsample raw")
    _agree(_nchw(y1, B, OH, OH, Cout), c["act"], dt, "conv1 scale / shift / ReLU")
    _agree(_nchw(yd1, B, OH, OH, Cout), c["pred"], dt, "downsample scale / shift")
    _stats_agree(st, c["raw"], "conv1 statistics")
    _stats_agree(std, c["rawd"], "downsample statistics")


# ----------------------------------------------------------------------------------------------------------------------
# the packed stem: plain conv and fused conv + pool; the signed-zero row
# ----------------------------------------------------------------------------------------------------------------------
def _stem_pack(L, lib, dev, x, w, dt=BF):
    B = x.shape[0]
    qdt, st = L.qt_dtype(dt), L.stream_ptr()
    imd, wd = x.float().to(dev), w.float().to(dev)
    xpad = _out((B, 230, 232, 4), dt, dev)
    wp = _out((64, 8, 32), dt, dev)
    L.check(lib.qt_pack_stem_input(qdt, L.ptr(imd), L.ptr(xpad), B, st), "qt_pack_stem_input")
    L.check(lib.qt_pack_stem_weight(qdt, L.ptr(wd), L.ptr(wp), 8, st), "qt_pack_stem_weight")
    torch.cuda.synchronize()
    return imd, xpad, wp


def _stem_pooled(L, lib, dev, imd, xpad, wp, sc, sh, B):
    out = {}
    for name in ("qt_stem_conv_pool", "qt_stem_conv_pool_nchw"):
        pooled = _out((B, 56, 56, 64), BF, dev)
        src = xpad if name == "qt_stem_conv_pool" else imd
        L.check(getattr(lib, name)(L.qt_dtype(BF), L.ptr(src), L.ptr(wp), 8, L.ptr(sc), L.ptr(sh), L.ptr(pooled), B,
                                   L.stream_ptr()), name)
        torch.cuda.synchronize()
        out[name] = pooled.cpu().permute(0, 3, 1, 2)
    return out


@pytest.mark.parametrize("stem_conv", [1, 0], ids=["dedicated", "generic"])
def test_stem_conv_nonfinite(stem_conv):
    """conv_stem_kernel (qt_set_stem_conv(1), the default) and the generic half-K-step tile behind the same packed descriptor.
    The packed operands pad the 7x7 window to 8 rows x 8 pixels with zero WEIGHTS over real pixels: both kernels read the
    eighth pixel (and the generic tile the eighth tap row) as zero, or a planted value one pixel right of or one row below
    the window would reach the output as 0 * inf (5655 and 4887 NaN outputs where torch has 4183, before that)."""
    dev, L, lib = _env()
    c = N.fwd_case("stem_b1")
    N.conditions(c["raw_c"], c["pre_c"], c["act"], c["images"])
    B = c["row"]["cfg"][0]
    imd, xpad, wp = _stem_pack(L, lib, dev, c["x"], c["w"])
    sc, sh = c["scale"].float().to(dev), c["shift"].float().to(dev)
    d = _desc(L, BF, L.QT_CONV_FWD, B, (230, 232), (112, 112), 32, 64, 8, 2, 0)
    d.kw = 1
    d.src_img_stride, d.src_row_stride, d.src_pix_stride = 230 * 232 * 4, 232 * 4, 4
    lib.qt_set_stem_conv(stem_conv)
    try:
        y, st = _conv(L, lib, dev, d, xpad, wp, (B * 112 * 112, 64), BF, stats_rows=lib.qt_conv2d_stats_rows(ctypes.byref(d)))
        d.relu = 1
        ya, _ = _conv(L, lib, dev, d, xpad, wp, (B * 112 * 112, 64), BF, sc, sh)
    finally:
        lib.qt_set_stem_conv(-1)
    _agree(_nchw(y, B, 112, 112, 64), c["raw"], BF, "raw output")
    _agree(_nchw(ya, B, 112, 112, 64), c["act"], BF, "scale / shift / ReLU")
    _stats_agree(st, c["raw"], "statistics rows")


def test_stem_conv_pool_nonfinite():
    dev, L, lib = _env()
    c = N.fwd_case("stem_b1")
    N.conditions(c["raw_c"], c["pre_c"], c["act"], c["images"])
    assert bool(torch.isnan(c["pooled"]).any()) and bool((c["pooled"] == N.INF).any())
    B = c["row"]["cfg"][0]
    imd, xpad, wp = _stem_pack(L, lib, dev, c["x"], c["w"])
    sc, sh = c["scale"].float().to(dev), c["shift"].float().to(dev)
    for name, pooled in _stem_pooled(L, lib, dev, imd, xpad, wp, sc, sh, B).items():
        _agree(pooled, c["pooled"], BF, name)


def test_stem_conv_pool_negative_zero_loses_to_a_positive_neighbour():
    dev, L, lib = _env()
    c = N.signed_zero_stem_case()
    N.signed_zero_conditions(c)
    B = c["row"]["cfg"][0]
    imd, xpad, wp = _stem_pack(L, lib, dev, c["x"], c["w"])
    sc, sh = c["scale"].float().to(dev), c["shift"].float().to(dev)
    assert bool(torch.signbit(sh[c["channel"]]))                               # the -0.0 shift reached the device
    for name, pooled in _stem_pooled(L, lib, dev, imd, xpad, wp, sc, sh, B).items():
        assert E.same(pooled, c["pooled"], BF), (name, E.first_mismatch(pooled, c["pooled"], BF))


# ----------------------------------------------------------------------------------------------------------------------
# 3-D convolutions of the clip models
# ----------------------------------------------------------------------------------------------------------------------
def test_first_conv3d_nonfinite():
    dev, L, lib = _env()
    c = N.c3_case("first_w32")
    clean = c["clean"]
    N.conditions(c["raw_c"], c["pre_c"], c["act"], c["images"])
    B, T, H, W = c["row"]["cfg"]
    dt = BF
    qdt, st = L.qt_dtype(dt), L.stream_ptr()
    cd = c["x"].permute(0, 2, 1, 3, 4).contiguous().float().to(dev)
    wp = torch.zeros(64, 128)
    wp[:32, :81] = clean["w"].permute(0, 2, 3, 4, 1).reshape(32, 81).float()
    wp = wp.to(dev, dt)
    sc, sh = clean["scale"].float().to(dev), clean["shift"].float().to(dev)
    rows = lib.qt_conv3d_first_stats_rows(B, T, H, W)
    assert rows > 0
    y, y3 = _out((T, B, H, W, 32), dt, dev), _out((T, B, H, W, 32), dt, dev)
    part = _out((rows, 2, 64), torch.float32, dev)
    L.check(lib.qt_conv3d_first_fwd(qdt, L.ptr(cd), L.ptr(wp), L.ptr(y), None, None, 0, L.ptr(part), B, T, H, W, st), "stats")
    L.check(lib.qt_conv3d_first_fwd(qdt, L.ptr(cd), L.ptr(wp), L.ptr(y3), L.ptr(sc), L.ptr(sh), 1, None, B, T, H, W, st), "affine")
    torch.cuda.synchronize()
    _agree(_ncthw(y, 32), c["raw"], dt, "raw + statistics")
    _agree(_ncthw(y3, 32), c["act"], dt, "scale / shift / ReLU")
    _stats_agree(part[:, :, :32], c["raw"], "statistics rows")
    assert bool(torch.isnan(c["pooled"]).any()) and bool((c["pooled"] == N.INF).any())
    for pc in (64, 32):
        pooled = _out((T, B, H // 2, W // 2, pc), dt, dev)
        L.check(lib.qt_conv3d_first_fwd_pool(qdt, L.ptr(cd), L.ptr(wp), L.ptr(pooled), pc, L.ptr(sc), L.ptr(sh), B, T, H, W, st),
                "qt_conv3d_first_fwd_pool")
        torch.cuda.synchronize()
        _agree(_ncthw(pooled, 32), c["pooled"], dt, ("conv + scale / shift / ReLU + max pool", pc))


def test_slab_conv3d_nonfinite():
    dev, L, lib = _env()
    c = N.c3_case("c32_xc32")
    clean = c["clean"]
    N.conditions(c["raw_c"], c["pre_c"], c["act"], c["images"])
    B, T, H, W = c["row"]["cfg"]
    xc, dt = c["row"]["xc"], BF
    qdt, st = L.qt_dtype(dt), L.stream_ptr()
    xd = torch.full((T, B, H, W, xc), 3.0, dtype=dt)
    xd[..., :32] = _tb(c["x"]).to(dt)
    xd = xd.to(dev)
    wp = torch.full((64, 27, 64), 3.0, dtype=dt)
    wp[:, :, :32] = clean["w"].permute(0, 2, 3, 4, 1).reshape(64, 27, 32).to(dt)
    wp = wp.to(dev)
    sc, sh = clean["scale"].float().to(dev), clean["shift"].float().to(dev)
    rows = lib.qt_conv3d_c32_stats_rows(B, T, H, W)
    assert rows > 0
    y, y3 = _out((T, B, H, W, 64), dt, dev), _out((T, B, H, W, 64), dt, dev)
    part = _out((rows, 2, 64), torch.float32, dev)
    L.check(lib.qt_conv3d_c32_fwd(qdt, L.ptr(xd), xc, L.ptr(wp), L.ptr(y), None, None, 0, L.ptr(part), B, T, H, W, st), "stats")
    L.check(lib.qt_conv3d_c32_fwd(qdt, L.ptr(xd), xc, L.ptr(wp), L.ptr(y3), L.ptr(sc), L.ptr(sh), 1, None, B, T, H, W, st), "affine")
    torch.cuda.synchronize()
    _agree(_ncthw(y, 64), c["raw"], dt, "raw + statistics")
    _agree(_ncthw(y3, 64), c["act"], dt, "scale / shift / ReLU")
    _stats_agree(part, c["raw"], "statistics rows")


# ----------------------------------------------------------------------------------------------------------------------
# thin GEMMs
# ----------------------------------------------------------------------------------------------------------------------
def test_linear_relu_nonfinite():
    dev, L, lib = _env()
    c = N.gemm_case("lin_one_tile", relu=1)
    clean = c["clean"]
    N.conditions(c["raw_c"], c["pre_c"], c["act"], c["images"])
    M, Nn, K = c["row"]["cfg"]
    nbytes = lib.qt_linear_workspace_bytes(M, Nn, K)
    ws = torch.full((max(nbytes, 1),), 0xFF, dtype=torch.uint8, device=dev)
    y = _out((M, Nn), BF, dev)
    xd, wd, bd = c["x"].to(BF).to(dev), clean["w"].to(BF).to(dev), clean["bias"].float().to(dev)
    L.check(lib.qt_linear_bf16(L.ptr(xd), L.ptr(wd), L.ptr(bd), 1, L.ptr(y), M, Nn, K, L.ptr(ws), nbytes,
                               L.stream_ptr()), "qt_linear_bf16")
    torch.cuda.synchronize()
    _agree(y, c["act"], BF, "qt_linear_bf16 relu=1")


@pytest.mark.parametrize("K", [64, 448], ids=["thread_kernel", "wave_kernel"])
@pytest.mark.parametrize("cdt", [F32, BF], ids=["f32", "bf16"])
def test_gemm_small_relu_nonfinite(K, cdt):
    """qt_gemm_small with bias and ReLU: K = 64 takes the one-thread-per-output kernel, K = 448 a wave per output"""
    dev, L, lib = _env()
    M, Nn = 5, 12
    g = E.gen(900 + K)
    x = N.plant(E.ints((M, K), 1, g), {64: 3, 448: 1}[K], 1, 2)   # (seeds for which every class appears; asserted below)
    w = E.weights((Nn, K), 1 / 2, 1, g)
    bias = E.ints((Nn,), 4, g)
    pre = x @ w.t() + bias
    rule = N.gemm_rule(x, w)
    assert torch.equal(N.classes(pre), rule) and all(bool((rule == k).any()) for k in (N.NAN, N.PINF, N.NINF, N.FIN))
    assert bool(torch.isfinite(pre[2:]).all())
    C = _out((M, Nn), cdt, dev)
    d = GemmSmallDesc(M, Nn, K, L.qt_dtype(F32), L.qt_dtype(F32), L.qt_dtype(cdt), K, 1, K, 1, Nn, 1, 0)
    xd, wd, bd = x.float().to(dev), w.float().to(dev), bias.float().to(dev)
    L.check(lib.qt_gemm_small(ctypes.byref(d), L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(C), L.stream_ptr()), "qt_gemm_small")
    torch.cuda.synchronize()
    _agree(C, F.relu(pre), cdt, "qt_gemm_small relu")


# ----------------------------------------------------------------------------------------------------------------------
# elementwise: qt_bn_act, the attention gate, qt_bn_finalize
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("residual", ["none", "plain", "affine"])
def test_bn_act_nonfinite(dt, residual):
    dev, L, lib = _env()
    c = N.bn_act_case()
    M, C = c["y"].shape
    f = lambda t: t.float().to(dev)
    y, res = c["y"].to(dt).to(dev), c["res"].to(dt).to(dev)
    rs, rb = (f(c["rscale"]), f(c["rshift"])) if residual == "affine" else (None, None)
    sc, sh = f(c["scale"]), f(c["shift"])
    for relu in (0, 1):
        ref, rule = N.bn_act_ref(c, residual, relu)
        assert torch.equal(N.classes(ref), rule)
        out, out1 = _out((M, C), dt, dev), _out((M, C), dt, dev)
        bits = torch.zeros((M, C // 8), dtype=torch.uint8, device=dev)
        args = (L.qt_dtype(dt), L.ptr(y), L.ptr(sc), L.ptr(sh), L.ptr(res) if residual != "none" else None,
                L.ptr(rs), L.ptr(rb), relu)
        L.check(lib.qt_bn_act(*args, L.ptr(out), M, C, L.stream_ptr()), "qt_bn_act")
        L.check(lib.qt_bn_act_mask(*args, L.ptr(out1), L.ptr(bits), M, C, L.stream_ptr()), "qt_bn_act_mask")
        torch.cuda.synchronize()
        _agree(out, ref, dt, ("qt_bn_act", residual, relu))
        _agree(out1, ref, dt, ("qt_bn_act_mask", residual, relu))


def test_attention_gate_nonfinite():
    """a NaN in one vector of image 0, a +inf in one of image 1 whose hidden weights are all non-zero: act (post-ReLU hidden),
    alpha and the fused output carry NaN / +inf where torch's float64 gate does; image 2 stays finite and close"""
    dev, L, lib = _env()
    B, ld, col0 = 3, 128, 64
    g = E.gen(33)
    v = torch.rand(B, 16, 64, generator=g, dtype=torch.float64)
    w1 = torch.randn(32, 64, generator=g, dtype=torch.float64) * 0.3
    b1 = torch.randn(32, generator=g, dtype=torch.float64) * 0.1
    w2 = torch.randn(1, 32, generator=g, dtype=torch.float64) * 0.5
    b2 = torch.randn(1, generator=g, dtype=torch.float64) * 0.1
    v[0, 3, 7] = float("nan")
    v[1, 5, 9] = N.INF
    v, w1, b1, w2, b2 = (t.float().double() for t in (v, w1, b1, w2, b2))
    a = F.relu(F.linear(v, w1, b1))
    alpha = F.softmax(F.linear(a, w2, b2).squeeze(-1), dim=1)
    out = (v * alpha.unsqueeze(-1)).sum(1)
    assert bool(torch.isnan(a[0, 3]).all()) and bool((a[1, 5] == N.INF).any()) and bool((a[1, 5] == 0).any())
    assert bool(torch.isnan(alpha[:2]).all()) and bool(torch.isfinite(out[2]).all())
    f32 = dict(dtype=torch.float32, device=dev)
    act, al = _out((B, 16, 32), F32, dev), _out((B, 16), F32, dev)
    fused = torch.zeros(B, ld, **f32)
    dv = [t.float().to(dev) for t in (v, w1, b1, w2, b2)]
    L.check(lib.qt_attention_gate(L.qt_dtype(F32), L.ptr(dv[0]), L.ptr(dv[1]), L.ptr(dv[2]), L.ptr(dv[3]), L.ptr(dv[4]),
                                  L.ptr(act), L.ptr(al), L.ptr(fused), B, ld, col0, L.stream_ptr()), "qt_attention_gate")
    torch.cuda.synchronize()
    got = fused[:, col0:col0 + 64].cpu().double()
    for name, gt, ref in (("act", act.cpu().double(), a), ("alpha", al.cpu().double(), alpha), ("out", got, out)):
        assert torch.equal(N.classes(gt), N.classes(ref)), (name, int(torch.isnan(gt).sum()), int(torch.isnan(ref).sum()))
        fin = torch.isfinite(ref)
        assert rel_err(gt[fin], ref[fin]) <= 1e-5, name      # (the bound tests/test_attention_gpu.py holds the f32 gate to)


def test_bn_finalize_nonfinite():
    dev, L, lib = _env()
    c = N.finalize_case()
    ref = N.finalize_ref(c)
    partial = c["partial"].to(dev)
    rows, _, C = partial.shape
    assert lib.qt_stats_capacity_rows(rows) == rows
    outs = {k: _out((C,), F32, dev) for k in ("mean", "invstd", "scale", "shift")}
    rm, rv = c["rmean"].to(dev), c["rvar"].to(dev)
    gamma, beta = c["gamma"].to(dev), c["beta"].to(dev)
    nbt = torch.zeros(1, dtype=torch.int64, device=dev)
    L.check(lib.qt_bn_finalize(L.ptr(partial), rows, C, c["count"], L.ptr(gamma), L.ptr(beta),
                               L.ptr(rm), L.ptr(rv), L.ptr(nbt), 0.1, 1e-5, L.ptr(outs["mean"]), L.ptr(outs["invstd"]),
                               L.ptr(outs["scale"]), L.ptr(outs["shift"]), L.stream_ptr()), "qt_bn_finalize")
    torch.cuda.synchronize()
    outs["running_mean"], outs["running_var"] = rm, rv
    # the kernel is the same double arithmetic on the same f32 rows, rounded to f32 once: 2^-23 of the magnitudes that meet
    mag = dict(mean=ref["mean"].abs(), invstd=ref["invstd"].abs(), scale=ref["scale"].abs(),
               shift=c["beta"].double().abs() + (ref["mean"] * ref["scale"]).abs(),
               running_mean=c["rmean"].double().abs() + ref["mean"].abs(),
               running_var=c["rvar"].double().abs() + ref["running_var"].abs())
    for k, r in ref.items():
        got = outs[k].cpu().double()
        assert torch.equal(N.classes(got), N.classes(r)), (k, got.tolist(), r.tolist())
        fin = torch.isfinite(r)
        assert bool(((got - r).abs()[fin] <= 2.0 ** -22 * mag[k][fin]).all()), k


# ----------------------------------------------------------------------------------------------------------------------
# max pools: ATen's value and argmax
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
def test_stem_pool_nonfinite(dt):
    dev, L, lib = _env()
    c = N.stem_pool_case()
    B = c["y"].shape[0]
    yd = nhwc(c["y"]).to(dt).to(dev)
    sc, sh = c["scale"].float().to(dev), c["shift"].float().to(dev)
    pooled, ymax = _out((B, 56, 56, 64), dt, dev), _out((B, 56, 56, 64), dt, dev)
    arg = torch.full((B, 56, 56, 64), 0xFF, dtype=torch.uint8, device=dev)
    L.check(lib.qt_stem_pool(L.qt_dtype(dt), L.ptr(yd), L.ptr(sc), L.ptr(sh), L.ptr(pooled), L.ptr(arg), L.ptr(ymax), B,
                             L.stream_ptr()), "qt_stem_pool")
    torch.cuda.synchronize()
    _agree(pooled.cpu().permute(0, 3, 1, 2), c["out"], dt, "pooled")
    # the argmax where it is unique by ATen's rule: a NaN window (last NaN) and a window with one strict maximum
    code = arg.cpu().permute(0, 3, 1, 2)
    nanw = torch.isnan(c["out"])
    assert torch.equal(code[nanw], c["code"][nanw]), "argmax of a NaN window is its last NaN"
    assert torch.equal(code, c["code"]), "argmax (first maximum in scan order, last NaN)"
    _agree(ymax.cpu().permute(0, 3, 1, 2), c["ymax"], dt, "y at the argmax")


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
def test_quad_pool_nonfinite(dt):
    dev, L, lib = _env()
    c = N.quad_pool_case()
    B = c["flat"].shape[0]
    ld = 4608
    qd = nhwc(c["q"]).to(dt).to(dev)
    dst = _out((B, ld), dt, dev)
    L.check(lib.qt_quad_pool(L.qt_dtype(dt), L.ptr(qd), L.ptr(dst), B, ld, 0, L.stream_ptr()), "qt_quad_pool")
    torch.cuda.synchronize()
    _agree(dst, c["flat"], dt, "qt_quad_pool")


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("pt", [1, 2])
def test_pool3d_max_nonfinite(pt, dt):
    dev, L, lib = _env()
    c = N.pool3d_case(pt)
    B, C, T, H, W = c["x"].shape
    xd = _tb(c["x"]).to(dt).to(dev)
    ps = (T // pt, B, H // 2, W // 2, C)
    out, only = _out(ps, dt, dev), _out(ps, dt, dev)
    arg = torch.full(ps, 0xFF, dtype=torch.uint8, device=dev)
    q, st = L.qt_dtype(dt), L.stream_ptr()
    L.check(lib.qt_pool3d_max(q, L.ptr(xd), L.ptr(out), L.ptr(arg), T, B, H, W, C, pt, st), "qt_pool3d_max")
    L.check(lib.qt_pool3d_max(q, L.ptr(xd), L.ptr(only), None, T, B, H, W, C, pt, st), "qt_pool3d_max (no argmax)")
    torch.cuda.synchronize()
    _agree(_ncthw(out, C), c["out"], dt, "pooled")
    _agree(_ncthw(only, C), c["out"], dt, "pooled (no argmax)")
    assert torch.equal(_ncthw(arg, C), c["code"]), "argmax (first maximum in scan order, last NaN)"


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("pt", [1, 2])
def test_pool3d_bn_relu_max_nonfinite(pt, dt):
    dev, L, lib = _env()
    c = N.pool3d_fused_case(pt)
    B, C, T, H, W = c["y"].shape
    yd = _tb(c["y"]).to(dt).to(dev)
    sc, sh = c["scale"].float().to(dev), c["shift"].float().to(dev)
    ps = (T // pt, B, H // 2, W // 2, C)
    out, ymax, ev = _out(ps, dt, dev), _out(ps, dt, dev), _out(ps, dt, dev)
    arg = torch.full(ps, 0xFF, dtype=torch.uint8, device=dev)
    q, st = L.qt_dtype(dt), L.stream_ptr()
    L.check(lib.qt_pool3d_bn_relu_max(q, L.ptr(yd), L.ptr(sc), L.ptr(sh), L.ptr(out), L.ptr(arg), L.ptr(ymax), T, B, H, W, C, C, pt,
                                      st), "qt_pool3d_bn_relu_max")
    L.check(lib.qt_pool3d_bn_relu_max(q, L.ptr(yd), L.ptr(sc), L.ptr(sh), L.ptr(ev), None, None, T, B, H, W, C, C, pt, st),
            "qt_pool3d_bn_relu_max (eval)")
    torch.cuda.synchronize()
    _agree(_ncthw(out, C), c["out"], dt, "pooled")
    _agree(_ncthw(ev, C), c["out"], dt, "pooled (eval form)")
    assert torch.equal(_ncthw(arg, C), c["code"]), "argmax (first maximum in scan order, last NaN)"
    _agree(_ncthw(ymax, C), c["ymax"], dt, "y at the argmax")


# ----------------------------------------------------------------------------------------------------------------------
# model level, against the CPU oracle
# ----------------------------------------------------------------------------------------------------------------------
def _oracle():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import oracle.quadtree_oracle as o
    return o


def _images(B, salt):
    synth = pkg("synth")
    return synth.synth_images(B, salt=salt), synth.synth_pose_features(B, salt=salt)


def _clips(B, T, HW, salt):
    synth = pkg("synth")
    return (synth.synth_images(B * T, salt=salt, size=HW).view(B, T, 3, HW, HW),
            synth.synth_pose_features(B * T, salt=salt, realistic=True).view(B, T, 47))


def _model(kind, dt):
    """(module with synth weights, oracle forward(sd, x, f, **kw) -> logits, sd transform, inputs, a conv weight key)"""
    P, synth, o = pkg(), pkg("synth"), _oracle()
    ident = lambda sd: sd
    if kind == "quadtree":
        m, fwd, tr, (x, f), key = (P.QuadtreeCNN(12, dropout_rate=0.0, compute_dtype=dt), o.quadtree_forward, ident, _images(2, 0),
                                   "base_cnn.layer2.0.conv1.weight")
    elif kind == "standard":
        m, tr, (x, f), key = P.StandardResNetCNN(12, dropout_rate=0.0, compute_dtype=dt), ident, _images(2, 0), "base_cnn.layer2.0.conv1.weight"
        fwd = lambda sd, x, f, **kw: o.standard_resnet_forward(sd, x, **kw)
    elif kind == "attention":
        m, fwd, tr, (x, f) = P.AttentionHierarchicalCNN(12, dropout_rate=0.0, compute_dtype=dt), o.attention_forward, o.attention_sd_to_base, _images(2, 0)
        key = "features_extractor.5.0.conv1.weight"
    elif kind == "cnn_lstm":
        m, fwd, tr = P.CnnLstm(12, sequence_length=3, dropout_rate=0.0, compute_dtype=dt), o.cnn_lstm_forward, o.cnn_lstm_sd_to_base
        xi, fi = _images(6, 7)
        x, f, key = xi.view(2, 3, 3, 224, 224), fi.view(2, 3, 47), "cnn_backbone.5.0.conv1.weight"
    elif kind == "quadtree3d":
        m, fwd, tr = P.Quadtree3DCNN(12, sequence_length=5, mode="quadtree_3d_fusion", dropout_rate=0.0, compute_dtype=dt), \
            o.quadtree3d_forward, ident
        (x, f), key = _clips(2, 5, 64, 31), "conv3d_block2.0.weight"
    else:
        m, fwd, tr = P.Ji3DCNN(12, sequence_length=4, dropout_rate=0.0, compute_dtype=dt), o.ji3d_forward, ident
        (x, f), key = _clips(2, 4, 64, 32), "visual_stream.2.0.weight"
    m.load_state_dict(synth.synth_state_dict(m))
    assert key in m.state_dict(), key
    return m, fwd, tr, x.clone(), f.clone(), key


KINDS = ["quadtree", "standard", "attention", "cnn_lstm", "quadtree3d", "ji3d"]


def _pattern_agrees(got, ref, dt, what, untouched=None):
    got, ref = got.detach().float().cpu(), ref.detach().float()
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), (what, "isnan", torch.isnan(got).tolist(), torch.isnan(ref).tolist())
    assert torch.equal(torch.isinf(got) * torch.sign(got).nan_to_num(), torch.isinf(ref) * torch.sign(ref).nan_to_num()), (what, "isinf")
    if untouched is not None:
        assert bool(torch.isfinite(ref[untouched]).all()), what
        assert rel_err(got[untouched], ref[untouched]) <= LOGIT_TOL[dt], (what, rel_err(got[untouched], ref[untouched]))


def _poke(x, value):
    """the value into one pixel of image / clip 0 (a middle frame of a clip)"""
    x = x.clone()
    if x.dim() == 5:
        x[0, x.shape[1] // 2, 1, x.shape[-2] // 2, x.shape[-1] // 3] = value
    else:
        x[0, 1, x.shape[-2] // 2, x.shape[-1] // 3] = value
    return x


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("value", [float("nan"), N.INF], ids=["nan_pixel", "inf_pixel"])
@pytest.mark.parametrize("kind", KINDS)
def test_eval_with_a_nonfinite_pixel_follows_the_oracle(kind, value, dt):
    dev, _, _ = _env()
    m, fwd, tr, x, f, _ = _model(kind, dt)
    x = _poke(x, value)
    sd = tr({k: v.detach().clone() for k, v in m.state_dict().items()})
    with torch.no_grad():
        ref = fwd(sd, x, f)
    assert bool(torch.isnan(ref[0]).any() | torch.isinf(ref[0]).any()) and bool(torch.isfinite(ref[1:]).all())
    m = m.to(dev).eval()
    with torch.no_grad():
        fused = m(x.to(dev), f.to(dev))
    _pattern_agrees(fused, ref, dt, (kind, "no_grad forward"), slice(1, None))
    kept = m(x.to(dev), f.to(dev))
    _pattern_agrees(kept, ref, dt, (kind, "forward with grad enabled"), slice(1, None))


@pytest.mark.parametrize("kind", KINDS)
def test_eval_with_a_nan_conv_weight_follows_the_oracle(kind):
    dev, _, _ = _env()
    dt = F32
    m, fwd, tr, x, f, key = _model(kind, dt)
    sd0 = m.state_dict()
    ptr = sd0[key].data_ptr()
    new = {k: v.detach().clone() for k, v in sd0.items()}
    for k, v in sd0.items():
        if v.data_ptr() == ptr:
            new[k].view(-1)[5] = float("nan")
    m.load_state_dict(new)
    with torch.no_grad():
        ref = fwd(tr({k: v.detach().clone() for k, v in m.state_dict().items()}), x, f)
    assert bool(torch.isnan(ref).any())
    m = m.to(dev).eval()
    with torch.no_grad():
        got = m(x.to(dev), f.to(dev))
    _pattern_agrees(got, ref, dt, (kind, "NaN weight", key))


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_train_step_with_a_nan_pixel_follows_the_oracle(kind, dt):
    """logits, loss, every BatchNorm running buffer: isnan as in the oracle; a parameter gradient that is NaN in the oracle
    holds a NaN"""
    dev, _, _ = _env()
    o = _oracle()
    synth = pkg("synth")
    m, fwd, tr, x, f, _ = _model(kind, dt)
    x = _poke(x, float("nan"))
    y = synth.synth_labels(x.shape[0], 12, salt=3)
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    leaves = {n: sd0[n].clone().requires_grad_(True) for n, p in m.named_parameters() if p.requires_grad}   # (frozen backbones)
    sd = tr({k: leaves.get(k, v.clone()) for k, v in sd0.items()})
    ref = fwd(sd, x, f, train=True, dropout_p=0.0)
    ref_loss = F.cross_entropy(ref, y)
    ref_loss.backward()
    m = m.to(dev).train()
    logits = m(x.to(dev), f.to(dev))
    loss = F.cross_entropy(logits, y.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    _pattern_agrees(logits, ref, dt, (kind, "train logits"))
    assert bool(torch.isnan(loss)) == bool(torch.isnan(ref_loss)), (float(loss), float(ref_loss))
    bufs = tr({k: v.detach().cpu() for k, v in m.named_buffers()})      # under the names the oracle's buffers go by
    checked = 0
    for k, v in bufs.items():
        if k.endswith(("running_mean", "running_var")):
            assert torch.equal(torch.isnan(v.float()), torch.isnan(sd[k].detach().float())), (kind, k)
            checked += 1
    assert checked > 0
    params = dict(m.named_parameters())
    nan_grads = 0
    for n, leaf in leaves.items():
        if leaf.grad is not None and bool(torch.isnan(leaf.grad).any()):
            assert params[n].grad is not None and bool(torch.isnan(params[n].grad).any()), (kind, n)
            nan_grads += 1
    assert nan_grads > 0
