"""Every convolution kernel path against the float64 reference on the integer-grid cases of tests/_exact.py: the comparison
is torch.equal throughout (no tolerance).  conditions() runs on the reference before a kernel result is looked at; the rows
are the ones tests/test_exact_data_cpu.py checks without a GPU.  The kernels are driven by the launch helpers of the existing
test files; the path a row names is confirmed the way those files do it (qt_conv2d_stats_rows mirrors the dispatch, the
workspace size tells the streaming weight-gradient kernels, qt_set_* switches force a path).  Rows with a field `walk` are
there for the second and later work items of a persistent kernel's workgroups: that every workgroup takes that many items is
asserted from the grid the library reports before a result is looked at (a failure, never a skip).  The stem and layer-1
ring kernels walk contiguous shares of their tiles: their walk rows assert what E.WALKS records of the share table (a third
tile, first and last tiles of an image on later trips, four tiles and two window wraps on the ring), from the reported grid
or, for the fused stem and the stem weight gradient, which have no query, from the launch code's min(tiles, 256).

The BatchNorm-backward link sums of the patch-resident stride-1 data gradients stay with tests/test_conv_pt_gpu.py; the
ring kernel's and the merged stride-2 forms' get a dyadic xhat here and are compared exactly."""
import ctypes

import pytest
import torch

import _exact as E
from _exact import BF, F32
from _guard import Guard
from _stem_bounds import tile_ranges
from _util import pkg
from test_conv_gpu import PackItem, nhwc, run_conv, run_wgrad
from test_conv_pt_gpu import _maxwg, _pt, tiles
from test_mask_bits_gpu import pack_bits
from test_conv_s2_gpu import run_pair
from test_stem_gpu import _stem_conv

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _same(got, ref, dt, what, walk=None):
    """torch.equal against the reference in the output type; the message names the first differing element and, for a map
    [N][C][H][W] of the walk row `walk`, the tile, workgroup and trip it belongs to (E.locate)"""
    got = got.cpu()
    if not E.same(got, ref, dt):
        bad = E.first_mismatch(got, ref, dt)
        where = E.locate(walk, bad[0]) if walk and walk.get("walk") and walk["name"] in E.WALKS else None
        assert False, (what, "first mismatch (index, got, want, count):", bad, where)


def _nchw(y, n, h, w, c):
    return y.cpu().view(n, h, w, c).permute(0, 3, 1, 2)


def _desc(L, dt, mode, B, in_hw, out_hw, kin, kout, k, s, p, quad=0):
    d = L.ConvDesc()
    d.dtype, d.mode, d.batch = L.qt_dtype(dt), mode, B
    d.in_h, d.in_w = in_hw
    d.out_h, d.out_w = out_hw
    d.k_per_tap, d.n_out, d.kh, d.kw, d.stride, d.pad, d.quad = kin, kout, k, k, s, p, quad
    d.src_img_stride, d.src_row_stride, d.src_pix_stride = in_hw[0] * in_hw[1] * kin, in_hw[1] * kin, kin
    return d


def _path_rows(L, d):
    """stats rows of the descriptor: (default dispatch, with the ring and the patch-resident kernels switched off)"""
    lib = L.lib()
    on = lib.qt_conv2d_stats_rows(ctypes.byref(d))
    lib.qt_set_patch_conv(0)
    lib.qt_set_pt_conv(0)
    try:
        off = lib.qt_conv2d_stats_rows(ctypes.byref(d))
    finally:
        lib.qt_set_patch_conv(-1)
        lib.qt_set_pt_conv(-1)
    return on, off


def _check_path(L, row, d, B, H, M):
    """M: rows of the implicit GEMM.  The generic tile emits one statistics row per pixel tile: 256 pixels on the 256 x 128
    three-stage tile, 128 on the 128 x 64 / 128 x 128 two-stage tiles"""
    on, off = _path_rows(L, d)
    if row["path"] == "generic":
        assert off == -(-M // (256 if row.get("tile256") else 128)), (off, M)
        assert on == off or row.get("pt_off"), (on, off)
    elif row["path"] == "ring":
        # one row per workgroup of the persistent kernel: min(tiles, 256) workgroups take contiguous shares of the 256-position
        # tiles of the padded grid.  A `walk` row is there for a share's third and later tiles (the window wraps with the third)
        assert on == min(E.ring_tiles(B, H), 256) and on != off and off == -(-M // 128), (on, off)
        if row.get("walk"):
            _walk_precondition(row, E.ring_tiles(B, H), on)
            f = E.share_facts(E.ring_tiles(B, H), on)
            assert f["least"] >= row["walk"] >= 3 and f["most"] > f["least"], f
    else:
        assert row["path"] == "pt" and on == 2 * (B if row.get("quad") else tiles(B, H)) and on != off, (on, off)
        assert off == -(-M // 128)


class _nothing:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _walks(L, row):
    """the patch-resident kernel runs with one workgroup (every item walked by it) and with the default grid"""
    if row["path"] == "pt":
        return [_maxwg(L, 1), _maxwg(L, 0)]
    return [_pt(L, False)] if row.get("pt_off") else [_nothing()]


# ----------------------------------------------------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------------------------------------------------
FWD, FWD_IDS = E.expand(E.FWD_ROWS)


@pytest.mark.parametrize("row,dt", FWD, ids=FWD_IDS)
def test_forward_is_bit_exact(row, dt):
    dev = _dev()
    L = pkg("_lib")
    c = E.fwd_data(row)
    E.fwd_conditions(c, dt)
    if row.get("frames"):
        return _forward_27_taps(L, dev, row, dt, c)
    B, Cin, Cout, H, k, s, p = row["cfg"]
    mode = row["mode"]
    Ho = (H + 2 * p - k) // s + 1
    n_img = c["x"].shape[0]
    quad, strides = 0, None
    if row.get("quad"):
        quad = row["quad"]
        S = 4 if quad == 4 else 2
        strides = (S * S * H * H * Cin, S * H * Cin, Cin)
        xd = nhwc(c["base"]).to(dev, dt)
    elif row.get("slice_of"):
        Cw = row["slice_of"]
        wide = E.ints((B, H, H, Cw), 1, E.gen(row["seed"] + 1))
        wide[..., 64:64 + Cin] = nhwc(c["x"])
        strides = (H * H * Cw, H * Cw, Cw)
        xd = wide.to(dev, dt).view(-1)[64:]
    else:
        xd = nhwc(c["x"]).to(dev, dt)
    wd = c["w"].permute(0, 2, 3, 1).contiguous().to(dev, dt)
    resd = nhwc(c["res"]).to(dev, dt).view(-1, Cout)
    sc, sh = c["scale"].float().to(dev), c["shift"].float().to(dev)
    d = _desc(L, dt, L.QT_CONV_FWD, B, (H, H), (Ho, Ho), Cin, Cout, k, s, p, quad)
    if strides:
        d.src_img_stride, d.src_row_stride, d.src_pix_stride = strides
    _check_path(L, row, d, B, H, n_img * Ho * Ho)
    mr = n_img * Ho * Ho
    for ctx in _walks(L, row):
        with ctx:
            y, st = run_conv(L, dt, xd, wd, B, (H, H), (Ho, Ho), Cin, Cout, k, k, s, p, L.QT_CONV_FWD, quad=quad,
                             want_stats=True, strides=strides, m_rows=mr)
            ya, _ = run_conv(L, dt, xd, wd, B, (H, H), (Ho, Ho), Cin, Cout, k, k, s, p, L.QT_CONV_FWD, quad=quad, relu=1,
                             scale=sc, shift=sh, residual=resd, strides=strides, m_rows=mr)
        _same(_nchw(y, n_img, Ho, Ho, Cout), c["raw"], dt, "raw output", row)
        _same(_nchw(ya, n_img, Ho, Ho, Cout), c["act"], dt, "scale / shift / residual / ReLU epilogue", row)
        if mode == "A":
            assert E.stats_equal(st, c["raw"]), "statistics rows"


def _forward_27_taps(L, dev, row, dt, c):
    """kt = 3: the 27-tap launch on time-major clips, raw + statistics and the fused epilogue"""
    B, Cin, Cout, H, k, s, p = row["cfg"]
    T = row["frames"]
    xd = c["x"].permute(2, 0, 3, 4, 1).contiguous().to(dev, dt)                  # [T][B][H][W][C]
    wf = c["w"].permute(0, 2, 3, 4, 1).contiguous().to(dev, dt)                  # [O][kt][kh][kw][I]
    resd = c["res"].permute(2, 0, 3, 4, 1).contiguous().to(dev, dt).view(-1, Cout)
    sc, sh = c["scale"].float().to(dev), c["shift"].float().to(dev)
    d = _desc(L, dt, L.QT_CONV_FWD, T * B, (H, H), (H, H), Cin, Cout, 3, 1, 1)
    d.kt, d.frames = 3, T
    rows = L.lib().qt_conv2d_stats_rows(ctypes.byref(d))
    gd = Guard(dev)
    xd, wf, resd, sc, sh = (gd.input(n, t) for n, t in (("x", xd), ("w", wf), ("residual", resd), ("scale", sc), ("shift", sh)))
    y = gd.output("y", (T * B * H * H, Cout), dt)
    st = gd.output("stats", (rows, 2, Cout), torch.float32)   # (the generic tile stores every partial row)
    io = L.ConvIO(L.ptr(xd), L.ptr(wf), L.ptr(y), None, None, None, None, L.ptr(st))
    L.check(L.lib().qt_conv2d_igemm(ctypes.byref(d), ctypes.byref(io), L.stream_ptr()), "qt_conv2d_igemm kt=3")
    d.relu = 1
    ya = gd.output("y_act", (T * B * H * H, Cout), dt)
    io = L.ConvIO(L.ptr(xd), L.ptr(wf), L.ptr(ya), L.ptr(sc), L.ptr(sh), L.ptr(resd), None, None)
    L.check(L.lib().qt_conv2d_igemm(ctypes.byref(d), ctypes.byref(io), L.stream_ptr()), "qt_conv2d_igemm kt=3")
    gd.check()

    def back(t):
        return t.cpu().view(T, B, H, H, Cout).permute(1, 4, 0, 2, 3)
    _same(back(y), c["raw"], dt, "raw output")
    _same(back(ya), c["act"], dt, "epilogue")
    assert E.stats_equal(st, c["raw"]), "statistics rows"


S2, S2_IDS = E.expand(E.S2_ROWS)


@pytest.mark.parametrize("row,dt", S2, ids=S2_IDS)
def test_stride2_pair_is_bit_exact(row, dt):
    """qt_conv_s2_pair (run_pair asserts qt_conv_s2_pair_supported): both raw outputs with their statistics, both eval epilogues"""
    dev = _dev()
    L = pkg("_lib")
    c = E.s2_data(row)
    E.s2_conditions(c, dt)
    B, Cin, Cout, H, maxwg = row["cfg"]
    OH = H // 2
    xd = nhwc(c["x"]).to(dev, dt)
    wc = c["w"].permute(0, 2, 3, 1).contiguous().to(dev, dt)
    wdd = c["wd"].view(Cout, Cin).contiguous().to(dev, dt)
    f = [c[n].float().to(dev) for n in ("sc", "sh", "sd", "shd")]
    L.lib().qt_set_conv_s2_max_workgroups(maxwg)
    try:
        y0, yd0, st, std = run_pair(L, dt, xd, wc, wdd, B, H, Cin, Cout, want_stats=True)
        y1, yd1, _, _ = run_pair(L, dt, xd, wc, wdd, B, H, Cin, Cout, relu_conv=1, sc=f[0], sh=f[1], sd=f[2], shd=f[3])
    finally:
        L.lib().qt_set_conv_s2_max_workgroups(0)
    _same(_nchw(y0, B, OH, OH, Cout), c["raw"], dt, "conv1 raw")
    _same(_nchw(yd0, B, OH, OH, Cout), c["rawd"], dt, "downsample raw")
    _same(_nchw(y1, B, OH, OH, Cout), c["act"], dt, "conv1 scale / shift / ReLU")
    _same(_nchw(yd1, B, OH, OH, Cout), c["pred"], dt, "downsample scale / shift")
    if row["mode"] == "A":
        assert E.stats_equal(st, c["raw"]) and E.stats_equal(std, c["rawd"])


def _stem_walk_precondition(row, B, grid):
    """the stem walk rows are there for what E.stem_walk_reaches() names, on `grid` workgroups (the count the library
    reports, or the launch code's where there is no query).  A failure, not a skip"""
    per, cap, want = E.WALKS[row["name"]]
    assert grid == min(per * B, cap), (row["name"], "workgroups", grid, "expected", min(per * B, cap))
    f = E.share_facts(per * B, grid, per)
    assert f["items"] >= row["walk"] * grid + 1 and E.stem_walk_reaches(f), (row["name"], f)


def _packed_stem_conv(L, row, c, imd, wd, sc, sh):
    """qt_conv2d_igemm on the packed descriptor: conv_stem_kernel (qt_set_stem_conv(1)) raw + statistics and scale / shift /
    ReLU, on a walk row its two other instantiations as well (raw alone; scale / shift / ReLU with the statistics, which
    are those of the raw accumulators); the generic half-K-step tile behind the same descriptor (qt_set_stem_conv(0))"""
    lib = L.lib()
    dt, mode = BF, row["mode"]
    rows = {}
    try:
        for on in (1, 0):
            lib.qt_set_stem_conv(on)
            y, st = _stem_conv(L, dt, imd, wd, 8, True)
            rows[on] = st.shape[0]
            if on and row.get("walk"):   # (the statistics rows of conv_stem_kernel are its workgroups)
                _stem_walk_precondition(row, row["cfg"][0], rows[on])
            _same(y.cpu().permute(0, 3, 1, 2), c["raw"], dt, ("raw + statistics", on), row)
            if mode == "A":
                assert E.stats_equal(st, c["raw"]), on
            del y
            ya, _ = _stem_conv(L, dt, imd, wd, 8, False, sc, sh, relu=1)
            _same(ya.cpu().permute(0, 3, 1, 2), c["act"], dt, ("scale / shift / ReLU", on), row)
            del ya
            if on and row.get("walk"):
                y, _ = _stem_conv(L, dt, imd, wd, 8, False)
                _same(y.cpu().permute(0, 3, 1, 2), c["raw"], dt, "raw", row)
                del y
                ya, st = _stem_conv(L, dt, imd, wd, 8, True, sc, sh, relu=1)
                assert st.shape[0] == rows[on]
                _same(ya.cpu().permute(0, 3, 1, 2), c["act"], dt, "scale / shift / ReLU + statistics", row)
                assert E.stats_equal(st, c["raw"]), "statistics beside scale / shift / ReLU"
                del ya
    finally:
        lib.qt_set_stem_conv(-1)
    assert rows[1] != rows[0]          # the dedicated kernel keeps its own row count: it was the path taken


@pytest.mark.parametrize("row", E.STEM_ROWS, ids=E.ids(E.STEM_ROWS))
def test_packed_stem_is_bit_exact(row):
    """conv_stem.hip (qt_set_stem_conv(1)) and the generic half-K-step tile behind the same packed descriptor
    (qt_set_stem_conv(0)); qt_stem_conv_pool and qt_stem_conv_pool_nchw against relu -> max pool of the reference"""
    dev = _dev()
    L = pkg("_lib")
    lib = L.lib()
    dt = BF
    qdt = L.qt_dtype(dt)
    c = E.stem_data(row)
    mode = row["mode"]
    E.conditions(c["raw"], c["araw"], dt, mode, w=c["w"], acts=[c["x"]], stats=(mode == "A"))
    E.conditions(c["pre"], c["apre"], dt, mode, zeros=False)
    B = row["cfg"][0]
    only = row.get("only", ("conv", "pool"))
    imd, wd = c["x"].float().to(dev), c["w"].float().to(dev)
    sc, sh = c["scale"].float().to(dev), c["shift"].float().to(dev)
    if "conv" in only:
        _packed_stem_conv(L, row, c, imd, wd, sc, sh)
    if "pool" not in only:
        return
    if row.get("walk"):
        # qt_stem_conv_pool and qt_stem_conv_pool_nchw have no query: both launch min(28 B, 256) workgroups on contiguous
        # shares of the B * 28 tiles (two pooled rows each) -- conv_stem.hip
        _stem_walk_precondition(row, B, 256)
    st_ = L.stream_ptr()
    gd = Guard(dev)
    imd, wd, sc, sh = gd.input("image", imd), gd.input("w", wd), gd.input("scale", sc), gd.input("shift", sh)
    xpad = gd.output("xpad", (B, 230, 232, 4), dt)       # the packers write every element, zero borders included
    L.check(lib.qt_pack_stem_input(qdt, L.ptr(imd), L.ptr(xpad), B, st_), "qt_pack_stem_input")
    wp = gd.output("w_packed", (64, 8, 32), dt)
    L.check(lib.qt_pack_stem_weight(qdt, L.ptr(wd), L.ptr(wp), 8, st_), "qt_pack_stem_weight")
    gd.check()
    for name in ("qt_stem_conv_pool", "qt_stem_conv_pool_nchw"):
        pooled = gd.output(name, (B, 56, 56, 64), dt)
        src = xpad if name == "qt_stem_conv_pool" else imd
        L.check(getattr(lib, name)(qdt, L.ptr(src), L.ptr(wp), 8, L.ptr(sc), L.ptr(sh), L.ptr(pooled), B, st_), name)
        gd.check()
        _same(pooled.cpu().permute(0, 3, 1, 2), c["pooled"], dt, name, row)


# ----------------------------------------------------------------------------------------------------------------------
# data gradients
# ----------------------------------------------------------------------------------------------------------------------
DG, DG_IDS = E.expand(E.DGRAD_ROWS)


@pytest.mark.parametrize("row,dt", DG, ids=DG_IDS)
def test_data_gradient_is_bit_exact(row, dt):
    """plain, and with residual + ReLU mask whose source holds +0.0 and -0.0 (both mask)"""
    dev = _dev()
    L = pkg("_lib")
    c = E.dgrad_data(row)
    E.dgrad_conditions(c, dt)
    B, Cin, Cout, H, k, s, p = row["cfg"]
    Ho = (H + 2 * p - k) // s + 1
    dyd = nhwc(c["dy"]).to(dev, dt)
    wt = c["w"].permute(1, 2, 3, 0).contiguous().to(dev, dt)       # [Cin][kh][kw][Cout]
    od = nhwc(c["other"]).to(dev, dt).view(-1, Cin)
    ad = nhwc(c["act"]).to(dev, dt).view(-1, Cin)
    assert bool((torch.signbit(ad) & (ad == 0)).any())             # the -0.0 reached the device
    d = _desc(L, dt, L.QT_CONV_DGRAD, B, (Ho, Ho), (H, H), Cout, Cin, k, s, p)
    _check_path(L, row, d, B, H, B * H * H)
    bits = pack_bits(nhwc(c["act"] > 0).view(-1, Cin)).to(dev)     # the packed form of the same mask: one bit per element
    for ctx in _walks(L, row):
        with ctx:
            y0, _ = run_conv(L, dt, dyd, wt, B, (Ho, Ho), (H, H), Cout, Cin, k, k, s, p, L.QT_CONV_DGRAD)
            y1, _ = run_conv(L, dt, dyd, wt, B, (Ho, Ho), (H, H), Cout, Cin, k, k, s, p, L.QT_CONV_DGRAD, residual=od,
                             relu_mask=ad)
            gd = Guard(dev)
            g_dy, g_w, g_res, g_bits = gd.input("dy", dyd), gd.input("w", wt), gd.input("residual", od), gd.input("mask_bits", bits)
            y2 = gd.output("y", (B * H * H, Cin), dt)
            io = L.ConvIO(L.ptr(g_dy), L.ptr(g_w), L.ptr(y2), None, None, L.ptr(g_res), None, None)
            io.relu_mask_bits = g_bits.data_ptr()
            L.check(L.lib().qt_conv2d_igemm(ctypes.byref(d), ctypes.byref(io), L.stream_ptr()), "qt_conv2d_igemm (mask bits)")
            gd.check()
        _same(_nchw(y0, B, H, H, Cin), c["dx"], dt, "plain", row)
        _same(_nchw(y1, B, H, H, Cin), c["out"], dt, "residual + mask", row)
        _same(_nchw(y2, B, H, H, Cin), c["out"], dt, "residual + packed mask bits", row)
    if row["path"] == "ring":
        _ring_links(L, dev, row, dt, c, d, dyd, wt, od, ad)


def _ring_links(L, dev, row, dt, c, d, dyd, wt, od, ad):
    """the BatchNorm-backward link sums of the ring kernel (sum g, sum g * xhat of the value it writes): ONE partial row per
    workgroup, accumulated in registers over every tile of its share.  One link on the plain gradient, two links behind
    residual + ReLU mask; dyadic xhat, so that every sum is exact"""
    B, Cin, _, H = row["cfg"][:4]
    rows = L.lib().qt_conv2d_stats_rows(ctypes.byref(d))
    links = [_dyadic_links(c, Cin, row["seed"] + 9000 + j) for j in range(2)]
    gd = Guard(dev)
    g_dy, g_w, g_res, g_msk = gd.input("dy", dyd), gd.input("w", wt), gd.input("residual", od), gd.input("relu_mask", ad)
    dev_links = [(gd.input(f"bn{j}_y", nhwc(ybn).to(dt).view(-1, Cin)), gd.input(f"bn{j}_mean", mean.float()),
                  gd.input(f"bn{j}_invstd", invstd.float())) for j, (ybn, mean, invstd, _) in enumerate(links)]
    for with_ops in (False, True):
        n = 2 if with_ops else 1
        parts = [gd.output(f"bn{j}_partial{n}", (rows, 2, Cin), torch.float32) for j in range(n)]
        out = gd.output(f"dx{n}", (B * H * H, Cin), dt)
        io = L.ConvIO(L.ptr(g_dy), L.ptr(g_w), L.ptr(out), None, None, L.ptr(g_res) if with_ops else None,
                      L.ptr(g_msk) if with_ops else None, None)
        io.bn0_y, io.bn0_mean, io.bn0_invstd = (t.data_ptr() for t in dev_links[0])
        io.bn0_partial = parts[0].data_ptr()
        if n == 2:
            io.bn1_y, io.bn1_mean, io.bn1_invstd = (t.data_ptr() for t in dev_links[1])
            io.bn1_partial = parts[1].data_ptr()
        L.check(L.lib().qt_conv2d_igemm(ctypes.byref(d), ctypes.byref(io), L.stream_ptr()), "qt_conv2d_igemm (links)")
        gd.check()
        ref = c["out"] if with_ops else c["dx"]
        _same(_nchw(out, B, H, H, Cin), ref, dt, ("links", n), row)
        for j in range(n):
            assert _links_equal(parts[j], ref, links[j][3]), ("BatchNorm-backward link sums", n, j)


S2D, S2D_IDS = E.expand(E.S2D_ROWS)


def _dyadic_links(c, Cin, seed):
    """ybn in {-1, 0, 1}, integer mean, invstd in {1, 2, 0.5}: xhat and every g * xhat are exact"""
    g = E.gen(seed)
    ybn = E.ints(c["out"].shape, 1, g)
    mean = E.ints((Cin,), 1, g)
    invstd = torch.tensor([1.0, 2.0, 0.5], dtype=torch.float64)[torch.randint(0, 3, (Cin,), generator=g)]
    xhat = (ybn - E.bcast(mean, ybn)) * E.bcast(invstd, ybn)
    return ybn, mean, invstd, xhat


def _links_equal(part, out, xhat):
    assert float((out.abs() * xhat.abs()).sum((0, 2, 3)).max()) <= E.CAP and float(out.abs().sum((0, 2, 3)).max()) <= E.CAP
    want = torch.stack([out.sum((0, 2, 3)), (out * xhat).sum((0, 2, 3))])
    return torch.equal(part.double().sum(0).cpu(), want)


@pytest.mark.parametrize("row,dt", S2D, ids=S2D_IDS)
def test_stride2_data_gradient_is_bit_exact(row, dt):
    dev = _dev()
    L = pkg("_lib")
    lib = L.lib()
    c = E.s2d_data(row)
    E.dgrad_conditions(c, dt)
    B, Cin, Cout, H, k, _, p = row["cfg"]
    Ho = (H + 2 * p - k) // 2 + 1
    qdt = L.qt_dtype(dt)
    gd = Guard(dev)
    dyd = gd.input("dy", nhwc(c["dy"]).to(dt))
    res = gd.input("residual", nhwc(c["other"]).to(dt).view(-1, Cin))
    msk = gd.input("relu_mask", nhwc(c["act"]).to(dt).view(-1, Cin))
    wsrc = gd.input("w", c["w"].float().contiguous())
    if row["form"] == "classes":
        offs, khs, kws = (ctypes.c_longlong * 4)(), (ctypes.c_int * 4)(), (ctypes.c_int * 4)()
        wd = gd.output("w_classes", (Cout * Cin * k * k,), dt)       # the four classes back to back: every element written
        L.check(lib.qt_pack_dgrad_s2(qdt, L.ptr(wsrc), L.ptr(wd), Cout, Cin, k, offs, khs, kws, L.stream_ptr()), "qt_pack_dgrad_s2")
        gd.check()
        # k = 3: the four classes tile the image, every pixel is written.  k = 1: only class (0,0) is, the rest keeps the zeros
        out = gd.output("dx", (B * H * H, Cin), dt) if k == 3 else gd.output("dx", (B * H * H, Cin), dt, fill=0)
        esz = 2 if dt == BF else 4
        for cls in range(4):
            if khs[cls] * kws[cls] == 0:
                continue
            d = _desc(L, dt, L.QT_CONV_FWD, B, (Ho, Ho), (H // 2, H // 2), Cout, Cin, 1, 1, 0)
            d.kh, d.kw = khs[cls], kws[cls]
            d.dst_sub, d.dst_h, d.dst_w, d.dst_off_h, d.dst_off_w = 2, H, H, cls >> 1, cls & 1
            io = L.ConvIO(L.ptr(dyd), ctypes.c_void_p(wd.data_ptr() + offs[cls] * esz), L.ptr(out), None, None,
                          L.ptr(res), L.ptr(msk), None)
            L.check(lib.qt_conv2d_igemm(ctypes.byref(d), ctypes.byref(io), L.stream_ptr()), "qt_conv2d_igemm")
        gd.check()
        got, ref = _nchw(out, B, H, H, Cin), c["out"]
        if k == 1:   # pixels no tap reaches were never written: only class (0,0) is defined
            got, ref = got[:, :, ::2, ::2], ref[:, :, ::2, ::2]
        return _same(got, ref, dt, "parity classes")
    extra = row["form"] == "merged5"
    if extra:
        op = gd.output("w_merged5", (20 * Cout * Cin,), dt, fill=0)   # [4 Cin][5 slots][Cout]; unused slots stay zero
        wdsrc = gd.input("w_down", c["wd"].float().contiguous())
        items = (PackItem * 2)(PackItem(wsrc.data_ptr(), None, op.data_ptr(), Cout, Cin, 3, 3),
                               PackItem(wdsrc.data_ptr(), None, op.data_ptr(), Cout, Cin, 1, 4))
        L.check(lib.qt_pack_weights_batched(qdt, ctypes.cast(items, ctypes.c_void_p), 2, L.stream_ptr()), "qt_pack_weights_batched")
        maps = gd.input("dy_maps", torch.stack([nhwc(c["dy"]).to(dt), nhwc(c["dyd"]).to(dt)]))   # both maps in one allocation
        src = maps[0]
    else:
        op = gd.output("w_merged", (16 * Cout * Cin,), dt)            # NaN: the packer zeroes the unused slots
        L.check(lib.qt_pack_dgrad_s2_merged(qdt, L.ptr(wsrc), L.ptr(op), Cout, Cin, L.stream_ptr()), "qt_pack_dgrad_s2_merged")
        src = dyd
    gd.check()
    d = _desc(L, dt, L.QT_CONV_FWD, B, (Ho, Ho), (Ho, Ho), Cout, 4 * Cin, 2, 1, 0)
    d.dst_sub, d.dst_h, d.dst_w, d.dst_off_h, d.dst_off_w, d.dst_merge = 2, H, H, 0, 0, Cin
    d.dst_merge_extra = 1 if extra else 0
    rows, rows_off = _path_rows(L, d)
    assert rows > 0 and rows % 4 == 0
    if row["path"] == "pt":
        assert rows == 2 * 4 * ((B + 3) // 4) and rows != rows_off
    else:
        assert rows == rows_off
    ybn, mean, invstd, xhat = _dyadic_links(c, Cin, row["seed"] + 9000)
    yb = gd.input("bn_y", nhwc(ybn).to(dt).view(-1, Cin))
    md, isd = gd.input("bn_mean", mean.float()), gd.input("bn_invstd", invstd.float())
    for with_ops in (False, True):
        part = gd.output(f"bn_partial{int(with_ops)}", (rows, 2, Cin), torch.float32)
        out = gd.output(f"dx{int(with_ops)}", (B * H * H, Cin), dt)   # every pixel belongs to one class
        io = L.ConvIO(src.data_ptr(), L.ptr(op), L.ptr(out), None, None, L.ptr(res) if with_ops else None,
                      L.ptr(msk) if with_ops else None, None, L.ptr(yb), L.ptr(md), L.ptr(isd), L.ptr(part), None, None, None, None)
        if extra:
            io.extra_src = maps[1].data_ptr()
        L.check(lib.qt_conv2d_igemm(ctypes.byref(d), ctypes.byref(io), L.stream_ptr()), "qt_conv2d_igemm")
        gd.check()
        ref = c["out"] if with_ops else c["dx"]
        _same(_nchw(out, B, H, H, Cin), ref, dt, ("merged", with_ops))
        assert _links_equal(part, ref, xhat), ("BatchNorm-backward link sums", with_ops)


# ----------------------------------------------------------------------------------------------------------------------
# weight gradients (f32 outputs)
# ----------------------------------------------------------------------------------------------------------------------
WG, WG_IDS = E.expand(E.WGRAD_ROWS)


def _oihw(dw, Cout, k, Cin):
    return dw.cpu().view(Cout, k, k, Cin).permute(0, 3, 1, 2)


@pytest.mark.parametrize("row,dt", WG, ids=WG_IDS)
def test_weight_gradient_is_bit_exact(row, dt):
    dev = _dev()
    L = pkg("_lib")
    lib = L.lib()
    c = E.wgrad_data(row)
    E.wgrad_conditions(c)
    B, Cin, Cout, H, k, s, p = row["cfg"]
    W = row.get("W", H)
    S = row.get("quad", 0)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    path = row["path"]
    xd = nhwc(c["base"] if S else c["x"]).to(dev, dt)
    dyd = nhwc(c["dy"]).to(dev, dt)
    strides = (S * H * S * W * Cin, S * W * Cin, Cin) if S else None
    quad = {0: 0, 2: 1 if path == "generic" else 2, 4: 4}[S]
    d = _desc(L, dt, L.QT_CONV_FWD, B, (H, W), (Ho, Wo), Cin, Cout, k, s, p, quad)
    if strides:
        d.src_img_stride, d.src_row_stride, d.src_pix_stride = strides
    args = (B, (H, W), (Ho, Wo), Cin, Cout, k, k, s, p)

    def streaming_entry_points(what):
        """_oihw into NaN-filled scratch, and _oihw_on twice back to back on alternating workspaces (sum on a side stream)"""
        nbytes = lib.qt_conv2d_wgrad_workspace_bytes(ctypes.byref(d))
        assert nbytes > 0, "the streaming kernel was expected to take this shape"
        gd = Guard(dev)
        g_dy, g_x = gd.input("dy", dyd), gd.input("x", xd)
        ws = [gd.workspace(f"ws{j}", nbytes) for j in range(2)]       # exactly the queried size
        gr = [gd.output(f"grad{j}", (Cout, Cin, k, k), torch.float32) for j in range(3)]
        L.check(lib.qt_conv2d_wgrad_oihw(ctypes.byref(d), L.ptr(g_dy), L.ptr(g_x), L.ptr(gr[0]), L.ptr(ws[0]),
                                         nbytes, L.stream_ptr()), "qt_conv2d_wgrad_oihw")
        torch.cuda.synchronize()
        _same(gr[0], c["dw"], F32, (what, "oihw"))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        for j in (0, 1):
            ws[j].fill_(0xFF)
        torch.cuda.synchronize()
        for j in (0, 1):
            L.check(lib.qt_conv2d_wgrad_oihw_on(ctypes.byref(d), L.ptr(g_dy), L.ptr(g_x), L.ptr(gr[1 + j]), L.ptr(ws[j]),
                                                nbytes, L.stream_ptr(), ctypes.c_void_p(side.cuda_stream)),
                    "qt_conv2d_wgrad_oihw_on")
        gd.check()
        _same(gr[1], c["dw"], F32, (what, "oihw_on, first"))
        _same(gr[2], c["dw"], F32, (what, "oihw_on, second"))

    try:
        if path == "generic":
            lib.qt_set_wgrad_patch_min_width(0)
            lib.qt_set_wgrad_s2(0)
            assert lib.qt_conv2d_wgrad_workspace_bytes(ctypes.byref(d)) == 0       # no streaming kernel behind this descriptor
            dw = run_wgrad(L, dt, dyd, xd, *args, quad=quad, strides=strides)
            _same(_oihw(dw, Cout, k, Cin), c["dw"], F32, "generic")
        elif path == "stream":
            for v in row["variants"]:
                lib.qt_set_wgrad_patch_variant(v)
                lib.qt_set_wgrad_patch_min_width(7)
                if row.get("prove_tile"):
                    # at variant 3 the launcher falls back to the ring kernel only where the tile geometry of the padded grid
                    # (H + 1) x (W + 1) does not fit.  The region form has no fallback and is eligible only where that same
                    # geometry fits: 2 x 2 regions of (H - 1) / 2 pixels share this row's padded grid
                    R = (H - 1) // 2
                    assert H == W and 2 * (R + 1) == H + 1 and R >= 7
                    dr = _desc(L, dt, L.QT_CONV_FWD, B, (R, R), (R, R), Cin, Cout, 3, 1, 1, 2)
                    dr.src_img_stride, dr.src_row_stride = 4 * R * R * Cin, 2 * R * Cin
                    assert lib.qt_conv2d_wgrad_workspace_bytes(ctypes.byref(dr)) > 0, "the tile-resident kernel does not fit"
                dw = run_wgrad(L, dt, dyd, xd, *args)
                _same(_oihw(dw, Cout, k, Cin), c["dw"], F32, (v, "atomic"))
                dw = run_wgrad(L, dt, dyd, xd, *args, workspace=True)
                _same(_oihw(dw, Cout, k, Cin), c["dw"], F32, (v, "workspace"))
                streaming_entry_points(v)
        elif path == "s2":
            streaming_entry_points("parity planes")
        else:
            assert path == "region"
            streaming_entry_points("regions")
    finally:
        lib.qt_set_wgrad_patch_min_width(-1)
        lib.qt_set_wgrad_patch_variant(-1)
        lib.qt_set_wgrad_s2(-1)


LW, LW_IDS = E.expand(E.LWGRAD_ROWS)


@pytest.mark.parametrize("row,dt", LW, ids=LW_IDS)
def test_linear_weight_gradient_is_bit_exact(row, dt):
    dev = _dev()
    L = pkg("_lib")
    c = E.lwgrad_data(row)
    E.lwgrad_conditions(c)
    rows, out, inn = row["cfg"]
    gd = Guard(dev)
    dw = gd.output("dw", (out, inn), torch.float32)
    dyd, xd = gd.input("dy", c["dy"].to(dt)), gd.input("x", c["x"].to(dt))
    for _ in range(2):   # (a second call over the first result: nothing is accumulated)
        L.check(L.lib().qt_linear_wgrad(L.qt_dtype(dt), L.ptr(dyd), L.ptr(xd), L.ptr(dw), rows, out, inn, L.stream_ptr()),
                "qt_linear_wgrad")
    gd.check()
    _same(dw, c["dw"], F32, "qt_linear_wgrad")


@pytest.mark.parametrize("row", E.LINEAR_ROWS, ids=E.ids(E.LINEAR_ROWS))
def test_linear_splitk_is_bit_exact(row):
    dev = _dev()
    L = pkg("_lib")
    lib = L.lib()
    c = E.gemm_data(row)
    E.gemm_conditions(c, BF)
    M, N, K = row["cfg"]
    nbytes = lib.qt_linear_workspace_bytes(M, N, K)
    gd = Guard(dev)
    ws = gd.workspace("ws", nbytes)
    y = gd.output("y", (M, N), BF)
    xd, wd = gd.input("x", c["x"].to(BF)), gd.input("w", c["w"].to(BF))
    bd = gd.input("bias", c["bias"].float() if c["bias"] is not None else None)
    L.check(lib.qt_linear_bf16(L.ptr(xd), L.ptr(wd), L.ptr(bd), row["relu"], L.ptr(y), M, N, K, L.ptr(ws), nbytes,
                               L.stream_ptr()), "qt_linear_bf16")
    gd.check()
    _same(y, c["out"], BF, "qt_linear_bf16")


# ----------------------------------------------------------------------------------------------------------------------
# stem gradients
# ----------------------------------------------------------------------------------------------------------------------
SD, SD_IDS = E.expand(E.STEMD_ROWS)


@pytest.mark.parametrize("row,dt", SD, ids=SD_IDS)
def test_stem_data_gradient_is_bit_exact(row, dt):
    """qt_stem_dgrad: the f32 image gradient from conv1's gradient map [B][112][112][64] and the f32 OIHW filter"""
    dev = _dev()
    L = pkg("_lib")
    c = E.dgrad_data(row)
    E.dgrad_conditions(c, F32)
    B = row["cfg"][0]
    if row.get("walk"):
        # stem_dgrad.hip: tiles of 16 block rows (bf16) / 8 block rows (f32) x 16 blocks of the 112 x 112 map = 49 / 98 per
        # image, on a persistent grid of at most 256 workgroups whatever the device
        ntiles = B * (49 if dt == BF else 98)
        assert ntiles >= row["walk"] * 256 + 1, ("not every workgroup takes", row["walk"], "tiles:", ntiles, "tiles")
    gd = Guard(dev)
    dyd = gd.input("dy", nhwc(c["dy"]).to(dt))
    wd = gd.input("w", c["w"].float().contiguous())
    dx = gd.output("dx", (B, 3, 224, 224), torch.float32)
    L.check(L.lib().qt_stem_dgrad(L.qt_dtype(dt), L.ptr(dyd), L.ptr(wd), L.ptr(dx), B, L.stream_ptr()), "qt_stem_dgrad")
    gd.check()
    _same(dx, c["dx"], F32, "qt_stem_dgrad")


SW, SW_IDS = E.expand(E.STEMW_ROWS)


@pytest.mark.parametrize("row,dt", SW, ids=SW_IDS)
def test_stem_weight_gradient_is_bit_exact(row, dt):
    """qt_conv2d_wgrad on the packed stem descriptor (bf16: the raw-row kernel; f32: the generic 64 x 224 tile), unpacked to OIHW"""
    dev = _dev()
    L = pkg("_lib")
    lib = L.lib()
    c = E.wgrad_data(row)
    E.wgrad_conditions(c)
    B = row["cfg"][0]
    if row.get("walk"):
        # stem_wgrad_rows_kernel<false> (bf16) has no query: min(56 B, 256) workgroups on contiguous shares of the B * 56
        # two-row tiles, the split tests/_stem_bounds.py restates; a partial filter per workgroup, summed over its share
        shares = tile_ranges(B)
        per, cap, want = E.WALKS[row["name"]]
        assert len(shares) == min(per * B, cap) and min(e - b for b, e in shares) >= row["walk"], (B, len(shares))
        assert any(e - b >= 3 for b, e in shares) and per * B >= row["walk"] * len(shares) + 1
        assert bool((c["dy"].view(B, 64, 56, 2, 112) != 0).any(4).any(3).any(1).all()), "a two-row tile without a gradient"
    qdt, st = L.qt_dtype(dt), L.stream_ptr()
    gd = Guard(dev)
    imd = gd.input("image", c["x"].float())
    xpad = gd.output("xpad", (B, 230, 232, 4), dt)
    L.check(lib.qt_pack_stem_input(qdt, L.ptr(imd), L.ptr(xpad), B, st), "qt_pack_stem_input")
    gd.check()
    dyd = gd.input("dy", nhwc(c["dy"]).to(dt))
    d = _desc(L, dt, L.QT_CONV_FWD, B, (230, 232), (112, 112), 32, 64, 7, 2, 0)
    d.kw = 1
    d.src_pix_stride, d.src_row_stride, d.src_img_stride = 4, 232 * 4, 230 * 232 * 4
    dw = gd.output("dw", (64, 7, 32), torch.float32, fill=0)          # zeros: qt_conv2d_wgrad accumulates (dw += ...)
    L.check(lib.qt_conv2d_wgrad(ctypes.byref(d), L.ptr(dyd), L.ptr(xpad), L.ptr(dw), st), "qt_conv2d_wgrad")
    grad = gd.output("grad", (64, 3, 7, 7), torch.float32)
    L.check(lib.qt_unpack_stem_wgrad(L.ptr(dw), L.ptr(grad), 0, st), "qt_unpack_stem_wgrad")
    gd.check()
    _same(grad, c["dw"], F32, "packed stem weight gradient")


# ----------------------------------------------------------------------------------------------------------------------
# 3-D convolutions of the clip models (time-major maps [T][B][H][W][C])
# ----------------------------------------------------------------------------------------------------------------------
def _tb(t):
    """[B][C][T][H][W] -> [T][B][H][W][C]"""
    return t.permute(2, 0, 3, 4, 1).contiguous()


def _ncthw(y, C):
    """[T][B][H][W][>= C] on the device -> [B][C][T][H][W] on the host"""
    return y.cpu()[..., :C].permute(1, 4, 0, 2, 3)


def _walk_precondition(row, items, rows):
    """a `walk` row is there for the second and later items of a workgroup: with `rows` workgroups (the grid the library
    reports) every one of them must take at least row["walk"] items.  A failure, not a skip: on a device where this does not
    hold the row tests nothing it was added for"""
    assert rows > 0 and items >= row["walk"] * rows + 1, (row["name"], "items", items, "workgroups", rows, "walk", row["walk"])


C3F, C3F_IDS = E.expand(E.C3F_ROWS)


@pytest.mark.parametrize("row,dt", C3F, ids=C3F_IDS)
def test_first_conv3d_is_bit_exact(row, dt):
    """qt_conv3d_first_fwd (raw + statistics, plain, scale / shift / ReLU), qt_conv3d_first_fwd_pool (64- and 32-channel rows),
    qt_conv3d_first_dgrad (f32 clip gradient; MFMA form and the direct kernel), qt_conv3d_first_wgrad and
    qt_conv3d_first_wgrad_fused (32- and 64-channel pooled rows)"""
    dev = _dev()
    L = pkg("_lib")
    lib = L.lib()
    c = E.c3_data(row, 3, 32)
    B, T, H, W = row["cfg"]
    qdt, st = L.qt_dtype(dt), L.stream_ptr()
    if row.get("walk"):
        # (clip, 4-row slab) items on the grid the library reports (one statistics row per workgroup).  qt_conv3d_first_dgrad
        # has no query of its own: it launches by the same rule (at most 2 x CUs workgroups) over the same items at one column
        # tile per row (W <= 112), so the forward's row count is its grid too
        assert W <= 112
        _walk_precondition(row, B * (H // 4), lib.qt_conv3d_first_stats_rows(B, T, H, W))
    if "fwd" in row["only"]:
        E.c3_conditions(c, dt, "fwd")
        gd = Guard(dev)
        cd = gd.input("clip", c["x"].permute(0, 2, 1, 3, 4).contiguous().float())  # the f32 clip [B][T][3][H][W]
        wp = torch.zeros(64, 128)                                                  # element ((kt*3 + kh)*3 + kw)*3 + c
        wp[:32, :81] = c["w"].permute(0, 2, 3, 4, 1).reshape(32, 81).float()
        wp = gd.input("w", wp.to(dt))
        sc, sh = gd.input("scale", c["scale"].float()), gd.input("shift", c["shift"].float())
        rows = lib.qt_conv3d_first_stats_rows(B, T, H, W)
        assert rows > 0, "conv3d_first.hip was expected to take this shape"
        y, y2, y3 = (gd.output(n, (T, B, H, W, 32), dt) for n in ("y_stats", "y_plain", "y_affine"))
        part = gd.output("stats", (rows, 2, 64), torch.float32)
        L.check(lib.qt_conv3d_first_fwd(qdt, L.ptr(cd), L.ptr(wp), L.ptr(y), None, None, 0, L.ptr(part), B, T, H, W, st), "stats")
        L.check(lib.qt_conv3d_first_fwd(qdt, L.ptr(cd), L.ptr(wp), L.ptr(y2), None, None, 0, None, B, T, H, W, st), "plain")
        L.check(lib.qt_conv3d_first_fwd(qdt, L.ptr(cd), L.ptr(wp), L.ptr(y3), L.ptr(sc), L.ptr(sh), 1, None, B, T, H, W, st), "affine")
        gd.check()
        _same(_ncthw(y, 32), c["raw"], dt, "raw + statistics")
        _same(_ncthw(y2, 32), c["raw"], dt, "raw")
        _same(_ncthw(y3, 32), c["act"], dt, "scale / shift / ReLU")
        if row["mode"] == "A":
            assert E.stats_equal(part[:, :, :32], c["raw"]) and bool((part[:, :, 32:] == 0).all())
        for pc in (64, 32):
            pooled = gd.output(f"pooled{pc}", (T, B, H // 2, W // 2, pc), dt)
            L.check(lib.qt_conv3d_first_fwd_pool(qdt, L.ptr(cd), L.ptr(wp), L.ptr(pooled), pc, L.ptr(sc), L.ptr(sh), B, T, H, W, st),
                    "qt_conv3d_first_fwd_pool")
            gd.check()
            _same(_ncthw(pooled, 32), c["pooled"], dt, ("conv + scale / shift / ReLU + max pool", pc))
            assert bool((pooled[..., 32:] == 0).all())
    if "dgrad" in row["only"]:
        E.c3_conditions(c, F32, "dgrad")
        gd = Guard(dev)
        dyd = gd.input("dy", _tb(c["dyf"]).to(dt))
        wd = gd.input("w", c["wg"].float().contiguous())                           # nn.Conv3d's [32][3][3][3][3], f32
        dx = gd.output("dx", (B, T, 3, H, W), torch.float32)
        L.check(lib.qt_conv3d_first_dgrad(qdt, L.ptr(dyd), L.ptr(wd), L.ptr(dx), B, T, H, W, st), "qt_conv3d_first_dgrad")
        gd.check()
        _same(dx.cpu().permute(0, 2, 1, 3, 4), c["dx"], F32, "qt_conv3d_first_dgrad")
    if "wgrad" in row["only"]:
        E.c3_conditions(c, F32, "wgrad")
        nws = lib.qt_conv3d_first_wgrad_workspace_bytes(B, T, H, W)
        assert nws > 0
        gd = Guard(dev)
        cd1 = gd.input("clip", c["x1"].permute(0, 2, 1, 3, 4).contiguous().float())
        dyd = gd.input("dy", _tb(c["dy"]).to(dt))
        ws = gd.workspace("ws", nws)
        dw = gd.output("dw", (32, 3, 3, 3, 3), torch.float32)
        L.check(lib.qt_conv3d_first_wgrad(qdt, L.ptr(cd1), L.ptr(dyd), L.ptr(dw), L.ptr(ws), nws, B, T, H, W, st),
                "qt_conv3d_first_wgrad")
        gd.check()
        _same(dw, c["dw"], F32, "qt_conv3d_first_wgrad")
    if "fused" in row["only"]:
        for cp in (32, 64):
            f = E.c3_fused_data(c, cp)
            E.c3_fused_conditions(f)
            gd = Guard(dev)
            cd1 = gd.input("clip", c["x1"].permute(0, 2, 1, 3, 4).contiguous().float())
            ws = gd.workspace("ws", nws)                                           # a fresh NaN workspace per pooled width
            yd = gd.input("y", _tb(f["y"]).to(dt))
            dout = gd.input("dout", _tb(f["dout"]).to(dt))
            arg = gd.input("argmax", _tb(f["arg"]))
            sc, sh = gd.input("scale", f["scale"].float()), gd.input("shift", f["shift"].float())
            mean, invstd = gd.input("mean", f["mean"].float()), gd.input("invstd", f["invstd"].float())
            coef = gd.input("coef", f["coef"].float().contiguous())
            dwf = gd.output("dw_fused", (32, 3, 3, 3, 3), torch.float32)
            L.check(lib.qt_conv3d_first_wgrad_fused(qdt, L.ptr(cd1), L.ptr(yd), L.ptr(dout), L.ptr(arg), cp, L.ptr(mean),
                                                    L.ptr(invstd), L.ptr(sc), L.ptr(sh), L.ptr(coef), L.ptr(dwf), L.ptr(ws),
                                                    nws, B, T, H, W, st), "qt_conv3d_first_wgrad_fused")
            # the unfused kernel on the reference's dy: the same contraction
            dyd = gd.input("dy", _tb(f["dy"]).to(dt))
            dwu = gd.output("dw_unfused", (32, 3, 3, 3, 3), torch.float32)
            L.check(lib.qt_conv3d_first_wgrad(qdt, L.ptr(cd1), L.ptr(dyd), L.ptr(dwu), L.ptr(ws), nws, B, T, H, W, st),
                    "qt_conv3d_first_wgrad")
            gd.check()
            _same(dwu, f["dw"], F32, ("qt_conv3d_first_wgrad on the formed dy", cp))
            _same(dwf, f["dw"], F32, ("qt_conv3d_first_wgrad_fused", cp))


C32, C32_IDS = E.expand(E.C32_ROWS)


@pytest.mark.parametrize("row,dt", C32, ids=C32_IDS)
def test_second_conv3d_is_bit_exact(row, dt):
    """qt_conv3d_c32_fwd (raw + statistics, plain, scale / shift / ReLU), qt_conv3d_c32_dgrad (64- and 32-channel rows) and
    qt_conv3d_c32_wgrad; the padding channels of 64-channel input rows and of the packed filters hold a non-zero value that
    must never be read"""
    dev = _dev()
    L = pkg("_lib")
    lib = L.lib()
    c = E.c3_data(row, 32, 64)
    B, T, H, W = row["cfg"]
    xc = row["xc"]
    qdt, st = L.qt_dtype(dt), L.stream_ptr()

    def rows_of(x):
        xd = torch.full((T, B, H, W, xc), 3.0, dtype=dt)
        xd[..., :32] = _tb(x).to(dt)
        return xd
    assert lib.qt_conv3d_c32_stats_rows(B, T, H, W) > 0, "conv3d_slab.hip was expected to take this shape"
    if row.get("walk"):   # (clip, 2-row slab) items; forward, data gradient and weight gradient launch the same grid
        _walk_precondition(row, B * (H // 2), lib.qt_conv3d_c32_stats_rows(B, T, H, W))
    if "fwd" in row["only"]:
        E.c3_conditions(c, dt, "fwd")
        gd = Guard(dev)
        xd = gd.input("x", rows_of(c["x"]))
        wp = torch.full((64, 27, 64), 3.0, dtype=dt)                               # [O][tap][I padded]
        wp[:, :, :32] = c["w"].permute(0, 2, 3, 4, 1).reshape(64, 27, 32).to(dt)
        wp = gd.input("w", wp)
        sc, sh = gd.input("scale", c["scale"].float()), gd.input("shift", c["shift"].float())
        rows = lib.qt_conv3d_c32_stats_rows(B, T, H, W)
        y, y2, y3 = (gd.output(n, (T, B, H, W, 64), dt) for n in ("y_stats", "y_plain", "y_affine"))
        part = gd.output("stats", (rows, 2, 64), torch.float32)
        L.check(lib.qt_conv3d_c32_fwd(qdt, L.ptr(xd), xc, L.ptr(wp), L.ptr(y), None, None, 0, L.ptr(part), B, T, H, W, st), "stats")
        L.check(lib.qt_conv3d_c32_fwd(qdt, L.ptr(xd), xc, L.ptr(wp), L.ptr(y2), None, None, 0, None, B, T, H, W, st), "plain")
        L.check(lib.qt_conv3d_c32_fwd(qdt, L.ptr(xd), xc, L.ptr(wp), L.ptr(y3), L.ptr(sc), L.ptr(sh), 1, None, B, T, H, W, st), "affine")
        gd.check()
        _same(_ncthw(y, 64), c["raw"], dt, "raw + statistics")
        _same(_ncthw(y2, 64), c["raw"], dt, "raw")
        _same(_ncthw(y3, 64), c["act"], dt, "scale / shift / ReLU")
        if row["mode"] == "A":
            assert E.stats_equal(part, c["raw"])
    if "dgrad" in row["only"]:
        E.c3_conditions(c, dt, "dgrad")
        gd = Guard(dev)
        dyd = gd.input("dy", _tb(c["dyf"]).to(dt))
        wdp = torch.full((64, 27, 64), 3.0, dtype=dt)                              # [I padded][tap][O]
        wdp[:32] = c["wg"].permute(1, 2, 3, 4, 0).reshape(32, 27, 64).to(dt)
        wdp = gd.input("w", wdp)
        nscr = lib.qt_conv3d_c32_dgrad_scratch_bytes(B, T, H, W)
        for dxc in (64, 32):
            scr = gd.workspace(f"scratch{dxc}", nscr)                              # exactly the queried size, NaN
            dx = gd.output(f"dx{dxc}", (T, B, H, W, dxc), dt)
            L.check(lib.qt_conv3d_c32_dgrad(qdt, L.ptr(dyd), L.ptr(wdp), L.ptr(dx), dxc, L.ptr(scr), nscr, B, T, H, W, st),
                    "qt_conv3d_c32_dgrad")
            gd.check()
            _same(_ncthw(dx, 32), c["dx"], dt, ("qt_conv3d_c32_dgrad", dxc))
            assert bool((dx[..., 32:] == 0).all())
    if "wgrad" in row["only"]:
        E.c3_conditions(c, F32, "wgrad")
        gd = Guard(dev)
        xd1 = gd.input("x", rows_of(c["x1"]))
        dyd = gd.input("dy", _tb(c["dy"]).to(dt))
        nws = lib.qt_conv3d_c32_wgrad_workspace_bytes(B, T, H, W)
        assert nws > 0
        ws = gd.workspace("ws", nws)
        dwt = gd.output("dw", (64, 32, 3, 3, 3), torch.float32)
        L.check(lib.qt_conv3d_c32_wgrad(qdt, L.ptr(xd1), xc, L.ptr(dyd), L.ptr(dwt), L.ptr(ws), nws, B, T, H, W, st),
                "qt_conv3d_c32_wgrad")
        gd.check()
        _same(dwt, c["dw"], F32, "qt_conv3d_c32_wgrad")
