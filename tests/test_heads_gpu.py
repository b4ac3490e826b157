"""The kernels that finish the three non-ResNet heads, through the C ABI, against float64 restatements of the same operation on
exactly the values the kernel reads, inside error bounds DERIVED from the kernel's own f32 arithmetic (tests/_head_bounds.py;
tests/test_head_bounds_cpu.py shows that correct f32 arithmetic meets them and that six wrong versions miss them):
  * csrc/lstm.hip: every instantiation (H = 64, 188 with its partial last wave, 256), T = 1 / 2 / 16, one sequence and several,
    b_hh given and NULL, dhout / dlast given and NULL, gates that saturate to exactly 0 and 1 (__expf overflows), the refusal of
    another H, the guards of the transpose;
  * csrc/attention.hip: the region pool with dead lanes in its last workgroup, HW < 4 (partial-sum lanes that own no position),
    the second trip of its backward's grid-stride loop; the gate with a flat, a peaked (underflowing) and an exactly uniform
    softmax and with vectors of both signs;
  * csrc/video3d.hip: the clip pool's unrolled loop, its tail, idle threads and a partly idle second channel slice; the
    BatchNorm3d partial sums row by row, capped row counts, empty slabs, refused channel counts.
Every case prints max(|err| / bound) and asserts <= 1; outputs are pre-filled with NaN where a region must stay untouched.

Reference behaviour: nn.LSTM, the attention head of AttentionHierarchicalCNN (Quadtree_from scratch/models.py:34-38, 62-89),
nn.AdaptiveAvgPool2d / nn.AdaptiveAvgPool3d and nn.BatchNorm3d's batch statistics."""

import pytest
import torch

import _head_bounds as Hb
from _util import pkg

pytestmark = pytest.mark.gpu

NAN = float("nan")
QT_ERR_INVALID_ARG, QT_ERR_UNSUPPORTED = -1, -3
F32, BF16 = torch.float32, torch.bfloat16
DTS = [F32, BF16]


def _env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    L = pkg("_lib")
    return torch.device("cuda:0"), L, L.lib()


def _nan(shape, dt, dev):
    return torch.full(shape, NAN, dtype=dt, device=dev)


def _all_nan(t):
    return bool(torch.isnan(t.float()).all())


def _report(name, got, ref, bound):
    r = Hb.ratio(got, ref, bound)
    print(f"  err/bound {name}: {r:.3f}")
    assert r <= 1.0, (name, r)


# ----------------------------------------------------------------------------------------------------------------------
# LSTM
# ----------------------------------------------------------------------------------------------------------------------
def _lstm_forward(L, lib, dev, xproj, whh_t, bhh, H):
    B, T, _ = xproj.shape
    outs = [_nan((B, T, n), F32, dev) for n in (4 * H, H, H, H)]
    st = lib.qt_lstm_forward(L.ptr(xproj), L.ptr(whh_t), L.ptr(bhh), *(L.ptr(o) for o in outs), B, T, H, L.stream_ptr())
    torch.cuda.synchronize()
    return st, outs


@pytest.mark.parametrize("regime", Hb.LSTM_REGIMES)
@pytest.mark.parametrize("BT", Hb.LSTM_BT)
@pytest.mark.parametrize("H", Hb.LSTM_H)
def test_lstm_forward_vs_float64(H, BT, regime):
    dev, L, lib = _env()
    B, T = BT
    xproj, whh, bhh, _, _ = Hb.lstm_inputs(H, B, T, regime)
    xd, wt, bd = xproj.to(dev), whh.t().contiguous().to(dev), bhh.to(dev)
    for bias, bias_dev in ((bhh, bd), (None, None)):
        st, outs = _lstm_forward(L, lib, dev, xd, wt, bias_dev, H)
        L.check(st, "qt_lstm_forward")
        gates, cell, hprev, hout = (o.cpu() for o in outs)
        if regime == "saturated":
            assert bool((gates == 0).any()) and bool((gates == 1).any())
        assert Hb.lstm_chain_exact(hprev, hout)
        tag = f"lstm fwd H={H} B={B} T={T} {regime} {'bhh' if bias is not None else 'no bhh'}"
        for name, got, ref, bound in Hb.lstm_fwd_facts(xproj, whh, bias, gates, cell, hprev, hout):
            _report(f"{tag} {name}", got, ref, bound)


@pytest.mark.parametrize("regime", Hb.LSTM_REGIMES)
@pytest.mark.parametrize("BT", Hb.LSTM_BT)
@pytest.mark.parametrize("H", Hb.LSTM_H)
def test_lstm_backward_vs_float64(H, BT, regime):
    dev, L, lib = _env()
    B, T = BT
    xproj, whh, bhh, dhout, dlast = Hb.lstm_inputs(H, B, T, regime)
    gates, cell = Hb.lstm_forward_f64(xproj, whh, bhh)
    gd, cd, wd, dhd, dld = (t.to(dev) for t in (gates, cell, whh, dhout, dlast))
    for which in Hb.LSTM_GRADS:
        dh, dh_dev = (dhout, dhd) if which != "dlast" else (None, None)
        dl, dl_dev = (dlast, dld) if which != "dhout" else (None, None)
        dg = _nan((B, T, 4 * H), F32, dev)
        L.check(lib.qt_lstm_backward(L.ptr(dh_dev), L.ptr(dl_dev), L.ptr(gd), L.ptr(cd), L.ptr(wd), L.ptr(dg), B, T, H,
                                     L.stream_ptr()), "qt_lstm_backward")
        got = dg.cpu()
        tag = f"lstm bwd H={H} B={B} T={T} {regime} {which}"
        _report(f"{tag} whole chain", got, *Hb.lstm_bwd_ref(gates, cell, whh, dh, dl))
        _report(f"{tag} step by step", got, *Hb.lstm_bwd_ref(gates, cell, whh, dh, dl, got))


def test_lstm_refuses_other_hidden_size():
    dev, L, lib = _env()
    H, B, T = 128, 2, 3
    xproj, whh, bhh, dhout, dlast = (t.to(dev) for t in Hb.lstm_inputs(H, B, T, "normal"))
    st, outs = _lstm_forward(L, lib, dev, xproj, whh.t().contiguous(), bhh, H)
    assert st == QT_ERR_UNSUPPORTED and all(_all_nan(o) for o in outs)
    gates, cell = torch.rand(B, T, 4 * H, device=dev), torch.rand(B, T, H, device=dev)
    dg = _nan((B, T, 4 * H), F32, dev)
    st = lib.qt_lstm_backward(L.ptr(dhout), L.ptr(dlast), L.ptr(gates), L.ptr(cell), L.ptr(whh), L.ptr(dg), B, T, H,
                              L.stream_ptr())
    torch.cuda.synchronize()
    assert st == QT_ERR_UNSUPPORTED and _all_nan(dg)


@pytest.mark.parametrize("shape", Hb.TRANSPOSE_SHAPES)
def test_transpose_guards(shape):
    dev, L, lib = _env()
    rows, cols = shape
    src = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows)).to(dev)
    dst = _nan((cols * rows + 64,), F32, dev)
    L.check(lib.qt_transpose_f32(L.ptr(src), L.ptr(dst), rows, cols, L.stream_ptr()), "qt_transpose_f32")
    assert torch.equal(dst[:rows * cols].view(cols, rows), src.t()) and _all_nan(dst[rows * cols:])


# ----------------------------------------------------------------------------------------------------------------------
# attention gate
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B", Hb.ATT_B)
@pytest.mark.parametrize("regime", Hb.ATT_REGIMES)
def test_attention_gate_vs_float64(regime, B, dt):
    dev, L, lib = _env()
    ld, col0 = Hb.ATT_LD, Hb.ATT_COL0
    v, w1, b1, w2, b2, d = Hb.att_inputs(B, regime, dt)
    vd, w1d, b1d, w2d, b2d, dd = (t.to(dev) for t in (v, w1, b1, w2, b2, d))
    act, alpha = _nan((B, Hb.NV, Hb.DH), F32, dev), _nan((B, Hb.NV), F32, dev)
    fused = _nan((B, ld), dt, dev)
    L.check(lib.qt_attention_gate(L.qt_dtype(dt), L.ptr(vd), L.ptr(w1d), L.ptr(b1d), L.ptr(w2d), L.ptr(b2d), L.ptr(act),
                                  L.ptr(alpha), L.ptr(fused), B, ld, col0, L.stream_ptr()), "qt_attention_gate")
    fused = fused.cpu()
    assert _all_nan(fused[:, :col0]) and _all_nan(fused[:, col0 + Hb.DV:])
    tag = f"attention {regime} B={B} {dt}"
    for name, got, ref, bound in Hb.att_fwd_facts(v, w1, b1, w2, b2, act.cpu(), alpha.cpu(), fused[:, col0:col0 + Hb.DV], dt):
        _report(f"{tag} fwd {name}", got, ref, bound)
    if regime == "dead":
        assert bool((alpha == 1.0 / 16).all())
    # backward: a pure function of operands the test supplies (act / alpha of the float64 forward, rounded to f32)
    a64, _, al64, _ = Hb.att_forward_f64(v, w1, b1, w2, b2)
    a32, al32 = a64.float(), al64.float()
    ad, ald = a32.to(dev), al32.to(dev)
    ds, dpre, dv = _nan((B, Hb.NV), F32, dev), _nan((B, Hb.NV, Hb.DH), F32, dev), _nan((B, Hb.NV, Hb.DV), F32, dev)
    L.check(lib.qt_attention_gate_bwd(L.qt_dtype(dt), L.ptr(dd), L.ptr(vd), L.ptr(ad), L.ptr(ald), L.ptr(w1d), L.ptr(w2d),
                                      L.ptr(ds), L.ptr(dpre), L.ptr(dv), B, ld, col0, L.stream_ptr()), "qt_attention_gate_bwd")
    ref = Hb.att_bwd_ref(d[:, col0:col0 + Hb.DV], v, a32, al32, w1, w2)
    ds = ds.cpu()
    for name, got in (("ds", ds), ("dpre", dpre.cpu()), ("dv", dv.cpu()), ("ds_sum", ds.double().sum(1))):
        _report(f"{tag} bwd {name}", got, *ref[name])
    if regime == "dead":
        assert bool((dpre == 0).all())


# ----------------------------------------------------------------------------------------------------------------------
# region average pool
# ----------------------------------------------------------------------------------------------------------------------
def _region_bwd(L, lib, dev, x, d, B, S, dt, ddt, ld, col0):
    _, HW, C = x.shape
    g = _nan(tuple(x.shape), dt, dev)
    L.check(lib.qt_region_avgpool_bwd(L.qt_dtype(dt), L.ptr(d), L.qt_dtype(ddt), L.ptr(x), L.ptr(g), B, S, HW, C, ld, col0,
                                      L.stream_ptr()), "qt_region_avgpool_bwd")
    return g


@pytest.mark.parametrize("dts", Hb.REGION_DTYPES)
@pytest.mark.parametrize("shape", Hb.REGION_SHAPES)
def test_region_avgpool_vs_float64(shape, dts):
    dev, L, lib = _env()
    B, S, HW, C = shape
    dt, ddt = dts
    R, col0 = S * S, Hb.REGION_COL0
    ld = R * C + Hb.REGION_PAD
    x, d = Hb.region_inputs(B, S, HW, C, dt, ddt)
    xd, dd = x.to(dev), d.to(dev)
    dst = _nan((B, ld), ddt, dev)
    L.check(lib.qt_region_avgpool(L.qt_dtype(dt), L.ptr(xd), L.ptr(dst), L.qt_dtype(ddt), B, S, HW, C, ld, col0,
                                  L.stream_ptr()), "qt_region_avgpool")
    dst = dst.cpu()
    assert _all_nan(dst[:, :col0]) and _all_nan(dst[:, col0 + R * C:])
    tag = f"region pool B={B} S={S} HW={HW} C={C} {dt}->{ddt}"
    _report(tag, dst[:, col0:col0 + R * C], *Hb.region_ref(x, B, S, ddt))
    g = _region_bwd(L, lib, dev, xd, dd, B, S, dt, ddt, ld, col0)
    _report(f"{tag} bwd", g.cpu(), *Hb.region_bwd_ref(d[:, col0:col0 + R * C], x, B, S, dt))


def test_region_avgpool_bwd_second_grid_trip():
    """B = 335: 4 202 240 channel groups for 16384 x 256 threads: the first batch at which some threads take a second trip"""
    dev, L, lib = _env()
    B, S, HW, C = Hb.REGION_LARGE
    R, col0 = S * S, Hb.REGION_COL0
    ld = R * C + Hb.REGION_PAD
    assert B * R * HW * (C // 8) > 16384 * 256 >= (B - 1) * R * HW * (C // 8)
    x, d = Hb.region_inputs(B, S, HW, C, BF16, BF16, device=dev)
    g = _region_bwd(L, lib, dev, x, d, B, S, BF16, BF16, ld, col0)
    _report("region pool bwd, second trip", g, *Hb.region_bwd_ref(d[:, col0:col0 + R * C], x, B, S, BF16))


# ----------------------------------------------------------------------------------------------------------------------
# clip average pool
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", Hb.TB_SHAPES)
def test_avgpool_tb_vs_float64(shape, dt):
    dev, L, lib = _env()
    T, B, HW, C = shape
    ld, col0 = C + Hb.TB_PAD, Hb.TB_COL0
    x, d = Hb.tb_inputs(T, B, HW, C, dt)
    xd, dd = x.to(dev), d.to(dev)
    dst = _nan((B, ld), F32, dev)
    L.check(lib.qt_avgpool_tb(L.qt_dtype(dt), L.ptr(xd), L.ptr(dst), T, B, HW, C, ld, col0, L.stream_ptr()), "qt_avgpool_tb")
    dst = dst.cpu()
    assert _all_nan(dst[:, :col0]) and _all_nan(dst[:, col0 + C:])
    tag = f"avgpool_tb T={T} B={B} HW={HW} C={C} {dt}"
    _report(tag, dst[:, col0:col0 + C], *Hb.tb_ref(x))
    g = _nan((T, B, HW, C), dt, dev)
    L.check(lib.qt_avgpool_tb_bwd(L.qt_dtype(dt), L.ptr(dd), L.ptr(g), T, B, HW, C, ld, col0, L.stream_ptr()),
            "qt_avgpool_tb_bwd")
    _report(f"{tag} bwd", g.cpu(), *Hb.tb_bwd_ref(d[:, col0:col0 + C], shape, dt))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C,col0", [(0, 8), (64, -8)])
def test_avgpool_tb_refuses_what_its_siblings_refuse(C, col0, dt):
    """C = 0 and a negative col0, as qt_region_avgpool / qt_attention_gate refuse them: invalid argument, nothing written"""
    dev, L, lib = _env()
    T, B, HW, ld = 2, 2, 4, 128
    x = torch.randn(T, B, HW, 64).to(dev, dt)
    d = torch.randn(B, ld).to(dev)
    dst, g = _nan((B, ld), F32, dev), _nan((T, B, HW, 64), dt, dev)
    st1 = lib.qt_avgpool_tb(L.qt_dtype(dt), L.ptr(x), L.ptr(dst), T, B, HW, C, ld, col0, L.stream_ptr())
    st2 = lib.qt_avgpool_tb_bwd(L.qt_dtype(dt), L.ptr(d), L.ptr(g), T, B, HW, C, ld, col0, L.stream_ptr())
    torch.cuda.synchronize()
    assert st1 == QT_ERR_INVALID_ARG and st2 == QT_ERR_INVALID_ARG
    assert _all_nan(dst) and _all_nan(g)


# ----------------------------------------------------------------------------------------------------------------------
# BatchNorm3d partial sums
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", Hb.BN_SHAPES)
def test_bn_stats_per_row_vs_float64(shape, dt):
    dev, L, lib = _env()
    M, C = shape
    rows = lib.qt_bn_stats_rows(M, C)
    assert rows == Hb.bn_stats_rows(M)
    y = Hb.bn_inputs(M, C, dt)
    yd = y.to(dev)
    part = _nan((rows + 1, 2, C), F32, dev)
    L.check(lib.qt_bn_stats(L.qt_dtype(dt), L.ptr(yd), M, C, L.ptr(part), L.stream_ptr()), "qt_bn_stats")
    part = part.cpu()
    assert _all_nan(part[rows:])
    if M == 262145:
        assert rows == 1024 and bool((part[1021:1024] == 0).all())
    _report(f"bn_stats M={M} C={C} {dt}", part[:rows], *Hb.bn_stats_ref(y, rows))


@pytest.mark.parametrize("C", Hb.BN_REFUSED_C)
def test_bn_stats_refuses_channel_counts(C):
    dev, L, lib = _env()
    M = 16
    y = torch.randn(M, C).to(dev)
    part = _nan((1, 2, C), F32, dev)
    st = lib.qt_bn_stats(L.qt_dtype(F32), L.ptr(y), M, C, L.ptr(part), L.stream_ptr())
    torch.cuda.synchronize()
    assert st == QT_ERR_INVALID_ARG and _all_nan(part)
