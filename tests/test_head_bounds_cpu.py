"""The bounds and float64 references of tests/_head_bounds.py, checked WITHOUT a GPU.  A torch-f32 restatement of each kernel's
arithmetic (the same summation split where the kernel documents one: four accumulators over m % 4 in the LSTM forward, even /
odd accumulators per gate block in its backward, four position lanes folded pairwise in the region pool, position lanes added
in ascending order in the clip pool and the BatchNorm3d sums) stands in for the kernel at every case of
tests/test_heads_gpu.py and must meet every bound; the median bound / |ref| is printed so that a vacuous bound shows.  Then
six deliberately wrong restatements must MISS the bounds at the same inputs: a bound a mutant passes is too loose."""
import math

import pytest
import torch

import _head_bounds as Hb

F32, BF16 = torch.float32, torch.bfloat16
DTS = [F32, BF16]
LOG2E = torch.tensor(math.log2(math.e), dtype=F32)


def _ok(name, got, ref, bound):
    r = Hb.ratio(got, ref, bound)
    print(f"  {name}: err/bound {r:.3f}, median bound/|ref| {Hb.vacuity(ref, bound):.2e}")
    assert r <= 1.0, (name, r)


def _misses(name, got, ref, bound):
    r = Hb.ratio(got, ref, bound)
    print(f"  mutant {name}: err/bound {r:.3g}")
    assert r > 1.0, (name, r)


def fexp(x):
    """__expf: exp2 of the rounded product with log2 e"""
    return torch.exp2(x * LOG2E)


def sigmoid(x):
    return 1.0 / (1.0 + fexp(-x))


def seq_sum(terms, init=None):
    """terms added one after the other in f32, along dim 0"""
    a = torch.zeros_like(terms[0]) if init is None else init
    for k in range(terms.shape[0]):
        a = a + terms[k]
    return a


# ----------------------------------------------------------------------------------------------------------------------
# LSTM
# ----------------------------------------------------------------------------------------------------------------------
def lstm_fwd_standin(xproj, whh, bhh, order="ifgo"):
    B, T, H4 = xproj.shape
    H = H4 // 4
    Wt = whh.t().contiguous()                                    # [H][4H]
    h, c = torch.zeros(B, H), torch.zeros(B, H)
    gates, cell, hprev, hout = (torch.empty(B, T, n) for n in (H4, H, H, H))
    tanh_rows = slice(2 * H, 3 * H) if order == "ifgo" else slice(3 * H, 4 * H)
    for t in range(T):
        hprev[:, t] = h
        a = xproj[:, t] + bhh if bhh is not None else xproj[:, t].clone()
        part = [(h[:, q::4, None] * Wt[None, q::4]).sum(1, dtype=F32) for q in range(4)]
        a = ((a + part[0]) + part[1]) + (part[2] + part[3])
        act = sigmoid(a)
        act[:, tanh_rows] = torch.tanh(a[:, tanh_rows])
        gi, gf = act[:, :H], act[:, H:2 * H]
        gg, go = (act[:, 2 * H:3 * H], act[:, 3 * H:]) if order == "ifgo" else (act[:, 3 * H:], act[:, 2 * H:3 * H])
        c = gf * c + gi * gg
        h = go * torch.tanh(c)
        gates[:, t], cell[:, t], hout[:, t] = act, c, h
    return gates, cell, hprev, hout


def lstm_bwd_standin(gates, cell, whh, dhout, dlast, wrong=None):
    B, T, H4 = gates.shape
    H = H4 // 4
    dh_rec, dc_next = torch.zeros(B, H), torch.zeros(B, H)
    dgates = torch.empty(B, T, H4)
    for t in range(T - 1, -1, -1):
        dh = dh_rec
        if dhout is not None:
            dh = dh + dhout[:, t]
        if dlast is not None and t == T - 1:
            dh = dh + dlast
        gi, gf, gg, go = gates[:, t].split(H, -1)
        c = cell[:, t]
        cp = cell[:, t - 1] if t > 0 else torch.zeros(B, H)
        if wrong == "daf_from_c_t":
            cp = c
        tc = torch.tanh(c)
        dc = dc_next + dh * go * (1.0 - tc * tc)
        dG = torch.cat([dc * gg * gi * (1.0 - gi), dc * cp * gf * (1.0 - gf), dc * gi * (1.0 - gg * gg),
                        dh * tc * go * (1.0 - go)], -1)
        dc_next = dc * gf
        dgates[:, t] = dG
        sp = []
        for k in range(4):
            blk, Wk = dG[:, k * H:(k + 1) * H], whh[k * H:(k + 1) * H]
            even = (blk[:, 0::2, None] * Wk[None, 0::2]).sum(1, dtype=F32)
            sp.append(even + (blk[:, 1::2, None] * Wk[None, 1::2]).sum(1, dtype=F32))
        dh_rec = (sp[0] + sp[1]) + (sp[2] + sp[3])
    return dgates


@pytest.mark.parametrize("regime", Hb.LSTM_REGIMES)
@pytest.mark.parametrize("BT", Hb.LSTM_BT)
@pytest.mark.parametrize("H", Hb.LSTM_H)
def test_lstm_forward_bounds(H, BT, regime):
    B, T = BT
    xproj, whh, bhh, _, _ = Hb.lstm_inputs(H, B, T, regime)
    for bias in (bhh, None):
        gates, cell, hprev, hout = lstm_fwd_standin(xproj, whh, bias)
        if regime == "saturated":   # the premise: gates reach exactly 0 and 1, __expf overflows
            assert bool((gates == 0).any()) and bool((gates == 1).any()) and float(xproj.abs().max()) > 89.0
        assert Hb.lstm_chain_exact(hprev, hout)
        for name, got, ref, bound in Hb.lstm_fwd_facts(xproj, whh, bias, gates, cell, hprev, hout):
            _ok(f"lstm fwd {name}", got, ref, bound)
    wg = lstm_fwd_standin(xproj, whh, bhh, order="ifog")
    name, got, ref, bound = Hb.lstm_fwd_facts(xproj, whh, bhh, *wg)[0]
    _misses("gate order i, f, o, g", got, ref, bound)


@pytest.mark.parametrize("regime", Hb.LSTM_REGIMES)
@pytest.mark.parametrize("BT", Hb.LSTM_BT)
@pytest.mark.parametrize("H", Hb.LSTM_H)
def test_lstm_backward_bounds(H, BT, regime):
    B, T = BT
    xproj, whh, bhh, dhout, dlast = Hb.lstm_inputs(H, B, T, regime)
    gates, cell = Hb.lstm_forward_f64(xproj, whh, bhh)
    for which in Hb.LSTM_GRADS:
        dh = dhout if which != "dlast" else None
        dl = dlast if which != "dhout" else None
        got = lstm_bwd_standin(gates, cell, whh, dh, dl)
        _ok(f"lstm bwd {which}, whole chain", got, *Hb.lstm_bwd_ref(gates, cell, whh, dh, dl))
        _ok(f"lstm bwd {which}, step by step", got, *Hb.lstm_bwd_ref(gates, cell, whh, dh, dl, got))
    # (a T = 1 run has no c_{t-1}: the mutant is the correct kernel there only if c_0 == 0, which it is not)
    wrong = lstm_bwd_standin(gates, cell, whh, dhout, dlast, wrong="daf_from_c_t")
    _misses("daf from c_t, whole chain", wrong, *Hb.lstm_bwd_ref(gates, cell, whh, dhout, dlast))
    _misses("daf from c_t, step by step", wrong, *Hb.lstm_bwd_ref(gates, cell, whh, dhout, dlast, wrong))


# ----------------------------------------------------------------------------------------------------------------------
# attention gate
# ----------------------------------------------------------------------------------------------------------------------
def att_fwd_standin(v, w1, b1, w2, b2, dt):
    B = v.shape[0]
    a = seq_sum(torch.stack([w1[:, k] * v[:, :, k:k + 1] for k in range(Hb.DV)]), b1.expand(B, Hb.NV, Hb.DH).clone())
    act = a.clamp_min(0.0)
    s = seq_sum(torch.stack([w2[h] * act[:, :, h] for h in range(Hb.DH)]), b2.expand(B, Hb.NV).clone())
    e = fexp(s - s.max(1, keepdim=True).values)
    alpha = e * (1.0 / seq_sum(e.t().contiguous()))[:, None]
    out = seq_sum(torch.stack([alpha[:, j, None] * v[:, j] for j in range(Hb.NV)]))
    return act, alpha, out.to(dt)


def att_bwd_standin(d, v, act, alpha, w1, w2, wrong=None):
    dout = d.float()
    da = seq_sum(torch.stack([dout[:, None, c] * v[:, :, c] for c in range(Hb.DV)]))
    t = seq_sum((alpha * da).t().contiguous())[:, None]
    ds = alpha * da if wrong == "ds_without_t" else alpha * (da - t)
    dpre = torch.where(act > 0, ds[:, :, None] * w2, torch.zeros(()))
    dv = seq_sum(torch.stack([w1[h] * dpre[:, :, h, None] for h in range(Hb.DH)]), alpha[:, :, None] * dout[:, None, :])
    return ds, dpre, dv


def _att_premise(regime, v, w1, b1, w2, b2):
    act, s, alpha, _ = Hb.att_forward_f64(v, w1, b1, w2, b2)
    if regime == "peaked":
        assert float((s.max(1).values - s.min(1).values).min()) > 100.0
        assert float(alpha.min()) < Hb.TINY and float(alpha.max(1).values.min()) > 0.5
    elif regime == "dead":
        assert float(act.max()) == 0.0
    elif regime == "signed":
        assert float(v.min()) < -1.0
    return act.float(), alpha.float()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B", Hb.ATT_B)
@pytest.mark.parametrize("regime", Hb.ATT_REGIMES)
def test_attention_gate_bounds(regime, B, dt):
    v, w1, b1, w2, b2, d = Hb.att_inputs(B, regime, dt)
    act64, alpha64 = _att_premise(regime, v, w1, b1, w2, b2)
    act, alpha, out = att_fwd_standin(v, w1, b1, w2, b2, dt)
    for name, got, ref, bound in Hb.att_fwd_facts(v, w1, b1, w2, b2, act, alpha, out, dt):
        _ok(f"attention fwd {name}", got, ref, bound)
    if regime == "dead":
        assert bool((alpha == 1.0 / 16).all())
    dc = d[:, Hb.ATT_COL0:Hb.ATT_COL0 + Hb.DV]
    ref = Hb.att_bwd_ref(dc, v, act64, alpha64, w1, w2)
    ds, dpre, dv = att_bwd_standin(dc, v, act64, alpha64, w1, w2)
    for name, got in (("ds", ds), ("dpre", dpre), ("dv", dv), ("ds_sum", ds.double().sum(1))):
        _ok(f"attention bwd {name}", got, *ref[name])
    if regime == "dead":
        assert bool((dpre == 0).all())
    wds, wdpre, wdv = att_bwd_standin(dc, v, act64, alpha64, w1, w2, wrong="ds_without_t")
    _misses("ds = alpha * dalpha", wds, *ref["ds"])
    _misses("ds = alpha * dalpha (its sum)", wds.double().sum(1), *ref["ds_sum"])
    if regime != "dead":   # (dv sees ds only through the live hidden units)
        _misses("ds = alpha * dalpha (dv)", wdv, *ref["dv"])


# ----------------------------------------------------------------------------------------------------------------------
# region average pool
# ----------------------------------------------------------------------------------------------------------------------
def region_standin(x, B, S, ddt, slot_fn):
    R, (_, HW, C) = S * S, x.shape
    xf = x.float()
    p = [xf[:, q::4].sum(1, dtype=F32) for q in range(4)]
    m = ((p[0] + p[1]) + (p[2] + p[3])) * (torch.tensor(1.0) / HW)
    out = torch.empty(B, R * C)
    out[:, Hb._slot_index(S, C, slot_fn, x.device).reshape(-1)] = m.view(B, R * C)
    return out.to(ddt)


def region_bwd_standin(d, x, B, S, slot_fn):
    R, (_, HW, C) = S * S, x.shape
    idx = Hb._slot_index(S, C, slot_fn, x.device).reshape(-1)
    per = d.float()[:, idx].reshape(B * R, 1, C) * (torch.tensor(1.0) / HW)
    return torch.where(x.float() > 0, per, torch.zeros(())).to(x.dtype)


def _row_major(r, S):
    return r


@pytest.mark.parametrize("dts", Hb.REGION_DTYPES)
@pytest.mark.parametrize("shape", Hb.REGION_SHAPES)
def test_region_avgpool_bounds(shape, dts):
    B, S, HW, C = shape
    dt, ddt = dts
    x, d = Hb.region_inputs(B, S, HW, C, dt, ddt)
    dc = d[:, Hb.REGION_COL0:Hb.REGION_COL0 + S * S * C]
    ref, bound = Hb.region_ref(x, B, S, ddt)
    _ok("region avgpool", region_standin(x, B, S, ddt, Hb.slot), ref, bound)
    bref, bbound = Hb.region_bwd_ref(dc, x, B, S, dt)
    _ok("region avgpool bwd", region_bwd_standin(dc, x, B, S, Hb.slot), bref, bbound)
    if S == 4:
        _misses("row-major slots", region_standin(x, B, S, ddt, _row_major), ref, bound)
        _misses("row-major slots (bwd)", region_bwd_standin(dc, x, B, S, _row_major), bref, bbound)


# ----------------------------------------------------------------------------------------------------------------------
# clip average pool
# ----------------------------------------------------------------------------------------------------------------------
def lane_sum(rows, lanes):
    """rows [..., n, C]: lane l adds rows l, l + lanes, ... then the lanes are added in ascending order"""
    n = rows.shape[-2]
    pad = (-n) % lanes
    if pad:
        rows = torch.cat([rows, rows.new_zeros(*rows.shape[:-2], pad, rows.shape[-1])], -2)
    per = rows.view(*rows.shape[:-2], -1, lanes, rows.shape[-1]).sum(-3, dtype=F32)
    return seq_sum(per.movedim(-2, 0).contiguous())


def tb_standin(x, wrong=None):
    T, B, HW, C = x.shape
    G = C // 8
    R = 256 // min(G, 32)
    s = lane_sum(x.float().permute(1, 0, 2, 3).reshape(B, T * HW, C), R)
    return s * (torch.tensor(1.0) / (HW if wrong == "divide_by_hw" else T * HW))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", Hb.TB_SHAPES)
def test_avgpool_tb_bounds(shape, dt):
    T, B, HW, C = shape
    x, d = Hb.tb_inputs(T, B, HW, C, dt)
    ref, bound = Hb.tb_ref(x)
    _ok("avgpool_tb", tb_standin(x), ref, bound)
    dc = d[:, Hb.TB_COL0:Hb.TB_COL0 + C]
    bref, bbound = Hb.tb_bwd_ref(dc, shape, dt)
    inv = torch.tensor(1.0) / (T * HW)
    _ok("avgpool_tb bwd", (dc * inv).view(1, B, 1, C).expand(T, B, HW, C).to(dt), bref, bbound)
    if T > 1:   # (at T = 1 the two divisors are the same number)
        _misses("divide by HW", tb_standin(x, wrong="divide_by_hw"), ref, bound)
        _misses("divide by HW (bwd)", (dc * (torch.tensor(1.0) / HW)).view(1, B, 1, C).expand(T, B, HW, C).to(dt), bref, bbound)


# ----------------------------------------------------------------------------------------------------------------------
# BatchNorm3d partial sums
# ----------------------------------------------------------------------------------------------------------------------
def bn_standin(y, rows, wrong=None):
    M, C = y.shape
    slab = -(-M // rows)
    lanes = 256 // (C // 8)
    yf = torch.cat([y.float(), torch.zeros(rows * slab - M, C)]).view(rows, slab, C)
    if wrong == "drop_last_row":
        yf = yf.clone()
        n = (M - torch.arange(rows) * slab).clamp(0, slab)
        live = n > 0
        yf[torch.arange(rows)[live], (n - 1)[live]] = 0.0
    return torch.stack([lane_sum(yf, lanes), lane_sum(yf * yf, lanes)], 1)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", Hb.BN_SHAPES)
def test_bn_stats_bounds(shape, dt):
    M, C = shape
    y = Hb.bn_inputs(M, C, dt)
    rows = Hb.bn_stats_rows(M)
    ref, bound = Hb.bn_stats_ref(y, rows)
    assert ref.shape == (rows, 2, C)
    if M == 262145:
        assert rows == 1024 and bool((ref[1021:] == 0).all()) and bool((bound[1021:] == 0).all())
        assert bool((ref[1020, 1] > 0).all())
    _ok("bn_stats", bn_standin(y, rows), ref, bound)
    _misses("last row of each slab dropped", bn_standin(y, rows, wrong="drop_last_row"), ref, bound)
