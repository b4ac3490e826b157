"""Float64 references and DERIVED error bounds for the kernels that finish the three non-ResNet heads: the LSTM recurrence
(csrc/lstm.hip), the region average pool and the attention gate (csrc/attention.hip), the clip average pool and the BatchNorm3d
partial sums (csrc/video3d.hip).  Shared by tests/test_heads_gpu.py (the kernels on the GPU) and tests/test_head_bounds_cpu.py
(a torch-f32 restatement in the kernel's place meets every bound, six deliberately wrong restatements miss them).

Every reference is computed in float64 from exactly the f32 / bf16 values the kernel reads; every bound is evaluated per output
element by tests/_bounds.py's rule:
  * a sum of n f32 terms costs sum_bound(n, sum |term|) = (n + 8) 2^-24 sum |term| whatever the order of summation (the 8 spare
    roundings also cover a reciprocal formed once per thread and the product with it);
  * every other f32 operation costs one rounding U of its result; a product of k factors that carry errors e_i costs
    prod (|r_i| + e_i) - prod |r_i| plus k roundings of the whole product (_prod: k - 1 products, one spare for the U^2 terms);
  * a differentiable function f of an argument that is off by d costs |f'(ref)| d + d^2 (|f''| <= 2 for tanh and the logistic
    function: the remainder of the Taylor expansion is at most d^2);
  * + stored() where the output is bf16.
The recurrences are pinned step by step: a step is checked from the state the kernel itself stored for the step before, and
the links of the chain (hprev[t] == hout[t-1]) are bit-exact, so no tolerance grows with T.

ASSUMPTION (this extends the block of tests/_loss_ref.py; the ROCm device-math accuracy table is not shipped with the toolkit
this suite runs against, and NOBODY HAS MEASURED THESE FIGURES ON THIS HARDWARE):
  * tanhf of the device library meets the OpenCL 3.0 single-precision figure, tanh <= 5 ulp (ULP_TANH);
  * __expf(x) is the hardware exp2 of fl(x * log2 e).  The rounding of log2 e and of the product moves the exponent by at most
    2 U |x log2 e|, a relative error of 2 U |x| in the result: that part is derived.  The instruction itself is ASSUMED good to
    2 ulp (ULP_FEXP), and a result below the smallest normal number may be flushed to zero: an absolute floor of 2^-126
    (FEXP_FLOOR).  1 / (1 + __expf(-x)) inherits the floor: where __expf overflows the quotient is exactly 0 and the true value
    is below 2^-126.
One ulp is at most 2^-23 relative.  Nothing here is fitted to what a kernel returns."""
import torch

from _bounds import U, UB, ratio, stored, sum_bound  # noqa: F401  (re-exported to the tests)

F32, BF16 = torch.float32, torch.bfloat16
ULP_TANH = 5
ULP_FEXP = 2
R_TANH = 2 * U * ULP_TANH
R_FEXP = 2 * U * ULP_FEXP
FEXP_FLOOR = 2.0 ** -126
TINY = 2.0 ** -126       # smallest normal f32: what a flushed result may be off by


def fexp_rel(x):
    """relative error of __expf(x): the argument's two roundings (derived) + the instruction (assumed)"""
    return 2 * U * x.abs() + R_FEXP


def vacuity(ref, bound):
    """median bound / |ref| over the elements with ref != 0: a vacuous bound shows as a figure near or above 1"""
    m = ref != 0
    if not bool(m.any()):
        return 0.0
    return float((bound[m] / ref[m].abs()).median())


def _prod(*fs):
    """product of factors (ref, err): (ref, err) with one rounding per factor.  A partial product below the smallest normal
    number is off by up to 2^-126 in absolute terms (gradual underflow or a flush), times the factors still to come"""
    ref = hi = lo = big = None
    for r, e in fs:
        a = r.abs()
        ref = r if ref is None else ref * r
        hi = a + e if hi is None else hi * (a + e)
        lo = a if lo is None else lo * a
        big = (a + e).clamp_min(1.0) if big is None else big * (a + e).clamp_min(1.0)
    return ref, (hi - lo).clamp_min(0.0) + len(fs) * (U * hi + TINY * big)


# ----------------------------------------------------------------------------------------------------------------------
# LSTM (torch gate order i, f, g, o)
# ----------------------------------------------------------------------------------------------------------------------
LSTM_H = [64, 188, 256]
LSTM_BT = [(1, 1), (5, 2), (3, 16)]
LSTM_REGIMES = ["normal", "saturated"]
LSTM_GRADS = ["dhout", "dlast", "both"]
TRANSPOSE_SHAPES = [(1, 1), (33, 31), (752, 188), (5, 1000)]


def lstm_inputs(H, B, T, regime, seed=0):
    """xproj [B][T][4H], W_hh [4H][H], b_hh [4H], dhout [B][T][H], dlast [B][H] (f32, CPU).  saturated: xproj x 30, so that
    gates reach exactly 0 and 1 and __expf(-x) overflows"""
    g = torch.Generator().manual_seed(1000 * H + 10 * T + B + seed)
    xproj = torch.randn(B, T, 4 * H, generator=g)
    if regime == "saturated":
        xproj = xproj * 30.0
        xproj[:, :, 1::16] = torch.sign(xproj[:, :, 1::16]) * 120.0   # every 16th row of every gate block: |x| > 88.8 for sure
    whh = torch.randn(4 * H, H, generator=g) / H ** 0.5
    bhh = torch.randn(4 * H, generator=g) * 0.1
    dhout = torch.randn(B, T, H, generator=g)
    dlast = torch.randn(B, H, generator=g)
    return xproj, whh, bhh, dhout, dlast


def _is_g(H):
    m = torch.zeros(4 * H, dtype=torch.bool)
    m[2 * H:3 * H] = True
    return m


def _gate_act(pre, d, H):
    """(ref, bound) of the activated gates from the float64 pre-activation and its bound d"""
    sig, th = torch.sigmoid(pre), torch.tanh(pre)
    g = _is_g(H)
    ref = torch.where(g, th, sig)
    der = torch.where(g, 1.0 - th * th, sig * (1.0 - sig))
    # 1 / (1 + e), e = __expf(-a): e's relative error moves the quotient by sig (1 - sig) times it, e's floor by sig^2 times
    # it; the sum 1 + e and the division round once each
    own_sig = sig * (1.0 - sig) * fexp_rel(pre.abs() + d) + sig * sig * FEXP_FLOOR + 2 * U * sig + TINY
    own_tanh = R_TANH * th.abs() + TINY
    return ref, der * d + d * d + torch.where(g, own_tanh, own_sig)


def lstm_fwd_facts(xproj, whh, bhh, gates, cell, hprev, hout):
    """[(name, got, ref, bound)] of one forward run, each step conditioned on the state the kernel stored (f32 tensors on the
    CPU; bhh may be None).  The chain links are lstm_chain_exact's."""
    H = whh.shape[1]
    hp, W = hprev.double(), whh.double()
    pre = xproj.double() + hp @ W.t()
    mag = xproj.double().abs() + hp.abs() @ W.abs().t()
    if bhh is not None:
        pre = pre + bhh.double()
        mag = mag + bhh.double().abs()
    gref, gbound = _gate_act(pre, sum_bound(H + 2, mag), H)
    gk = gates.double()
    gi, gf, gg, go = gk.split(H, -1)
    ck = cell.double()
    cprev = torch.cat([torch.zeros_like(ck[:, :1]), ck[:, :-1]], 1)
    p1, p2 = gf * cprev, gi * gg
    href = go * torch.tanh(ck)
    return [("gates", gates, gref, gbound),
            ("cell", cell, p1 + p2, 3 * (U * (p1.abs() + p2.abs()) + TINY)),   # two products and the sum, or their underflow
            ("hout", hout, href, (R_TANH + 2 * U) * href.abs() + TINY)]     # tanhf, the product (and a spare)


def lstm_chain_exact(hprev, hout):
    return bool(torch.equal(hprev[:, 1:], hout[:, :-1])) and bool((hprev[:, 0] == 0).all())


def lstm_forward_f64(xproj, whh, bhh):
    """gates [B][T][4H] and cell [B][T][H] of a float64 forward, rounded to f32: the backward kernel's inputs"""
    B, T, H4 = xproj.shape
    H = H4 // 4
    W = whh.double()
    h = torch.zeros(B, H, dtype=torch.float64)
    c = torch.zeros(B, H, dtype=torch.float64)
    gates, cell = [], []
    for t in range(T):
        a = xproj[:, t].double() + h @ W.t() + (bhh.double() if bhh is not None else 0.0)
        i, f, g, o = a.split(H, -1)
        i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
        c = f * c + i * g
        h = o * torch.tanh(c)
        gates.append(torch.cat([i, f, g, o], -1))
        cell.append(c)
    return torch.stack(gates, 1).float().contiguous(), torch.stack(cell, 1).float().contiguous()


def lstm_bwd_ref(gates, cell, whh, dhout, dlast, dgates_k=None):
    """(dgates ref, bound) [B][T][4H]: the float64 recurrence with a running error bound beside it.  The kernel is linear in
    (dh_rec, dc_next) given gates and cell, so the bound of a step is its local roundings, sum_bound(4H, |dgates| |W_hh|) of the
    recurrent product, and the previous step's bound pushed through |W_hh|, |gf| and |go (1 - tc^2)|.
    That bound is valid but multiplies by the norm of |W_hh| times the gate slopes at every step: at H = 256 its median is
    0.08 |ref| after 5 steps and 9e4 |ref| after 15, where it says nothing.  With dgates_k (what the kernel stored) the step
    is conditioned as the forward's are: dh_rec of step t is the float64 product of the kernel's own dgates[t + 1] with W_hh,
    off by that product's sum_bound only, and the one bound that still runs is dc_next's, through |gf| <= 1.  By induction
    from t = T - 1, which depends on the inputs alone, that pins every step.  The tests assert both."""
    B, T, H4 = gates.shape
    H = H4 // 4
    W = whh.double()
    Wa = W.abs()
    z = torch.zeros(B, H, dtype=torch.float64)
    dh_rec, e_h, dc_next, e_c = z, z, z, z
    ref = torch.zeros(B, T, H4, dtype=torch.float64)
    bound = torch.zeros(B, T, H4, dtype=torch.float64)
    for t in range(T - 1, -1, -1):
        gi, gf, gg, go = gates[:, t].double().split(H, -1)
        c = cell[:, t].double()
        cp = cell[:, t - 1].double() if t > 0 else z
        if dgates_k is not None and t < T - 1:
            dk = dgates_k[:, t + 1].double()
            dh_rec, e_h = dk @ W, sum_bound(4 * H, dk.abs() @ Wa)
        dh, mag = dh_rec, dh_rec.abs() + e_h
        if dhout is not None:
            dh, mag = dh + dhout[:, t].double(), mag + dhout[:, t].double().abs()
        if dlast is not None and t == T - 1:
            dh, mag = dh + dlast.double(), mag + dlast.double().abs()
        e_dh = e_h + 2 * U * mag                                            # at most two sums
        tc = torch.tanh(c)
        e_tc = R_TANH * tc.abs() + TINY
        s = 1.0 - tc * tc
        e_s = 2 * tc.abs() * e_tc + e_tc * e_tc + U * tc * tc + U * s       # the square, the difference
        q, e_q = _prod((dh, e_dh), (go, z), (s, e_s))
        dc = dc_next + q
        e_dc = e_c + e_q + U * (dc_next.abs() + e_c + q.abs() + e_q)
        om = lambda x: (1.0 - x, U * (1.0 - x).abs())                       # noqa: E731  (1 - gate: one rounding)
        sg = 1.0 - gg * gg
        dai = _prod((dc, e_dc), (gg, z), (gi, z), om(gi))
        daf = _prod((dc, e_dc), (cp, z), (gf, z), om(gf))
        dag = _prod((dc, e_dc), (gi, z), (sg, U * gg * gg + U * sg.abs()))
        dao = _prod((dh, e_dh), (tc, e_tc), (go, z), om(go))
        ref[:, t] = torch.cat([dai[0], daf[0], dag[0], dao[0]], -1)
        bound[:, t] = torch.cat([dai[1], daf[1], dag[1], dao[1]], -1)
        dc_next, e_c = _prod((dc, e_dc), (gf, z))
        dh_rec = ref[:, t] @ W
        e_h = bound[:, t] @ Wa + sum_bound(4 * H, (ref[:, t].abs() + bound[:, t]) @ Wa)
    return ref, bound


# ----------------------------------------------------------------------------------------------------------------------
# attention gate: Linear(64, 32) - ReLU - Linear(32, 1), softmax over 16 scores, weighted sum of the 16 vectors
# ----------------------------------------------------------------------------------------------------------------------
NV, DV, DH = 16, 64, 32
ATT_B = [1, 7]
ATT_REGIMES = ["flat", "peaked", "dead", "signed"]
ATT_LD, ATT_COL0 = 1216, 1024
PEAK_SCALE = 80.0


def att_inputs(B, regime, dt, seed=31):
    """v [B][16][64], w1 [32][64], b1 [32], w2 [32], b2 [1] (f32) and the gradient d [B][ld] in dt.  flat: the inputs of
    tests/test_attention_gpu.py; peaked: w2 x 80 (score spread > 100: weights underflow, one is about 1); dead: b1 = -10 (no
    hidden unit fires: all scores equal b2); signed: v of both signs"""
    g = torch.Generator().manual_seed(seed + B)
    v = torch.rand(B, NV, DV, generator=g)
    w1 = torch.randn(DH, DV, generator=g) * 0.3
    b1 = torch.randn(DH, generator=g) * 0.1
    w2 = torch.randn(DH, generator=g) * 0.5
    b2 = torch.randn(1, generator=g) * 0.1
    d = torch.randn(B, ATT_LD, generator=g).to(dt)
    if regime == "peaked":
        w2 = w2 * PEAK_SCALE
    elif regime == "dead":
        b1 = torch.full((DH,), -10.0)
    elif regime == "signed":
        v = torch.randn(B, NV, DV, generator=g)
    return v, w1, b1, w2, b2, d


def att_forward_f64(v, w1, b1, w2, b2):
    """float64 (act, scores, alpha, out)"""
    act = (v.double() @ w1.double().t() + b1.double()).clamp_min(0.0)
    s = act @ w2.double() + b2.double()
    alpha = torch.softmax(s, 1)
    return act, s, alpha, (alpha.unsqueeze(-1) * v.double()).sum(1)


def att_fwd_facts(v, w1, b1, w2, b2, act, alpha, out, dt):
    """[(name, got, ref, bound)]: act from the inputs; alpha from the act the kernel stored; out from the alpha it stored.
    out: the 64 columns [B][64] in dt."""
    vd, W1, W2 = v.double(), w1.double(), w2.double()
    pre = vd @ W1.t() + b1.double()
    aref = pre.clamp_min(0.0)                                               # |max(a, 0) - max(b, 0)| <= |a - b|
    abound = sum_bound(DV + 1, vd.abs() @ W1.abs().t() + b1.double().abs())
    ak = act.double()
    s = ak @ W2 + b2.double()                                               # [B][16]
    ds = sum_bound(DH + 1, ak @ W2.abs() + b2.double().abs())
    mx, imx = s.max(1, keepdim=True)
    x = s - mx
    # e_j = __expf(fl(s_j - max)): the argument is off by both scores' bounds and its own rounding
    darg = ds + ds.gather(1, imx) + U * x.abs()
    rho = torch.expm1(darg) + torch.exp(darg) * fexp_rel(x.abs() + darg)
    alref = torch.softmax(s, 1)
    rden = (alref * rho).sum(1, keepdim=True) + (NV + 8) * U                # the 16-term sum of the e_j
    assert float(rden.max()) < 0.5
    # 1 / den and the product round once each; every flushed e_j moves alpha by at most 2^-126 / den, the product may flush too
    albound = alref * (rho + rden + 2 * U) / (1.0 - rden) + (NV + 2) * FEXP_FLOOR / (1.0 - rden)
    alk = alpha.double()
    oref = (alk.unsqueeze(-1) * vd).sum(1)
    obound = stored(sum_bound(NV, (alk.unsqueeze(-1) * vd.abs()).sum(1)), oref, dt)
    return [("act", act, aref, abound), ("alpha", alpha, alref, albound), ("out", out, oref, obound)]


def att_bwd_ref(d, v, act, alpha, w1, w2):
    """{name: (ref, bound)} of ds [B][16], dpre [B][16][32], dv [B][16][64] and ds_sum [B] (the sum over the 16 scores, zero up
    to the rounding of alpha).  d: the 64 columns [B][64].  A pure function of its arguments: act is an input, so no ReLU can
    flip.  The bound of ds carries the cancellation alpha (dalpha - t): it is relative to |dalpha| + |t|."""
    dd, vd, al, W1, W2 = d.double(), v.double(), alpha.double(), w1.double(), w2.double()
    da = (vd * dd.unsqueeze(1)).sum(-1)                                     # [B][16]
    e_da = sum_bound(DV, (vd.abs() * dd.abs().unsqueeze(1)).sum(-1))
    t = (al * da).sum(1, keepdim=True)
    e_t = (al * e_da).sum(1, keepdim=True) + sum_bound(NV, (al * (da.abs() + e_da)).sum(1, keepdim=True))
    diff = da - t
    e_diff = e_da + e_t + U * (da.abs() + t.abs() + e_da + e_t)
    ds = al * diff
    e_ds = al * e_diff + U * al * (diff.abs() + e_diff) + TINY
    live = act.double() > 0
    zero = torch.zeros((), dtype=torch.float64)
    dpre = torch.where(live, ds.unsqueeze(-1) * W2, zero)
    e_dpre = torch.where(live, (e_ds.unsqueeze(-1) + U * (ds.abs() + e_ds).unsqueeze(-1)) * W2.abs(), zero)
    first = al.unsqueeze(-1) * dd.unsqueeze(1)
    dv = first + dpre @ W1
    e_dv = e_dpre @ W1.abs() + sum_bound(DH + 1, first.abs() + (dpre.abs() + e_dpre) @ W1.abs())
    return {"ds": (ds, e_ds), "dpre": (dpre, e_dpre), "dv": (dv, e_dv), "ds_sum": (ds.sum(1), e_ds.sum(1))}


# ----------------------------------------------------------------------------------------------------------------------
# region average pool: x [B*R][HW][C] -> dst[b][col0 + slot(r) * C + c]
# ----------------------------------------------------------------------------------------------------------------------
REGION_SHAPES = [(3, 2, 196, 24), (5, 4, 49, 72), (2, 2, 1, 8), (2, 4, 3, 64)]      # (B, S, HW, C)
REGION_DTYPES = [(F32, F32), (BF16, BF16), (BF16, F32)]                            # (map, dst)
REGION_LARGE = (335, 2, 196, 128)   # 1340 * 196 * 16 = 4 202 240 groups > 16384 * 256: some threads take a second trip
REGION_PAD, REGION_COL0 = 64, 32


def slot(r, S):
    """row-major region index -> the reference's concatenation order: tests/test_attention_gpu.py's independent restatement"""
    from test_attention_gpu import _slot
    return _slot(r, S)


def region_inputs(B, S, HW, C, dt, ddt, seed=21, device="cpu"):
    """x (conv + ReLU output: about half exact zeros) in dt, the gradient d [B][ld] in ddt"""
    R = S * S
    g = torch.Generator(device=device).manual_seed(seed + B + HW)
    x = torch.relu(torch.randn(B * R, HW, C, generator=g, device=device)).to(dt)
    d = torch.randn(B, R * C + REGION_PAD, generator=g, device=device).to(ddt)
    return x, d


def _slot_index(S, C, slot_fn, device):
    """column (without col0) of element (r, c): [R][C]"""
    R = S * S
    s = torch.tensor([slot_fn(r, S) for r in range(R)], device=device)
    return s[:, None] * C + torch.arange(C, device=device)[None, :]


def region_ref(x, B, S, ddt, slot_fn=slot):
    """(ref, bound) [B][R*C] in destination order: HW terms, the product with 1 / HW, the store"""
    R, (_, HW, C) = S * S, x.shape
    xd = x.double()
    m = (xd.sum(1) / HW).view(B, R * C)
    a = (xd.abs().sum(1) / HW).view(B, R * C)
    idx = _slot_index(S, C, slot_fn, x.device).reshape(-1)
    ref, mag = torch.empty_like(m), torch.empty_like(a)
    ref[:, idx], mag[:, idx] = m, a
    return ref, stored(sum_bound(HW, mag) + U * ref.abs(), ref, ddt)


def region_bwd_ref(d, x, B, S, dt, slot_fn=slot):
    """(ref, bound) [B*R][HW][C]; d: the R*C columns [B][R*C]"""
    R, (_, HW, C) = S * S, x.shape
    idx = _slot_index(S, C, slot_fn, x.device).reshape(-1)
    per = d.double()[:, idx].reshape(B * R, 1, C) / HW
    ref = torch.where(x.double() > 0, per, torch.zeros((), dtype=torch.float64, device=x.device))
    return ref, stored(sum_bound(1, ref.abs()), ref, dt)


# ----------------------------------------------------------------------------------------------------------------------
# clip average pool: x [T][B][HW][C] -> dst[b][col0 + c] (f32)
# ----------------------------------------------------------------------------------------------------------------------
TB_SHAPES = [(2, 2, 49, 512), (8, 3, 196, 64), (1, 2, 1, 8), (2, 1, 12, 96), (3, 2, 7, 320)]   # (T, B, HW, C)
TB_PAD, TB_COL0 = 36, 20


def tb_inputs(T, B, HW, C, dt, seed=6):
    g = torch.Generator().manual_seed(seed + T + HW)
    x = (torch.randn(T, B, HW, C, generator=g) + 0.25).to(dt)
    d = torch.randn(B, C + TB_PAD, generator=g)
    return x, d


def tb_ref(x):
    T, B, HW, C = x.shape
    xd = x.double()
    ref = xd.sum((0, 2)) / (T * HW)
    return ref, sum_bound(T * HW, xd.abs().sum((0, 2)) / (T * HW)) + U * ref.abs()


def tb_bwd_ref(d, shape, dt):
    """d: the C columns [B][C]"""
    T, B, HW, C = shape
    ref = (d.double() / (T * HW)).view(1, B, 1, C).expand(T, B, HW, C).contiguous()
    return ref, stored(sum_bound(1, ref.abs()), ref, dt)


# ----------------------------------------------------------------------------------------------------------------------
# BatchNorm3d partial sums: y [M][C] -> partial [rows][2][C], row i = rows [i * slab, min(M, (i + 1) * slab)) of y
# ----------------------------------------------------------------------------------------------------------------------
BN_SHAPES = [(255, 8), (256, 8), (257, 8), (70001, 64), (513, 1024), (513, 2048), (300000, 8), (262145, 8)]   # (M, C)
BN_REFUSED_C = [24, 4, 4096]


def bn_stats_rows(M):
    """qt_bn_stats_rows restated: at most 1024 slabs of at least 256 rows"""
    return min(1024, max(1, -(-M // 256)))


def bn_inputs(M, C, dt, seed=6):
    g = torch.Generator().manual_seed(seed + M + C)
    return (torch.randn(M, C, generator=g) * 1.5 + 0.25).to(dt)


def bn_stats_ref(y, rows):
    """(ref, bound) [rows][2][C], per partial row: n_i terms each"""
    M, C = y.shape
    slab = -(-M // rows)
    yd = y.double()
    pad = rows * slab - M
    if pad:
        yd = torch.cat([yd, yd.new_zeros(pad, C)])
    yd = yd.view(rows, slab, C)
    n = (M - torch.arange(rows) * slab).clamp(0, slab).double().view(rows, 1, 1)
    ref = torch.stack([yd.sum(1), (yd * yd).sum(1)], 1)
    mag = torch.stack([yd.abs().sum(1), (yd * yd).sum(1)], 1)
    return ref, (n + 8) * U * mag
