"""Non-finite inputs for the forward kernels: NaN, +inf and -inf planted into the activations of the integer-grid rows of
tests/_exact.py, and the CLASS (finite, NaN, +inf, -inf) every output element must then have.  No GPU code here:
tests/test_nonfinite_gpu.py runs the kernels, tests/test_nonfinite_cpu.py shows that the rule below equals IEEE float64
arithmetic of torch on the CPU.

Rule.  The finite operands are small integers, so no sum of them overflows: the class of an output does not depend on the
order of summation, and a correct kernel must return it.  With the input indicators isnan(x), x == +inf, x == -inf and the
weight indicators w > 0, w < 0, w == 0:
  a term is NaN if its input is NaN, or if its input is infinite and its weight is zero;
  an output is NaN if any of its terms is NaN or if terms of both infinities meet; otherwise it is the infinity present;
  otherwise it is finite -- and then no planted value lies in its receptive field: it equals the clean row's output.
A dyadic scale keeps the class or, when negative, swaps the infinities; a finite shift and residual change nothing; relu
keeps NaN and +inf and sends -inf to (a finite) zero.  Weights, scale, shift and residual stay finite.

The expectation a kernel is compared with is torch's float64 result on the planted operands (`raw`, `pre`, `act`): the
positions of NaN / +inf / -inf must agree exactly, every finite element under the E.same rule of the clean rows.
conditions() asserts, on the reference alone, that a row holds every class in a share of 0.5 % .. 50 % and leaves an image
untouched where there is more than one.

Pool rows (pool_windows_*): windows with one NaN among larger finite values, of NaN only, +inf beside NaN, -inf only; value
and argmax are ATen's, read off F.max_pool*d(..., return_indices=True): a NaN wins every comparison, so the argmax of a
window with NaNs is its LAST NaN in scan order."""
import torch
import torch.nn.functional as F

import _exact as E

FIN, NAN, PINF, NINF = 0, 1, 2, 3
INF = float("inf")
LO, HI = 0.005, 0.5


def classes(t):
    """int8 class of every element"""
    t = t.double()
    c = torch.zeros(t.shape, dtype=torch.int8)
    c[torch.isnan(t)] = NAN
    c[t == INF] = PINF
    c[t == -INF] = NINF
    return c


def plant(x, seed, n_each=3, images=None):
    """a copy of x with n_each NaN, +inf and -inf at seeded, distinct positions inside the first `images` images (dim 0)"""
    x = x.clone()
    n_img = x.shape[0] if images is None else images
    per = x[0].numel()
    pos = torch.randperm(n_img * per, generator=E.gen(seed))[:3 * n_each]
    flat = x.view(-1)
    for j, v in enumerate((float("nan"), INF, -INF)):
        flat[pos[j * n_each:(j + 1) * n_each]] = v
    return x


def _f(b):
    return b.double()


def conv_rule(x, w, s, p):
    """class of conv(x, w) by the rule: float64 convolutions of 0 / 1 indicators, finite arithmetic only"""
    xn, xp, xm = _f(torch.isnan(x)), _f(x == INF), _f(x == -INF)
    wp, wn, wz = _f(w > 0), _f(w < 0), _f(w == 0)
    conv = lambda a, b: E._conv(a, b, s, p)
    nan_terms = conv(xn, torch.ones_like(w)) + conv(xp + xm, wz)
    pos = conv(xp, wp) + conv(xm, wn)
    neg = conv(xp, wn) + conv(xm, wp)
    assert bool(torch.isfinite(nan_terms).all() and torch.isfinite(pos).all() and torch.isfinite(neg).all())
    c = torch.zeros(pos.shape, dtype=torch.int8)
    c[pos > 0] = PINF
    c[neg > 0] = NINF
    c[(nan_terms > 0) | ((pos > 0) & (neg > 0))] = NAN
    return c


def gemm_rule(x, w):
    """x [M][K], w [N][K]: the same rule for y = x w^T"""
    return conv_rule(x.t()[None, :, :, None], w[:, :, None, None], 1, 0)[0, :, :, 0].t()


def scale_rule(c, scale):
    """a non-zero per-channel scale (dim 1): a negative one swaps the infinities"""
    assert bool((scale != 0).all())
    neg = E.bcast(scale < 0, c).expand_as(c)
    out = c.clone()
    out[neg & (c == PINF)] = NINF
    out[neg & (c == NINF)] = PINF
    return out


def relu_rule(c):
    out = c.clone()
    out[c == NINF] = FIN
    return out


def sum_rule(c, dims):
    """class of a sum over `dims` of elements of class c (finite parts cannot overflow)"""
    n, p, m = (_f(c == k).sum(dims) for k in (NAN, PINF, NINF))
    out = torch.zeros(n.shape, dtype=torch.int8)
    out[p > 0] = PINF
    out[m > 0] = NINF
    out[(n > 0) | ((p > 0) & (m > 0))] = NAN
    return out


def square_rule(c):
    out = c.clone()
    out[c == NINF] = PINF
    return out


def conditions(raw_c, pre_c, act, n_img_touched=None):
    """on the reference alone: every class before the ReLU; NaN, +inf and a zero that came from -inf behind it; the share of
    non-finite outputs inside [0.5 %, 50 %]; an untouched image where n_img_touched images of more were planted"""
    for c, what in ((raw_c, "raw"), (pre_c, "pre-activation")):
        for k, name in ((NAN, "NaN"), (PINF, "+inf"), (NINF, "-inf"), (FIN, "finite")):
            assert bool((c == k).any()), f"no {name} among the {what} outputs"
        share = float((c != FIN).double().mean())
        assert LO <= share <= HI, f"share of non-finite {what} outputs {share:.4f} outside [{LO}, {HI}]"
    assert bool(torch.isnan(act).any()) and bool((act == INF).any()) and not bool((act == -INF).any())
    assert bool(((pre_c == NINF) & (act == 0)).any()), "no zero that came from -inf"
    if n_img_touched is not None and n_img_touched < raw_c.shape[0]:
        assert bool((raw_c[n_img_touched:] == FIN).all()) and bool((pre_c[n_img_touched:] == FIN).all())


def finite_equal(got, clean):
    """where `got` is finite it equals `clean` bit for bit (float64)"""
    fin = torch.isfinite(got)
    return torch.equal(got[fin], clean[fin])


# ----------------------------------------------------------------------------------------------------------------------
# rows: (table of tests/_exact.py, row name) -> (seed, planted values of each kind, images planted into).  The seeds were
# searched so that conditions() holds; three values of each kind wherever that can meet the 0.5 % .. 50 % band.  s2_56 takes
# 100 of each: the 1x1 / 2 downsample of 16 images sees one planted pixel in four, each in one of its 12544 output pixels.
# lin_one_tile takes one of each in two of its five rows: a planted value reaches every output of its row (20 % each)
# ----------------------------------------------------------------------------------------------------------------------
def _row(table, name):
    return next(r for r in table if r["name"] == name)


PLANTS = {
    "generic_3x3": (E.FWD_ROWS, 1, 3, 1),
    "generic_1x1_s2": (E.FWD_ROWS, 1, 3, 1),
    "generic_3x3_rounded": (E.FWD_ROWS, 1, 3, 2),
    "ring_b1": (E.FWD_ROWS, 1, 3, 1),
    "pt_7_ragged": (E.FWD_ROWS, 1, 3, 17),
    "pt_14_rounded": (E.FWD_ROWS, 1, 3, 15),
    "taps27": (E.FWD_ROWS, 1, 3, 1),
    "s2_56": (E.S2_ROWS, 1, 100, 15),
    "stem_b1": (E.STEM_ROWS, 1, 3, 1),
    "first_w32": (E.C3F_ROWS, 1, 3, 1),
    "c32_xc32": (E.C32_ROWS, 1, 3, 1),
    "lin_one_tile": (E.LINEAR_ROWS, 3, 1, 2),
}


def row_of(name):
    return _row(PLANTS[name][0], name)


def fwd_case(name):
    """a forward row of FWD_ROWS / STEM_ROWS (no residual, + pooled) with planted activations: clean tensors under 'clean',
    torch-float64 results raw / pre / act (/ pooled), rule classes raw_c / pre_c / act_c"""
    table, seed, n_each, images = PLANTS[name]
    row = _row(table, name)
    stem = table is E.STEM_ROWS
    clean = E.stem_data(row) if stem else E.fwd_data(row)
    _, _, _, _, k, s, p = row["cfg"]
    x = plant(clean["x"], seed, n_each, images)
    w, scale, shift = clean["w"], clean["scale"], clean["shift"]
    raw = E._conv(x, w, s, p)
    pre = raw * E.bcast(scale, raw) + E.bcast(shift, raw)
    if not stem:
        pre = pre + clean["res"]
    c = dict(row=row, clean=clean, x=x, w=w, scale=scale, shift=shift, res=None if stem else clean["res"], raw=raw, pre=pre,
             act=F.relu(pre), images=images)
    c["raw_c"] = conv_rule(x, w, s, p)
    c["pre_c"] = scale_rule(c["raw_c"], scale)
    c["act_c"] = relu_rule(c["pre_c"])
    if stem:
        c["pooled"], c["pooled_idx"] = F.max_pool2d(c["act"], 3, 2, 1, return_indices=True)
    return c


def s2_case(name):
    """the stride-2 pair: conv1 3x3 / 2 (scale / shift / ReLU) and the 1x1 / 2 downsample (scale / shift) of the same input"""
    table, seed, n_each, images = PLANTS[name]
    row = _row(table, name)
    clean = E.s2_data(row)
    x = plant(clean["x"], seed, n_each, images)
    raw, rawd = F.conv2d(x, clean["w"], None, 2, 1), F.conv2d(x, clean["wd"], None, 2, 0)
    pre = raw * E.bcast(clean["sc"], raw) + E.bcast(clean["sh"], raw)
    pred = rawd * E.bcast(clean["sd"], raw) + E.bcast(clean["shd"], raw)
    c = dict(row=row, clean=clean, x=x, raw=raw, rawd=rawd, pre=pre, pred=pred, act=F.relu(pre), images=images)
    c["raw_c"], c["rawd_c"] = conv_rule(x, clean["w"], 2, 1), conv_rule(x, clean["wd"], 2, 0)
    c["pre_c"], c["pred_c"] = scale_rule(c["raw_c"], clean["sc"]), scale_rule(c["rawd_c"], clean["sd"])
    c["act_c"] = relu_rule(c["pre_c"])
    return c


def c3_case(name):
    """a 3-D row (first conv 3 -> 32, slab conv 32 -> 64): conv, scale / shift, ReLU, MaxPool3d((1, 2, 2))"""
    table, seed, n_each, images = PLANTS[name]
    row = _row(table, name)
    cin, cout = (3, 32) if table is E.C3F_ROWS else (32, 64)
    clean = E.c3_data(row, cin, cout)
    x = plant(clean["x"], seed, n_each, images)
    raw = F.conv3d(x, clean["w"], None, 1, 1)
    pre = raw * E.bcast(clean["scale"], raw) + E.bcast(clean["shift"], raw)
    c = dict(row=row, clean=clean, x=x, raw=raw, pre=pre, act=F.relu(pre), images=images)
    c["raw_c"] = conv_rule(x, clean["w"], 1, 1)
    c["pre_c"] = scale_rule(c["raw_c"], clean["scale"])
    c["act_c"] = relu_rule(c["pre_c"])
    c["pooled"], c["pooled_idx"] = F.max_pool3d(c["act"], (1, 2, 2), return_indices=True)
    return c


def gemm_case(name, relu=1):
    """a thin-GEMM row with ReLU: y = relu(x w^T + bias)"""
    table, seed, n_each, images = PLANTS[name]
    row = _row(table, name)
    clean = E.gemm_data(row)
    x = plant(clean["x"], seed, n_each, images)
    raw = x @ clean["w"].t()
    pre = raw + (clean["bias"] if clean["bias"] is not None else 0)
    c = dict(row=row, clean=clean, x=x, raw=raw, pre=pre, act=F.relu(pre) if relu else pre, images=images)
    c["raw_c"] = gemm_rule(x, clean["w"])
    c["pre_c"] = c["raw_c"].clone()
    c["act_c"] = relu_rule(c["pre_c"])
    return c


def stats_classes(raw_c):
    """classes of the per-channel sum and sum of squares of an [N][C][...] map of class raw_c: [2][C]"""
    dims = [d for d in range(raw_c.dim()) if d != 1]
    return torch.stack([sum_rule(raw_c, dims), sum_rule(square_rule(raw_c), dims)])


def stats_ref(raw):
    """the float64 sums themselves (NaN / inf included)"""
    return E.channel_sums(raw)


# ----------------------------------------------------------------------------------------------------------------------
# elementwise and pool rows
# ----------------------------------------------------------------------------------------------------------------------
def bn_act_case(M=96, C=64, seed=11):
    """qt_bn_act: out = relu?(y * scale + shift + (res * rscale + rshift)); y holds the planted values, everything else is
    finite; rows M/2.. are left untouched"""
    g = E.gen(seed)
    y = plant(E.ints((M, C), 8, g), seed, 3, M // 2)
    scale, shift = E.affine(C, g)
    res = E.ints((M, C), 8, g)
    rscale, rshift = E.affine(C, g)
    return dict(y=y, scale=scale, shift=shift, res=res, rscale=rscale, rshift=rshift, y_c=classes(y))


def bn_act_ref(c, residual, relu):
    v = c["y"] * c["scale"] + c["shift"]
    if residual == "plain":
        v = v + c["res"]
    elif residual == "affine":
        v = v + c["res"] * c["rscale"] + c["rshift"]
    rule = scale_rule(c["y_c"], c["scale"])
    return (F.relu(v), relu_rule(rule)) if relu else (v, rule)


def _special_windows(a, windows, g):
    """write the four special window kinds into a map; `windows` yields index tuples of the cells of one window each, in
    scan order.  kinds: one NaN among larger finite values; NaN only; +inf beside NaN (NaN first and NaN last); -inf only"""
    kinds = ("one_nan", "all_nan", "inf_then_nan", "nan_then_inf", "ninf_only", "two_nans")
    for j, cells in enumerate(windows):
        kind = kinds[j % len(kinds)]
        n = len(cells)
        if kind == "one_nan":
            a[cells[int(torch.randint(0, n, (1,), generator=g))]] = float("nan")
        elif kind == "all_nan":
            for i in cells:
                a[i] = float("nan")
        elif kind == "inf_then_nan":
            a[cells[0]], a[cells[n - 1]] = INF, float("nan")
        elif kind == "nan_then_inf":
            a[cells[0]], a[cells[n - 1]] = float("nan"), INF
        elif kind == "ninf_only":
            for i in cells:
                a[i] = -INF
        else:
            a[cells[0]], a[cells[n // 2]] = float("nan"), float("nan")
    return a


def pool3d_case(pt, seed=21, shape=(2, 8, 4, 8, 8)):
    """MaxPool3d((pt, 2, 2)) on x [B][C][T][H][W]: integer values, special windows in image 0 / the first channels"""
    B, C, T, H, W = shape
    g = E.gen(seed + pt)
    x = E.ints(shape, 8, g)
    wins = []
    for j in range(12):
        c, to, ho, wo = j % C, (j // 2) % (T // pt), (j * 3 + j // C) % (H // 2), (j * 5) % (W // 2)
        wins.append([(0, c, to * pt + dt, ho * 2 + dh, wo * 2 + dw) for dt in range(pt) for dh in range(2) for dw in range(2)])
    assert len({w[0] for w in wins}) == len(wins)
    x = _special_windows(x, wins, g)
    out, idx = F.max_pool3d(x, (pt, 2, 2), return_indices=True)
    t, h, w = idx // (H * W), (idx // W) % H, idx % W
    code = ((t % pt) * 2 + h % 2) * 2 + w % 2
    return dict(x=x, out=out, code=code.to(torch.uint8), pt=pt)


def pool3d_fused_case(pt, seed=31, shape=(2, 8, 4, 8, 8)):
    """BatchNorm3d as scale / shift + ReLU + MaxPool3d((pt, 2, 2)) of a raw conv output y with special windows; the planted
    channels get scale +1 so that the window kinds survive the affine (a -inf window pools to relu's 0)"""
    B, C, T, H, W = shape
    c = pool3d_case(pt, seed, shape)
    g = E.gen(seed + 100 + pt)
    scale, shift = E.affine(C, g)
    y = c["x"]
    a = F.relu(y * E.bcast(scale, y) + E.bcast(shift, y))
    out, idx = F.max_pool3d(a, (pt, 2, 2), return_indices=True)
    t, h, w = idx // (H * W), (idx // W) % H, idx % W
    code = ((t % pt) * 2 + h % 2) * 2 + w % 2
    ymax = y.flatten(2).gather(2, idx.flatten(2)).view(out.shape)
    return dict(y=y, scale=scale, shift=shift, act=a, out=out, code=code.to(torch.uint8), ymax=ymax, pt=pt)


def stem_pool_case(seed=41, B=2):
    """qt_stem_pool: relu(y * scale + shift) on [B][64][112][112], 3x3 / 2 pad 1 max pool, argmax position kh * 3 + kw and
    y at the argmax.  Special windows sit in image 0 (the border windows (0, 0) and (55, 55) among them)"""
    C, H, P = 64, 112, 56
    g = E.gen(seed)
    y = E.ints((B, C, H, H), 8, g)
    scale, shift = E.affine(C, g)
    wins = []
    for j in range(12):
        c = j * 5 % C
        ph, pw = ((0, 0), (55, 55))[j] if j < 2 else (3 + (j * 7) % 50, 2 + (j * 11) % 50)
        cells = [(0, c, h, w) for h in range(ph * 2 - 1, ph * 2 + 2) for w in range(pw * 2 - 1, pw * 2 + 2) if 0 <= h < H and 0 <= w < H]
        wins.append(cells)
    y = _special_windows(y, wins, g)
    a = F.relu(y * E.bcast(scale, y) + E.bcast(shift, y))
    out, idx = F.max_pool2d(a, 3, 2, 1, return_indices=True)
    h, w = idx // H, idx % H
    ph = torch.arange(P).view(1, 1, P, 1)
    pw = torch.arange(P).view(1, 1, 1, P)
    code = (h - (2 * ph - 1)) * 3 + (w - (2 * pw - 1))
    ymax = y.flatten(2).gather(2, idx.flatten(2)).view(out.shape)
    return dict(y=y, scale=scale, shift=shift, act=a, out=out, code=code.to(torch.uint8), ymax=ymax)


def quad_pool_case(seed=51, B=2):
    """qt_quad_pool: MaxPool2d(2, 2) (floor: 7 -> 3) of q [B * 4][128][7][7], flattened in NCHW order per quadrant"""
    g = E.gen(seed)
    q = E.ints((B * 4, 128, 7, 7), 8, g)
    wins = []
    for j in range(12):
        c, ph, pw = j * 9 % 128, j % 3, (j // 3) % 3
        wins.append([(j % 4, c, ph * 2 + dh, pw * 2 + dw) for dh in range(2) for dw in range(2)])
    q = _special_windows(q, wins, g)
    out = F.max_pool2d(q, 2, 2)
    return dict(q=q, out=out, flat=out.reshape(B, 4 * 128 * 9))


def pool_conditions(x_windows_out):
    """a pool row's pooled reference holds NaN, +inf and -inf or (behind a ReLU) the zero of a -inf window"""
    out = x_windows_out
    assert bool(torch.isnan(out).any()) and bool(torch.isfinite(out).any())


def signed_zero_stem_case(seed=61):
    """the fused stem pool on a channel with scale -1 and shift -0.0 whose conv output is exactly 0 next to positive
    neighbours: pre = 0 * -1 + -0.0 = -0.0; a ReLU that lets -0.0 (bf16 0x8000) through must not win a maximum taken on
    16-bit patterns.  Returns the stem row's tensors with that channel's epilogue replaced"""
    row = _row(E.STEM_ROWS, "stem_b1")
    c = E.stem_data(row)
    raw = c["raw"]
    # the channel with the most exact zeros that have a positive-after-ReLU neighbour under scale -1
    zeros = (raw == 0).flatten(2).sum(2)[0]
    ch = int(zeros.argmax())
    scale, shift = c["scale"].clone(), c["shift"].clone()
    scale[ch], shift[ch] = -1.0, -0.0
    pre = raw * E.bcast(scale, raw) + E.bcast(shift, raw)
    act = F.relu(pre)
    pooled = F.max_pool2d(act, 3, 2, 1)
    return dict(row=row, x=c["x"], w=c["w"], raw=raw, scale=scale, shift=shift, pre=pre, act=act, pooled=pooled, channel=ch)


def signed_zero_conditions(c):
    ch, pre = c["channel"], c["pre"]
    neg0 = (pre[0, ch] == 0) & torch.signbit(pre[0, ch])
    assert bool(neg0.any()), "no -0.0 pre-activation"
    # some pooled window holds a -0.0 and a positive value: the positive value is the maximum
    has_neg0 = F.max_pool2d(neg0.double()[None, None], 3, 2, 1)[0, 0] > 0
    assert bool((has_neg0 & (c["pooled"][0, ch] > 0)).any()), "no window with -0.0 beside a positive neighbour"


# ----------------------------------------------------------------------------------------------------------------------
# qt_bn_finalize on partial sums that hold NaN / +-inf
# ----------------------------------------------------------------------------------------------------------------------
def finalize_case(rows=5, C=16, seed=71):
    """partial [rows][2][C] (sum, sum of squares) of `count` values per channel; channels 0..5 hold non-finite sums
    (NaN sum; NaN squares; +inf sum and squares; -inf sum, +inf squares; both infinities among the rows; +inf squares only)"""
    g = E.gen(seed)
    count = 64 * rows
    v = torch.randn(rows, 64, C, generator=g, dtype=torch.float64)
    partial = torch.stack([v.sum(1), (v * v).sum(1)], 1).float()
    nan = float("nan")
    partial[1, 0, 0] = nan
    partial[2, 1, 1] = nan
    partial[0, 0, 2], partial[0, 1, 2] = INF, INF
    partial[3, 0, 3], partial[3, 1, 3] = -INF, INF
    partial[0, 0, 4], partial[4, 0, 4], partial[0, 1, 4] = INF, -INF, INF
    partial[2, 1, 5] = INF
    gamma = 0.5 + torch.rand(C, generator=g, dtype=torch.float64)
    beta = torch.randn(C, generator=g, dtype=torch.float64)
    rmean = torch.randn(C, generator=g, dtype=torch.float64)
    rvar = 0.5 + torch.rand(C, generator=g, dtype=torch.float64)
    return dict(partial=partial, count=count, gamma=gamma.float(), beta=beta.float(), rmean=rmean.float(), rvar=rvar.float())


def finalize_ref(c, momentum=0.1, eps=1e-5):
    """float64 restatement of train-mode BatchNorm's statistics from the partial sums: mean = s1 / n, var = s2 / n - mean^2
    (clamped at 0 as the kernel does for finite values; a NaN stays), invstd, scale = gamma invstd, shift = beta - mean scale,
    running statistics with the unbiased variance"""
    p = c["partial"].double()
    n = c["count"]
    s1, s2 = p[:, 0].sum(0), p[:, 1].sum(0)
    mean = s1 / n
    var = s2 / n - mean * mean
    var = torch.where(var < 0, torch.zeros_like(var), var)      # (a NaN compares false and stays)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = c["gamma"].double() * invstd
    shift = c["beta"].double() - mean * scale
    rm = (1 - momentum) * c["rmean"].double() + momentum * mean
    rv = (1 - momentum) * c["rvar"].double() + momentum * var * (n / (n - 1))
    return dict(mean=mean, invstd=invstd, scale=scale, shift=shift, running_mean=rm, running_var=rv)
