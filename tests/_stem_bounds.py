"""Inputs, a hand-written float64 reference and DERIVED error bounds for the stem tail: bn1 -> ReLU -> MaxPool2d(3, 2, 1) on
conv1's output, its backward, and the one-launch stem backward that contracts d(loss)/d(conv1 output) with the packed image
(qt_stem_pool, qt_stem_pool_bwd, qt_stem_bn_bwd_reduce / _sums / _apply in csrc/elementwise.hip, qt_stem_bn_bwd_wgrad_ws in
csrc/conv_wgrad.hip).  Shared by tests/test_stem_tail_gpu.py (the kernels) and tests/test_stem_bounds_cpu.py (the reference
against torch, a torch-f32 restatement of every kernel inside every bound, the conditions below, the path table).

Geometry is fixed at compile time (112 x 112 x 64 -> 56 x 56 x 64, packed image [B][230][232][4]); the batch is the only free
shape.  BATCHES = 1, 3, 11: 11 is the smallest batch at which the one-launch backward gives a workgroup three tiles (both LDS
buffers reused), lets a workgroup cross an image boundary, puts a last-row tile (rp == 55, whose second pooled row is not
loaded) into a reused buffer, caps the grids of the reduce (2048) and sums (1024) kernels and takes the tail of the light sums
kernel's two-element loop (paths(): the kernels' own formulas, asserted by the CPU test).  Not covered here but in
tests/test_grid_caps_gpu.py (the table of tests/_grid_caps.py): the 16384-block cap of qt_stem_pool_bwd (B = 42) and of
qt_stem_pool / qt_stem_bn_bwd_apply (B = 168), on the three images of case(kind, 3) repeated, and the back edge of the light
sums kernel's two-element loop (B = 16).  The bf16 instantiation of the general sums kernel is reachable only through a
process-wide environment switch that is read once; it is left out.

Two input classes, everything NHWC:
  grid    y = k / 8 + offset[c], k an integer in [-16, 16], offsets in {0, +-1, +-2, +-6}; scale[c] in {+-1, +-2, +-0.5, 0},
          shift[c] a multiple of 1/8 in [-2, 2]; d(pooled) a multiple of 1/8, |d| <= 4; mean a multiple of 1/8, invstd a power
          of two.  y * scale + shift is exact in f32 (with or without FMA contraction) AND in bf16, windows hold many positive
          ties, whole channels are masked, two zero-scale channels tie all nine taps.  Every decision and every sum of the
          forward, of g and of the BatchNorm-backward sums is exact: results are compared bit for bit.
  random  y normal with channel means up to +-6 and standard deviations down to 0.25, on the bf16 grid of multiples of 2^-5
          with |y| < 8; scale / shift drawn like the grid class, so that y * scale + shift is still exact in f32 and the
          float64 reference takes the very decisions the kernel takes (no position is excluded at comparison time; an inexact
          element fails the builder); mean / invstd are the true batch statistics and coef the float64 BatchNorm-backward
          coefficients, each rounded to f32 once and handed to kernel and reference alike.  Compared inside bounds.

Bound rule: that of tests/_bounds.py (sum_bound / stored), evaluated per output element in float64 on the kernel's own chain of
operations.  Every constant below is a chain length read from the kernel, or a unit roundoff.  Nothing is fitted to what a
kernel returns."""
import functools

import torch

import _bounds as Bd

BATCHES = [1, 3, 11]
H = W = 112
P = 56
C = 64
NT = 56                      # tiles (pairs of conv1 rows) per image in the one-launch backward
U, F32, BF16 = Bd.U, torch.float32, torch.bfloat16

# channel tables: offset by c % 7, scale by (c // 7) % 7; 49 <= c < 64 repeats the start of the table with other shifts
OFFSETS = [0.0, 1.0, -1.0, 2.0, -2.0, 6.0, -6.0]
SCALES = [1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 0.0]
ZERO_POS, ZERO_NEG = 42, 43  # zero-scale channels with shift +0.5 (all nine taps tie at 0.5) and -0.5 (everything masked)
FIRST_VALID_TAP = {"interior": 0, "top": 3, "left": 1, "corner": 4}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def channel_tables(seed):
    c = torch.arange(C)
    offset = torch.tensor(OFFSETS, dtype=torch.float64)[c % 7]
    scale = torch.tensor(SCALES, dtype=torch.float64)[(c // 7) % 7]
    shift = torch.randint(-16, 17, (C,), generator=_gen(seed)).double() / 8
    shift[ZERO_POS], shift[ZERO_NEG] = 0.5, -0.5
    assert scale[ZERO_POS] == 0 and scale[ZERO_NEG] == 0
    return offset, scale, shift


def affine_exact(y, scale, shift):
    """y * scale + shift as the kernels form it: the same value from f32 multiply-then-add, from one fused multiply-add
    (float64 of f32 operands rounded once) and from float64.  Returns (all elements exact in f32, all exact in bf16)."""
    yf, sf, hf = y.float(), scale.float(), shift.float()
    assert torch.equal(yf.double(), y) and torch.equal(sf.double(), scale) and torch.equal(hf.double(), shift)
    v = y * scale + shift
    two = (yf * sf + hf).double()
    fma = v.float().double()
    in_f32 = bool(torch.equal(two, v)) and bool(torch.equal(fma, v))
    return in_f32, in_f32 and bool(torch.equal(v.to(BF16).double(), v))


# ----------------------------------------------------------------------------------------------------------------------
# the float64 reference
# ----------------------------------------------------------------------------------------------------------------------
def forward_ref(y, scale, shift, wins=torch.gt):
    """relu(y * scale + shift) -> MaxPool2d(3, 2, 1): nine strided slices of the -inf padded map, updated with `>` in scan
    order (the first maximum wins; taps outside the map never win).  y [B][112][112][64] float64.
    Returns act, pooled, code (kh * 3 + kw, uint8), y_at_max."""
    B = y.shape[0]
    act = (y * scale + shift).clamp_min(0.0)
    ap = torch.full((B, H + 2, W + 2, C), float("-inf"), dtype=torch.float64)
    ap[:, 1:H + 1, 1:W + 1] = act
    yp = torch.zeros((B, H + 2, W + 2, C), dtype=torch.float64)
    yp[:, 1:H + 1, 1:W + 1] = y
    best = torch.full((B, P, P, C), float("-inf"), dtype=torch.float64)
    code = torch.zeros((B, P, P, C), dtype=torch.uint8)
    ymax = torch.zeros((B, P, P, C), dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            s = ap[:, kh:kh + H:2, kw:kw + W:2]
            upd = wins(s, best)   # (the CPU test swaps in torch.ge to show that the tie rule is observable)
            best = torch.where(upd, s, best)
            code = torch.where(upd, torch.full_like(code, kh * 3 + kw), code)
            ymax = torch.where(upd, yp[:, kh:kh + H:2, kw:kw + W:2], ymax)
    return act, best, code, ymax


def gather_ref(d, code, act):
    """g[n][h][w][c] = (act > 0) * sum of the <= 4 pooled cells whose code points at (h, w); also the sum of |d| behind it"""
    B = d.shape[0]
    gp = torch.zeros((B, H + 2, W + 2, C), dtype=d.dtype)   # (float64 for the reference; the CPU test restates it in f32)
    ga = torch.zeros_like(gp)
    for kh in range(3):
        for kw in range(3):
            hit = torch.where(code == kh * 3 + kw, d, torch.zeros_like(d))
            gp[:, kh:kh + H:2, kw:kw + W:2] += hit
            ga[:, kh:kh + H:2, kw:kw + W:2] += hit.abs()
    on = act > 0
    zero = torch.zeros((), dtype=d.dtype)
    return torch.where(on, gp[:, 1:H + 1, 1:W + 1], zero), torch.where(on, ga[:, 1:H + 1, 1:W + 1], zero)


def sums_ref(g, y, mean, invstd):
    """sum g, sum g * xhat over positions, and the magnitudes the bounds need: sum |g|, sum |g xhat|, sum |g y|"""
    t = g * ((y - mean) * invstd)
    red = (0, 1, 2)
    return {"s1": g.sum(red), "s2": t.sum(red), "a1": g.abs().sum(red), "a2": t.abs().sum(red), "agy": (g * y).abs().sum(red)}


def dy_ref(g, y, mean, invstd, coef):
    ca, cb, cc = coef
    return ca * (g - cb - (y - mean) * invstd * cc)


def to_nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def wgrad_ref(image, dy):
    """conv1's weight gradient [64][3][7][7] (float64) from dy [B][112][112][64] and the image [B][3][224][224]"""
    return torch.nn.grad.conv2d_weight(image, (C, 3, 7, 7), to_nchw(dy), stride=2, padding=3)


def pack_image(image, dt):
    """[B][3][224][224] -> the packed [B][230][232][4] input of the stem (3 rows / columns of zeros in front, channel 3 zero)"""
    B = image.shape[0]
    x = torch.zeros((B, 230, 232, 4), dtype=dt)
    x[:, 3:227, 3:227, :3] = image.permute(0, 2, 3, 1).to(dt)
    return x


def pack_wgrad(dw):
    """OIHW [64][3][7][7] -> the kernel's [64][7][8][4]: (kh, kw, c); kw == 7 and c == 3 are not part of the filter"""
    out = torch.zeros((C, 7, 8, 4), dtype=dw.dtype)
    out[:, :, :7, :3] = dw.permute(0, 2, 3, 1)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# bounds
# ----------------------------------------------------------------------------------------------------------------------
def g_bound(g, gabs, dt):
    """qt_stem_pool_bwd: at most four f32 additions, one store"""
    return Bd.stored(Bd.sum_bound(4, gabs), g, dt)


def _per_thread(total, grid):
    return -(-total // (grid * 256))


def reduce_rows(B):
    return min(-(-B * H * W * 8 // 256), 2048)


def sums_rows(B):
    return min(-(-B * P * P * 8 // 256), 1024)


def chain_reduce(B):
    """stem_pool_bwd_kernel<T, 1>: positions per thread (8 channels each), the <= 4 additions of the gather and the 3
    operations of g * (y - mean) * invstd in front of them, the 32 rows of the block's table"""
    return _per_thread(B * H * W * 8, reduce_rows(B)) + 4 + 3 + 32


def chain_sums(B):
    """stem_bn_bwd_sums_kernel: cells per thread (8 channels each), the 3 operations of a term, 32 rows"""
    return _per_thread(B * P * P * 8, sums_rows(B)) + 3 + 32


def chain_light(B):
    """stem_bn_bwd_sums_light_kernel: cells per thread (4 channels each), the correction (2 operations), 2 butterfly steps and
    the sum of 4 waves (3 additions, counted as 4 steps with the product of a term)"""
    return _per_thread(B * P * P * 16, sums_rows(B)) + 2 + 4


def sums_bound(S, n):
    return Bd.sum_bound(n, S["a1"]), Bd.sum_bound(n, S["a2"])


def light_bound(S, n, mean, invstd):
    """(sum g v - mean sum g) invstd: the errors of the two cancelling sums are scaled by invstd and do not cancel"""
    b1, b2 = sums_bound(S, n)
    return b1, b2 + (S["agy"] + mean.abs() * S["a1"]) * invstd * (n + 8) * U


DY_CHAIN = 6   # both forms: no operand of dy passes through more than six f32 roundings


def dy_bound(ref, g, y, mean, invstd, coef, dt):
    """stem_bn_bwd_apply2x2_kernel: ca * (g - cb - (y - mean) * invstd * cc)"""
    ca, cb, cc = coef
    mag = ca.abs() * (g.abs() + cb.abs() + ((y - mean) * invstd * cc).abs())
    return Bd.stored(Bd.sum_bound(DY_CHAIN, mag), ref, dt)


def dy_bound_folded(ref, g, y, mean, invstd, coef, dt):
    """the one-launch backward: k1 g - k3 y + k4 with k1 = ca, k3 = ca invstd cc, k4 = k3 mean - ca cb (two fused
    multiply-adds per element): |k3 y| and |k3 mean| in place of |ca xhat cc|"""
    ca, cb, cc = coef
    k3 = ca * invstd * cc
    mag = (ca * g).abs() + (k3 * y).abs() + (k3 * mean).abs() + (ca * cb).abs()
    return Bd.stored(Bd.sum_bound(DY_CHAIN, mag), ref, dt)


def wgrad_chain(B):
    """pixels one workgroup adds into an accumulator (tiles per workgroup x 224) + the sum of <= 256 partial filters"""
    grid = min(B * NT, 256)
    most = max((b + 1) * B * NT // grid - b * B * NT // grid for b in range(grid))
    return most * 224 + 256


def wgrad_bound(image, dy, dyb, B):
    """sum over pixels of |x| * (bound of dy at the pixel: the bf16 rounding of the gradient tile goes straight into the
    products) + the f32 summation of the exact products"""
    xa = image.abs()
    return wgrad_ref(xa, dyb) + Bd.sum_bound(wgrad_chain(B), wgrad_ref(xa, dy.abs()))


# ----------------------------------------------------------------------------------------------------------------------
# which paths a batch reaches (the kernels' own formulas)
# ----------------------------------------------------------------------------------------------------------------------
def tile_ranges(B):
    """stem_wgrad_rows_kernel: t_beg = b * ntiles / grid, t_end = (b + 1) * ntiles / grid over min(ntiles, 256) workgroups"""
    nt = B * NT
    grid = min(nt, 256)
    return [(b * nt // grid, (b + 1) * nt // grid) for b in range(grid)]


def paths(B):
    r = tile_ranges(B)
    total4 = B * P * P * 16
    stride = sums_rows(B) * 256
    # stem_bn_bwd_sums_light_kernel: `for (; i + stride < total4; i += 2 * stride)` then `if (i < total4)`, for every thread
    i0 = torch.arange(stride)
    trips = ((total4 - i0 - stride + 2 * stride - 1) // (2 * stride)).clamp_min(0)
    tail = bool((i0 + trips * 2 * stride < total4).any())
    return {
        "three_tiles": any(e - b >= 3 for b, e in r),
        "crosses_image": any(t % NT == NT - 1 and t + 1 < e for b, e in r for t in range(b, e)),
        "last_row_in_reused_buffer": any(t % NT == NT - 1 and t - b >= 2 for b, e in r for t in range(b, e)),
        "reduce_capped": -(-B * H * W * 8 // 256) > 2048,
        "sums_capped": -(-B * P * P * 8 // 256) > 1024,
        "light_tail": tail,
    }


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def _statistics(y, exact):
    m = y.mean((0, 1, 2))
    var = ((y - m) ** 2).mean((0, 1, 2))
    inv = 1.0 / torch.sqrt(var + Bd.EPS)
    if exact:   # a multiple of 1/8 and a power of two
        return torch.round(m * 8) / 8, torch.exp2(torch.round(torch.log2(inv)))
    return m.float().double(), inv.float().double()


def _build(kind, B):
    g = _gen({"grid": 500, "random": 600}[kind] + B)
    offset, scale, shift = channel_tables(7 if kind == "grid" else 8)
    if kind == "grid":
        y = torch.randint(-16, 17, (B, H, W, C), generator=g).double() / 8 + offset
        d = torch.randint(-32, 33, (B, P, P, C), generator=g).double() / 8
    else:
        std = 0.25 + 1.75 * torch.rand(C, generator=g, dtype=torch.float64)
        mu = (torch.rand(C, generator=g, dtype=torch.float64) * 2 - 1) * 6
        y = torch.randn((B, H, W, C), generator=g, dtype=torch.float64) * std + mu
        y = (torch.round(y * 32) / 32).clamp(-8 + 1 / 32, 8 - 1 / 32)
        d = torch.randn((B, P, P, C), generator=g).to(BF16).double()
    assert torch.equal(y.to(BF16).double(), y) and torch.equal(d.to(BF16).double(), d)
    in_f32, in_bf16 = affine_exact(y, scale, shift)
    assert in_f32 and (in_bf16 or kind == "random"), "y * scale + shift must be exact for EVERY element"
    mean, invstd = _statistics(y, exact=kind == "grid")
    gamma = (0.5 + torch.rand(C, generator=g, dtype=torch.float64)) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)
    act, pooled, code, ymax = forward_ref(y, scale, shift)
    gg, gabs = gather_ref(d, code, act)
    S = sums_ref(gg, y, mean, invstd)
    M = B * H * W
    coef = torch.stack([gamma * invstd, S["s1"] / M, S["s2"] / M]).float().double()   # qt_bn_bwd_finalize's [3][C], as f32
    dy = dy_ref(gg, y, mean, invstd, coef)
    return dict(kind=kind, B=B, y=y, d=d, scale=scale, shift=shift, mean=mean, invstd=invstd, gamma=gamma, coef=coef, act=act,
                pooled=pooled, code=code, ymax=ymax, g=gg, gabs=gabs, S=S, dy=dy, exact_bf16=in_bf16)


@functools.lru_cache(maxsize=None)
def case(kind, B):
    """one (class, batch): inputs and every reference, float64 on the CPU, computed once and shared (callers must not write)"""
    return _build(kind, B)


@functools.lru_cache(maxsize=None)
def dense_wgrad(B):
    """random class: bf16-representable image, conv1's weight gradient of the reference dy and its bound.  Both forms are held
    to ONE bound: the folded form's bound of dy dominates the apply kernel's (|k3 y| + |k3 mean| >= |k3 (y - mean)|) up to the
    float64 rounding of the two expressions where y and mean have opposite signs, so the larger of the two is taken"""
    c = case("random", B)
    image = torch.randn((B, 3, 224, 224), generator=_gen(700 + B)).to(BF16).double()
    dyb = torch.maximum(dy_bound_folded(c["dy"], c["g"], c["y"], c["mean"], c["invstd"], c["coef"], BF16),
                        dy_bound(c["dy"], c["g"], c["y"], c["mean"], c["invstd"], c["coef"], BF16))
    return image, wgrad_ref(image, c["dy"]), wgrad_bound(image, c["dy"], dyb, B)


def consistent_case(B):
    """random-class y with gamma / beta of both signs and the TRUE float64 statistics: scale = gamma invstd, shift = beta -
    mean scale, as a training step has them (reference against autograd only; nothing here goes to a kernel)"""
    g = _gen(800 + B)
    y = case("random", B)["y"]
    gamma = (0.5 + torch.rand(C, generator=g, dtype=torch.float64)) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)
    beta = torch.randn(C, generator=g, dtype=torch.float64) * 0.5
    d = torch.randn((B, P, P, C), generator=g, dtype=torch.float64)
    m = y.mean((0, 1, 2))
    inv = 1.0 / torch.sqrt(((y - m) ** 2).mean((0, 1, 2)) + Bd.EPS)
    return y, d, gamma, beta, m, inv


def clear_caches():
    """the cached cases hold about 1.5 GB of float64 maps: the test modules drop them when they are done"""
    for f in (case, dense_wgrad, sparse_probe):
        f.cache_clear()


# ----------------------------------------------------------------------------------------------------------------------
# grid-class conditions and the sparse probe
# ----------------------------------------------------------------------------------------------------------------------
def grid_shares(c):
    """shares of pooled cells: positive maximum attained by more than one tap / positive maximum / maximum exactly 0"""
    B = c["B"]
    ap = torch.full((B, H + 2, W + 2, C), float("-inf"), dtype=torch.float64)
    ap[:, 1:H + 1, 1:W + 1] = c["act"]
    hits = torch.zeros((B, P, P, C), dtype=torch.int32)
    for kh in range(3):
        for kw in range(3):
            hits += (ap[:, kh:kh + H:2, kw:kw + W:2] == c["pooled"]).int()
    pos = c["pooled"] > 0
    return (float(((hits > 1) & pos).double().mean()), float(pos.double().mean()), float((c["pooled"] == 0).double().mean()))


PROBE_VALUES = [0.5, -0.5, 1.0, -1.0, 2.0, -2.0]


@functools.lru_cache(maxsize=None)
def sparse_probe(B):
    """grid class, coef = (1, 0, 0): dy = g exactly.  d(pooled) is zero except ONE cell per tile of the one-launch backward (B * 56
    cells): for tile (image, rp) a cell whose recorded maximum lies in conv rows 2 rp, 2 rp + 1 -- in pooled row rp with a tap of
    window row 1 or 2, or (rp % 3 == 2, rp < 55) in pooled row rp + 1 with a tap of window row 0 -- at varying columns, in a
    channel of positive scale, with a positive activation, value from PROBE_VALUES.  Tile 53's cell is of the second form: it
    sits in pooled row 54 and also has a positive activation four conv rows below its maximum, where a stale copy of row 54 read
    as the missing row 56 by the rp == 55 tile would put it.  The image is on a 1/8 grid (|x| <= 4): every filter element is a
    short sum of exact products: bit for bit.  Returns d, coef, image, dw [64][3][7][7], the cells."""
    c = case("grid", B)
    g = _gen(900 + B)
    code, pooled, act, scale = c["code"], c["pooled"], c["act"], c["scale"]
    chans = torch.nonzero(scale > 0).flatten()
    d = torch.zeros((B, P, P, C), dtype=torch.float64)
    cells = []
    for n in range(B):
        for rp in range(NT):
            below = rp % 3 == 2 and rp < NT - 1
            row = rp + 1 if below else rp
            kk = code[n, row][:, chans].long()                                  # [56][channels]
            ok = (pooled[n, row][:, chans] > 0) & ((kk // 3 == 0) if below else (kk // 3 >= 1))
            if below:   # active four conv rows further down as well (column of the maximum, same channel)
                hh = 2 * row - 1 + 4
                ww = (2 * torch.arange(P).view(P, 1) - 1 + kk % 3).clamp(0, W - 1)
                ok &= act[n, hh][:, chans].gather(0, ww) > 0 if hh < H else True
            cand = torch.nonzero(ok)
            assert len(cand) >= 8, (n, rp)
            want = (37 * rp + 11 * n) % P                                         # columns vary over 0 .. 55
            b, ci = cand[torch.argmin((cand[:, 0] - want).abs() * 64 + (cand[:, 1] - (rp + n) % len(chans)).abs())].tolist()
            d[n, row, b, chans[ci]] = PROBE_VALUES[int(torch.randint(0, 6, (1,), generator=g))]
            cells.append((n, rp, row, b, int(chans[ci]), int(code[n, row, b, chans[ci]])))
    coef = torch.stack([torch.ones(C), torch.zeros(C), torch.zeros(C)]).double()
    image = torch.randint(-32, 33, (B, 3, 224, 224), generator=g).double() / 8
    gg, _ = gather_ref(d, code, act)
    assert int((gg != 0).sum()) == B * NT                                        # every cell reaches its position
    rows = torch.nonzero(gg.abs().sum((2, 3)))                                   # (image, conv row) pairs that hold a gradient
    assert sorted({(int(n), int(h) // 2) for n, h in rows}) == [(n, rp) for n in range(B) for rp in range(NT)]
    return d, coef, image, wgrad_ref(image, gg), cells
