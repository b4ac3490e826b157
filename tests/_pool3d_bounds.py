"""Inputs, a hand-written float64 reference, conditions, DERIVED error bounds and a path table for the kernels between the clip
models' convolutions (csrc/video3d.hip): MaxPool3d (qt_pool3d_max, qt_pool3d_max_bwd), the fused BatchNorm3d + ReLU + MaxPool3d
forward and backward (qt_pool3d_bn_relu_max, qt_pool3d_bn_bwd_apply: the general kernel and the resident-grid one) and the
packers (qt_pack_conv3d_block: element-per-thread and LDS-tile kernel, qt_unpack_conv3d_wgrad, qt_pack_clip27).  Shared by
tests/test_pool3d_gpu.py (the kernels) and tests/test_pool3d_bounds_cpu.py (the reference against torch, a torch-f32 restatement
of every kernel through the same comparisons, the conditions below, the path table, restatements damaged on purpose).

Everything is NHWC, time-major: [T][B][H][W][C].  Kernel = stride = (pool_t, 2, 2), floor mode.  The reference is strided slices
of the window taps, updated with `>` in (t, h, w) scan order (the first maximum wins); no torch pooling is used.

Two input classes:
  grid    y = k / 8 + offset[c], k an integer in [-16, 16], offsets in {0, +-1, +-2, +-6}; scale[c] in {+-1, +-2, +-0.5, 0}, shift
          a multiple of 1/8; mean a multiple of 1/8, invstd a power of two (1, 1/8 or 1/64 of the rounded true one in turn, so
          that dy lies on a 1/512 grid and a bf16 store of it rounds: >= 3 % of the values, >= 1 % exact halves, asserted); coef
          [3][C] dyadic (a in {1, 0.5}, b a multiple of 1/8, c in {1, 2}); d(pooled) a multiple of 1/8, |d| <= 4.  y * scale + shift is exact in f32 (with or without FMA contraction)
          and in bf16 (_stem_bounds.affine_exact), and so is every operation of dy: the reference takes every decision the kernel
          takes and every result is compared BIT FOR BIT, 0 % of the elements left out.  Zero-scale channels: with shift +0.5 all
          taps tie and the recorded code must be 0; with shift -0.5 everything is masked (pooled 0, code 0, gradient 0).
          bf16 runs with C >= 64 also carry eight ROUNDING-TIE channels (TIE_CH): scale 1, shift 8, y one of the 128 bf16 values in
          [0.5, 1).  y + 8 is exact in f32; bf16 collapses it to steps of 2^-4, and the kernel compares the ROUNDED activation
          (`(T)fmaxf(...)`), as the two-kernel form did.  The reference rounds before it compares.
  random  y normal, on the bf16 grid of multiples of 2^-5 with |y| < 8, channel means up to +-6, standard deviations down to 0.25;
          scale / shift as above (decisions still exact, nothing excluded); mean / invstd the true batch statistics and coef the
          float64 BatchNorm-backward coefficients, each rounded to f32 once and handed to kernel and reference alike.  pooled,
          codes, y_at_max, dx and g are still exact (they are selections); dy is compared inside dy_bound().

Conditions (asserted by the builder on the reference alone, for the maps with C >= 64; the maps of cases c2 and c3 hold 8 and 432
windows, too few for a share to mean anything): >= 5 % of the windows of the grid class with a positive maximum attained more
than once, >= 10 % of the windows fully masked, >= 5 % of the windows of the rounding-tie channels whose winner bf16 rounding
changes.

Bound rule: that of tests/_bounds.py (sum_bound / stored / ratio), per output element in float64 on the kernel's own chain.  Every
constant is a chain length read from the kernel or a unit roundoff; nothing is fitted to what a kernel returns.

Shapes (SHAPES) and why:
  c1  T5 B3 H9 W11 C64   the workhorse; pool_t = 2 drops a frame, a row and a column (zero in dx / g, dy = a (-b - xhat c) there);
                         also the narrow-row forms (y_channels 32, dy_channels 32 / 64)
  c2  T=pool_t B1 H2 W2 C8   one window per channel group, one output frame, one 16-byte group per row
  c3  T3 B2 H4 W6 C24    3 groups per row: 256 % 3 != 0, the resident-grid kernel must not be taken even when the threshold is 1
  L1  c1 at C256         resident grid (S = 327 680 threads), n < S: part of the grid idle
  L2  T2 B2 H59 W61 C256 S < n < 2 S: the second row of a trip live for some threads and dead for others
  L3  T3 B2 H59 W61 C256, pool_t 2   2 S < n < 3 S: a second trip whose second row is dead; dropped frame, row and column

The 65 536-block cap of the pool kernels and of qt_pack_clip27 needs more than 16.7 M groups: tests/test_grid_caps_gpu.py reaches
it with build(.., dims=) of a slab of 4099 images per frame, repeated along the batch (the table of tests/_grid_caps.py; pool_t = 1,
the grid class).  NOT reached: QTCNN_PACK3D_TILED=0 and QTCNN_POOL3D_APPLY_LIGHT=0 are read once per process and have no setter."""
import functools

import torch

import _bounds as Bd
import _stem_bounds as Sb

U, F32, BF16 = Bd.U, torch.float32, torch.bfloat16
DTYPES = {"f32": F32, "bf16": BF16}

SHAPES = {  # name: (T (None: pool_t), B, H, W, C)
    "c1": (5, 3, 9, 11, 64), "c2": (None, 1, 2, 2, 8), "c3": (3, 2, 4, 6, 24),
    "L1": (5, 3, 9, 11, 256), "L2": (2, 2, 59, 61, 256), "L3": (3, 2, 59, 61, 256),
}
LIGHT_CASES = [("L1", 1), ("L1", 2), ("L2", 1), ("L3", 2)]
OFFSETS, SCALES = Sb.OFFSETS, Sb.SCALES
TIE_CH = list(range(16, 24))          # one 16-byte group of rounding-tie channels (bf16 grid class, C >= 64)
MIN_TIES, MIN_MASKED, MIN_ROUNDING = 0.05, 0.10, 0.05

# the launchers' constants
LIGHT_THREADS = 1280 * 256            # pool3d_bn_bwd_apply_light_kernel: dim3(256 * 5) blocks of 256
LIGHT_MIN_DEFAULT = 1 << 20           # groups, qt_set_pool3d_apply_light_min(0)
POOL_GRID_CAP = 65536
PACK_GRID_CAP = 4096                  # qt_pack_conv3d_block (element kernel) and qt_unpack_conv3d_wgrad
PK3_TO, PK3_TI = 32, 16


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def shape(name, pt):
    T, B, H, W, C = SHAPES[name]
    return (pt if T is None else T), B, H, W, C


def pooled_shape(T, B, H, W, C, pt):
    return T // pt, B, H // 2, W // 2, C


# ----------------------------------------------------------------------------------------------------------------------
# the float64 reference
# ----------------------------------------------------------------------------------------------------------------------
def tap_code(dt, dh, dw):
    return (dt * 2 + dh) * 2 + dw


def _taps(pt):
    return [(dt, dh, dw) for dt in range(pt) for dh in range(2) for dw in range(2)]


def _slice(t, pt, tap):
    """the positions of window tap (dt, dh, dw) inside the pooled part of a full-size map [T][B][H][W][C]"""
    dt, dh, dw = tap
    To, Ho, Wo = t.shape[0] // pt, t.shape[2] // 2, t.shape[3] // 2
    return t[dt:To * pt:pt, :, dh:Ho * 2:2, dw:Wo * 2:2]


def window_max(act, raw, pt, wins=torch.gt, code=tap_code):
    """MaxPool3d (pt, 2, 2) of act, floor mode: the taps in (t, h, w) scan order, updated with `>` (the first maximum wins).
    Returns the maximum, its tap code (uint8) and `raw` at that tap.  (The CPU test passes torch.ge / another numbering to show
    that both are observable.)"""
    first = _slice(act, pt, (0, 0, 0))
    best = torch.full(first.shape, float("-inf"), dtype=act.dtype)
    idx = torch.zeros(first.shape, dtype=torch.uint8)
    rmax = torch.zeros(first.shape, dtype=raw.dtype)
    for tap in _taps(pt):
        s = _slice(act, pt, tap)
        upd = wins(s, best)
        best = torch.where(upd, s, best)
        idx = torch.where(upd, torch.full_like(idx, code(*tap)), idx)
        rmax = torch.where(upd, _slice(raw, pt, tap), rmax)
    return best, idx, rmax


def scatter(d, idx, pt, full, code=tap_code):
    """max-pool backward: every pooled cell sends d to the position its code names; the floor-mode remainder stays zero"""
    out = torch.zeros(full, dtype=d.dtype)
    for tap in _taps(pt):
        _slice(out, pt, tap).copy_(torch.where(idx == code(*tap), d, torch.zeros((), dtype=d.dtype)))
    return out


def activation(y, scale, shift, dt):
    """relu(y * scale + shift) as the fused kernel compares it: rounded to the activation type"""
    a = (y * scale + shift).clamp_min(0.0)
    return a.to(BF16).double() if dt == BF16 else a


def dy_ref(g, y, mean, invstd, coef):
    ca, cb, cc = coef
    return ca * (g - cb - (y - mean) * invstd * cc)


def sums_ref(g, y, mean, invstd):
    """sum g, sum g * xhat over every position of the full-size map, and the sums of magnitudes the bounds need"""
    t = g * ((y - mean) * invstd)
    red = (0, 1, 2, 3)
    return {"s1": g.sum(red), "s2": t.sum(red), "a1": g.abs().sum(red), "a2": t.abs().sum(red)}


# ----------------------------------------------------------------------------------------------------------------------
# bounds
# ----------------------------------------------------------------------------------------------------------------------
DY_CHAIN = 6   # ca * (g - cb - (y - mean) * invstd * cc): six f32 operations, both apply kernels


def dy_bound(ref, g, y, mean, invstd, coef, dt):
    ca, cb, cc = coef
    mag = ca.abs() * (g.abs() + cb.abs() + ((y - mean) * invstd * cc).abs())
    return Bd.stored(Bd.sum_bound(DY_CHAIN, mag), ref, dt)


def reduce_chain(cells, rows):
    """qt_bn_bwd_reduce over `cells` pooled rows in `rows` partial rows: the rule of tests/test_elementwise_gpu.py"""
    return -(-cells // rows) + 40


# ----------------------------------------------------------------------------------------------------------------------
# the comparisons (the kernels on the GPU and their torch-f32 restatements on the CPU go through the same ones)
# ----------------------------------------------------------------------------------------------------------------------
def same(got, ref):
    """equal by value (-0.0 == +0.0; a NaN left in the buffer equals nothing)"""
    return tuple(got.shape) == tuple(ref.shape) and bool(torch.equal(got.double(), ref.double()))


def forward_failures(c, pooled, code, ymax, Cy=None):
    """the fused forward's three outputs [To][B][Ho][Wo][C] against the reference: channels < Cy bit for bit, zeros above"""
    C = c["shape"][4]
    Cy = C if Cy is None else Cy
    assert same(c["pooled"].to(c["dt"]), c["pooled"])          # the maximum is a value of the activation type: nothing to round
    bad = []
    for name, got, ref in (("pooled", pooled, c["pooled"]), ("argmax", code, c["code"]), ("y_at_max", ymax, c["ymax"])):
        if got is None:
            continue
        if not same(got[..., :Cy], ref[..., :Cy]):
            bad.append(name)
        if not bool((got[..., Cy:] == 0).all()):
            bad.append(name + " padding")
    return bad


def pool_failures(c, pooled, code):
    return [n for n, got, ref in (("pooled", pooled, c["xpooled"]), ("argmax", code, c["xcode"])) if not same(got, ref)]


def dy_check(c, dy, Cy=None, Cd=None):
    """dy [T][B][H][W][Cd] -> (failures, max |err| / bound or None): grid class against ref.to(dt) bit for bit (the store's
    round-to-nearest-even included), random class inside dy_bound(); the channels from Cy up are zero"""
    C = c["shape"][4]
    Cy = C if Cy is None else Cy
    Cd = C if Cd is None else Cd
    bad, r = [], None
    if tuple(dy.shape) != tuple(c["shape"][:4]) + (Cd,):
        return ["dy shape"], None
    ref = c["dy"][..., :Cy]
    if c["kind"] == "grid":
        if not same(dy[..., :Cy], ref.to(c["dt"])):
            bad.append("dy")
    else:
        k = [v[..., :Cy] for v in (c["g"], c["y"], c["mean"], c["invstd"], c["coef"])]
        r = Bd.ratio(dy[..., :Cy], ref, dy_bound(ref, *k, c["dt"]))
        if not r <= 1.0:
            bad.append(f"dy outside its bound ({r:.3f})")
    if not bool((dy[..., Cy:] == 0).all()):
        bad.append("dy padding")
    return bad, r


def bn_sums_ratios(c, part, cells, dgamma, dbeta, coef):
    """the model's chain qt_bn_bwd_reduce (pooled side: dout, pooled, y_at_max over `cells` rows) -> qt_bn_bwd_finalize against
    the float64 sums over the FULL-SIZE map: the partial rows inside the reduce bound, dgamma / dbeta / coef inside the finalize
    bound of the rows the kernel read plus the reduce bound they inherit.  {name: max |err| / bound}"""
    S, (T, B, H, W, C) = c["S"], c["shape"]
    M, rows = T * B * H * W, part.shape[0]
    n = reduce_chain(cells, rows)
    b1, b2 = Bd.sum_bound(n, S["a1"]), Bd.sum_bound(n, S["a2"])
    p = part.double()
    fin = Bd.bwd_finalize_ref(part, M, c["gamma"], c["invstd"], None, None, folded=rows > 1024)
    return {"sum g": Bd.ratio(p[:, 0].sum(0), S["s1"], b1), "sum g xhat": Bd.ratio(p[:, 1].sum(0), S["s2"], b2),
            "dgamma": Bd.ratio(dgamma, S["s2"], fin["dgamma"][1] + b2), "dbeta": Bd.ratio(dbeta, S["s1"], fin["dbeta"][1] + b1),
            "coef0": Bd.ratio(coef[0], c["gamma"] * c["invstd"], fin["coef0"][1]),
            "coef1": Bd.ratio(coef[1], S["s1"] / M, fin["coef1"][1] + b1 / M),
            "coef2": Bd.ratio(coef[2], S["s2"] / M, fin["coef2"][1] + b2 / M)}


# ----------------------------------------------------------------------------------------------------------------------
# which kernel and which of its paths a launch takes (the launchers' own formulas)
# ----------------------------------------------------------------------------------------------------------------------
def apply_groups(T, B, H, W, Cd):
    return T * B * H * W * (Cd // 8)


def light_taken(dt, C, Cy, Cd, n, light_min=LIGHT_MIN_DEFAULT):
    """qt_pool3d_bn_bwd_apply's dispatch"""
    return dt == BF16 and C == Cy and C == Cd and 256 % (C // 8) == 0 and n >= light_min


def light_paths(n, S=LIGHT_THREADS):
    """pool3d_bn_bwd_apply_light_kernel: `for (i = i0; i < n; i += 2 * S)`, rows u = 0, 1 at i + u * S, live[u] = i + u * S < n"""
    i0 = torch.arange(S)
    trips, mixed, dead_second = 0, False, False
    k = 0
    while bool((i0 + 2 * k * S < n).any()):
        live0 = i0 + 2 * k * S < n
        live1 = i0 + (2 * k + 1) * S < n
        trips += 1
        mixed |= bool(live1.any()) and bool((live0 & ~live1).any())
        dead_second |= k >= 1 and not bool(live1.any())
        k += 1
    return {"idle_threads": n < S, "second_row_live": n > S, "second_row_mixed": mixed, "trips": trips,
            "later_trip_second_row_dead": dead_second}


def pool_grid(n):
    return min(max(-(-n // 256), 1), POOL_GRID_CAP)


PACK_TILE = [(64, 64, 32, 64), (40, 64, 48, 64), (128, 128, 64, 64)]          # (O, O_pad, I, I_pad)
PACK_ELEMENT = [(20, 64, 24, 64), (256, 256, 184, 192)]
PACK_FIRST = [(32, 64, 3), (5, 8, 4)]                                          # (O, O_pad, I)


def pack_kernel(O, Op, I, Ip, first, aligned=True):
    """qt_pack_conv3d_block's condition"""
    return "tile" if (not first and Op % 64 == 0 and Ip % 64 == 0 and I % PK3_TI == 0 and aligned) else "element"


def pack_total(Op, Ip, first):
    return (Op * 128 if first else Op * 27 * Ip) + 5 * Op


def grid_strided(total, cap=PACK_GRID_CAP):
    """a grid-stride loop takes a second pass"""
    return total > cap * 256


# ----------------------------------------------------------------------------------------------------------------------
# the packers, restated as plain indexing of the layouts in the kernels' comments
# ----------------------------------------------------------------------------------------------------------------------
VEC_PAD = [0.0, 1.0, 0.0, 0.0, 1.0]    # bias, gamma, beta, running_mean, running_var


def pack_ref(w, Op, Ip, first, vecs):
    """w [O][I][27] -> (wf, wd or None, vec): wf [Op][27][Ip], wd [Ip][27][Op]; first layer: wf [Op][128], K index tap * I + c;
    vec [5][Op], rows padded with VEC_PAD (a missing vector is all pad)"""
    O, I, _ = w.shape
    if first:
        wf = torch.zeros(Op, 128, dtype=w.dtype)
        wf[:O, :27 * I] = w.permute(0, 2, 1).reshape(O, 27 * I)
        wd = None
    else:
        wf = torch.zeros(Op, 27, Ip, dtype=w.dtype)
        wf[:O, :, :I] = w.permute(0, 2, 1)
        wd = torch.zeros(Ip, 27, Op, dtype=w.dtype)
        wd[:I, :, :O] = w.permute(1, 2, 0)
    vec = torch.tensor(VEC_PAD, dtype=torch.float32).view(5, 1).repeat(1, Op)
    for k, v in enumerate(vecs):
        if v is not None:
            vec[k, :O] = v
    return wf, wd, vec


def unpack_ref(dw, O, I, Op, Ip, first):
    """first == 0: dw [3][Op][9][Ip] (one block per frame tap); first == 1: dw [Op][128] -> dW [O][I][27]"""
    if first:
        return dw.view(Op, 128)[:O, :27 * I].reshape(O, 27, I).permute(0, 2, 1).contiguous()
    return dw.view(3, Op, 9, Ip)[:, :O, :, :I].permute(1, 3, 0, 2).reshape(O, I, 27).contiguous()


def forward_operand_as_wgrad(wf, Op, Ip, first):
    """the packed forward operand regrouped the way qt_conv2d_wgrad writes the weight gradient"""
    return wf.view(Op, 128) if first else wf.view(Op, 3, 9, Ip).permute(1, 0, 2, 3).contiguous()


def pack_weights(O, I, seed, integer=False):
    """random f32 weights [O][I][27]; every 50th one sits exactly on a bf16 tie (a bf16 value plus half its unit in the last
    place: round-to-nearest-even and truncation differ on all of them, round-half-away on half)"""
    g = _gen(seed)
    if integer:
        return torch.randint(-100, 101, (O, I, 27), generator=g).float()
    w = torch.randn(O * I * 27, generator=g) * 0.1
    t = w[::50].to(BF16).float().view(torch.int32) | 0x8000
    w[::50] = t.view(torch.float32)
    return w.view(O, I, 27)


def bf16_tie_share(w):
    bits = w.contiguous().view(torch.int32) & 0xFFFF
    return float((bits == 0x8000).double().mean())


def pack_vectors(O, seed):
    g = _gen(seed)
    return [None] + [torch.randn(O, generator=g) for _ in range(4)]     # no bias: a null entry in the pointer table


def clip27_ref(clips):
    """[B][T][3][H][W] -> [T][B][H][W][128]: element ((kt * 3 + kh) * 3 + kw) * 3 + c = x[b][t + kt - 1][c][h + kh - 1][w + kw - 1]"""
    B, T, _, H, W = clips.shape
    xp = torch.zeros(B, T + 2, 3, H + 2, W + 2, dtype=clips.dtype)
    xp[:, 1:T + 1, :, 1:H + 1, 1:W + 1] = clips
    ref = torch.zeros(T, B, H, W, 128, dtype=clips.dtype)
    for kt in range(3):
        for kh in range(3):
            for kw in range(3):
                for c in range(3):
                    ref[..., ((kt * 3 + kh) * 3 + kw) * 3 + c] = xp[:, kt:kt + T, c, kh:kh + H, kw:kw + W].permute(1, 0, 2, 3)
    return ref


CLIP_SHAPES = [(2, 3, 6, 5), (1, 1, 1, 1), (2, 1, 3, 4), (1, 2, 1, 5), (3, 4, 5, 1)]    # (B, T, H, W)


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def channel_tables(C, seed):
    """offset by c % 7, scale by (c // 7) % 7 as the stem tests; zero-scale channels get shift +0.5 / -0.5 in turn (a width
    below 49 has none in the table: its last two channels are made zero-scale)"""
    c = torch.arange(C)
    offset = torch.tensor(OFFSETS, dtype=torch.float64)[c % 7]
    scale = torch.tensor(SCALES, dtype=torch.float64)[(c // 7) % 7]
    shift = torch.randint(-16, 17, (C,), generator=_gen(seed)).double() / 8
    if int((scale == 0).sum()) < 2:
        scale[C - 2:] = 0.0
    zero = torch.nonzero(scale == 0).flatten()
    shift[zero[0::2]], shift[zero[1::2]] = 0.5, -0.5
    return offset, scale, shift


def _statistics(y, exact):
    red = (0, 1, 2, 3)
    m = y.mean(red)
    var = ((y - m) ** 2).mean(red)
    inv = 1.0 / torch.sqrt(var + Bd.EPS)
    if exact:   # a multiple of 1/8 and a power of two
        return torch.round(m * 8) / 8, torch.exp2(torch.round(torch.log2(inv)))
    return m.float().double(), inv.float().double()


def shares(c):
    """shares of windows: positive maximum attained by more than one tap / fully masked (pooled == 0)"""
    hits = torch.zeros(c["pooled"].shape, dtype=torch.int32)
    for tap in _taps(c["pt"]):
        hits += (_slice(c["act"], c["pt"], tap) == c["pooled"]).int()
    return float(((hits > 1) & (c["pooled"] > 0)).double().mean()), float((c["pooled"] == 0).double().mean())


def rounding_share(c):
    """rounding-tie channels: share of windows whose winning tap differs between the rounded and the unrounded activation"""
    raw = (c["y"] * c["scale"] + c["shift"]).clamp_min(0.0)
    _, unrounded, _ = window_max(raw, c["y"], c["pt"])
    return float((unrounded[..., TIE_CH] != c["code"][..., TIE_CH]).double().mean())


def build(kind, name, pt, dtn, dims=None):
    """one (class, shape, pool_t, type): inputs and every reference, float64 on the CPU.  dims: a (T, B, H, W, C) of the caller's
    in place of SHAPES[name], drawn with the name's seed (tests/test_grid_caps_gpu.py: the slab its periodic cases repeat)"""
    dt = DTYPES[dtn]
    T, B, H, W, C = dims or shape(name, pt)
    To, _, Ho, Wo, _ = pooled_shape(T, B, H, W, C, pt)
    seed = {"grid": 1000, "random": 2000}[kind] + 40 * list(SHAPES).index(name) + 4 * pt + (dt == BF16)
    g = _gen(seed)
    offset, scale, shift = channel_tables(C, seed)
    if kind == "grid":
        y = torch.randint(-16, 17, (T, B, H, W, C), generator=g).double() / 8 + offset
        d = torch.randint(-32, 33, (To, B, Ho, Wo, C), generator=g).double() / 8
    else:
        std = 0.25 + 1.75 * torch.rand(C, generator=g, dtype=torch.float64)
        mu = (torch.rand(C, generator=g, dtype=torch.float64) * 2 - 1) * 6
        y = torch.randn((T, B, H, W, C), generator=g, dtype=torch.float64) * std + mu
        y = (torch.round(y * 32) / 32).clamp(-8 + 1 / 32, 8 - 1 / 32)
        d = torch.randn((To, B, Ho, Wo, C), generator=g).to(BF16).double()
    tie = kind == "grid" and dt == BF16 and C >= 64
    plain = torch.ones(C, dtype=torch.bool)
    if tie:
        y[..., TIE_CH] = 0.5 + torch.randint(0, 128, (T, B, H, W, len(TIE_CH)), generator=g).double() / 256
        scale[TIE_CH], shift[TIE_CH] = 1.0, 8.0
        plain[TIE_CH] = False
    assert torch.equal(y.to(BF16).double(), y) and torch.equal(d.to(BF16).double(), d)
    in_f32, _ = Sb.affine_exact(y, scale, shift)
    _, in_bf16 = Sb.affine_exact(y[..., plain], scale[plain], shift[plain])
    assert in_f32 and (in_bf16 or kind == "random"), "y * scale + shift must be exact for EVERY element"
    mean, invstd = _statistics(y, exact=kind == "grid")
    if kind == "grid":   # still a power of two; the smaller ones put (y - mean) * invstd on a 1/512 grid: dy then NEEDS its rounding
        invstd = invstd * torch.exp2(-3.0 * (torch.arange(C) % 3).double())

    act = activation(y, scale, shift, dt)
    pooled, code, ymax = window_max(act, y, pt)
    gcell = torch.where(pooled > 0, d, torch.zeros((), dtype=torch.float64))
    gg = scatter(gcell, code, pt, (T, B, H, W, C))
    S = sums_ref(gg, y, mean, invstd)
    M = T * B * H * W
    if kind == "grid":
        ch = torch.arange(C)
        gamma = None
        coef = torch.stack([torch.tensor([1.0, 0.5], dtype=torch.float64)[ch % 2],
                            torch.randint(-8, 9, (C,), generator=g).double() / 8,
                            torch.tensor([1.0, 2.0], dtype=torch.float64)[(ch // 2) % 2]])
    else:
        gamma = (0.5 + torch.rand(C, generator=g, dtype=torch.float64)) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)
        gamma = gamma.float().double()
        coef = torch.stack([gamma * invstd, S["s1"] / M, S["s2"] / M]).float().double()   # qt_bn_bwd_finalize's [3][C], as f32
    dy = dy_ref(gg, y, mean, invstd, coef)
    if kind == "grid":
        assert torch.equal(dy.float().double(), dy), "every operation of dy must be exact in f32"
        low = dy.float().contiguous().view(torch.int32) & 0xFFFF          # what a bf16 store rounds away
        rounded, halfway = float((low != 0).double().mean()), float((low == 0x8000).double().mean())
        assert C < 64 or (rounded >= 0.03 and halfway >= 0.01), (rounded, halfway)   # round-to-nearest-even shows, ties included
    # the plain pool sees the affine map without the ReLU (negative maxima, no flood of zeros), in the activation type
    x = (y * scale + shift).to(dt).double()
    xpooled, xcode, _ = window_max(x, x, pt)
    dx = scatter(d, xcode, pt, (T, B, H, W, C))
    c = dict(kind=kind, name=name, pt=pt, dt=dt, shape=(T, B, H, W, C), y=y, d=d, scale=scale, shift=shift, mean=mean,
             invstd=invstd, gamma=gamma, coef=coef, act=act, pooled=pooled, code=code, ymax=ymax, g=gg, S=S, dy=dy, x=x,
             xpooled=xpooled, xcode=xcode, dx=dx, tie=tie)
    if C >= 64:
        ties, masked = shares(c)
        c["shares"] = (ties, masked, rounding_share(c) if tie else None)
        assert masked >= MIN_MASKED and (kind != "grid" or ties >= MIN_TIES), c["shares"]
        assert not tie or c["shares"][2] >= MIN_ROUNDING, c["shares"]
    return c


@functools.lru_cache(maxsize=None)
def case(kind, name, pt, dtn):
    """build(), computed once and shared (callers must not write).  The L maps are large: their tests call build() instead."""
    assert not name.startswith("L")
    return build(kind, name, pt, dtn)


def clear_caches():
    case.cache_clear()
