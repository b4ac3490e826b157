"""Integer-grid data for BIT-EXACT convolution tests, the conditions that make the exactness argument hold, and the case
tables.  No GPU code here: tests/test_conv_exact_gpu.py runs the kernels on these rows, tests/test_exact_data_cpu.py runs a
torch-f32 stand-in on the same rows (the expectations are reachable by correct f32 arithmetic in any order, and every listed
kind of damage is caught).

Argument.  Operands are small integers (exact in bf16 and f32), so every product is an integer.  If for an output element
sum_i |term_i| <= 2^24, every partial sum of its terms, in ANY order and grouping (K-chunks, split-K partials, f32 atomics, the
accumulators of an MFMA), is an integer of magnitude <= 2^24 and therefore exact in f32: every correct kernel returns the same
bits as the float64 reference.  The epilogue keeps this: a dyadic per-channel scale (+-1, 2, 0.5), an integer shift and an
integer residual give multiples of 0.5 far below 2^24.
  mode A ("representable"): the float64 reference is itself representable in the output type: expected = ref.
  mode B ("rounded", bf16 outputs only): larger magnitudes; the f32 value is still exact and many values sit on a bf16 tie:
  expected = ref.to(bfloat16), one round-to-nearest-even of an exactly known value.
conditions() asserts all of it on the reference alone, before a kernel result is looked at.

The rows cover: every 2-D convolution path forward, data gradient and weight gradient (generic tiles, ring, patch-resident,
stride-2 pair and parity classes, region rows), the packed stem and its gradients, the thin GEMMs, and the 3-D convolutions
of the clip models.  Rows with a field `walk` = n are shapes at which a persistent kernel's capped grid gives EVERY workgroup
at least n work items (item, item + grid, ...): the state that survives from one item to the next -- the LDS ring of frame
slabs, the register prefetch of the next item's first slab or tile, the per-workgroup statistics rows and partial filters --
is then part of the result.  The GPU test asserts that precondition from the grid the library reports; walk_items() is the
same walk on the host for the CPU twin.  The stem and layer-1 ring kernels split their tiles into CONTIGUOUS shares instead
(share_items(), share_facts(); the rows stem_walk, stem_pool_walk, stem_wgrad_walk, ring_walk): what their state holds from
tile to tile -- two input buffers, a sliding window of 640 rows with a 48-row mirror, the conv tile of the fused pool --
depends on a tile's place in its workgroup's share and in its image, and WALKS records what each row reaches."""

import torch
import torch.nn.functional as F

CAP = 2.0 ** 24
BF, F32 = torch.bfloat16, torch.float32


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------------------------------------------------------------------
# generators (float64 tensors holding small integers / dyadic values)
# ----------------------------------------------------------------------------------------------------------------------
def ints(shape, mag, g, keep=1.0):
    """uniform integers in [-mag, mag]; keep < 1: only that share of the entries stays, the rest is 0"""
    t = torch.randint(-mag, mag + 1, tuple(shape), generator=g).double()
    if keep < 1.0:
        t = t * (torch.rand(tuple(shape), generator=g) < keep)
    return t


def weights(shape, density, mag, g, sparse_every=0):
    """[O][I][taps...]: +-(1..mag) at `density`, 0 elsewhere; one entry of every (o, tap) slice is forced non-zero.
    sparse_every = n: every n-th output channel keeps ONLY its forced +-1 entries (few terms: small outputs, exact zeros)"""
    shape = tuple(shape)
    val = torch.randint(1, mag + 1, shape, generator=g).double() * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    w = val * (torch.rand(shape, generator=g) < density)
    one = (shape[0], 1) + shape[2:]
    idx = torch.randint(0, shape[1], one, generator=g)
    forced = (torch.randint(0, 2, one, generator=g) * 2 - 1).double()
    if sparse_every:
        thin = torch.zeros(shape, dtype=torch.float64).scatter_(1, idx, forced)
        sel = (torch.arange(shape[0]) % sparse_every == 0).view((-1,) + (1,) * (len(shape) - 1))
        w = torch.where(sel, thin, w)
    cur = w.gather(1, idx)
    return w.scatter_(1, idx, torch.where(cur != 0, cur, forced))


def mask_source(shape, g):
    """{-1, -0.0, +0.0, 1}: the zeros of a ReLU-mask source come in both signs, and both must mask"""
    t = torch.randint(-1, 2, tuple(shape), generator=g).double()
    neg0 = (t == 0) & (torch.rand(tuple(shape), generator=g) < 0.5)
    return torch.where(neg0, torch.full_like(t, -0.0), t)


def affine(C, g):
    """per-channel dyadic scale in {1, 2, -1, 0.5} and integer shift in [-4, 4]"""
    scale = torch.tensor([1.0, 2.0, -1.0, 0.5], dtype=torch.float64)[torch.randint(0, 4, (C,), generator=g)]
    return scale, torch.randint(-4, 5, (C,), generator=g).double()


def bcast(v, t):
    return v.view((1, -1) + (1,) * (t.dim() - 2))


# ----------------------------------------------------------------------------------------------------------------------
# conditions
# ----------------------------------------------------------------------------------------------------------------------
def bf16_tie(ref):
    """exactly half way between two neighbouring bf16 values (ref: float64 holding f32-exact values)"""
    f = ref.float()
    assert torch.equal(f.double(), ref)
    return (f.view(torch.int32) & 0xFFFF) == 0x8000


def conditions(ref, absref, dt, mode, *, w=None, acts=(), zeros=True, stats=False):
    """ref: float64 reference [N][C][...]; absref: the same operation on absolute values (sum of |terms| per element).
    w: [O][I][taps...] operand whose (o, tap) slices must each hold a non-zero; acts: [N][C][...] operands whose every
    (image, channel) must hold a non-zero; zeros: the 1 % .. 15 % band of exact zeros; stats: the per-channel statistics caps."""
    assert ref.dtype == torch.float64 and ref.shape == absref.shape
    assert float(absref.max()) <= CAP, "a partial sum could leave the exact range of f32"
    if stats:   # y and y * y are exact; any partial row is a sub-sum of the non-negative terms |y|, y * y of these totals
        dims = [d for d in range(ref.dim()) if d != 1]
        assert float(ref.abs().sum(dims).max()) <= CAP and float((ref * ref).sum(dims).max()) <= CAP
    if mode == "A":
        assert torch.equal(ref.to(dt).double(), ref), "mode A: reference not representable in the output type"
    else:
        assert dt == BF and mode == "B"
        assert torch.equal(ref.float().double(), ref)
        tie = float(bf16_tie(ref).double().mean())
        unrep = float((ref.to(BF).double() != ref).double().mean())
        assert tie >= 0.01 and unrep >= 0.25, f"mode B does not test the rounding: ties {tie:.4f}, unrepresentable {unrep:.4f}"
    if w is not None:
        assert bool((w != 0).any(dim=1).all()), "an (output channel, tap) slice of the weights is all zero"
    for a in acts:
        assert bool((a.flatten(2) != 0).any(dim=2).all()), "an input channel of an image is all zero"
    if zeros:
        z = float((ref == 0).double().mean())
        assert 0.01 <= z <= 0.15, f"share of exact zeros {z:.4f} outside [0.01, 0.15]"


def channel_sums(ref):
    """float64 per-channel sum and sum of squares of an [N][C][...] reference: what the partial statistics rows must add to"""
    dims = [d for d in range(ref.dim()) if d != 1]
    return torch.stack([ref.sum(dims), (ref * ref).sum(dims)])


# ----------------------------------------------------------------------------------------------------------------------
# magnitudes per mode: (activation magnitude, share of activations kept, weight magnitude)
# ----------------------------------------------------------------------------------------------------------------------
def _mags(row):
    if row["mode"] == "A":
        return 1, row.get("xkeep", 1.0), 1
    return row.get("xmag", 8), row.get("xkeep", 0.5), 8


def _conv(x, w, s, p):
    return {4: F.conv2d, 5: F.conv3d}[x.dim()](x, w, None, s, p)


def fwd_data(row):
    """forward convolution: x [B][Cin][H][W] (quad rows: the 2x2 regions of a [B][Cin][2H][2W] map, stacked [B*4]), w [O][I][k][k],
    raw = conv, pre = raw * scale + shift + residual, act = relu(pre) -- all float64, with the |.| twins for conditions()"""
    B, Cin, Cout, H, k, s, p = row["cfg"]
    W = row.get("W", H)
    mode = row["mode"]
    xm, keep, wm = _mags(row)
    g = gen(row["seed"])
    c = {"row": row}
    if row.get("quad"):
        S = 4 if row["quad"] == 4 else 2
        base = ints((B, Cin, S * H, S * W), xm, g, keep)
        c["base"] = base
        x = torch.stack([base[:, :, (q // S) * H:(q // S + 1) * H, (q % S) * W:(q % S + 1) * W] for q in range(S * S)], 1)
        x = x.reshape(B * S * S, Cin, H, W)
    elif row.get("frames"):
        x = ints((B, Cin, row["frames"], H, W), xm, g, keep)
    else:
        x = ints((B, Cin, H, W), xm, g, keep)
    if row.get("zero_block"):      # a blank patch: exact zeros in every output channel
        lo, hi = row["zero_block"]
        x[..., lo:hi, lo:hi] = 0
    kk = (k,) * (x.dim() - 2)
    w = weights((Cout, Cin) + kk, row["density"], wm, g, row.get("sparse_every", 0))
    raw, araw = _conv(x, w, s, p), _conv(x.abs(), w.abs(), s, p)
    scale, shift = affine(Cout, g)
    res = ints(raw.shape, 8, g)
    pre = raw * bcast(scale, raw) + bcast(shift, raw) + res
    apre = araw * bcast(scale.abs(), raw) + bcast(shift.abs(), raw) + res.abs()
    c.update(x=x, w=w, raw=raw, araw=araw, scale=scale, shift=shift, res=res, pre=pre, apre=apre, act=F.relu(pre))
    return c


def fwd_conditions(c, dt):
    row = c["row"]
    mode = row["mode"]
    conditions(c["raw"], c["araw"], dt, mode, w=c["w"], acts=[c["x"]], stats=(mode == "A"))
    conditions(c["pre"], c["apre"], dt, mode, zeros=False)     # (the exact zeros a ReLU sees are those of `pre`)
    assert bool((c["pre"] == 0).any())


def dgrad_data(row):
    """data gradient: dy [B][Cout][Ho][Wo], w [Cout][Cin][k][k] -> dx = conv2d_input, out = (dx + other) * (act > 0)"""
    B, Cin, Cout, H, k, s, p = row["cfg"]
    mode = row["mode"]
    xm, keep, wm = _mags(row)
    g = gen(row["seed"])
    Ho = (H + 2 * p - k) // s + 1
    dy = ints((B, Cout, Ho, Ho), xm, g, keep)
    wt = weights((Cin, Cout, k, k), row["density"], wm, g, row.get("sparse_every", 0))   # slices of the dgrad operand
    w = wt.transpose(0, 1).contiguous()
    shape = (B, Cin, H, H)
    dx = torch.nn.grad.conv2d_input(shape, w, dy, s, p)
    adx = torch.nn.grad.conv2d_input(shape, w.abs(), dy.abs(), s, p)
    other = ints(shape, 8, g)
    act = mask_source(shape, g)
    pre = dx + other
    return {"row": row, "dy": dy, "w": w, "wt": wt, "dx": dx, "adx": adx, "other": other, "act": act, "pre": pre,
            "apre": adx + other.abs(), "out": pre * (act > 0)}


def dgrad_conditions(c, dt):
    mode = c["row"]["mode"]
    conditions(c["dx"], c["adx"], dt, mode, w=c["wt"], acts=[c["dy"]], zeros=c["row"].get("zeros", True))
    conditions(c["pre"], c["apre"], dt, mode, zeros=False)
    z = (c["act"] == 0)
    assert bool((z & torch.signbit(c["act"])).any()) and bool((z & ~torch.signbit(c["act"])).any())
    assert bool((z & (c["pre"] != 0)).any())    # a zero of either sign masks a non-zero value somewhere


def wgrad_data(row):
    """weight gradient: x [B][Cin][H][W], dy [B][Cout][Ho][Wo] (thinned to `keep`) -> dw [Cout][Cin][k][k]; quad = S: the S x S
    regions of a [B][Cin][S*H][S*W] map, stacked"""
    B, Cin, Cout, H, k, s, p = row["cfg"]
    W = row.get("W", H)
    S = row.get("quad", 0)
    g = gen(row["seed"])
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    c = {"row": row}
    if S:
        base = ints((B, Cin, S * H, S * W), 1, g)
        c["base"] = base
        x = torch.stack([base[:, :, (q // S) * H:(q // S + 1) * H, (q % S) * W:(q % S + 1) * W] for q in range(S * S)], 1)
        x = x.reshape(B * S * S, Cin, H, W)
    else:
        x = ints((B, Cin, H, W), 1, g)
    dy = ints((x.shape[0], Cout, Ho, Wo), 1, g, row["keep"])
    dw = torch.nn.grad.conv2d_weight(x, (Cout, Cin, k, k), dy, s, p)
    adw = torch.nn.grad.conv2d_weight(x.abs(), (Cout, Cin, k, k), dy.abs(), s, p)
    c.update(x=x, dy=dy, dw=dw, adw=adw)
    return c


def wgrad_conditions(c):
    conditions(c["dw"], c["adw"], F32, "A", acts=[c["x"], c["dy"]])


def gemm_data(row):
    """rows x K times K x N on the grid: y = x w^T (+ bias) (relu) for qt_linear_bf16, dw = dy^T x for qt_linear_wgrad"""
    M, N, K = row["cfg"]
    mode = row["mode"]
    xm, keep, wm = _mags(row)
    g = gen(row["seed"])
    x = ints((M, K), xm, g, keep)
    w = weights((N, K), row["density"], wm, g, row.get("sparse_every", 0))
    bias = ints((N,), 4, g) if row.get("bias") else None
    pre = x @ w.t() + (bias if bias is not None else 0)
    apre = x.abs() @ w.abs().t() + (bias.abs() if bias is not None else 0)
    return {"row": row, "x": x, "w": w, "bias": bias, "pre": pre, "apre": apre, "out": F.relu(pre) if row.get("relu") else pre}


def gemm_conditions(c, dt):
    x = c["x"]
    conditions(c["pre"].t()[None], c["apre"].t()[None], dt, c["row"]["mode"], w=c["w"], acts=[x.t()[None]])


# ----------------------------------------------------------------------------------------------------------------------
# case tables.  cfg = (B, Cin, Cout, H, k, stride, pad); path = the kernel the dispatch must take (checked by the GPU test)
# ----------------------------------------------------------------------------------------------------------------------
def _r(name, cfg, dts, mode, density, seed, **kw):
    return dict(name=name, cfg=cfg, dts=dts, mode=mode, density=density, seed=seed, **kw)


BOTH = (F32, BF)
B_KW = dict(sparse_every=4)   # mode B: every fourth output channel thin, so that exact zeros stay in the wanted band

FWD_ROWS = [
    _r("generic_3x3", (2, 64, 64, 12, 3, 1, 1), BOTH, "A", 1 / 8, 101, path="generic"),
    _r("generic_3x3_s2", (1, 64, 128, 28, 3, 2, 1), BOTH, "A", 1 / 8, 102, path="generic"),
    _r("generic_1x1_s2", (2, 64, 128, 28, 1, 2, 0), BOTH, "A", 1 / 2, 103, path="generic"),
    _r("generic_m49", (1, 512, 512, 7, 3, 1, 1), BOTH, "A", 1 / 8, 104, path="generic"),
    _r("generic_k2304_s2", (1, 256, 512, 14, 3, 2, 1), BOTH, "A", 1 / 8, 105, path="generic"),
    _r("generic_3x3_rounded", (3, 128, 128, 14, 3, 1, 1), (BF,), "B", 1.0, 106, path="generic", **B_KW),
    _r("generic_slice", (2, 64, 64, 12, 3, 1, 1), BOTH, "A", 1 / 8, 107, path="generic", slice_of=192),
    _r("generic_quadrant", (3, 256, 128, 7, 3, 1, 1), BOTH, "A", 1 / 8, 108, path="generic", quad=1),
    _r("generic_regions_4x4", (2, 128, 64, 7, 3, 1, 1), BOTH, "A", 1 / 8, 120, path="generic", quad=4),
    # the one large case: M = 65856 >= 65536 pixels, 36 K-steps, N > 64 -- the 256 x 128 three-stage tile (conv_pt switched off)
    _r("tile_256x128", (84, 256, 128, 28, 3, 1, 1), (BF,), "A", 1 / 8, 109, path="generic", pt_off=True, tile256=True),
    _r("ring_b1", (1, 64, 64, 56, 3, 1, 1), (BF,), "A", 1 / 8, 110, path="ring"),
    _r("ring_b3_ragged", (3, 64, 64, 56, 3, 1, 1), (BF,), "A", 1 / 8, 111, path="ring"),
    _r("ring_rounded", (1, 64, 64, 56, 3, 1, 1), (BF,), "B", 1.0, 112, path="ring", xmag=16, zero_block=(20, 30), **B_KW),
    # 80 images: 1052 tiles of 256 padded positions in contiguous shares of 4-5 on the ring kernel's 256 workgroups: the
    # 640-row window wraps twice (window indices 640 and 1280), the mirror is refreshed, all five phases (256 k) mod 640 run
    _r("ring_walk", (80, 64, 64, 56, 3, 1, 1), (BF,), "A", 1 / 16, 121, path="ring", walk=4),
    _r("ring_walk_rounded", (80, 64, 64, 56, 3, 1, 1), (BF,), "B", 1.0, 122, path="ring", xmag=16, zero_block=(20, 30), walk=4,
       **B_KW),
    _r("pt_28", (16, 128, 128, 28, 3, 1, 1), BOTH, "A", 1 / 8, 113, path="pt"),
    _r("pt_14_bn256", (16, 128, 256, 14, 3, 1, 1), BOTH, "A", 1 / 8, 114, path="pt"),
    _r("pt_7_ragged", (18, 128, 128, 7, 3, 1, 1), BOTH, "A", 1 / 8, 115, path="pt"),
    _r("pt_14_rounded", (16, 128, 128, 14, 3, 1, 1), (BF,), "B", 1.0, 116, path="pt", **B_KW),
    _r("pt_quadrant", (16, 256, 128, 7, 3, 1, 1), BOTH, "A", 1 / 8, 117, path="pt", quad=1),
    _r("taps27", (2, 64, 64, 8, 3, 1, 1), BOTH, "A", 1 / 16, 118, path="generic", frames=3),
    _r("taps27_t1", (3, 64, 64, 8, 3, 1, 1), BOTH, "A", 1 / 8, 119, path="generic", frames=1),
]

# qt_conv_s2_pair: cfg = (B, Cin, Cout, H_in, max workgroups); the 1x1 downsample takes density `ddown`
S2_ROWS = [
    _r("s2_56", (16, 64, 128, 56, 0), BOTH, "A", 1 / 8, 201, ddown=1 / 2),
    _r("s2_28_walk", (20, 128, 256, 28, 8), BOTH, "A", 1 / 8, 202, ddown=1 / 2),
    _r("s2_14_walk", (16, 256, 512, 14, 5), BOTH, "A", 1 / 8, 203, ddown=1 / 4),
    _r("s2_14_rounded", (16, 256, 512, 14, 5), (BF,), "B", 1.0, 204, ddown=1.0, xmag=16, xkeep=1.0, zero_block=(5, 8)),
]

# packed stem (conv_stem.hip, bf16): 7x7 / 2 on [B][3][224][224]
STEM_ROWS = [
    _r("stem_b1", (1, 3, 64, 224, 7, 2, 3), (BF,), "A", 1 / 2, 301),
    _r("stem_b1_rounded", (1, 3, 64, 224, 7, 2, 3), (BF,), "B", 1.0, 302, xmag=16, xkeep=1.0, zero_block=(60, 100)),
    # contiguous tile shares (STEM_WALKS, share_facts): the smallest batches at which a workgroup of conv_stem_kernel (39) /
    # of the fused stem (21) takes three tiles, reuses its first input buffer, and meets the first and the last tile of an
    # image as its second and as its third tile.  `only`: the kernels the batch was chosen for.  stem_walk thins the image
    # to 1/2: the forced weight entries alone would put a channel's sum of squares over 2^24 at 39 images
    _r("stem_walk", (39, 3, 64, 224, 7, 2, 3), (BF,), "A", 1 / 8, 303, xkeep=1 / 2, only=("conv",), walk=2),
    _r("stem_pool_walk", (21, 3, 64, 224, 7, 2, 3), (BF,), "A", 1 / 4, 304, only=("pool",), walk=2),
    _r("stem_pool_walk_rounded", (21, 3, 64, 224, 7, 2, 3), (BF,), "B", 1.0, 305, xmag=16, xkeep=1.0, zero_block=(60, 100),
       only=("pool",), walk=2),
]

DGRAD_ROWS = [
    _r("generic_3x3", (2, 64, 64, 12, 3, 1, 1), BOTH, "A", 1 / 8, 401, path="generic"),
    _r("generic_3x3_s2", (1, 64, 128, 28, 3, 2, 1), BOTH, "A", 1 / 4, 402, path="generic"),
    _r("generic_rounded", (2, 128, 128, 14, 3, 1, 1), (BF,), "B", 1.0, 403, path="generic", **B_KW),
    _r("ring", (1, 64, 64, 56, 3, 1, 1), (BF,), "A", 1 / 8, 404, path="ring"),
    _r("ring_walk", (80, 64, 64, 56, 3, 1, 1), (BF,), "A", 1 / 16, 408, path="ring", walk=4),   # see FWD_ROWS
    _r("pt_28", (16, 128, 128, 28, 3, 1, 1), BOTH, "A", 1 / 8, 405, path="pt"),
    _r("pt_7_ragged", (18, 128, 128, 7, 3, 1, 1), BOTH, "A", 1 / 8, 406, path="pt"),
    _r("pt_14_rounded", (16, 128, 256, 14, 3, 1, 1), (BF,), "B", 1.0, 407, path="pt", **B_KW),
]

# stride-2 data gradients on parity classes: cfg = (B, Cin, Cout, H, k, 2, pad); form: merged / merged5 (downsample as the
# fifth tap slot) / classes (one launch per parity class)
S2D_ROWS = [
    _r("merged_generic", (2, 64, 128, 28, 3, 2, 1), BOTH, "A", 1 / 4, 501, form="merged", path="generic"),
    _r("merged_pt", (16, 256, 512, 14, 3, 2, 1), BOTH, "A", 1 / 8, 502, form="merged", path="pt"),
    _r("merged5", (2, 64, 128, 28, 3, 2, 1), BOTH, "A", 1 / 4, 503, form="merged5", path="generic"),
    _r("merged5_small", (1, 64, 64, 12, 3, 2, 1), BOTH, "A", 1 / 2, 504, form="merged5", path="generic"),
    _r("classes_3x3", (1, 64, 128, 28, 3, 2, 1), BOTH, "A", 1 / 4, 505, form="classes", path="generic"),
    _r("classes_1x1", (1, 64, 128, 28, 1, 2, 0), BOTH, "A", 1.0, 506, form="classes", path="generic", zeros=False),
]

# weight gradients (f32 outputs: mode A).  keep = share of dy kept non-zero (fewer terms: exact zeros among the outputs)
WGRAD_ROWS = [
    _r("generic_3x3", (2, 64, 64, 12, 3, 1, 1), BOTH, "A", None, 601, keep=1.0, path="generic"),
    _r("generic_3x3_s2", (1, 64, 128, 28, 3, 2, 1), BOTH, "A", None, 602, keep=1.0, path="generic"),
    _r("generic_1x1_s2", (2, 64, 128, 28, 1, 2, 0), BOTH, "A", None, 603, keep=1 / 2, path="generic"),
    _r("generic_quadrant", (3, 256, 128, 7, 3, 1, 1), BOTH, "A", None, 604, keep=1.0, path="generic", quad=2),
    _r("generic_64x128", (2, 128, 64, 12, 3, 1, 1), (BF,), "A", None, 615, keep=1.0, path="generic"),
    # plain images whose padded grid (16 x 16, 32 x 32) is that of a region row: the tile-resident kernel provably fits
    _r("tile_15", (3, 64, 64, 15, 3, 1, 1), (BF,), "A", None, 616, keep=1.0, path="stream", variants=(3,), prove_tile=True),
    _r("tile_31", (1, 64, 128, 31, 3, 1, 1), (BF,), "A", None, 617, keep=1.0, path="stream", variants=(3,), prove_tile=True),
    _r("stream_56", (1, 64, 64, 56, 3, 1, 1), (BF,), "A", None, 605, keep=1 / 4, path="stream", variants=(3, 0, 2)),
    _r("stream_14", (3, 128, 64, 14, 3, 1, 1), (BF,), "A", None, 606, keep=1.0, path="stream", variants=(3, 0, 2)),
    _r("stream_7", (6, 64, 128, 7, 3, 1, 1), (BF,), "A", None, 607, keep=1.0, path="stream", variants=(3, 0, 2)),
    _r("tile_9x31", (3, 128, 64, 9, 3, 1, 1), (BF,), "A", None, 608, keep=1.0, path="stream", variants=(3,), W=31),
    _r("tile_7x7_b1", (1, 64, 64, 7, 3, 1, 1), (BF,), "A", None, 609, keep=1.0, path="stream", variants=(3,)),
    _r("s2_planes_3x3", (2, 64, 128, 28, 3, 2, 1), (BF,), "A", None, 610, keep=1.0, path="s2"),
    _r("s2_planes_1x1", (2, 64, 128, 28, 1, 2, 0), (BF,), "A", None, 611, keep=1.0, path="s2"),
    _r("s2_planes_rect", (4, 64, 128, 20, 3, 2, 1), (BF,), "A", None, 612, keep=1.0, path="s2", W=12),
    _r("region_2x2", (3, 256, 128, 7, 3, 1, 1), (BF,), "A", None, 613, keep=1.0, path="region", quad=2),
    _r("region_4x4", (2, 128, 64, 7, 3, 1, 1), (BF,), "A", None, 614, keep=1 / 2, path="region", quad=4),
]

# cfg = (rows, out, in): qt_linear_wgrad (dw = dy^T x, f32)
LWGRAD_ROWS = [
    _r("lw_small", (64, 128, 192), BOTH, "A", None, 701, keep=1.0),
    _r("lw_long_rows", (4096, 128, 64), BOTH, "A", None, 702, keep=1 / 4),
    _r("lw_ragged", (37, 320, 448), BOTH, "A", None, 703, keep=1.0),
]

# qt_linear_bf16: cfg = (M, N, K)
LINEAR_ROWS = [
    _r("lin_one_tile", (5, 64, 64), (BF,), "A", 1 / 2, 811, bias=True, relu=0),
    _r("lin_seven_ksteps", (200, 192, 448), (BF,), "A", 1 / 8, 802, bias=False, relu=1),
    _r("lin_splitk", (37, 2688, 5376), (BF,), "A", 1 / 16, 803, bias=True, relu=1),
    _r("lin_splitk_rounded", (37, 2688, 5376), (BF,), "B", 1 / 4, 804, bias=False, relu=1, xmag=16, sparse_every=16),
    _r("lin_rounded", (200, 192, 448), (BF,), "B", 1.0, 805, bias=False, relu=0, xmag=16, sparse_every=16),
]


# qt_stem_dgrad (f32 image gradient from a bf16 / f32 gradient map) and the packed-stem weight gradient
STEMD_ROWS = [
    _r("stem_dgrad", (1, 3, 64, 224, 7, 2, 3), BOTH, "A", 1 / 8, 901),
    # 11 images: 539 tiles (bf16) / 1078 tiles (f32) on the persistent grid of 256: 2-3 and 4-5 tiles per workgroup
    _r("stem_dgrad_walk", (11, 3, 64, 224, 7, 2, 3), BOTH, "A", 1 / 8, 903, walk=2),
]
STEMW_ROWS = [
    _r("stem_wgrad", (1, 3, 64, 224, 7, 2, 3), BOTH, "A", None, 902, keep=0.1),
    # 11 images: 616 two-row tiles in contiguous shares of 2-3 on the 256 workgroups of stem_wgrad_rows_kernel (bf16); dy is
    # thin enough for exact zeros among 9408 sums over 138 k positions, and every tile still holds a non-zero dy
    _r("stem_wgrad_walk", (11, 3, 64, 224, 7, 2, 3), BOTH, "A", None, 904, keep=0.003, walk=2),
]

# 3-D convolutions of the clip models (bf16 kernels): cfg = (B, T, H, W); `only`: the parts of the row a shape admits
C3F_ROWS = [   # qt_conv3d_first_*: 3 -> 32 channels from the f32 clip
    _r("first_t1_w16", (3, 1, 8, 16), (BF,), "A", 1 / 2, 911, keep=1.0, only=("fwd", "dgrad")),       # T = 1, smallest w
    _r("first_w256", (2, 3, 4, 256), (BF,), "A", 1 / 2, 912, keep=0.2, only=("fwd", "dgrad", "wgrad", "fused")),   # widest w
    _r("first_w32", (2, 2, 8, 32), (BF,), "A", 1 / 2, 913, keep=0.8, only=("fwd", "dgrad", "wgrad", "fused")),
    _r("first_rounded", (2, 3, 8, 32), (BF,), "B", 1.0, 914, xmag=32, xkeep=1.0, zero_block=(2, 6), only=("fwd",)),
    _r("first_dgrad_general", (1, 2, 6, 20), BOTH, "A", 1 / 2, 915, keep=1.0, only=("dgrad",)),   # the direct kernel
    # 3 x 344 = 1032 (clip, 4-row slab) items on a grid capped at 2 x CUs = 512: every workgroup walks 2 items, eight walk 3,
    # and consecutive items of a workgroup lie in different clips.  keep: see c32_walk
    _r("first_walk", (3, 2, 1376, 32), (BF,), "A", 1 / 2, 916, keep=0.004, only=("fwd", "dgrad", "wgrad", "fused"), walk=2),
]
C32_ROWS = [   # qt_conv3d_c32_*: 32 -> 64 channels on frame slabs; xc = channels per input row (32, or 64 with padding)
    _r("c32_t1_w16", (3, 1, 8, 16), (BF,), "A", 1 / 8, 921, keep=1.0, xc=64, only=("fwd", "dgrad")),   # T = 1, smallest w
    # (no weight gradient at T = 1: two thirds of it, the outer frame taps, is zero by construction)
    _r("c32_w128", (1, 2, 8, 128), (BF,), "A", 1 / 8, 922, keep=0.4, xc=64, only=("fwd", "dgrad", "wgrad")),
    _r("c32_xc32", (1, 5, 12, 64), (BF,), "A", 1 / 8, 923, keep=0.2, xc=32, only=("fwd", "dgrad", "wgrad")),
    _r("c32_rounded", (1, 5, 12, 64), (BF,), "B", 1.0, 924, xc=32, zero_block=(2, 8), only=("fwd",), **B_KW),
    # (clip, 2-row slab) items on a grid capped at the CU count (256): 516 items = 2-3 per workgroup; 780 items = 3-4 per
    # workgroup with odd T (the ring slot of an item's last frame is not the one the next item starts in).  The small `keep`:
    # a weight gradient contracted over 10^5 positions has almost no exact zeros unless dy is thin; every work item still
    # holds a non-zero dy
    _r("c32_walk", (3, 2, 344, 16), (BF,), "A", 1 / 8, 925, keep=0.01, xc=32, only=("fwd", "dgrad", "wgrad"), walk=2),
    _r("c32_walk3", (5, 3, 312, 16), (BF,), "A", 1 / 8, 926, keep=0.01, xc=64, only=("fwd", "dgrad", "wgrad"), walk=2),
]


def c3_data(row, cin, cout):
    """nn.Conv3d(cin, cout, 3, padding 1): forward with scale / shift / ReLU and MaxPool3d((1, 2, 2)); data and weight gradient
    of a gradient map thinned to `keep` (their own +-1 operands: f32 / mode-A outputs)"""
    B, T, H, W = row["cfg"]
    xm, keep, wm = _mags(row)
    g = gen(row["seed"])
    x = ints((B, cin, T, H, W), xm, g, keep)
    if row.get("zero_block"):
        lo, hi = row["zero_block"]
        x[..., lo:hi, lo:hi] = 0
    w = weights((cout, cin, 3, 3, 3), row["density"], wm, g, row.get("sparse_every", 0))
    raw, araw = F.conv3d(x, w, None, 1, 1), F.conv3d(x.abs(), w.abs(), None, 1, 1)
    scale, shift = affine(cout, g)
    pre = raw * bcast(scale, raw) + bcast(shift, raw)
    c = {"row": row, "x": x, "w": w, "raw": raw, "araw": araw, "scale": scale, "shift": shift, "pre": pre,
         "apre": araw * bcast(scale.abs(), raw) + bcast(shift.abs(), raw), "act": F.relu(pre)}
    c["pooled"] = F.max_pool3d(c["act"], (1, 2, 2)) if H % 2 == 0 and W % 2 == 0 else None
    if row["mode"] == "A":
        x1 = ints((B, cin, T, H, W), 1, g)
        dy = ints(raw.shape, 1, g, row["keep"])
        dyf = ints(raw.shape, 1, g)
        wt = weights((cin, cout, 3, 3, 3), row["density"], 1, g)
        wg = wt.transpose(0, 1).contiguous()
        c.update(x1=x1, dy=dy, dyf=dyf, wt=wt, wg=wg,
                 dx=torch.nn.grad.conv3d_input(x1.shape, wg, dyf, 1, 1),
                 adx=torch.nn.grad.conv3d_input(x1.shape, wg.abs(), dyf.abs(), 1, 1),
                 dw=torch.nn.grad.conv3d_weight(x1, w.shape, dy, 1, 1),
                 adw=torch.nn.grad.conv3d_weight(x1.abs(), w.shape, dy.abs(), 1, 1))
    return c


def c3_fused_data(c, cp):
    """qt_conv3d_first_wgrad_fused: the weight gradient of a dy the kernel forms itself from the raw conv output y, the gradient
    `dout` of the pooled map [B][cp][T][H/2][W/2], the argmax map of MaxPool3d((1, 2, 2)) (window position (h & 1) * 2 + (w & 1))
    and the BatchNorm-backward coefficients:  g = dout at the argmax where y * scale + shift > 0, else 0;
    dy = a (g - b - (y - mean) invstd c), stored as bf16.  On the grid: y integer, mean and b integer, invstd in {1, 0.5},
    c in {1, 2}, a in {1, 0.5}, dout in {-1, 0, 1}: dy is a multiple of 1/4 that bf16 holds exactly (asserted by
    c3_fused_conditions), in the kernel's own form ka g + kb - y kc as well.  cp: channels per pooled row (32, or 64 with padding)"""
    row = c["row"]
    g = gen(row["seed"] + 7000 + cp)
    x1, w = c["x1"], c["w"]
    y = F.conv3d(x1, w, None, 1, 1)
    B, C, T, H, W = y.shape
    scale, shift = c["scale"], c["shift"]
    pre = y * bcast(scale, y) + bcast(shift, y)
    _, idx = F.max_pool3d(F.relu(pre), (1, 2, 2), return_indices=True)          # flat index into T * H * W
    arg32 = (((idx // W) % H) % 2) * 2 + (idx % W) % 2
    arg = torch.randint(0, 4, (B, cp, T, H // 2, W // 2), generator=g)           # the padding channels hold any position
    arg[:, :32] = arg32
    dout = ints((B, cp, T, H // 2, W // 2), 1, g)
    pick = lambda n, vals: torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), (n,), generator=g)]
    mean, invstd = ints((32,), 2, g), pick(32, [1.0, 0.5])
    coef = torch.stack([pick(cp, [1.0, 0.5]), ints((cp,), 2, g), pick(cp, [1.0, 2.0])])
    up = lambda t: t[:, :32].repeat_interleave(2, 3).repeat_interleave(2, 4)
    hh = (torch.arange(H) % 2).view(1, 1, 1, H, 1)
    ww = (torch.arange(W) % 2).view(1, 1, 1, 1, W)
    gfull = torch.where((up(arg) == hh * 2 + ww) & (pre > 0), up(dout), torch.zeros((), dtype=torch.float64))
    a, b, cc = (bcast(coef[j, :32], y) for j in range(3))
    dy = a * (gfull - b - (y - bcast(mean, y)) * bcast(invstd, y) * cc)
    dw = torch.nn.grad.conv3d_weight(x1, w.shape, dy, 1, 1)
    adw = torch.nn.grad.conv3d_weight(x1.abs(), w.shape, dy.abs(), 1, 1)
    return {"row": row, "x1": x1, "w": w, "y": y, "pre": pre, "scale": scale, "shift": shift, "arg": arg.to(torch.uint8),
            "dout": dout, "mean": mean, "invstd": invstd, "coef": coef, "gate": up(arg) == hh * 2 + ww, "dy": dy, "dw": dw, "adw": adw}


def c3_fused_conditions(f):
    """every term x * dy is a multiple of 1/4: on the scale of quarters the sums are integers, so 4 * sum |terms| <= 2^24 keeps
    every partial sum exact.  y and dy must be exact in bf16.  dy is dense by construction (the - xhat c term is non-zero almost
    everywhere), so the weight gradient has no band of exact zeros; the zeros that matter here are those of the ReLU gate:
    some window maximum with a non-zero pooled gradient sits at y * scale + shift == 0 and must not pass"""
    dy, y = f["dy"], f["y"]
    assert torch.equal(y.to(BF).double(), y) and torch.equal(dy.to(BF).double(), dy), "y / dy not representable in bf16"
    assert torch.equal(dy * 4, (dy * 4).round())
    conditions(f["dw"] * 4, f["adw"] * 4, F32, "A", acts=[f["x1"], dy], zeros=False)
    up = f["dout"][:, :32].repeat_interleave(2, 3).repeat_interleave(2, 4)
    assert bool((f["gate"] & (f["pre"] == 0) & (up != 0)).any()), "no exact zero reaches the ReLU gate"
    assert bool((f["gate"] & (f["pre"] > 0) & (up != 0)).any())


def c3_conditions(c, dt, part):
    row = c["row"]
    mode = row["mode"]
    if part == "fwd":
        conditions(c["raw"], c["araw"], dt, mode, w=c["w"], acts=[c["x"]], stats=(mode == "A"))
        conditions(c["pre"], c["apre"], dt, mode, zeros=False)
    elif part == "dgrad":
        conditions(c["dx"], c["adx"], dt, "A", w=c["wt"], acts=[c["dyf"]])
    else:
        conditions(c["dw"], c["adw"], F32, "A", acts=[c["x1"], c["dy"]])


def walk_items(items, cap):
    """the walk of a persistent kernel on the host: grid = min(items, cap) workgroups, workgroup k takes items k, k + grid, ...
    Returns (grid, workgroup of every item, trip of every item: 0 for a workgroup's first item, 1 for its second, ...)"""
    grid = min(items, cap)
    i = torch.arange(items)
    return grid, i % grid, i // grid


def share_items(items, cap):
    """the other walk: grid = min(items, cap) workgroups, workgroup b takes the CONTIGUOUS share b * items / grid ..
    (b + 1) * items / grid - 1 (conv_stem.hip, stem_wgrad_rows_kernel, conv_l1_ring_kernel).  Returns (grid, workgroup of
    every item, trip of every item: 0 for the first item of its workgroup's share, 1 for the second, ...)"""
    grid = min(items, cap)
    beg = torch.arange(grid + 1) * items // grid
    i = torch.arange(items)
    wg = torch.bucketize(i, beg[1:], right=True)
    return grid, wg, i - beg[wg]


def share_facts(items, cap, per_image=0):
    """what a contiguous-share walk reaches.  least / most: items per workgroup, with_most: workgroups that take `most`.
    per_image = n (items are image * n + k): crossing = workgroups whose share goes on behind the last item of an image;
    first_as[t] / last_as[t] = workgroups that take the first (k = 0) / last (k = n - 1) item of an image on trip t"""
    grid, wg, trip = share_items(items, cap)
    n = torch.bincount(wg, minlength=grid)
    f = dict(items=items, grid=grid, least=int(n.min()), most=int(n.max()), with_most=int((n == n.max()).sum()))
    if per_image:
        k = torch.arange(items) % per_image
        f["crossing"] = int(((k == per_image - 1) & (trip < n[wg] - 1)).sum())
        f["first_as"] = {t: int(((k == 0) & (trip == t)).sum()) for t in (1, 2)}
        f["last_as"] = {t: int(((k == per_image - 1) & (trip == t)).sum()) for t in (1, 2)}
    return f


def stem_walk_reaches(f):
    """the state the stem walk rows are there for: a workgroup with three tiles (its first input buffer is reused), a share
    that crosses an image boundary, the first tile of an image (k = 0: rows skipped, a shorter fetch, no conv row -1) as a
    workgroup's second and as its third tile, the last tile of an image as its third"""
    return f["least"] >= 2 and f["most"] >= 3 and f["crossing"] > 0 and min(f["first_as"].values()) > 0 and f["last_as"][2] > 0


# (items per image, grid cap) of the kernels behind the walk rows, and the facts of their walks -- computed from the split
# above, asserted by tests/test_exact_data_cpu.py; the GPU test asserts what it needs of them again before it reads a result
WALKS = {
    "stem_walk": (28, 512, dict(items=1092, grid=512, least=2, most=3, with_most=68, crossing=20, first_as={1: 18, 2: 2},
                                last_as={1: 18, 2: 3})),
    "stem_pool_walk": (28, 256, dict(items=588, grid=256, least=2, most=3, with_most=76, crossing=11, first_as={1: 9, 2: 2},
                                     last_as={1: 9, 2: 3})),
    "stem_wgrad_walk": (56, 256, dict(items=616, grid=256, least=2, most=3, with_most=104)),
    "ring_walk": (0, 256, dict(items=1052, grid=256, least=4, most=5, with_most=28)),
}
WALKS["stem_pool_walk_rounded"], WALKS["ring_walk_rounded"] = WALKS["stem_pool_walk"], WALKS["ring_walk"]


def ring_tiles(B, H):
    """256-position tiles of the padded grid [B][H + 2][H + 2] the layer-1 ring kernel walks"""
    return -(-(B * (H + 2) * (H + 2)) // 256)


def locate(row, index):
    """where output element (n, c, h, w) of a walk row lies in the walk, for a failure message: its tile, the workgroup that
    takes it, the trip of that workgroup (0 = first tile of its share) and, for the stem, the tile's place k in its image.
    stem_walk: 4 conv rows per tile; the fused stem: 2 pooled rows per tile; ring: 256 positions of the padded grid"""
    per, cap, _ = WALKS[row["name"]]
    n, _, h, w = index
    B, H = row["cfg"][0], row["cfg"][3]
    if per == 0:
        items, tile = ring_tiles(B, H), (n * (H + 2) * (H + 2) + (h + 1) * (H + 2) + (w + 1)) // 256
    else:
        items, tile = per * B, n * per + h // (4 if "conv" in row["only"] else 2)
    grid, wg, trip = share_items(items, cap)
    where = dict(tile=tile, workgroup=int(wg[tile]), trip=int(trip[tile]))
    if per:
        where["k"] = tile % per
    return where


def ids(rows):
    return [r["name"] for r in rows]


def expand(rows):
    """(row, dtype) pairs and their ids"""
    pairs = [(r, dt) for r in rows for dt in r["dts"]]
    return pairs, [f"{r['name']}-{'bf16' if dt == BF else 'f32'}" for r, dt in pairs]


def lwgrad_data(row):
    rows, out, inn = row["cfg"]
    g = gen(row["seed"])
    x = ints((rows, inn), 1, g)
    dy = ints((rows, out), 1, g, row["keep"])
    return {"row": row, "x": x, "dy": dy, "dw": dy.t() @ x, "adw": dy.abs().t() @ x.abs()}


def lwgrad_conditions(c):
    conditions(c["dw"][None], c["adw"][None], F32, "A", acts=[c["x"].t()[None], c["dy"].t()[None]])


def s2_data(row):
    """conv1 3x3 / 2 pad 1 and the 1x1 / 2 downsample of a transition block on the same input; eval epilogues: scale / shift /
    ReLU on conv1, scale / shift on the downsample"""
    B, Cin, Cout, H, _ = row["cfg"]
    main = fwd_data(dict(row, cfg=(B, Cin, Cout, H, 3, 2, 1)))
    xm, keep, wm = _mags(row)
    g = gen(row["seed"] + 5000)
    x = main["x"]
    wd = weights((Cout, Cin, 1, 1), row["ddown"], wm, g, row.get("sparse_every", 0))
    rawd, arawd = F.conv2d(x, wd, None, 2, 0), F.conv2d(x.abs(), wd.abs(), None, 2, 0)
    sd, shd = affine(Cout, g)
    raw, araw, sc, sh = main["raw"], main["araw"], main["scale"], main["shift"]
    pre = raw * bcast(sc, raw) + bcast(sh, raw)
    pred = rawd * bcast(sd, raw) + bcast(shd, raw)
    return {"row": row, "x": x, "w": main["w"], "wd": wd, "raw": raw, "araw": araw, "rawd": rawd, "arawd": arawd,
            "sc": sc, "sh": sh, "sd": sd, "shd": shd, "pre": pre, "apre": araw * bcast(sc.abs(), raw) + bcast(sh.abs(), raw),
            "act": F.relu(pre), "pred": pred, "apred": arawd * bcast(sd.abs(), raw) + bcast(shd.abs(), raw)}


def s2_conditions(c, dt):
    mode = c["row"]["mode"]
    conditions(c["raw"], c["araw"], dt, mode, w=c["w"], acts=[c["x"]], stats=(mode == "A"))
    conditions(c["rawd"], c["arawd"], dt, mode, w=c["wd"], stats=(mode == "A"))
    conditions(c["pre"], c["apre"], dt, mode, zeros=False)
    conditions(c["pred"], c["apred"], dt, mode, zeros=False)


def s2d_data(row):
    """stride-2 data gradient of conv1 (3x3 / 2 or 1x1 / 2); merged5 adds the downsample's (1x1 / 2) gradient of a second map"""
    c = dgrad_data(row)
    if row["form"] == "merged5":
        B, Cin, Cout, H, k, s, p = row["cfg"]
        g = gen(row["seed"] + 5000)
        dyd = ints(c["dy"].shape, 1, g)
        wdt = weights((Cin, Cout, 1, 1), row["density"], 1, g)
        wd = wdt.transpose(0, 1).contiguous()
        shape = (B, Cin, H, H)
        c["dx"] = c["dx"] + torch.nn.grad.conv2d_input(shape, wd, dyd, 2, 0)
        c["adx"] = c["adx"] + torch.nn.grad.conv2d_input(shape, wd.abs(), dyd.abs(), 2, 0)
        c["pre"], c["apre"] = c["dx"] + c["other"], c["adx"] + c["other"].abs()
        c["out"] = c["pre"] * (c["act"] > 0)
        c.update(dyd=dyd, wd=wd)
    return c


def stem_data(row):
    c = fwd_data(row)
    raw, araw = c["raw"], c["araw"]
    c["pre"] = raw * bcast(c["scale"], raw) + bcast(c["shift"], raw)      # (the stem has no residual)
    c["apre"] = araw * bcast(c["scale"].abs(), raw) + bcast(c["shift"].abs(), raw)
    c["act"] = F.relu(c["pre"])
    c["pooled"] = F.max_pool2d(c["act"], 3, 2, 1)
    return c


# ----------------------------------------------------------------------------------------------------------------------
# the comparison both test files use
# ----------------------------------------------------------------------------------------------------------------------
def same(got, ref, dt):
    """torch.equal of a result with the float64 reference cast to the output type `dt` (mode A: conditions() has shown that
    cast to be exact; mode B: it is the one round-to-nearest-even the store must perform)"""
    want = ref.to(dt)
    got = got.to(want.device)
    assert got.dtype == dt and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    return torch.equal(got, want)


def first_mismatch(got, ref, dt):
    """(index, got, want) of the first differing element, for the failure message"""
    want = ref.to(dt)
    bad = (got.to(want.device) != want).nonzero()
    if not len(bad):
        return None
    i = tuple(int(v) for v in bad[0])
    return i, float(got[i]), float(want[i]), int(len(bad))


def stats_equal(partial, ref):
    """float64 sum of the kernel's partial rows [rows][2][C] == float64 per-channel sums of the reference"""
    return torch.equal(partial.double().sum(0).cpu(), channel_sums(ref))
