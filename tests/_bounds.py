"""Float64 references and DERIVED error bounds for the kernels around the convolutions (BatchNorm statistics / apply /
backward, pooling, dropout, thin GEMM).  Shared by tests/test_elementwise_gpu.py, tests/test_gemm_small_gpu.py (kernel on the
GPU) and tests/test_kernel_bounds_cpu.py (a torch-f32 restatement in the kernel's place: the bounds are satisfiable by correct
f32 arithmetic and the references are right).

Bound rule (standard forward error of the kernel's own arithmetic, evaluated per output element in float64):
  * a result that is a sum of n f32 products / terms:  |got - ref| <= (n + 8) * 2^-24 * sum_i |term_i|
  * + half a bf16 unit in the last place when the output is stored as bf16 (one round-to-nearest of an 8-bit significand:
    2^-9 |ref| at the top of a binade, 2^-8 |ref| at the bottom; see stored())
  * double accumulation (bn_finalize_kernel, bn_bwd_finalize_kernel at <= 1024 partial rows): the output's own f32 rounding,
    2 * 2^-24 * |ref|, plus 2^-53-level slack of the double sums; an explicit cancellation adds the cancelling magnitudes
Nothing here is fitted to what a kernel returns."""
import math

import numpy as np
import torch

U = 2.0 ** -24        # f32 unit roundoff
UB = 2.0 ** -8        # bf16: largest relative error of one round-to-nearest (8-bit significand: half an ulp of [1, 2))
UD = 2.0 ** -53       # f64 unit roundoff
MOMENTUM = float(np.float32(0.1))   # the kernels take momentum / eps as f32
EPS = float(np.float32(1e-5))
FOLD = 64             # rows the stage-1 kernel of a long partial table adds in f32


def sum_bound(n, abs_terms):
    return (n + 8) * U * abs_terms


def stored(bound, ref, dt):
    """+ the one round-to-nearest of a bf16 store: half a unit in the last place of the value stored.  bf16 keeps 8 significant
    bits, so that is 2^(e - 8) for a value in [2^e, 2^(e+1)): between 2^-9 |v| (top of a binade) and 2^-8 |v| (bottom).  A flat
    2^-9 |ref| is NOT met by a correctly rounded store (2.4431 -> 2.4375 is 1.2 * 2^-9 relative): the half-ulp of the largest
    magnitude the bound admits, |ref| + bound, is the tightest figure that correct arithmetic satisfies."""
    if dt != torch.bfloat16:
        return bound
    _, ex = torch.frexp(ref.abs() + bound)          # v = m * 2^ex, m in [0.5, 1): e = ex - 1
    half_ulp = torch.ldexp(torch.ones_like(ref), ex - 9)
    return bound + torch.where(ref.abs() + bound > 0, half_ulp, torch.zeros_like(ref))


def ratio(got, ref, bound):
    """max |got - ref| / bound (inf where a zero bound is missed, or for a non-finite result)"""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref).abs()
    inf = torch.full_like(err, float("inf"))
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), inf))
    return float(r.max()) if r.numel() else 0.0


# ----------------------------------------------------------------------------------------------------------------------
# BatchNorm statistics: partial[rows][2][C] -> mean / invstd / scale / shift / running statistics
# ----------------------------------------------------------------------------------------------------------------------
FIN_ROWS_DIRECT = [1, 15, 16, 17, 127, 128, 129, 1024]
FIN_ROWS_FOLDED = [1025, 1088, 1089, 8192]
FIN_C = [8, 24, 64, 520]
FIN_PER_ROW = 4   # samples behind each partial row


def fin_partial(rows, C, seed, device, per=FIN_PER_ROW):
    """per-row sums / sums of squares of random data (float64), rounded to f32: [rows][2][C]; odd channels sit 8 standard
    deviations off zero (E[x^2] / var = 65: the cancellation of E[x^2] - E[x]^2)"""
    g = torch.Generator(device=device).manual_seed(seed)
    std = 0.5 + 1.5 * torch.rand(C, generator=g, device=device, dtype=torch.float64)
    off = 8.0 * (torch.arange(C, device=device) % 2).double() * std
    x = torch.randn(rows, per, C, generator=g, device=device, dtype=torch.float64) * std + off
    return torch.stack([x.sum(1), (x * x).sum(1)], 1).float().contiguous(), rows * per


def fin_params(C, seed, device):
    g = torch.Generator().manual_seed(seed)
    gamma = (0.5 + torch.rand(C, generator=g)).to(device)
    beta = (torch.randn(C, generator=g) * 0.3).to(device)
    rmean = (torch.randn(C, generator=g) * 0.7).to(device)
    rvar = (0.3 + torch.rand(C, generator=g)).to(device)
    return gamma, beta, rmean, rvar


def bn_finalize_ref(partial, count, gamma, beta, rmean, rvar, folded):
    """{name: (ref, bound)} from the f32 partial rows the kernel reads.  folded: rows > 1024, where groups of 64 rows are first
    added in f32: that sum of 64 terms is allowed (64 + 2) * 2^-24 * sum|s|, i.e. 66 U sum|s2| / count on var and
    66 U sum|s1| / count on mean; invstd = (var + eps)^-1/2 moves by invstd^3 / 2 per unit of var (half the relative error of
    var where eps is negligible), scale by |gamma| times that, shift = beta - mean * scale by |mean| times that plus |scale| times
    the error of mean."""
    p = partial.double()
    rows, C = p.shape[0], p.shape[2]
    s1, s2 = p[:, 0].sum(0), p[:, 1].sum(0)
    a1, a2 = p[:, 0].abs().sum(0), p[:, 1].abs().sum(0)
    m = s1 / count
    var = (s2 / count - m * m).clamp_min(0.0)
    inv = 1.0 / torch.sqrt(var + EPS)
    g = gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64, device=p.device)
    b = beta.double() if beta is not None else torch.zeros(C, dtype=torch.float64, device=p.device)
    scale = g * inv
    shift = b - m * scale
    dd = (rows + 8) * 2 * UD                                  # the double sums
    dm = dd * a1 / count + (66 * U * a1 / count if folded else 0.0)
    dvar = dd * (a2 / count + 2 * m * m) + (66 * U * a2 / count if folded else 0.0)
    dinv = 0.5 * inv ** 3 * dvar
    out = {
        "mean": (m, 2 * U * m.abs() + dm),
        "invstd": (inv, 2 * U * inv + dinv),
        "scale": (scale, 2 * U * scale.abs() + g.abs() * dinv),
        "shift": (shift, 2 * U * shift.abs() + (m * g).abs() * dinv + dm * scale.abs() + 4 * UD * (b.abs() + (m * scale).abs())),
    }
    if rmean is not None:
        unb = count / (count - 1.0) if count > 1 else 1.0
        nm = (1.0 - MOMENTUM) * rmean.double() + MOMENTUM * m
        nv = (1.0 - MOMENTUM) * rvar.double() + MOMENTUM * var * unb
        out["running_mean"] = (nm, 2 * U * nm.abs() + MOMENTUM * dm + 4 * UD * (rmean.double().abs() + m.abs()))
        out["running_var"] = (nv, 2 * U * nv.abs() + MOMENTUM * unb * dvar + 4 * UD * (rvar.double().abs() + var))
    return out


def fold_f32(partial):
    """the f32 stage the launcher puts in front of a finalize kernel above 1024 rows (stand-in side): groups of 64 rows"""
    rows = partial.shape[0]
    pad = (-rows) % FOLD
    p = torch.cat([partial, partial.new_zeros((pad,) + tuple(partial.shape[1:]))]) if pad else partial
    return p.view(-1, FOLD, *partial.shape[1:]).sum(1, dtype=torch.float32)


# ----------------------------------------------------------------------------------------------------------------------
# out = relu?( y*scale + shift + (res ? res*res_scale + res_shift : 0) )
# ----------------------------------------------------------------------------------------------------------------------
ACT_SHAPES = [(1, 8), (7, 64), (3 * 56 * 56, 64), (50, 512)]
LARGE_M, LARGE_C = 786433, 64   # 1.5 passes of the 16384 x 256 grid in 8-channel groups, 3 strides + 16 in 4-channel groups


def act_inputs(M, C, dt, seed, device):
    g = torch.Generator(device=device).manual_seed(seed)
    y = (torch.randn(M, C, generator=g, device=device) * 1.5 + 0.25).to(dt)
    res = torch.randn(M, C, generator=g, device=device).to(dt)
    v = torch.rand(4, C, generator=g, device=device)
    return y, res, 0.5 + v[0], v[1] - 0.5, 0.5 + v[2], v[3] - 0.5


def bn_act_ref(y, sc, sh, res, rs, rb, relu, dt):
    t = y.double() * sc.double()
    mag = t.abs() + sh.double().abs()
    ref = t + sh.double()
    n = 2
    if res is not None:
        r = res.double() * rs.double() if rs is not None else res.double()
        ref = ref + r
        mag = mag + r.abs()
        n += 1
        if rb is not None:
            ref = ref + rb.double()
            mag = mag + rb.double().abs()
            n += 1
    if relu:
        ref = ref.clamp_min(0.0)   # |max(a, 0) - max(b, 0)| <= |a - b|
    return ref, stored(sum_bound(n, mag), ref, dt)


def pack_bits(mask_bool):
    """[M][C] bool -> [M][C/8] uint8, bit (c & 7) of byte c / 8"""
    M, C = mask_bool.shape
    w = (1 << torch.arange(8, device=mask_bool.device, dtype=torch.int32)).view(1, 1, 8)
    return (mask_bool.view(M, C // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8).contiguous()


# ----------------------------------------------------------------------------------------------------------------------
# BatchNorm backward: sums, coefficients, dy = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat))
# ----------------------------------------------------------------------------------------------------------------------
BWD_SHAPES = [(1, 8), (7, 64), (255, 64), (6272, 64), (392, 512), (37, 2048)]
BWD_C_ACCEPT = [8, 16, 24, 40, 64, 96, 512, 2048]


def bwd_inputs(M, C, dt, with_mask, seed, device):
    """g (mean 0.5: a real mean(g) term), y (per-channel offsets up to two standard deviations: a real Q*mean term), optional
    mask, and the batch statistics of y computed in float64 and rounded to f32"""
    gen = torch.Generator(device=device).manual_seed(seed)
    g = (torch.randn(M, C, generator=gen, device=device) + 0.5).to(dt)
    sig = 0.5 + torch.rand(C, generator=gen, device=device)
    mu = (torch.rand(C, generator=gen, device=device) * 4 - 2) * sig
    y = (torch.randn(M, C, generator=gen, device=device) * sig + mu).to(dt)
    mask = torch.randn(M, C, generator=gen, device=device).clamp_min(0).to(dt) if with_mask else None
    gamma = 0.5 + torch.rand(C, generator=gen, device=device)
    yd = y.double()
    mean = yd.mean(0)
    var = ((yd - mean) ** 2).mean(0)
    return g, mask, y, mean.float(), (1.0 / torch.sqrt(var + EPS)).float(), gamma


def _masked(g, mask):
    gd = g.double()
    return gd if mask is None else torch.where(mask.double() > 0, gd, torch.zeros_like(gd))


def bwd_sums_ref(g, mask, y, mean, invstd):
    """sum g, sum g*xhat and the sums of magnitudes the bound needs"""
    gm = _masked(g, mask)
    t = gm * ((y.double() - mean.double()) * invstd.double())
    return gm.sum(0), t.sum(0), gm.abs().sum(0), t.abs().sum(0)


def bwd_coef(g, mask, y, mean, invstd, gamma):
    """coef[3][C] f32 from the float64 sums (what a correct finalize hands to the apply pass)"""
    s1, s2, _, _ = bwd_sums_ref(g, mask, y, mean, invstd)
    M = g.shape[0]
    return torch.stack([gamma.double() * invstd.double(), s1 / M, s2 / M]).float().contiguous()


def bwd_apply_ref(g, mask, y, mean, invstd, coef, dt, light):
    """light: the kernel that folds dy = P g + Q y + R with Q = -ca cc invstd, R = -ca cb - Q mean once per thread: four terms,
    |Q y| and |Q mean| in place of |ca xhat cc|"""
    ca, cb, cc = coef.double()
    gm = _masked(g, mask)
    xh = (y.double() - mean.double()) * invstd.double()
    ref = ca * (gm - cb - xh * cc)
    if light:
        Q = ca * cc * invstd.double()
        mag = (ca * gm).abs() + (Q * y.double()).abs() + (ca * cb).abs() + (Q * mean.double()).abs()
        n = 4
    else:
        mag = (ca * gm).abs() + (ca * cb).abs() + (ca * xh * cc).abs()
        n = 3
    return ref, stored(sum_bound(n, mag), ref, dt), gm


def light_route(M, C, dt, mask, g_out):
    """qt_bn_bwd_apply's dispatch: the four-channel kernel needs a grid stride that is a multiple of the groups per row"""
    cgs = C // 4
    lgrid = min(max((M * cgs + 255) // 256, 1), 16384)
    return dt == torch.bfloat16 and mask is None and g_out is None and (lgrid * 256) % cgs == 0 and M * cgs < (1 << 29)


def bwd_partial_rows(M, C):
    """qt_bn_bwd_partial_rows: at most 2048 blocks, each of at least 8 trips of its 256 / (C / 8) row lanes"""
    RL = 256 // (C // 8)
    rpb = max(-(-M // 2048), RL * 8)
    return -(-M // rpb)


def bwd_finalize_ref(partial, count, gamma, invstd, dgamma0, dbeta0, folded):
    """dgamma0 / dbeta0: the pre-filled gradients when accumulating (the f32 add of two values that may cancel), else None"""
    p = partial.double()
    rows, C = p.shape[0], p.shape[2]
    s1, s2 = p[:, 0].sum(0), p[:, 1].sum(0)
    a1, a2 = p[:, 0].abs().sum(0), p[:, 1].abs().sum(0)
    dd = (rows + 8) * 2 * UD
    e1 = dd * a1 + (66 * U * a1 if folded else 0.0)
    e2 = dd * a2 + (66 * U * a2 if folded else 0.0)
    g = gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64, device=p.device)
    ca = g * invstd.double()
    out = {"coef0": (ca, 2 * U * ca.abs())}
    for name, s, e, pre in (("dgamma", s2, e2, dgamma0), ("dbeta", s1, e1, dbeta0)):
        if pre is None:
            out[name] = (s, 2 * U * s.abs() + e)
        else:
            r = s + pre.double()
            out[name] = (r, 2 * U * r.abs() + 2 * U * (s.abs() + pre.double().abs()) + e)
    if count > 0:
        out["coef1"] = (s1 / count, 2 * U * (s1 / count).abs() + e1 / count)
        out["coef2"] = (s2 / count, 2 * U * (s2 / count).abs() + e2 / count)
    else:
        z = torch.zeros_like(s1)
        out["coef1"] = (z, z)
        out["coef2"] = (z, z)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# eval-mode scale / shift (f32 arithmetic: add, sqrt, divide, multiply: 4 roundings)
# ----------------------------------------------------------------------------------------------------------------------
def bn_eval_ref(gamma, beta, rmean, rvar):
    inv = 1.0 / torch.sqrt(rvar.double() + EPS)
    s = gamma.double() * inv
    t = rmean.double() * s
    return {"scale": (s, 4 * U * s.abs()), "invstd": (inv, 4 * U * inv),
            "shift": (beta.double() - t, 4 * U * (beta.double().abs() + t.abs()))}


# ----------------------------------------------------------------------------------------------------------------------
# pooling
# ----------------------------------------------------------------------------------------------------------------------
POOL_HW = [1, 49, 50]
POOL_C = [8, 256, 512]
POOL_BATCH = [1, 5]
POOL_PLACE = [None, (5376, 4608)]   # None: (C, 0)


def pool_inputs(batch, hw, C, dt, seed, device):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, hw, C, generator=g)
    x[:, ::3, 1::4] = 0.0     # exact zeros and negative zeros: x > 0 is false for both
    x[:, 1::3, 2::4] = -0.0
    d = torch.randn(batch, C, generator=g)
    return x.to(device, dt), d.to(device, dt)


def avgpool_ref(x, dt):
    hw = x.shape[1]
    xd = x.double()
    ref = xd.sum(1) / hw
    return ref, stored(sum_bound(hw + 2, xd.abs().sum(1) / hw), ref, dt)   # hw terms, the reciprocal, the product


def avgpool_bwd_ref(d, x, dt):
    hw = x.shape[1]
    ref = torch.where(x.double() > 0, d.double().unsqueeze(1) / hw, torch.zeros((), dtype=torch.float64, device=x.device))
    return ref, stored(sum_bound(1, ref.abs()), ref, dt)


def quad_inputs(B, dt, seed=11):
    """q [B*4][7][7][128] on a grid of 16 levels (-1 .. 2.75 in steps of 1/4: exact in bf16), so that 2x2 windows hold positive
    ties; the largest value of every map (4.0) sits in row 6 and in column 6, which MaxPool2d(2, 2) drops on a 7x7 map"""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randint(0, 16, (B * 4, 7, 7, 128), generator=g).float() - 4.0) / 4.0
    q[:, 6, ::2, :] = 4.0
    q[:, ::2, 6, :] = 4.0
    d = torch.randn(B, 5376, generator=g)
    return q.to(dt), d.to(dt)


def quad_tie_share(q):
    """share of the 3x3 pooling windows whose positive maximum is attained more than once"""
    w = q.float()[:, :6, :6, :].reshape(-1, 3, 2, 3, 2, 128).permute(0, 1, 3, 5, 2, 4).reshape(-1, 4)
    mx = w.max(1, keepdim=True).values
    return float((((w == mx).sum(1) > 1) & (mx[:, 0] > 0)).double().mean())


def quad_pool_ref(q, d, B, ld, col0):
    """F.max_pool2d(q_nchw, 2, 2).flatten(1), quadrants concatenated; and the float64 autograd gradient of
    sum(relu(that) * d) w.r.t. q (the first maximum of a window takes the gradient, ReLU passes it where the maximum > 0)"""
    F = torch.nn.functional
    qd = q.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)    # [B*4][128][7][7]
    pooled = F.max_pool2d(qd, 2, 2).flatten(1).view(B, 4 * 1152)
    dd = d.double()[:, col0:col0 + 4608]
    (torch.relu(pooled) * dd).sum().backward()
    return pooled.detach(), qd.grad.permute(0, 2, 3, 1).contiguous()


# ----------------------------------------------------------------------------------------------------------------------
# dropout: caps from the binomial law of independent keeps with probability 1 - p
# ----------------------------------------------------------------------------------------------------------------------
DROP_ROWS, DROP_COLS = 2048, 512
DROP_P = [0.1, 0.5, 0.9]


def dropout_conditions(keep_a, keep_b, p):
    """keep_a / keep_b: [2048][512] bool masks of two seeds.  Returns a list of (name, value, lo, hi)."""
    N = keep_a.numel()
    pk = 1.0 - float(np.float32(p))
    s = math.sqrt(pk * (1 - pk) / N)
    q = pk * pk + (1 - pk) ** 2
    sq = math.sqrt(q * (1 - q) / N)
    rows, cols = keep_a.shape
    col = keep_a.double().mean(0)
    row = keep_a.double().mean(1)
    sc, sr = math.sqrt(pk * (1 - pk) / rows), math.sqrt(pk * (1 - pk) / cols)
    return [("kept share", float(keep_a.double().mean()), pk - 5 * s, pk + 5 * s),
            ("two seeds agree", float((keep_a == keep_b).double().mean()), q - 5 * sq, q + 5 * sq),
            ("column share min", float(col.min()), pk - 6 * sc, 1.0), ("column share max", float(col.max()), 0.0, pk + 6 * sc),
            ("row share min", float(row.min()), pk - 6 * sr, 1.0), ("row share max", float(row.max()), 0.0, pk + 6 * sr)]


# ----------------------------------------------------------------------------------------------------------------------
# thin GEMM: C[m][n] = relu?(acc? + bias[n] + sum_k A[m][k] B[n][k]),  n = K + 3 terms
# ----------------------------------------------------------------------------------------------------------------------
def gemm_ref(A, B, bias, cprev, relu, cdt):
    """A [M][K], B [N][K] logical views of the values the kernel reads; cprev: the pre-filled C when accumulating"""
    Ad, Bd = A.double(), B.double()
    K = A.shape[1]
    ref = Ad @ Bd.t()
    mag = Ad.abs() @ Bd.abs().t()
    if bias is not None:
        ref = ref + bias.double()
        mag = mag + bias.double().abs()
    if cprev is not None:
        ref = ref + cprev.double()
        mag = mag + cprev.double().abs()
    if relu:
        ref = ref.clamp_min(0.0)
    return ref, stored(sum_bound(K + 3, mag), ref, cdt)


F32, BF16 = torch.float32, torch.bfloat16
# (name, M, N, K, a_dtype, b_dtype, c_dtype, a k-strided, b k-strided, bias, relu, accumulate, C row padding, A offset); a case of
# 15 entries also pads the ROWS of both k-contiguous operands by that many (non-zero) elements, the way the fused feature matrix
# does: what a K loop reads past K is then in the buffer and in the result
GEMM_CASES = [
    # thread kernel (K <= 96)
    ("thread 5x94x47", 5, 94, 47, F32, F32, F32, 0, 0, 1, 1, 0, 0, 0),
    ("thread 1x1x1", 1, 1, 1, F32, F32, F32, 0, 0, 0, 0, 0, 0, 0),
    ("thread 3x12x96", 3, 12, 96, BF16, BF16, BF16, 0, 0, 1, 0, 0, 5, 0),
    ("thread 7x5x3", 7, 5, 3, F32, BF16, F32, 0, 0, 0, 1, 1, 0, 0),
    ("thread wgrad 94x47x5", 94, 47, 5, F32, F32, F32, 1, 1, 0, 0, 1, 0, 0),
    # wave kernel (K > 96, M or N < 32, not vectorisable)
    ("wave K=97", 3, 5, 97, F32, F32, F32, 0, 0, 1, 0, 0, 0, 0),
    ("wave K=257", 3, 5, 257, BF16, BF16, F32, 0, 0, 0, 1, 0, 3, 0),
    ("wave K=2688 A k-strided", 3, 12, 2688, F32, F32, F32, 1, 0, 1, 0, 1, 0, 0),
    ("wave K=100 (K % 8)", 3, 5, 100, BF16, F32, BF16, 0, 0, 1, 1, 0, 0, 0),
    ("wave f32 x bf16", 3, 12, 104, F32, BF16, F32, 0, 0, 0, 0, 0, 0, 0),
    ("wave A offset by 4", 3, 12, 104, BF16, BF16, F32, 0, 0, 1, 0, 0, 0, 4),
    ("wave f32 A offset by 4", 2, 40, 320, F32, F32, F32, 0, 0, 0, 0, 0, 0, 4),
    # K % 256 in (128, 192]: the only residues at which the bound of the 4 x 64 unrolled trip decides between trip and tail
    ("wave K=161 padded rows", 3, 5, 161, F32, F32, F32, 0, 0, 1, 0, 0, 0, 0, 95),
    ("wave K=449 padded rows", 2, 3, 449, BF16, F32, F32, 0, 0, 0, 0, 0, 0, 0, 63),
    # wave-vec kernel
    ("vec 3x12x2688 bf16 x bf16", 3, 12, 2688, BF16, BF16, BF16, 0, 0, 1, 0, 0, 4, 0),
    ("vec 3x12x2688 bf16 x f32", 3, 12, 2688, BF16, F32, F32, 0, 0, 1, 1, 0, 0, 0),
    ("vec 3x12x2688 f32 x f32", 3, 12, 2688, F32, F32, F32, 0, 0, 0, 0, 1, 0, 0),
    ("vec K=104", 5, 3, 104, BF16, BF16, F32, 0, 0, 0, 0, 0, 0, 0),
    ("vec K=2056", 2, 3, 2056, F32, F32, F32, 0, 0, 1, 0, 0, 0, 0),
    ("vec K=2056 bf16", 33, 3, 2056, BF16, BF16, F32, 0, 0, 0, 1, 1, 0, 0),
]
_TILE_DT = [(F32, F32, F32), (BF16, F32, F32), (F32, BF16, BF16), (BF16, BF16, BF16)]
_i = 0
for _M, _N, _K in [(33, 35, 97), (32, 32, 128), (64, 100, 188)]:
    for _ak in (0, 1):
        for _bk in (0, 1):
            _a, _b, _c = _TILE_DT[_i % 4]
            GEMM_CASES.append((f"tile {_M}x{_N}x{_K} a{'k' if _ak else 'r'} b{'k' if _bk else 'r'}", _M, _N, _K, _a, _b, _c,
                               _ak, _bk, _i % 2, (_i // 2) % 2, (_i // 3) % 2, 3 * (_i % 3 == 0), 0))
            _i += 1


def gemm_operands(case, device, seed=0):
    """storage tensors + the logical [M][K] / [N][K] views + strides, from one case tuple"""
    name, M, N, K, adt, bdt, cdt, ak, bk, has_bias, relu, acc, cpad, aoff = case[:14]
    rpad = case[14] if len(case) > 14 else 0
    g = torch.Generator().manual_seed(1000 + seed)

    def operand(R, dt, kstr, off):
        if kstr:   # stored [K][R]: row stride 1, k stride R
            flat = torch.randn(off + R * K, generator=g).to(device, dt)
            return flat, flat[off:], flat[off:].view(K, R).t(), 1, R
        flat = torch.randn(off + R * (K + rpad), generator=g).to(device, dt)
        return flat, flat[off:], flat[off:].view(R, K + rpad)[:, :K], K + rpad, 1

    fa, a_body, A, ars, aks = operand(M, adt, ak, aoff)
    fb, b_body, B, brs, bks = operand(N, bdt, bk, 0)
    bias = torch.randn(N, generator=g).to(device) if has_bias else None
    crs = N + cpad
    cfill = torch.randn(M, N, generator=g).to(device, cdt)
    return dict(a_keep=fa, b_keep=fb, a_ptr=a_body, b_ptr=b_body, A=A, B=B, ars=ars, aks=aks, brs=brs, bks=bks, bias=bias,
                crs=crs, cfill=cfill if acc else None)
