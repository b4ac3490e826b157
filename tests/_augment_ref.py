"""Float64 reference and the DERIVED f32 error bound of the frame-augmentation kernel (csrc/augment.hip), shared by
tests/test_augment_cpu.py (the reference's pieces against torch's own ops, a torch-f32 restatement of the kernel's operation
order against the bound) and tests/test_augment_gpu.py (the kernel against the same reference and bound).

The rule is the one include/qtcnn.h states (torchvision's float-tensor path): jitter ops in the row's order, nearest-neighbour
rotation with fill 0, separable reflected Gaussian blur, (v - mean) * inv_std.

The bound walks the same stages and carries a per-pixel absolute error e next to the value, u = 2^-24, from the kernel's own
operation order (a compiler that fuses a multiply into an add only removes a rounding):
  brightness  out = clamp(f a): one product.                                 e' = f e + u |f a|
  grey        fma(0.114, b, fma(0.587, g, 0.2989 r)): three roundings and three rounded constants, each at most u grey
              (all terms >= 0).                                              e_g = 0.2989 e_r + 0.587 e_g + 0.114 e_b + 4 u grey
  saturation  out = clamp(fma(f, a, t)), t = (1 - f) grey: 1 - f rounded, the product rounded, the fma rounded.
                                                    e' = f e + |1-f| e_g + u (2 |1-f| grey + f |a| + |1-f| grey)
  contrast    the same with m = sum / float(h w) for grey.  The sum: a thread adds ceil(chunk / 256) pixels in order, a binary
              tree over 256 threads (8 levels), 16 partials in order; all terms >= 0, so every partial sum is at most the total
              and the sum carries (ceil(chunk / 256) + 8 + 16) u; the division and float(h w) 2 more.
                                                    e_m = mean(e_g) + (ceil(chunk / 256) + 26) u m
  hue         exact map: out_c = V - CR phi_c(6 h + 6 shift), V = maxc, CR = maxc - minc, phi piecewise linear with slopes
              0, +-1, 6 h = k + (x - y) / CR.  For channel perturbations of at most e: |dV| <= e, |dCR| <= 2 e,
              CR d(6h) = d(x - y) - (x - y) / CR dCR, at most 4 e, so |d out| <= e + 2 e + 4 e = 7 e; the map is continuous
              across its sectors and at CR -> 0, so 7 e holds globally.  That is what keeps the bound valid near grey pixels:
              h is ill-conditioned there, but it only ever acts through CR phi.
              own roundings, inputs exact: CR rel. u, s = CR / maxc rel. 2 u, rc, gc, bc rel. 3 u (each in [0, 1]);
              h_raw abs. <= 16 u (worst branch 4 + gc - rc); / 6 + 1: 16/6 u + u + 2 u; fmod exact; + shift: 1.5 u; mod 1: u
              => h' abs. <= 9 u; 6 h': 6 * 9 u + 6 u = 60 u, and the output depends on 6 h' with slope at most V s = CR:
              60 u CR.  f = 6 h' - floor exact.  p = V (1 - s): 4 u V; q = V (1 - s f): 5 u V; t = V (1 - s (1 - f)): 6 u V.
                                                    e' = 7 max_c e + u (6 V + 60 CR)       (all three channels)
  rotation    a copy (or the fill 0): e' = e at the source pixel.  Undecided pixels (a float64 source coordinate within 1e-3
              of a half-integer) are left out of every comparison, or the angles are chosen so that there is none.
  blur        raw_k = exp(t_k), t_k = -0.5 (d / sigma)^2: t_k carries 3 roundings (relative), so exp(t_k) is off by
              3 u |t_k| relative, plus the function's own error and rounding, 3 u: rho_k = (3 |t_k| + 3) u.  S = sum raw_k in
              order: dS / S <= sum w_k rho_k + K u.  w_k = raw_k / S: |dw_k| <= w_k (rho_k + u + dS / S) =: ew_k.
              row pass, fma chain of kx terms:   e_r = blur_x(|T|; ewx) + kx u blur_x(|T|; wx) + blur_x(e; wx)
              column pass the same with ky on |R| <= blur_x(|T|; wx).
              (A raw weight below the f32 range is flushed to 0: an absolute 1e-38.)
  normalise   out = fma(v, inv_std, shift), shift = f32(-mean inv_std) formed on the host in double:
                                                    e' = |inv_std| e + u (|v inv_std| + 2 |mean inv_std|)
  and 2^-10 of the total for the products of the above.
Nothing here is fitted to what the kernel returns."""
import functools
import itertools
import math

import torch

U = 2.0 ** -24
PARTS = 16                 # QT_AUGMENT_PARTS
HUE_LIP, HUE_V, HUE_H = 7.0, 6.0, 60.0
SECOND_ORDER = 1.0 + 2.0 ** -10
UNDECIDED = 1e-3
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
NAN = float("nan")


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


MEAN32 = tuple(f32(m) for m in MEAN)
INV_STD32 = tuple(f32(1.0 / s) for s in STD)
NO_NORM = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


# ---------------------------------------------------------------------------------------------------------------------
# parameter rows
# ---------------------------------------------------------------------------------------------------------------------
def row(b=1.0, c=1.0, s=1.0, hue=0.0, order=(), deg=None, cs=1.0, sn=0.0, sigma=1.0):
    """one parameter row as 12 Python floats (rounded to f32 when the tensor is made); deg overrides (cs, sn)"""
    if deg is not None:
        cs, sn = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    slots = list(order) + [-1] * (4 - len(order))
    return [b, c, s, hue] + [float(x) for x in slots] + [cs, sn, sigma, 0.0]


def rows(list_of_rows):
    return torch.tensor(list_of_rows, dtype=torch.float32)


def row_valid(p, blur_on, use_contrast=True):
    p = [float(x) for x in p]
    if not all(math.isfinite(x) for x in p):
        return False
    ids = []
    for s in p[4:8]:
        if s == -1.0:
            continue
        if s not in (0.0, 1.0, 2.0, 3.0) or s in ids:
            return False
        ids.append(s)
    if blur_on and not p[10] > 0.0:
        return False
    if not use_contrast and 1.0 in ids:
        return False
    return True


# ---------------------------------------------------------------------------------------------------------------------
# the rule in float64: img is [3][h][w]
# ---------------------------------------------------------------------------------------------------------------------
def grey(img):
    return 0.2989 * img[0] + 0.587 * img[1] + 0.114 * img[2]


def blend(a, b, f):
    return torch.clamp(f * a + (1.0 - f) * b, 0.0, 1.0)       # torch.clamp keeps a NaN


def rgb_to_hsv(img):
    r, g, b = img[0], img[1], img[2]
    maxc = torch.max(img, dim=0).values                       # torch.max / min carry a NaN
    minc = torch.min(img, dim=0).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    crd = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / crd, (maxc - g) / crd, (maxc - b) / crd
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    return h, s, maxc


def hsv_to_rgb(h, s, v):
    i = torch.floor(h * 6.0)
    f = h * 6.0 - i
    nan = torch.isnan(i)
    k = torch.where(nan, torch.zeros_like(i), i).to(torch.int64) % 6
    p = torch.clamp(v * (1.0 - s), 0.0, 1.0)
    q = torch.clamp(v * (1.0 - s * f), 0.0, 1.0)
    t = torch.clamp(v * (1.0 - s * (1.0 - f)), 0.0, 1.0)
    table = ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))
    out = torch.zeros((3,) + tuple(h.shape), dtype=h.dtype)
    for c in range(3):
        for n in range(6):
            out[c] = torch.where(k == n, table[n][c], out[c])
        out[c] = torch.where(nan, torch.full_like(h, NAN), out[c])
    return out


def hue(img, shift):
    h, s, v = rgb_to_hsv(img)
    h = torch.remainder(h + shift, 1.0)
    return hsv_to_rgb(h, s, v)


def rotation_map(h, w, cs, sn):
    """float64 source coordinates (column xf, row yf) of every output pixel, [h][w] each"""
    j = torch.arange(w, dtype=torch.float64).view(1, w)
    i = torch.arange(h, dtype=torch.float64).view(h, 1)
    x = j + 0.5 - w / 2.0
    y = i + 0.5 - h / 2.0
    xf = cs * x - sn * y + w / 2.0 - 0.5
    yf = sn * x + cs * y + h / 2.0 - 0.5
    return xf, yf


def undecided_mask(h, w, cs, sn):
    xf, yf = rotation_map(h, w, cs, sn)
    near = lambda t: ((t - torch.floor(t)) - 0.5).abs() < UNDECIDED
    return near(xf) | near(yf)


def gather(img, sx, sy):
    """img [C][h][w] at integer (float64) source column sx / row sy, 0 outside"""
    _, h, w = img.shape
    inside = (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
    ix = sx.clamp(0, w - 1).long()
    iy = sy.clamp(0, h - 1).long()
    return torch.where(inside.unsqueeze(0), img[:, iy, ix], torch.zeros((), dtype=img.dtype))


def rotate(img, cs, sn):
    _, h, w = img.shape
    xf, yf = rotation_map(h, w, cs, sn)
    return gather(img, torch.round(xf), torch.round(yf))


def rotation_candidates(img, cs, sn):
    """the images an undecided pixel may take its value from: floor / ceil on each axis"""
    _, h, w = img.shape
    xf, yf = rotation_map(h, w, cs, sn)
    return [gather(img, fx(xf), fy(yf)) for fx in (torch.floor, torch.ceil) for fy in (torch.floor, torch.ceil)]


def taps(K, sigma):
    """normalised weights and the exponents t_k, float64"""
    d = torch.arange(K, dtype=torch.float64) - K // 2
    t = -0.5 * (d / sigma) ** 2
    raw = torch.exp(t)
    return raw / raw.sum(), t


def tap_errors(K, sigma):
    """ew_k >= |f32 weight - float64 weight| (docstring, blur)"""
    w, t = taps(K, sigma)
    if K == 1:
        return w, torch.zeros_like(w)          # the kernel sets the single raw weight to 1: 1 / 1 is exact
    rho = (3.0 * t.abs() + 3.0) * U
    dS = float((w * rho).sum()) + K * U
    return w, w * (rho + U + dS)


def _reflect_index(n, r):
    idx = torch.arange(-r, n + r)
    idx = torch.where(idx < 0, -idx, idx)
    return torch.where(idx >= n, 2 * (n - 1) - idx, idx)


def tap_filter(img, weights, dim):
    """out[i] = sum_k weights[k] img[reflect(i + k - K // 2)] along dim, the border reflected without repeating the edge; a
    NaN reaches exactly the outputs whose window holds it, as in the kernel"""
    n, K = img.shape[dim], len(weights)
    idx = _reflect_index(n, K // 2)
    out = torch.zeros_like(img)
    for k in range(K):
        out = out + float(weights[k]) * img.index_select(dim, idx[k:k + n])
    return out


def blur(img, kx, ky, sigma):
    return tap_filter(tap_filter(img, taps(kx, sigma)[0], 2), taps(ky, sigma)[0], 1)


def reference(images, params, kx=1, ky=1, norm=NO_NORM, use_contrast=True):
    """images f32 / f64 [N,3,h,w] (CPU), params f32 [N,12].  Returns (ref, bound, undecided): float64 [N,3,h,w] twice and a
    bool [N,h,w] of the outputs that an undecided rotation pixel reaches (through the blur window).  A malformed row gives
    NaN in ref and bound."""
    N, _, h, w = images.shape
    mean, inv_std = norm
    ref = torch.full((N, 3, h, w), NAN, dtype=torch.float64)
    bound = torch.full_like(ref, NAN)
    und = torch.zeros(N, h, w, dtype=torch.bool)
    blur_on = kx * ky > 1
    n_t = math.ceil(math.ceil(h * w / PARTS) / 256)
    for n in range(N):
        p = [float(x) for x in params[n]]
        if not row_valid(p, blur_on, use_contrast):
            continue
        v = images[n].double().clone()
        e = torch.zeros_like(v)

        def grey_err(v, e):
            return 0.2989 * e[0] + 0.587 * e[1] + 0.114 * e[2] + 4.0 * U * grey(v.abs())

        for slot in p[4:8]:
            if slot == 0.0:
                f = p[0]
                e = f * e + U * (f * v).abs()
                v = blend(v, torch.zeros_like(v), f)
            elif slot == 1.0 or slot == 2.0:
                f = p[int(slot)]
                g1 = abs(1.0 - f)
                g0, eg = grey(v), grey_err(v, e)
                if slot == 1.0:
                    eg = eg.mean() + (n_t + 8 + PARTS + 2) * U * g0.abs().mean()
                    g0 = g0.mean()
                e = f * e + g1 * eg + U * (2.0 * g1 * g0.abs() + f * v.abs() + g1 * g0.abs())
                v = blend(v, g0, f)
            elif slot == 3.0:
                V = torch.max(v, dim=0).values
                CR = V - torch.min(v, dim=0).values
                e = (HUE_LIP * e.max(dim=0).values + U * (HUE_V * V + HUE_H * CR)).expand(3, h, w).clone()
                v = hue(v, p[3])
        cs, sn = p[8], p[9]
        xf, yf = rotation_map(h, w, cs, sn)
        v = gather(v, torch.round(xf), torch.round(yf))
        e = gather(e, torch.round(xf), torch.round(yf))
        u_mask = undecided_mask(h, w, cs, sn).double().unsqueeze(0)
        if blur_on:
            sigma = p[10]
            (wx, ewx), (wy, ewy) = tap_errors(kx, sigma), tap_errors(ky, sigma)
            a = torch.nan_to_num(v.abs())                    # magnitudes only: a NaN value has no bound to meet
            e = torch.nan_to_num(e)
            a_r = tap_filter(a, wx, 2)
            e_r = tap_filter(a, ewx, 2) + kx * U * a_r + tap_filter(e, wx, 2)
            e = tap_filter(a_r, ewy, 1) + ky * U * tap_filter(a_r, wy, 1) + tap_filter(e_r, wy, 1)
            v = tap_filter(tap_filter(v, wx, 2), wy, 1)
            u_mask = tap_filter(tap_filter(u_mask, torch.ones(kx), 2), torch.ones(ky), 1)
        m = torch.tensor(mean, dtype=torch.float64).view(3, 1, 1)
        s = torch.tensor(inv_std, dtype=torch.float64).view(3, 1, 1)
        e = s.abs() * e + U * ((v * s).abs() + 2.0 * (m * s).abs())
        ref[n] = (v - m) * s
        bound[n] = torch.where(torch.isnan(ref[n]), torch.full_like(e, NAN), torch.nan_to_num(e) * SECOND_ORDER)
        und[n] = u_mask[0] > 0
    return ref, bound, und


def ratio(got, ref, bound, skip=None):
    """max |got - ref| / bound over the finite part of the reference outside `skip` [N,h,w] (inf for a non-finite result
    there; a zero bound asks for equality)"""
    ok = torch.isfinite(ref)
    if skip is not None:
        ok = ok & ~skip.unsqueeze(1)
    g = got.double()[ok]
    if not bool(torch.isfinite(g).all()):
        return float("inf")
    if not g.numel():
        return 0.0
    d, b = (g - ref[ok]).abs(), bound[ok]
    r = torch.where(d == 0, torch.zeros_like(d), d / b)
    return float(r.max())


def same_nan_pattern(got, ref):
    return bool((torch.isnan(got) == torch.isnan(ref)).all())


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's operation order in torch f32 (fused multiply-adds formed in double and rounded once)
# ---------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _t32(x):
    return torch.tensor(x, dtype=torch.float32)


def _clamp32(v):
    return torch.clamp(v, 0.0, 1.0)


def _grey32(v):
    return _fma(_t32(0.114), v[2], _fma(_t32(0.587), v[1], _t32(0.2989) * v[0]))


def _hue32(v, shift):
    r, g, b = v[0], v[1], v[2]
    bad = torch.isnan(r) | torch.isnan(g) | torch.isnan(b)
    maxc = torch.max(v, dim=0).values
    minc = torch.min(v, dim=0).values
    cr = maxc - minc
    eq = cr == 0
    one = torch.ones_like(cr)
    s = cr / torch.where(eq, one, maxc)
    crd = torch.where(eq, one, cr)
    rc, gc, bc = (maxc - r) / crd, (maxc - g) / crd, (maxc - b) / crd
    hh = torch.where(maxc == r, bc - gc, torch.where(maxc == g, (2.0 + rc) - bc, (4.0 + gc) - rc))
    hh = hh / 6.0 + 1.0
    hh = hh - torch.floor(hh)
    hh = hh + _t32(shift)
    hh = hh - torch.floor(hh)
    h6 = 6.0 * hh
    fi = torch.floor(h6)
    f = h6 - fi
    k = torch.nan_to_num(fi).long() % 6
    p = _clamp32(maxc * (1.0 - s))
    q = _clamp32(maxc * (1.0 - s * f))
    t = _clamp32(maxc * (1.0 - s * (1.0 - f)))
    table = ((maxc, t, p), (q, maxc, p), (p, maxc, t), (p, q, maxc), (t, p, maxc), (maxc, p, q))
    out = torch.zeros_like(v)
    for c in range(3):
        for n in range(6):
            out[c] = torch.where(k == n, table[n][c], out[c])
        out[c] = torch.where(bad, torch.full_like(out[c], NAN), out[c])
    return out


def _taps32(K, sigma):
    if K == 1:
        return torch.ones(1)
    d = torch.arange(K, dtype=torch.float32) - K // 2
    q = d / _t32(sigma)
    raw = torch.exp(-0.5 * (q * q))
    S = torch.zeros(())
    for k in range(K):
        S = S + raw[k]
    return raw / S


def kernel_f32(images, params, kx=1, ky=1, norm=NO_NORM, use_contrast=True, hue_sector_bug=False):
    """hue_sector_bug: a wrong version that takes the triple of sector i + 1 (it must miss the bound)"""
    N, _, h, w = images.shape
    mean, inv_std = norm
    out = torch.full((N, 3, h, w), NAN)
    blur_on = kx * ky > 1
    chunk = math.ceil(h * w / PARTS)
    for n in range(N):
        p32 = params[n].float()
        p = [float(x) for x in p32]
        if not row_valid(p, blur_on, use_contrast):
            continue
        v = images[n].float().clone()
        for slot in p[4:8]:
            if slot == 0.0:
                v = _clamp32(p32[0] * v)
            elif slot == 1.0:
                g = _grey32(v).flatten()
                parts = []
                for c0 in range(0, h * w, chunk):                       # a workgroup's chunk
                    seg = g[c0:c0 + chunk]
                    pad = torch.zeros(256 * math.ceil(seg.numel() / 256))
                    pad[:seg.numel()] = seg
                    lanes = pad.view(-1, 256)
                    acc = torch.zeros(256)
                    for rrow in lanes:                                  # thread t adds its pixels in order
                        acc = acc + rrow
                    sz = 128
                    while sz >= 1:                                      # the binary tree
                        acc = acc[:sz] + acc[sz:2 * sz]
                        sz //= 2
                    parts.append(acc[0])
                total = torch.zeros(())
                for part in parts:
                    total = total + part
                m = total / _t32(float(h * w))
                term = (1.0 - p32[1]) * m
                v = _clamp32(_fma(p32[1], v, term))
            elif slot == 2.0:
                term = (1.0 - p32[2]) * _grey32(v)
                v = _clamp32(_fma(p32[2], v, term))
            elif slot == 3.0:
                v = _hue32(v, p[3])
                if hue_sector_bug:
                    v = v.roll(1, 0)
        cs, sn = p32[8], p32[9]
        x = (torch.arange(w, dtype=torch.float32).view(1, w) + 0.5) - 0.5 * w
        y = (torch.arange(h, dtype=torch.float32).view(h, 1) + 0.5) - 0.5 * h
        xs = _fma(cs, x, -(sn * y))
        ys = _fma(sn, x, cs * y)
        sx = torch.round(xs + (0.5 * w - 0.5))
        sy = torch.round(ys + (0.5 * h - 0.5))
        v = gather(v, sx.double(), sy.double())
        wx, wy = _taps32(kx, p[10]), _taps32(ky, p[10])
        T = v[:, _reflect_index(h, ky // 2)][:, :, _reflect_index(w, kx // 2)]
        R = torch.zeros(3, h + 2 * (ky // 2), w)
        for k in range(kx):
            R = _fma(wx[k], T[:, :, k:k + w], R)
        acc = torch.zeros(3, h, w)
        for k in range(ky):
            acc = _fma(wy[k], R[:, k:k + h, :], acc)
        sc = torch.tensor([f32(s) for s in inv_std]).view(3, 1, 1)
        sh = torch.tensor([f32(-float(f32(m)) * float(f32(s))) for m, s in zip(mean, inv_std)]).view(3, 1, 1)
        out[n] = _fma(acc, sc, sh)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# inputs and cases
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(18, 21), (33, 130)]          # less than one 16 x 64 tile; ragged tiles on both axes, halos across tile borders
ORDERS = list(itertools.permutations(range(4)))
# 80 stands in for 90: at 90 degrees every source coordinate is a half-integer when h + w is odd (18 x 21, 33 x 130), so every
# pixel is undecided there
ANGLES = [10.0, -10.0, 3.7, -3.7, 80.0, 180.0, 45.0]


def make_images(n, h, w, seed):
    """random f32 images in [0, 1] whose first rows hold pure grey, black, white and saturated-primary pixels"""
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(n, 3, h, w, generator=g)
    special = torch.tensor([[0.5, 0.5, 0.5], [0, 0, 0], [1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1],
                            [1, 0, 1], [0.25, 0.25, 0.25], [1, 1, 0.999], [0.3, 0.3, 0.3000001]])
    k = min(w, special.shape[0])
    img[:, :, 0, :k] = special[:k].t()
    img[:, :, h - 1, w - k:] = special[:k].t()
    return img


def jitter_rows():
    """24 rows, one per order of the four ops, factors at both ends of the reference's ranges"""
    out = []
    for i, order in enumerate(ORDERS):
        lo = i % 2 == 0
        out.append(row(b=0.8 if lo else 1.2, c=1.2 if lo else 0.8, s=0.8 if (i // 2) % 2 else 1.2,
                       hue=0.1 if (i // 3) % 2 else -0.1, order=order))
    return rows(out)


def pythagorean_angles(limit_deg):
    """(cos, sin) with rational entries (m^2 - n^2, 2 m n) / (m^2 + n^2), by rising denominator, both signs: rotated pixel
    centres then fall on a lattice of that denominator, and a lattice that misses the half-integers leaves no pixel
    undecided"""
    out = []
    for m in range(2, 40):
        for n in range(1, m):
            if math.gcd(m, n) != 1 or (m - n) % 2 == 0:
                continue
            a, b, c = m * m - n * n, 2 * m * n, m * m + n * n
            for lo, hi in ((a, b), (b, a)):
                if math.degrees(math.asin(lo / c)) <= limit_deg:
                    out.append((c, hi / c, lo / c))
                    out.append((c, hi / c, -lo / c))
    return [(cs, sn) for _, cs, sn in sorted(out)]


@functools.lru_cache(maxsize=None)
def decided_angles(h, w, count=2, limit_deg=10.0):
    """the first `count` rotations of at most limit_deg (the reference's RandomRotation(10)) that leave no pixel of an h x w
    image undecided; a deterministic search, asserted by the CPU test"""
    found = []
    for cs, sn in pythagorean_angles(limit_deg):
        cs, sn = f32(cs), f32(sn)
        if not bool(undecided_mask(h, w, cs, sn).any()):
            found.append((cs, sn))
            if len(found) == count:
                return tuple(found)
    raise AssertionError(f"no decided rotation within {limit_deg} degrees at {h} x {w}")


CHAIN_SHAPES = [(24, 40), (33, 130)]


def chain_rows(h, w):
    """the reference's configuration: all four ops in four different orders, searched angles, sigma at both ends and between"""
    ang = decided_angles(h, w)
    cfg = [((0, 1, 2, 3), 0.8, 1.2, 0.9, 0.1, ang[0], 0.1), ((3, 2, 1, 0), 1.2, 0.8, 1.2, -0.1, ang[1], 0.5),
           ((2, 0, 3, 1), 1.1, 1.1, 0.8, 0.05, ang[0], 0.3), ((1, 3, 0, 2), 0.9, 0.9, 1.1, -0.03, ang[1], 0.45)]
    return rows([row(b=b, c=c, s=s, hue=hu, order=o, cs=a[0], sn=a[1], sigma=sg) for o, b, c, s, hu, a, sg in cfg])


def nan_case():
    """three 33 x 130 images, the middle one all NaN, turned by 45 degrees (no undecided pixel at this shape): the corners'
    fill stays 0 where the blur does not reach the NaN"""
    img = make_images(3, 33, 130, 23)
    img[1] = NAN
    return img, rows([row(order=(0, 2, 3), b=1.1, s=0.9, hue=0.05, deg=45.0, sigma=0.5)] * 3)
