"""Float64 reference and the DERIVED f32 error bound of the frame-preprocessing kernel (csrc/preprocess.hip), shared by
tests/test_preprocess_cpu.py (the reference against torch and PIL, a torch-f32 restatement of the kernel's operation order
against the bound) and tests/test_preprocess_gpu.py (the kernel against the same reference and bound).

The rule, per axis with crop length `in` and output length `out` (torch's antialiased bilinear resize):
    scale = in / out, support = max(scale, 1), center = scale (i + 0.5)
    taps j in [max(floor(center - support + 0.5), 0), min(floor(center + support + 0.5), in)), relative to the crop
    raw weight max(0, 1 - |(j - center + 0.5) / support|), divided by the sum over the taps
    value = sum_y w_y sum_x w_x u8;  out = (value / 255 - mean[c]) * inv_std[c];  a flip reverses the output columns

What the kernel does with it, and what each step costs in units of u = 2^-24 relative to A = sum |w_y| |w_x| u8 / 255 * inv_std
(all terms are non-negative, so A is the normalised value before the mean is taken off):
    w_j = float(m_j) / float(M), m_j = 2 max(in,out) - |2 out j + out - in (2i+1)| and M = sum m_j exact integers:
        one rounding of M, one division                                           2 per axis            -> 4
    horizontal sum of taps_x terms, fused multiply-adds, u8 exact in f32           taps_x
    vertical sum of taps_y terms over the f32 row sums                             taps_y
    scale_c = f32(inv_std / 255) formed on the host in double                       1
    out = fma(value, scale_c, shift_c): one rounding of |out| <= A + |mean inv_std|  1  (and 1 on the mean term)
    one tap at a window's end that the float64 window has and the integer window has not (or the reverse): its weight
        is a few f64 ulp, far below u; counted as                                   1
    second-order terms (products of the above)                                      1
    => c = 8
    shift_c = f32(-mean inv_std) formed on the host in double: one rounding, plus the fma's: 2 u |mean inv_std|.  With
        round-to-nearest each relative error is at most u / (1 + u), so the two and their product stay below 2 u.
  bound = u * ((taps_x + taps_y + 8) * A + 2 |mean[c] inv_std[c]|)
The second term is what is left at a black pixel, where A = 0 and the output is the rounded constant -mean inv_std.
Nothing here is fitted to what the kernel returns."""
import math

import torch

U = 2.0 ** -24
C_OPS = 8
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


MEAN32 = tuple(f32(m) for m in MEAN)              # what the descriptor carries
INV_STD32 = tuple(f32(1.0 / s) for s in STD)


# ---------------------------------------------------------------------------------------------------------------------
# windows and weights
# ---------------------------------------------------------------------------------------------------------------------
def window_f64(i, n_in, n_out):
    """(lo, [normalised weights]) by the rule as stated, in float64"""
    scale = n_in / n_out
    support = max(scale, 1.0)
    center = scale * (i + 0.5)
    lo = max(int(math.floor(center - support + 0.5)), 0)
    hi = min(int(math.floor(center + support + 0.5)), n_in)
    raw = [max(0.0, 1.0 - abs((j - center + 0.5) / support)) for j in range(lo, hi)]
    s = sum(raw)
    return lo, [r / s for r in raw]


def window_int(i, n_in, n_out):
    """(lo, [m_j]) with both ends and every raw weight in exact integers: center * 2 out = in (2i + 1)"""
    c2 = n_in * (2 * i + 1)
    sup2 = 2 * max(n_in, n_out)
    lo = max((c2 - sup2 + n_out) // (2 * n_out), 0)       # Python's // floors
    hi = min((c2 + sup2 + n_out) // (2 * n_out), n_in)
    return lo, [max(0, sup2 - abs(2 * n_out * j + n_out - c2)) for j in range(lo, hi)]


def axis_matrix(n_in, n_out):
    """float64 [n_out][n_in] resampling matrix of the rule, and the taps per output index that the kernel sums"""
    W = torch.zeros(n_out, n_in, dtype=torch.float64)
    taps = torch.zeros(n_out, dtype=torch.float64)
    for i in range(n_out):
        lo, w = window_f64(i, n_in, n_out)
        W[i, lo:lo + len(w)] = torch.tensor(w, dtype=torch.float64)
        taps[i] = len(window_int(i, n_in, n_out)[1])
    return W, taps


def box_valid(box, H, W):
    t, l, h, w = box
    return t >= 0 and l >= 0 and h >= 1 and w >= 1 and t + h <= H and l + w <= W


def reference(frames, boxes, flips, out_hw, bgr=False, mean=MEAN32, inv_std=INV_STD32):
    """frames: uint8 [N,H,W,3] (CPU); boxes: list of (top, left, height, width) or None; flips: list or None.
    Returns (ref, bound, grey): float64 [N,3,h,w] each; grey is the resized crop in grey levels before normalisation.
    An image whose box is not inside the frame is NaN in all three."""
    N, H, W, _ = frames.shape
    h, w = out_hw
    ref = torch.full((N, 3, h, w), float("nan"), dtype=torch.float64)
    bound = torch.full_like(ref, float("nan"))
    grey = torch.full_like(ref, float("nan"))
    cache = {}
    for b in range(N):
        box = (0, 0, H, W) if boxes is None else tuple(int(v) for v in boxes[b])
        if not box_valid(box, H, W):
            continue
        t, l, bh, bw = box
        if (bh, h) not in cache:
            cache[(bh, h)] = axis_matrix(bh, h)
        if (bw, w) not in cache:
            cache[(bw, w)] = axis_matrix(bw, w)
        (Wy, ty), (Wx, tx) = cache[(bh, h)], cache[(bw, w)]
        crop = frames[b, t:t + bh, l:l + bw, :].double().permute(2, 0, 1)      # [3][bh][bw]
        if bgr:
            crop = crop.flip(0)
        g = Wy @ crop @ Wx.t()                                                   # [3][h][w], all terms >= 0
        n = (ty.view(h, 1) + tx.view(1, w) + C_OPS).expand(3, h, w)
        if flips is not None and int(flips[b]):
            g, n = g.flip(-1), n.flip(-1)
        m = torch.tensor(mean, dtype=torch.float64).view(3, 1, 1)
        s = torch.tensor(inv_std, dtype=torch.float64).view(3, 1, 1)
        grey[b] = g
        ref[b] = (g / 255.0 - m) * s
        bound[b] = U * (n * (g / 255.0 * s.abs()) + 2.0 * (m * s).abs())
    return ref, bound, grey


def ratio(got, ref, bound):
    """max |got - ref| / bound over the finite part of the reference (inf for a non-finite result there)"""
    ok = torch.isfinite(ref)
    g = got.double()[ok]
    if not bool(torch.isfinite(g).all()):
        return float("inf")
    return float(((g - ref[ok]).abs() / bound[ok]).max()) if g.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's operation order in torch f32 (fused multiply-adds formed in double and rounded once)
# ---------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _axis_f32(n_in, n_out, shift=0, renormalise=True):
    """lo [n_out], weights f32 [n_out][kmax] (zero past each window): float(m_j) / float(M).
    shift: move every window by that many taps (a wrong version); renormalise=False: divide by the sum over the window
    before it is clipped to the crop (the other wrong version)."""
    los, ws = [], []
    for i in range(n_out):
        lo, m = window_int(i, n_in, n_out)
        M = sum(m)
        if not renormalise:
            c2, sup2 = n_in * (2 * i + 1), 2 * max(n_in, n_out)
            lo_u, hi_u = (c2 - sup2 + n_out) // (2 * n_out), (c2 + sup2 + n_out) // (2 * n_out)
            M = sum(max(0, sup2 - abs(2 * n_out * j + n_out - c2)) for j in range(lo_u, hi_u))
        los.append(min(max(lo + shift, 0), n_in - 1))
        ws.append(torch.tensor(m, dtype=torch.float32) / torch.tensor(float(M), dtype=torch.float32))
    kmax = max(len(x) for x in ws)
    Wm = torch.zeros(n_out, kmax)
    for i, x in enumerate(ws):
        Wm[i, :len(x)] = x
    return torch.tensor(los), Wm


def kernel_f32(frames, boxes, flips, out_hw, bgr=False, mean=MEAN32, inv_std=INV_STD32, shift=0, renormalise=True):
    N, H, W, _ = frames.shape
    h, w = out_hw
    out = torch.full((N, 3, h, w), float("nan"))
    for b in range(N):
        box = (0, 0, H, W) if boxes is None else tuple(int(v) for v in boxes[b])
        if not box_valid(box, H, W):
            continue
        t, l, bh, bw = box
        crop = frames[b, t:t + bh, l:l + bw, :].float().permute(2, 0, 1)
        if bgr:
            crop = crop.flip(0)
        xlo, wx = _axis_f32(bw, w, shift, renormalise)
        ylo, wy = _axis_f32(bh, h, shift, renormalise)
        hor = torch.zeros(3, bh, w)
        for k in range(wx.shape[1]):                                   # ascending taps, as the kernel
            hor = _fma(wx[:, k].view(1, 1, w), crop[:, :, (xlo + k).clamp(max=bw - 1)], hor)
        acc = torch.zeros(3, h, w)
        for k in range(wy.shape[1]):
            acc = _fma(wy[:, k].view(1, h, 1), hor[:, (ylo + k).clamp(max=bh - 1), :], acc)
        sc = torch.tensor([f32(float(s) / 255.0) for s in inv_std]).view(3, 1, 1)
        sh = torch.tensor([f32(-float(m) * float(s)) for m, s in zip(mean, inv_std)]).view(3, 1, 1)
        r = _fma(acc, sc, sh)
        out[b] = r.flip(-1) if flips is not None and int(flips[b]) else r
    return out


# ---------------------------------------------------------------------------------------------------------------------
# cases: (name, src_h, src_w, boxes or None, out_h, out_w); the batch is len(boxes) (1 for None unless stated)
# ---------------------------------------------------------------------------------------------------------------------
CASES = [
    ("downscale interior box", 97, 131, [(5, 7, 85, 113)], 24, 24),
    ("upscale", 20, 28, None, 64, 64),
    ("10x by 1x", 240, 30, None, 24, 30),
    ("four borders", 64, 80, [(0, 0, 40, 50), (24, 30, 40, 50), (0, 30, 64, 50), (10, 0, 54, 80)], 20, 27),
    ("one pixel wide / high", 30, 40, [(2, 5, 20, 1), (7, 3, 1, 30)], 8, 8),
    ("odd output width", 37, 53, [(1, 1, 33, 50)], 16, 23),
    ("three column tiles, odd width", 45, 310, [(2, 3, 40, 300)], 19, 131),
    ("24x on both axes", 96, 1560, None, 4, 65),
    ("realistic", 270, 480, [(0, 0, 270, 480), (13, 21, 250, 440)], 224, 224),
]
IDENTITY = ("box equal to output", 40, 50, [(3, 4, 24, 30)], 24, 30)


def make_frames(n, H, W, seed, row_pad=0, image_pad=0):
    """random NON-ZERO uint8 frames [n][H][W][3] as a view into a buffer whose padding (row_pad bytes after each row,
    image_pad bytes after each image) holds 255.  Returns (view, buffer)."""
    g = torch.Generator().manual_seed(seed)
    rs = 3 * W + row_pad
    ims = H * rs + image_pad
    buf = torch.full((n * ims,), 255, dtype=torch.uint8)
    view = buf.as_strided((n, H, W, 3), (ims, rs, 3, 1))
    view.copy_(torch.randint(1, 256, (n, H, W, 3), generator=g, dtype=torch.uint8))
    return view, buf


def case_inputs(case, seed=0):
    name, H, W, boxes, h, w = case
    n = 1 if boxes is None else len(boxes)
    frames, _ = make_frames(n, H, W, 100 + seed)
    return frames, boxes, (h, w)
