"""Float64 statements of the two Grad-CAM rules of include/qtcnn.h and the error bounds of the f32 kernels that evaluate them
(csrc/gradcam.hip), derived from the operations those kernels perform.  u = 2^-24, gamma(n) = n u / (1 - n u).

The map.  w_c = (sum_p grad[c,p]) / P, s_p = sum_c w_c act[c,p], r_p = max(s_p, 0), peak = max_p r_p, cam_p = r_p / peak.
  * Pooled weight: P - 1 additions in some fixed order and one division, every rounding relative to a partial sum of
    |grad[c,.]|:  |w^_c - w_c| <= e_c = gamma(P + 1) mean_p |grad[c,p]|.
  * Channel sum: a chain of fused multiply-adds (one rounding each, the product exact) inside a channel group, then the
    group sums, then the chunk sums.  A term passes through at most ceil(n/G) + min(G, n) - 1 <= n roundings inside a chunk
    of n <= 32 channels split over G groups and through k - 1 more over k chunks, and 32 + k - 1 <= C whenever k > 1: the
    summation depth is at most C, so
      |s^_p - s_p| <= E_p = sum_c e_c |act[c,p]| + gamma(C) sum_c (|w_c| + e_c) |act[c,p]|.
  * max(., 0) and max_p are exact and 1-Lipschitz: |r^_p - r_p| <= E_p, |peak^ - peak| <= Em = max_q E_q.
  * Division: |r^_p / peak^ - r_p / peak| <= (E_p + cam_p Em) / peak^ with peak^ >= peak - Em, then one rounding of a
    quotient that is at most 1:
      |cam^_p - cam_p| <= (E_p + cam_p Em) / (peak - Em) (1 + u) + u          (infinite unless peak > Em).
  The bound is homogeneous: scaling act or grad by a power of two scales E_p and peak alike (no underflow or overflow at the
  2^-40 .. 2^40 the tests use).  It blows up when the pooled weights cancel (gradients of zero channel mean): such inputs
  are ill-conditioned for every evaluation order and are not what the bound test feeds.

The overlay.  v = the four-tap sample, idx = v > 0 ? min(255, int(255 v)) : 0, out = uint8(floor(alpha lut[idx] + (1 - alpha) frame)).
  * Coordinate: the kernel rounds the scale src/dst once (relative u) and evaluates f = fma(d + 0.5, scale, -0.5) with d + 0.5
    exact: |f^ - f| <= u (d + 0.5) src/dst + u |f^| <= 2 u (src + 1) = dcoord(src); t = f - floor(f) is exact.  The sample is
    continuous and piecewise linear in f (the clamped taps included), with slope at most the largest difference D between
    two values of the map: a coordinate error moves it by at most dcoord D, also across a change of floor(f).
  * Lerp: a + t (b - a) as fma(t, fl(b - a), a), two roundings: off by at most u t |b - a| + u |result| <= 3 u M, M = max |map|
    (and exact when both taps are equal).  The second level takes the two row results, each off by 3 u M, with weights that
    add up to 1, and adds 3 u M of its own: 6 u M and second-order terms, gamma(7) M.
      |heat^ - v| <= eps = (dcoord(w) + dcoord(h)) D + gamma(7) M.
  * Index: 255 v is rounded once more (relative u), and v -> idx is monotone, so the kernel's index lies in
    [idx(v - eps'), idx(v + eps')], eps' = eps + u |v|: one or two admissible values while 255 eps' < 1.
  * Blend: f32 evaluation of a number in [0, 255] is off by far less than 1, but floor may land on either side of an
    integer: out is within 1 of floor(alpha lut[i] + (1 - alpha) frame) in float64 for one admissible i, in all three
    channels.  alpha = 0 and alpha = 1 are exact (fma(0, c, 1 f) = f, fma(1, c, 0 f) = c).
"""
import numpy as np

U = 2.0 ** -24
CAM_BOUND_CAP = 2.0 ** -10      # below one colour index (1 / 255)
MAP_SHAPES = ((1, 512, 49), (3, 70, 15), (2, 64, 1), (2, 1024, 98), (1, 8, 65), (2, 256, 1024), (1, 5, 2048))
GRAD_FORMS = ("noisy", "broadcast")


def gamma(n):
    return n * U / (1.0 - n * U)


def make_inputs(B, C, P, form, seed):
    """act = relu(N(0,1)); grad = m_c (1 + 0.25 N(0,1)) ('noisy') or m_c at every position ('broadcast', what the served
    hooks deliver: the layer feeds a global average pool), m_c ~ N(0.5, 1).  f32 [B,C,P] each."""
    rng = np.random.default_rng(1000 * seed + 7 * C + P)
    act = np.maximum(rng.standard_normal((B, C, P)), 0.0).astype(np.float32)
    m = 0.5 + rng.standard_normal((B, C, 1))
    noise = rng.standard_normal((B, C, P))
    grad = m * (1.0 + 0.25 * noise) if form == "noisy" else np.broadcast_to(m, (B, C, P))
    return act, np.ascontiguousarray(grad, dtype=np.float32)


def cam_ref(act, grad):
    """(cam [B,P], peak [B]) in float64; NaN is carried by both maxima as the rule says"""
    a, g = act.astype(np.float64), grad.astype(np.float64)
    w = g.mean(axis=2)
    with np.errstate(invalid="ignore"):
        s = np.einsum("bc,bcp->bp", w, a)
        s = np.where(np.isnan(a).any(axis=1) | np.isnan(w).any(axis=1)[:, None], np.nan, s)   # einsum may skip 0 * NaN
        r = np.maximum(s, 0.0)
        peak = r.max(axis=1)
        cam = np.where(peak[:, None] == 0.0, 0.0, r / np.where(peak == 0.0, 1.0, peak)[:, None])
    return cam, peak


def cam_bound(act, grad):
    """(bound on |cam^ - cam| [B,P], bound on |peak^ - peak| [B]) by the derivation above"""
    a, g = np.abs(act.astype(np.float64)), grad.astype(np.float64)
    B, C, P = a.shape
    w = g.mean(axis=2)
    e = gamma(P + 1) * np.abs(g).mean(axis=2)
    E = np.einsum("bc,bcp->bp", e, a) + gamma(C) * np.einsum("bc,bcp->bp", np.abs(w) + e, a)
    Em = E.max(axis=1)
    cam, peak = cam_ref(act, grad)
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = (E + cam * Em[:, None]) / (peak - Em)[:, None] * (1.0 + U) + U
    bound = np.where((peak > Em)[:, None], bound, np.inf)
    return bound, Em


def cam_ref_torch(act, grad):
    """the reference's recipe (resnet/grad_cam_analysis.py:306-324) with stock torch CPU ops in double, image by image"""
    import torch
    out = []
    for i in range(act.shape[0]):
        a = torch.from_numpy(act[i:i + 1]).double().clone()        # [1,C,P]
        g = torch.from_numpy(grad[i:i + 1]).double()
        pooled = torch.mean(g, dim=[2])
        for j in range(a.shape[1]):
            a[0, j, :] *= pooled[0, j]
        heat = torch.nn.functional.relu(torch.sum(a, dim=1).squeeze(0)).numpy()
        heat = np.maximum(heat, 0)
        heat = np.zeros_like(heat) if np.max(heat) == 0 else heat / np.max(heat)
        out.append(heat)
    return np.stack(out)


# ---- overlay ----------------------------------------------------------------------------------------------------------------
def _axis(dst, src):
    f = (np.arange(dst, dtype=np.float64) + 0.5) * (src / dst) - 0.5
    fl = np.floor(f)
    i = fl.astype(np.int64)
    return np.clip(i, 0, src - 1), np.clip(i + 1, 0, src - 1), f - fl


def heat_ref(cam, H, W):
    """float64 [B,H,W]: bilinear sample, half-pixel centres, taps clamped at the border"""
    c = cam.astype(np.float64)
    h, w = c.shape[1:]
    y0, y1, ty = _axis(H, h)
    x0, x1, tx = _axis(W, w)
    with np.errstate(invalid="ignore"):
        top = (1.0 - tx) * c[:, y0][:, :, x0] + tx * c[:, y0][:, :, x1]
        bot = (1.0 - tx) * c[:, y1][:, :, x0] + tx * c[:, y1][:, :, x1]
        return (1.0 - ty)[None, :, None] * top + ty[None, :, None] * bot


def heat_bound(cam):
    """eps [B,1,1] of the derivation above, per image (NaN for an image whose map holds a NaN)"""
    c = cam.astype(np.float64)
    h, w = c.shape[1:]
    flat = c.reshape(c.shape[0], -1)
    D = flat.max(axis=1) - flat.min(axis=1)
    M = np.abs(flat).max(axis=1)
    eps = (2.0 * U * (w + 1) + 2.0 * U * (h + 1)) * D + gamma(7) * M
    return eps[:, None, None]


def _idx(v):
    with np.errstate(invalid="ignore"):
        return np.where(v > 0.0, np.minimum(255.0, np.floor(255.0 * np.where(v > 0.0, v, 0.0))), 0.0).astype(np.int64)


def admissible(cam, H, W):
    """(lo, hi) int64 [B,H,W]: the kernel's colour index lies in lo .. hi; a NaN sample admits 0 only"""
    v, eps = heat_ref(cam, H, W), heat_bound(cam)
    e = eps + U * np.abs(v)
    lo, hi = _idx(v - e), _idx(v + e)
    nan = np.isnan(v)
    return np.where(nan, 0, lo), np.where(nan, 0, hi)


def blend_ref(lut, idx, frames, alpha):
    """floor(alpha lut[idx] + (1 - alpha) frame) in float64 with the f32 alpha the kernel receives: int64 [B,H,W,3]"""
    a = float(np.float32(alpha))
    return np.floor(a * lut.astype(np.float64)[idx] + (1.0 - a) * frames.astype(np.float64)).astype(np.int64)


def check_overlay(out, lohi, frames, lut, alpha, index=None):
    """every pixel of `out` within 1 of the float64 blend for one admissible index in all three channels (the index the kernel
    reports, when it reports one, which must itself be admissible).  lohi = admissible(cam, H, W).  Returns the largest
    number of admissible indices of a pixel."""
    lo, hi = lohi
    span = int((hi - lo).max()) + 1
    assert span <= 2, f"{span} admissible indices: the bound is too loose to test anything"
    o = out.astype(np.int64)
    if index is not None:
        ix = index.astype(np.int64)
        assert ((ix >= lo) & (ix <= hi)).all(), "a reported colour index is not admissible"
        ok = (np.abs(o - blend_ref(lut, ix, frames, alpha)) <= 1).all(axis=3)
    else:
        ok = np.zeros(lo.shape, dtype=bool)
        for k in range(span):
            ok |= (np.abs(o - blend_ref(lut, np.minimum(lo + k, hi), frames, alpha)) <= 1).all(axis=3)
    assert ok.all(), f"{int((~ok).sum())} of {ok.size} pixels are outside the admissible blend"
    return span


def make_frames(B, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)


def make_cam(B, h, w, seed):
    """a map as qt_gradcam_map leaves it: values in [0, 1], the maximum 1, some exact zeros"""
    rng = np.random.default_rng(seed)
    c = np.maximum(rng.standard_normal((B, h * w)), 0.0)
    c[:, 0] += 0.25   # never all zero
    return (c / c.max(axis=1, keepdims=True)).astype(np.float32).reshape(B, h, w)
