"""The rule of qt_annotate_u8 (include/qtcnn.h) restated in numpy int64 (every value fits: |cross| < 2^31), frame by frame
and primitive by primitive in painter's order, plus the inputs the annotation tests share.  Everything here is exact: the
only floating-point steps are the ones the rule names, an f32 product per landmark coordinate and rintf(confidence * 100)."""
import functools
import math

import numpy as np

NUM_LANDMARKS = 33
MAX_SEGMENTS = 64
COORD_LO, COORD_HI = np.float32(-8192.0), np.float32(16383.0)
GROW = 16                        # a primitive reaches at most max(T / 2, r) <= 15 pixels beyond its end points

# mp.solutions.pose.POSE_CONNECTIONS (35 pairs) and draw_enhanced_skeleton's twelve thick ones
POSE_CONNECTIONS = ((0, 1), (1, 2), (2, 3), (3, 7), (0, 4), (4, 5), (5, 6), (6, 8), (9, 10), (11, 12), (11, 13), (13, 15),
                    (15, 17), (15, 19), (15, 21), (17, 19), (12, 14), (14, 16), (16, 18), (16, 20), (16, 22), (18, 20),
                    (11, 23), (12, 24), (23, 24), (23, 25), (24, 26), (25, 27), (26, 28), (27, 29), (28, 30), (29, 31),
                    (30, 32), (27, 31), (28, 32))
MAJOR_SEGMENTS = ((11, 12), (23, 24), (11, 23), (12, 24), (11, 13), (12, 14), (13, 15), (14, 16), (23, 25), (24, 26),
                  (25, 27), (26, 28))


class Style:
    """qt_annotate_desc without the sizes; the defaults are FrameAnnotator's for BGR frames"""

    def __init__(self, **kw):
        self.min_visibility = 0.65
        self.thick_major, self.thick_minor, self.radius_hi, self.radius_lo = 5, 2, 3, 2
        self.line_hi, self.line_lo = (245, 66, 230), (0, 165, 255)
        self.point_hi, self.point_lo = (245, 117, 66), (0, 0, 255)
        self.origin = (10, 10)
        self.caption_colour = (0, 255, 0)
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


def default_segments():
    major = {frozenset(p) for p in MAJOR_SEGMENTS}
    return np.array([[a, b, int(frozenset((a, b)) in major)] for a, b in POSE_CONNECTIONS], np.uint8)


def pixel_positions(landmarks, H, W):
    """landmarks f32 [33,4] -> (P int64 [33,2], usable bool [33]): the f32 product truncated toward zero"""
    lm = np.asarray(landmarks, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        fx, fy = lm[:, 0] * np.float32(W), lm[:, 1] * np.float32(H)
        assert fx.dtype == np.float32
        usable = (fx >= COORD_LO) & (fx <= COORD_HI) & (fy >= COORD_LO) & (fy <= COORD_HI)     # false for NaN and inf
    P = np.zeros((NUM_LANDMARKS, 2), np.int64)
    P[usable, 0] = np.trunc(fx[usable]).astype(np.int64)
    P[usable, 1] = np.trunc(fy[usable]).astype(np.int64)
    return P, usable


def segment_covers(xs, ys, ax, ay, bx, by, T):
    """4 dist^2(q, segment AB) <= T^2 for the int64 pixel grids xs, ys, as the header evaluates it"""
    ax, ay, bx, by, T = int(ax), int(ay), int(bx), int(by), int(T)
    dx, dy = bx - ax, by - ay
    ex, ey = xs - ax, ys - ay
    L = dx * dx + dy * dy
    t = ex * dx + ey * dy
    at_a = 4 * (ex * ex + ey * ey) <= T * T
    if L == 0:
        return at_a
    fx, fy = xs - bx, ys - by
    at_b = 4 * (fx * fx + fy * fy) <= T * T
    cross = ex * dy - ey * dx
    assert np.abs(cross).max(initial=0) < 2 ** 31
    between = cross * cross <= (T * T * L) // 4
    return np.where(t <= 0, at_a, np.where(t >= L, at_b, between))


def disc_covers(xs, ys, cx, cy, r):
    ex, ey = xs - int(cx), ys - int(cy)
    return ex * ex + ey * ey <= int(r) * int(r)


def _window(H, W, xa, xb, ya, yb):
    """the part of the frame a primitive with end points in [xa, xb] x [ya, yb] can reach: slices and grids, or None"""
    x0, x1 = max(0, min(xa, xb) - GROW), min(W, max(xa, xb) + GROW + 1)
    y0, y1 = max(0, min(ya, yb) - GROW), min(H, max(ya, yb) + GROW + 1)
    if x0 >= x1 or y0 >= y1:
        return None
    ys, xs = np.mgrid[y0:y1, x0:x1].astype(np.int64)
    return (slice(y0, y1), slice(x0, x1)), xs, ys


def draw_skeleton(frame, landmarks, segments, style):
    """one frame [H,W,3], in place: the segments in list order, then the 33 discs"""
    H, W = frame.shape[:2]
    P, usable = pixel_positions(landmarks, H, W)
    vis = np.asarray(landmarks, np.float32)[:, 3]
    with np.errstate(invalid="ignore"):
        high = vis > np.float32(style.min_visibility)                    # a NaN visibility is low
    for a, b, major in np.asarray(segments, np.int64).reshape(-1, 3):
        if a > 32 or b > 32 or not (usable[a] and usable[b]):
            continue
        T = style.thick_major if major else style.thick_minor
        win = _window(H, W, P[a, 0], P[b, 0], P[a, 1], P[b, 1])
        if win is None:
            continue
        where, xs, ys = win
        hit = segment_covers(xs, ys, P[a, 0], P[a, 1], P[b, 0], P[b, 1], T)
        frame[where][hit] = style.line_hi if (high[a] and high[b]) else style.line_lo
    for j in range(NUM_LANDMARKS):
        if not usable[j]:
            continue
        win = _window(H, W, P[j, 0], P[j, 0], P[j, 1], P[j, 1])
        if win is None:
            continue
        where, xs, ys = win
        hit = disc_covers(xs, ys, P[j, 0], P[j, 1], style.radius_hi if high[j] else style.radius_lo)
        frame[where][hit] = style.point_hi if high[j] else style.point_lo


def confidence_digits(confidence):
    """(d0, d1, d2) of n = clamp((int)rintf(confidence * 100.0f), 0, 100), or None for a NaN"""
    c = np.float32(confidence)
    if np.isnan(c):
        return None
    with np.errstate(over="ignore"):
        r = np.rint(c * np.float32(100.0))
    n = int(min(max(r, np.float32(0.0)), np.float32(100.0)))
    return n // 100, n // 10 % 10, n % 10


def glyph_sequence(pred, confidence, C):
    """the atlas tiles of one frame's caption: [] when pred is outside [0, C)"""
    pred = int(pred)
    if not 0 <= pred < C:
        return []
    seq = [pred]
    digits = None if confidence is None else confidence_digits(confidence)
    if digits is not None:
        d0, d1, d2 = digits
        seq += [C + 13, C + 11, C + d0, C + 10, C + d1, C + d2, C + 12]      # ' ' '(' d0 '.' d1 d2 ')'
    return seq


def draw_caption(frame, glyphs, atlas, widths, style):
    """one frame, in place: the tiles at their pens, blended where the mask is > 0, clipped to the frame"""
    H, W = frame.shape[:2]
    gh, gw = atlas.shape[1:]
    pen, oy = int(style.origin[0]), int(style.origin[1])
    colour = np.array(style.caption_colour, np.int64)
    for g in glyphs:
        w = int(widths[g])
        if not 0 <= w <= gw:
            w = 0
        x0, x1 = max(pen, 0), min(pen + w, W)
        y0, y1 = max(oy, 0), min(oy + gh, H)
        if x0 < x1 and y0 < y1:
            m = atlas[g, y0 - oy:y1 - oy, x0 - pen:x1 - pen].astype(np.int64)[:, :, None]
            under = frame[y0:y1, x0:x1].astype(np.int64)
            blend = (m * colour + (255 - m) * under + 127) // 255
            frame[y0:y1, x0:x1] = np.where(m > 0, blend, under).astype(np.uint8)
        pen += w


def annotate(frames, landmarks=None, detected=None, segments=None, pred=None, confidence=None, atlas=None, widths=None,
             style=None):
    """frames uint8 [B,H,W,3] -> the annotated copy"""
    style = style or Style()
    out = np.array(frames, np.uint8, copy=True)
    for b in range(out.shape[0]):
        if landmarks is not None and (detected is None or detected[b] != 0):
            draw_skeleton(out[b], landmarks[b], segments, style)
        if pred is not None:
            C = atlas.shape[0] - 14
            glyphs = glyph_sequence(pred[b], None if confidence is None else confidence[b], C)
            draw_caption(out[b], glyphs, atlas, widths, style)
    return out


# ---- shared inputs ----------------------------------------------------------------------------------------------------------
def make_frames(B, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def make_landmarks(B, seed):
    """f32 [B,33,4]: x, y mostly inside the frame, some a little outside; visibility on both sides of 0.65"""
    rng = np.random.default_rng(seed)
    lm = np.empty((B, NUM_LANDMARKS, 4), np.float32)
    lm[:, :, :2] = rng.uniform(-0.1, 1.1, (B, NUM_LANDMARKS, 2))
    lm[:, :, 2] = rng.uniform(-1, 1, (B, NUM_LANDMARKS))
    lm[:, :, 3] = rng.uniform(0.3, 1.0, (B, NUM_LANDMARKS))
    return lm


def edge_landmarks(H, W):
    """One frame's landmarks placed by hand, as (landmarks f32 [33,4], segments uint8 [n,3]).  Pixel positions are put in as
    (p + 0.5) / size, whose f32 product truncates to p for the sizes the tests use (asserted)."""
    lm = np.zeros((NUM_LANDMARKS, 4), np.float32)
    lm[:, 3] = 0.9

    def put(j, px, py, vis=0.9):
        half = lambda p: p + 0.5 if p >= 0 else p - 0.5      # truncation is toward zero
        lm[j] = (np.float32(half(px) / W), np.float32(half(py) / H), 0.0, vis)

    def exactly(value, size):
        """an f32 whose f32 product with `size` is exactly `value`, or None"""
        x = np.float32(value / size)
        for cand in [x] + [f(x, np.float32(d)) for d in (np.inf, -np.inf) for f in (np.nextafter,)]:
            if cand * np.float32(size) == np.float32(value):
                return cand
        return None

    put(0, 0, 0)                        # on each border ...
    put(1, W - 1, 0)
    put(2, W - 1, H - 1)
    put(3, 0, H - 1)
    put(4, -1, H // 2)                  # ... and just outside it
    put(5, W, H // 2)
    put(6, W // 2, -1)
    put(7, W // 2, H)
    put(8, W // 3, H // 3)              # coincident end points (8, 9)
    put(9, W // 3, H // 3)
    put(10, 5, H // 2)                  # horizontal (10, 11), vertical (10, 12), 45 degrees (10, 13)
    put(11, 5 + min(W, H) // 3, H // 2)
    put(12, 5, H // 2 + min(W, H) // 3)
    put(13, 5 + min(W, H) // 3, H // 2 + min(W, H) // 3)
    far_x, far_y = exactly(16383.0, W), exactly(16383.0, H)   # usable: the last value of the range, on either axis
    assert far_x is not None or far_y is not None, (H, W)
    lm[14, :2] = (far_x, 0.5) if far_x is not None else (0.5, far_y)
    lm[15, :2] = (np.float32(16384.0 / W), 0.5)       # not usable
    lm[16, :2] = (np.nan, 0.5)
    lm[17, :2] = (0.5, np.inf)
    lm[18, :2] = (-np.inf, 0.5)
    put(19, W // 2, H // 2, vis=np.nan)                # a NaN visibility is low
    put(20, W // 2 + 7, H // 2 + 3, vis=0.2)
    put(21, -40, -40)                   # far outside: nothing of it reaches the frame
    for j in range(22, NUM_LANDMARKS):
        put(j, (j * 37) % W, (j * 53) % H, vis=0.9 if j % 2 else 0.5)
    P, usable = pixel_positions(lm, H, W)
    assert usable[14] and 16383 in P[14] and not usable[15:19].any() and usable[:14].all() and usable[19:].all()
    assert (P[0] == (0, 0)).all() and (P[2] == (W - 1, H - 1)).all() and (P[4] == (-1, H // 2)).all() and P[5, 0] == W
    assert (P[8] == P[9]).all() and P[10, 1] == P[11, 1] and P[10, 0] == P[12, 0]
    assert P[13, 0] - P[10, 0] == P[13, 1] - P[10, 1] > 0
    seg = [(0, 1, 1), (1, 2, 0), (2, 3, 1), (3, 0, 0), (4, 5, 1), (6, 7, 0), (8, 9, 1), (8, 9, 0), (10, 11, 1), (10, 12, 0),
           (10, 13, 1), (13, 10, 0), (10, 14, 1), (10, 15, 1), (16, 10, 0), (17, 10, 1), (18, 10, 1), (19, 20, 1), (20, 22, 0),
           (200, 10, 1), (10, 33, 1), (21, 21, 1), (22, 29, 1), (23, 30, 0), (24, 31, 1), (25, 32, 0), (0, 2, 1), (1, 3, 0)]
    return lm, np.array(seg, np.uint8)


@functools.lru_cache(maxsize=None)
def make_atlas(C=5, gh=11, gw=9, seed=77):
    """a synthetic atlas: random masks with zeros, 255s and everything between; widths 0, gw, gw + 1 and ordinary ones"""
    rng = np.random.default_rng(seed)
    atlas = rng.integers(0, 256, (C + 14, gh, gw), dtype=np.uint8)
    atlas[rng.random(atlas.shape) < 0.3] = 0
    atlas[rng.random(atlas.shape) < 0.1] = 255
    widths = rng.integers(1, gw + 1, C + 14).astype(np.int32)
    widths[0] = gw                      # class 0: the full tile
    widths[1] = 0                       # class 1: nothing, the confidence follows at once
    widths[2] = gw + 1                  # class 2: out of range, counts as 0
    widths[C + 13] = gw                 # ' '
    widths[C + 10] = 0                  # '.'
    widths[C + 12] = gw + 1             # ')'
    atlas.setflags(write=False)
    widths.setflags(write=False)
    return atlas, widths


# ---- the kernel's own walk, restated ----------------------------------------------------------------------------------------
def restated(frames, landmarks=None, detected=None, segments=None, pred=None, confidence=None, atlas=None, widths=None,
             style=None, out_mod16=0, in_place=False):
    """csrc/annotate.hip step by step in Python integers: per frame the head / 16-pixel groups / tail that follow from the
    address of `out` modulo 16, 4096-pixel tiles, the tile's list (grown bounding boxes, rectangles beside a stroke), each
    thread's sub-list, the
    backward walk with the narrowed tests (e.e <= floor(T^2 / 4), |cross| <= floor(sqrt(K)), every factor of a product below
    2^23), the caption's pens.  Pixels the kernel does not store
    keep the value 0xA5 (out of place) or the frame's (in place); the result must equal annotate() everywhere."""
    style = style or Style()
    B, H, W, _ = frames.shape
    HW = H * W
    out = frames.copy() if in_place else np.full_like(frames, 0xA5)
    tiles = max(1, -(-(HW // 16) // 256))
    for b in range(B):
        src, dst = frames[b].reshape(HW, 3), out[b].reshape(HW, 3)
        m = (out_mod16 + 3 * HW * b) % 16
        head = min((5 * m) % 16, HW)
        groups = (HW - head) // 16
        tail = HW - head - 16 * groups
        # 1. landmarks, caption
        skeleton = landmarks is not None and (detected is None or detected[b] != 0)
        prims = []               # (box, A, d, L, R2, M, colour) or None, in painter's order
        if skeleton:
            P, usable = pixel_positions(landmarks[b], H, W)
            with np.errstate(invalid="ignore"):
                high = np.asarray(landmarks[b], np.float32)[:, 3] > np.float32(style.min_visibility)
            todo = [(int(a), int(c), True, bool(mj)) for a, c, mj in np.asarray(segments).reshape(-1, 3)]
            todo += [(j, j, False, False) for j in range(NUM_LANDMARKS)]
            for ia, ib, is_seg, major in todo:
                if ia > 32 or ib > 32 or not (usable[ia] and usable[ib]):
                    prims.append(None)
                    continue
                if is_seg:
                    T = style.thick_major if major else style.thick_minor
                    R2, grow, T2 = T * T // 4, (T + 1) // 2, T * T
                    colour = style.line_hi if (high[ia] and high[ib]) else style.line_lo
                else:
                    r = style.radius_hi if high[ia] else style.radius_lo
                    R2, grow, T2 = r * r, r, 0
                    colour = style.point_hi if high[ia] else style.point_lo
                ax, ay, bx, by = int(P[ia, 0]), int(P[ia, 1]), int(P[ib, 0]), int(P[ib, 1])
                dx, dy = bx - ax, by - ay
                L = dx * dx + dy * dy
                assert L < 2 ** 31
                box = (min(ax, bx) - grow, min(ay, by) - grow, max(ax, bx) + grow, max(ay, by) + grow)
                prims.append((box, (ax, ay), (dx, dy), L, R2, math.isqrt((T2 * L) >> 2), colour))
        glyphs, pens = [], []
        if pred is not None:
            C = atlas.shape[0] - 14
            glyphs = glyph_sequence(pred[b], None if confidence is None else confidence[b], C)
            pen = int(style.origin[0])
            for g in glyphs:
                w = int(widths[g])
                pens.append(pen)
                pen += w if 0 <= w <= atlas.shape[2] else 0
            pens.append(pen)
        oy, gh = int(style.origin[1]), (atlas.shape[1] if atlas is not None else 1)
        cap_box = (pens[0], oy, pens[-1] - 1, oy + gh - 1) if glyphs else (0, 0, -1, -1)

        def mul24(u, v):
            assert -2 ** 23 <= u < 2 ** 23 and -2 ** 23 <= v < 2 ** 23 and abs(u * v) < 2 ** 30
            return u * v

        def meets(box, span):
            return box[0] <= span[2] and box[2] >= span[0] and box[1] <= span[3] and box[3] >= span[1]

        def beside(prim, span):
            # the rectangle lies wholly to one side of the stroke: cross is affine, its extremes are at the corners
            _, (ax, ay), (dx, dy), _, _, M, _ = prim
            c = [mul24(x - ax, dy) - mul24(y - ay, dx) for x in (span[0], span[2]) for y in (span[1], span[3])]
            return min(c) > M or max(c) < -M

        def reaches(prim, span):
            return meets(prim[0], span) and not beside(prim, span)

        def span_of(p0, p1):
            y0 = p0 // W
            x0 = p0 - y0 * W
            return (x0, y0, x0 + p1 - p0, y0) if x0 + (p1 - p0) < W else (0, y0, W - 1, p1 // W)

        def covers(prim, x, y):
            _, (ax, ay), (dx, dy), L, R2, M, _ = prim
            ex, ey = x - ax, y - ay
            t = mul24(ex, dx) + mul24(ey, dy)
            if L == 0 or t <= 0:
                return mul24(ex, ex) + mul24(ey, ey) <= R2
            if t >= L:
                return mul24(ex - dx, ex - dx) + mul24(ey - dy, ey - dy) <= R2
            return abs(mul24(ex, dy) - mul24(ey, dx)) <= M

        def shade(q, mine, my_cap):
            y, x = divmod(q, W)
            c = tuple(int(v) for v in src[q])
            for i in reversed(mine):
                if covers(prims[i], x, y):
                    c = prims[i][6]
                    break
            if my_cap and oy <= y < oy + gh and pens[0] <= x < pens[-1]:
                k = 0
                while x >= pens[k + 1]:
                    k += 1
                mk = int(atlas[glyphs[k], y - oy, x - pens[k]])
                if mk:
                    c = tuple((mk * cc + (255 - mk) * u + 127) // 255 for cc, u in zip(style.caption_colour, c))
            return c

        for tile in range(tiles):
            first, last = tile == 0, tile == tiles - 1
            p0 = 0 if first else head + tile * 4096
            p1 = (HW if last else head + (tile + 1) * 4096) - 1
            assert p1 >= p0
            T_span = span_of(p0, p1)
            listed = [i for i, p in enumerate(prims) if p is not None and reaches(p, T_span)]
            tile_cap = cap_box[2] >= cap_box[0] and meets(cap_box, T_span)
            if not listed and not tile_cap and in_place:
                continue

            def run(q0, n):
                span = span_of(q0, q0 + n - 1)
                mine = [i for i in listed if reaches(prims[i], span)]
                my_cap = tile_cap and meets(cap_box, span)
                if not mine and not my_cap and in_place:
                    return
                for q in range(q0, q0 + n):
                    assert p0 <= q <= p1
                    dst[q] = shade(q, mine, my_cap) if (mine or my_cap) else src[q]

            for tid in range(256):
                g = tile * 256 + tid
                if g < groups:
                    run(head + 16 * g, 16)
                if first and tid < head:
                    run(tid, 1)
                if last and tid < tail:
                    run(head + 16 * groups + tid, 1)
    return out
