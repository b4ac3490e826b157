"""Float64 statement of the sequence-feature rule of include/qtcnn.h (qt_pose_sequence_features) and the error bound of the
f32 kernel that evaluates it (csrc/pose_seq.hip), vectorised over frames; the per-clip history as the plain loop the
reference runs (a deque of two, pushed on detection only), and a Python walk of the kernel's tiling and backward search.

The rule is written once (`_rule`) over an arithmetic object:
  Bounded   every quantity is a pair (value in float64, bound on the distance of the kernel's f32 value from it), with the
            operations of tests/_pose_ref.py (its module text derives each of them): + - * / and sqrtf correctly rounded,
            u = 2^-24 relative per operation on top of the operands' bounds carried through, a contracted multiply-add
            covered by the two roundings of the model; sqrtf at ULP_SQRT and atan2f at ULP_ATAN2 ulp; an angle moves by at
            most asin(|(e_x, e_y)| / |(x, y)|) with its arguments; a quotient by (e_a + |a / b| e_b) / (|b| - e_b).
  Plain32   numpy float32, operation by operation, without contraction, numpy's float64 arctan2 rounded to f32 for atan2f:
            a restatement of the kernel that tests/test_pose_seq_cpu.py holds to the bound, so that a failure on the GPU
            is the kernel's and not the bound's.
Inputs are f32 and exact; W and H are integers below 2^24, exact in f32; 0.05f, 1e-6f, 0.5f and 3.0f are the kernel's own
f32 constants and exact here, 180 / pi is rounded (times_const).

ULP_ATAN2.  The angles here are taken in pixel space: |ba x bc| and ba . bc are up to W^2 ~ 10^6 times the arguments
scripts/measure_pose_ulp.py sampled for the 47-vector (normalised coordinates).  atan2f is a function of y / x and of the
quadrant, and neither the products nor the quotient come near f32's range at these sizes (|args| < 2^45), but that is an
argument, not a measurement, so the measurement was repeated on this kernel's own arguments (`function_arguments` below,
scripts/measure_pose_seq_ulp.py: 16 x 64 random frames at 640 x 480, 1920 x 1080 and 224 x 224 and the fixture's clips):
    measured on the MI355X    atan2f 1.97 ulp (9,775 arguments up to 5.3e6)    sqrtf 0.50 ulp (42,990 arguments up to 1.8e13)
    47-vector's arguments     atan2f 2.25 ulp                                  sqrtf 0.50 ulp      (tests/_pose_ref.py)
    constant                  ULP_ATAN2 = 4.5                                  ULP_SQRT = 1.0      twice the larger
(EXPERIMENTS.md, "Sequence pose features").

Discontinuities of the rule: sw > 0.05f W and hw > 0.05f W (columns 142-144).  Visibility compares are exact (f32 against
the f32 constant 0.65f), and whether a vector is zero is exact where it matters: a float64 zero vector has equal
coordinates, whose f32 products are equal too; a vector that is zero in f32 only has |(x, y)| below its bound, for which
the angle's bound is pi.  A frame whose sw (or, where sw does not decide, hw) lies within its bound of the threshold is
left out of the comparison of columns 142-144 (`excluded`) and counted; the tests assert that this is at most 1 % of the
frames.
"""
import numpy as np

import _pose_ref as R
from _pose_ref import V

NUM_LANDMARKS, NUM_FEATURES = 33, 443
TILE = 16                      # frames per workgroup (PS_ROWS of csrc/pose_seq.hip)
WAVE = 64
RAW, ZERO = 0, 1
VIS_MIN = np.float32(0.65)
SCALE_MIN = np.float32(0.05)
EPS = np.float32(1e-6)
ANGLE_TRIPLES = ((11, 13, 15), (12, 14, 16), (13, 11, 23), (14, 12, 24), (23, 25, 27), (24, 26, 28), (11, 23, 25), (12, 24, 26),
                 (0, 11, 23), (11, 12, 23))
ANGLE_NAMES = ["LEFT_ELBOW_ANGLE", "RIGHT_ELBOW_ANGLE", "LEFT_SHOULDER_ANGLE", "RIGHT_SHOULDER_ANGLE", "LEFT_KNEE_ANGLE",
               "RIGHT_KNEE_ANGLE", "LEFT_HIP_ANGLE", "RIGHT_HIP_ANGLE", "TORSO_VERTICAL_ANGLE", "TORSO_HORIZONTAL_ALIGNMENT"]
DIST_PAIRS = ((15, 16), (27, 28), (15, 23))
TORSO = (11, 12, 23, 24)
COL_ANGLE, COL_DIST, COL_REL, COL_DYN, COL_VAR = 132, 142, 145, 244, 442
FEATURE_NAMES = ([f"LM{j}_{c}" for j in range(33) for c in ("norm_x", "norm_y", "norm_z", "visibility")] + ANGLE_NAMES
                 + ["DIST_LR_WRIST_NORM", "DIST_LR_ANKLE_NORM", "DIST_L_WRIST_HIP_NORM"]
                 + [f"LM{j}_rel_{c}_norm" for j in range(33) for c in "xyz"]
                 + [f"LM{j}_{c}_px" for j in range(33) for c in ("vx", "vy", "vz", "ax", "ay", "az")] + ["TORSO_VAR_XY_RATIO"])
assert len(FEATURE_NAMES) == NUM_FEATURES
SEED = 1234
MEASURED_ATAN2, MEASURED_SQRT = 1.97, 0.5     # ulp, largest seen on the MI355X on this kernel's arguments (see above)
ULP_ATAN2, ULP_SQRT = 2.0 * max(MEASURED_ATAN2, R.MEASURED_ATAN2), 2.0 * max(MEASURED_SQRT, R.MEASURED_SQRT)
R_ATAN2, R_SQRT = 2 * R.U * ULP_ATAN2, 2 * R.U * ULP_SQRT      # one ulp is at most 2^-23 of the value


def make_clips(batch, frames, seed=SEED, undetected=0.0):
    """(landmarks f32 [batch,frames,33,4], detected uint8 [batch,frames]): every clip a random walk (steps of 0.02) from
    x, y ~ U(0,1), z ~ U(-0.5,0.5); visibility ~ U(0.5,1) per frame and landmark, so that about 70 % are visible; a share
    `undetected` of the frames without a pose."""
    rng = np.random.default_rng(seed)
    start = rng.random((batch, 1, NUM_LANDMARKS, 3), dtype=np.float32)
    start[..., 2] -= np.float32(0.5)
    steps = rng.standard_normal((batch, frames, NUM_LANDMARKS, 3), dtype=np.float32) * np.float32(0.02)
    steps[:, 0] = 0
    lm = np.empty((batch, frames, NUM_LANDMARKS, 4), np.float32)
    lm[..., :3] = start + np.cumsum(steps, axis=1, dtype=np.float32)
    lm[..., 3] = np.float32(0.5) + np.float32(0.5) * rng.random((batch, frames, NUM_LANDMARKS), dtype=np.float32)
    det = (rng.random((batch, frames)) >= undetected).astype(np.uint8)
    return lm, det


# ---- the history ------------------------------------------------------------------------------------------------------------
def plain_predecessors(det, hist_count=0):
    """The reference's loop over one clip: per frame the sources of its two predecessors, (most recent, second most recent):
    a frame index >= 0, -1 - k for slot k of the incoming history, or None.  Also the two sources after the last frame."""
    held = [-1 - k for k in range(min(int(hist_count), 2))]          # deque(maxlen=2), index 0 the most recent
    out = []
    for t, d in enumerate(det):
        out.append((held[0] if len(held) >= 1 else None, held[1] if len(held) >= 2 else None))
        if d:
            held = [t] + held[:1]
    return out, (held[0] if len(held) >= 1 else None, held[1] if len(held) >= 2 else None)


def kernel_predecessors(det, hist_count=0, tile=TILE, wave=WAVE):
    """The same by the kernel's scheme: per tile of `tile` frames a backward walk over the flags before it, `wave` flags per
    ballot, the highest set bits first, never below frame 0; what is missing from the incoming history; then one pass over
    the tile's flags.  Returns what plain_predecessors returns, and the largest number of ballots a tile took."""
    T = len(det)
    out, last, ballots = [], (None, None), 0
    for t0 in range(0, T, tile):
        found, steps = [], 0
        base = t0 - wave
        while len(found) < 2 and base > -wave:
            steps += 1
            mask = 0
            for lane in range(wave):
                t = base + lane
                assert t < t0
                if t >= 0 and det[t]:
                    mask |= 1 << lane
            while mask and len(found) < 2:
                hi = mask.bit_length() - 1
                found.append(base + hi)
                mask &= ~(1 << hi)
            base -= wave
        ballots = max(ballots, steps)
        k = 0
        while len(found) < 2 and k < min(int(hist_count), 2):
            found.append(-1 - k)
            k += 1
        found += [None] * (2 - len(found))
        # slots 0 and 1 hold the two sources, slot 2 + r frame t0 + r
        source = {0: found[0], 1: found[1]}
        p, pp = (0 if found[0] is not None else -1), (1 if found[1] is not None else -1)
        for r in range(min(tile, T - t0)):
            source[2 + r] = t0 + r
            out.append((source[p] if p >= 0 else None, source[pp] if pp >= 0 else None))
            if det[t0 + r]:
                pp, p = p, 2 + r
        last = (source[p] if p >= 0 else None, source[pp] if pp >= 0 else None)
    return out, last, ballots


def _resolve(lm, det, hist, hist_count):
    """per frame the landmarks of its two predecessors and whether both exist; the history after the last frame"""
    B, T = lm.shape[:2]
    one, two = np.zeros_like(lm), np.zeros_like(lm)
    both = np.zeros((B, T), dtype=bool)
    end, end_count = np.zeros((B, 2, NUM_LANDMARKS, 4), np.float32), np.zeros(B, np.uint8)
    for b in range(B):
        count = 0 if hist_count is None else int(hist_count[b])
        pick = lambda s: lm[b, s] if s >= 0 else hist[b, -1 - s]
        per_frame, last = plain_predecessors(det[b], count)
        for t, (s1, s2) in enumerate(per_frame):
            if s1 is not None and s2 is not None:
                one[b, t], two[b, t], both[b, t] = pick(s1), pick(s2), True
        for k, s in enumerate(last):
            if s is not None:
                end[b, k] = pick(s)
                end_count[b] += 1
    return one, two, both, end, end_count


# ---- two arithmetics --------------------------------------------------------------------------------------------------------
def _sqrt(a):       # _pose_ref.sqrt with this file's constant
    with np.errstate(invalid="ignore"):
        v = np.sqrt(a.v)
        e = v - np.sqrt(np.maximum(a.v - a.e, 0.0))
    return V(v, e + R_SQRT * (v + e))


def _atan2(y, x):   # _pose_ref.atan2 with this file's constant
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.arctan2(y.v, x.v)
        r, d = np.hypot(x.v, y.v), np.hypot(x.e, y.e)
        e = np.where(d == 0, 0.0, np.where(d < r, np.arcsin(np.minimum(d / np.where(r > 0, r, 1.0), 1.0)), np.pi))
    return V(v, e + R_ATAN2 * (np.abs(v) + e))


class Bounded:
    add, sub, mul, div, half, times_const = (staticmethod(f) for f in (R.add, R.sub, R.mul, R.div, R.half, R.times_const))
    sqrt, atan2 = staticmethod(_sqrt), staticmethod(_atan2)

    @staticmethod
    def num(x):
        return V(np.asarray(x, dtype=np.float64))

    @staticmethod
    def val(a):
        return a.v

    @staticmethod
    def sel(mask, a, b):
        return V(np.where(mask, a.v, b.v), np.where(mask, a.e, b.e))

    @staticmethod
    def near(a, b):
        return np.abs(a.v - b.v) <= a.e + b.e


class Plain32:
    f = np.float32
    add = staticmethod(lambda a, b: a + b)
    sub = staticmethod(lambda a, b: a - b)
    mul = staticmethod(lambda a, b: a * b)
    div = staticmethod(lambda a, b: a / b)
    sqrt = staticmethod(np.sqrt)
    half = staticmethod(lambda a: a * np.float32(0.5))
    atan2 = staticmethod(lambda y, x: np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(np.float32))
    times_const = staticmethod(lambda a, c: a * np.float32(c))
    num = staticmethod(lambda x: np.asarray(x, dtype=np.float32))
    val = staticmethod(lambda a: a)
    sel = staticmethod(lambda mask, a, b: np.where(mask, a, b))
    near = staticmethod(lambda a, b: np.zeros(np.shape(a), dtype=bool))


def _rule(A, cur, one, two, both, W, H, collect=None):
    """cur, one, two: f32 [n,33,4] (the frame and its two predecessors); both: bool [n]; W, H: [n].  Returns (columns: a list
    of 443 entries, each (quantity of A, NaN mask), near: bool [n]).  collect: a dict that receives the atan2f / sqrtf
    arguments."""
    n = cur.shape[0]
    Wv, Hv = A.num(W), A.num(H)
    vis = lambda arr, j: arr[:, j, 3] > VIS_MIN                        # exact; false for a NaN
    coord = lambda arr, j: [A.num(arr[:, j, k]) for k in range(3)]
    pixel = lambda arr, j: [A.mul(A.num(arr[:, j, 0]), Wv), A.mul(A.num(arr[:, j, 1]), Hv), A.mul(A.num(arr[:, j, 2]), Wv)]
    dot = lambda a, b: A.add(A.add(A.mul(a[0], b[0]), A.mul(a[1], b[1])), A.mul(a[2], b[2]))
    diff = lambda a, b: [A.sub(a[k], b[k]) for k in range(3)]
    never = np.zeros(n, dtype=bool)
    zero = A.num(np.zeros(n))

    def root(q):
        if collect is not None:
            collect["q"].append(A.val(q))
        return A.sqrt(q)

    def dist(a, b):
        d = diff(a, b)
        return root(dot(d, d))

    cols = [(A.num(cur[:, j, k]), never) for j in range(NUM_LANDMARKS) for k in range(4)]
    for (a, b, c) in ANGLE_TRIPLES:
        qb = pixel(cur, b)
        ba, bc = diff(pixel(cur, a), qb), diff(pixel(cur, c), qb)
        cr = [A.sub(A.mul(ba[1], bc[2]), A.mul(ba[2], bc[1])), A.sub(A.mul(ba[2], bc[0]), A.mul(ba[0], bc[2])),
              A.sub(A.mul(ba[0], bc[1]), A.mul(ba[1], bc[0]))]
        nothing = np.all([A.val(x) == 0 for x in ba], axis=0) | np.all([A.val(x) == 0 for x in bc], axis=0)
        y, x = root(dot(cr, cr)), dot(ba, bc)
        if collect is not None:
            seen = vis(cur, a) & vis(cur, b) & vis(cur, c) & ~nothing
            collect["y"].append(A.val(y)[seen])
            collect["x"].append(A.val(x)[seen])
        angle = A.sel(nothing, zero, A.times_const(A.atan2(y, x), R.DEG))
        cols.append((angle, ~(vis(cur, a) & vis(cur, b) & vis(cur, c))))
    shoulders, hips = vis(cur, 11) & vis(cur, 12), vis(cur, 23) & vis(cur, 24)
    sw = A.sel(shoulders, dist(pixel(cur, 11), pixel(cur, 12)), zero)
    hw = A.sel(hips, dist(pixel(cur, 23), pixel(cur, 24)), zero)
    least = A.mul(A.num(np.full(n, SCALE_MIN)), Wv)
    by_sw, by_hw = A.val(sw) > A.val(least), A.val(hw) > A.val(least)
    s = A.sel(by_sw, sw, A.sel(by_hw, hw, A.div(Hv, A.num(np.full(n, 3.0)))))
    near = (shoulders & A.near(sw, least)) | (~by_sw & hips & A.near(hw, least))
    for (i, j) in DIST_PAIRS:
        cols.append((A.div(dist(pixel(cur, i), pixel(cur, j)), s), ~(vis(cur, i) & vis(cur, j))))
    centre = [A.num(np.full(n, c)) for c in (0.5, 0.5, 0.0)]
    m = [A.sel(hips, A.half(A.add(A.num(cur[:, 23, k]), A.num(cur[:, 24, k]))), centre[k]) for k in range(3)]
    for j in range(NUM_LANDMARKS):
        p = coord(cur, j)
        cols += [(A.sub(p[k], m[k]), ~vis(cur, j)) for k in range(3)]
    for j in range(NUM_LANDMARKS):
        q1 = pixel(one, j)
        v = diff(pixel(cur, j), q1)
        acc = diff(v, diff(q1, pixel(two, j)))
        hole = ~(both & vis(cur, j) & vis(one, j) & vis(two, j))
        cols += [(x, hole) for x in v + acc]
    seen = np.stack([vis(cur, j) for j in TORSO], axis=1)
    count = seen.sum(axis=1)
    fn = A.num(np.maximum(count, 1))
    var = []
    for axis in (0, 1):
        vals = [A.num(cur[:, j, axis]) for j in TORSO]
        total = zero
        for k in range(4):
            total = A.sel(seen[:, k], A.add(total, vals[k]), total)
        mean = A.div(total, fn)
        q = zero
        for k in range(4):
            d = A.sub(vals[k], mean)
            q = A.sel(seen[:, k], A.add(q, A.mul(d, d)), q)
        var.append(A.div(q, fn))
    eps = A.num(np.full(n, EPS))
    cols.append((A.div(A.add(var[0], eps), A.add(var[1], eps)), count < 2))
    assert len(cols) == NUM_FEATURES
    return cols, near


def _inputs(lm, detected, sizes, hist, hist_count):
    lm = np.asarray(lm)
    assert lm.dtype == np.float32 and lm.ndim == 4 and lm.shape[2:] == (NUM_LANDMARKS, 4)
    B, T = lm.shape[:2]
    det = np.ones((B, T), np.uint8) if detected is None else np.asarray(detected).reshape(B, T)
    sizes = np.broadcast_to(np.asarray(sizes, dtype=np.int64).reshape(-1, 2), (B, 2))
    one, two, both, end, end_count = _resolve(lm, det, hist, hist_count)
    n = B * T
    W, H = (np.repeat(sizes[:, k], T).astype(np.float64) for k in range(2))
    dead = (det.reshape(n) == 0) | (W <= 0) | (H <= 0)
    return lm.reshape(n, 33, 4), one.reshape(n, 33, 4), two.reshape(n, 33, 4), both.reshape(n), W, H, dead, end, end_count


def features(lm, detected=None, sizes=(640, 480), hist=None, hist_count=None, mode=RAW):
    """lm: f32 [B,T,33,4]; detected: None or [B,T]; sizes: (W, H) or [B,2]; hist f32 [B,2,33,4] / hist_count [B]: the
    incoming history.  Returns (ref f64 [B,T,443], bound f64 [B,T,443] with inf at the excluded elements, excluded bool
    [B,T,443], history f32 [B,2,33,4] and counts uint8 [B] after the last frame)."""
    cur, one, two, both, W, H, dead, end, end_count = _inputs(lm, detected, sizes, hist, hist_count)
    n = cur.shape[0]
    with np.errstate(all="ignore"):
        cols, near = _rule(Bounded, cur, one, two, both, np.where(W > 0, W, 1.0), np.where(H > 0, H, 1.0))
    ref, bound = np.empty((n, NUM_FEATURES)), np.zeros((n, NUM_FEATURES))
    for c, (q, hole) in enumerate(cols):
        hole = hole | dead
        ref[:, c] = np.where(hole, np.nan, q.v)
        bound[:, c] = np.where(hole, 0.0, q.e)
    excluded = np.zeros((n, NUM_FEATURES), dtype=bool)
    excluded[:, COL_DIST:COL_DIST + 3] = (near & ~dead)[:, None]
    bound[excluded] = np.inf
    if mode == ZERO:
        hole = np.isnan(ref) & ~excluded
        ref, bound = np.where(hole, 0.0, ref), np.where(hole, 0.0, bound)
    shape = lm.shape[:2] + (NUM_FEATURES,)
    return ref.reshape(shape), bound.reshape(shape), excluded.reshape(shape), end, end_count


def restated(lm, detected=None, sizes=(640, 480), hist=None, hist_count=None):
    """the kernel's arithmetic in numpy f32 (Plain32): f32 [B,T,443], mode raw"""
    cur, one, two, both, W, H, dead, _, _ = _inputs(lm, detected, sizes, hist, hist_count)
    with np.errstate(all="ignore"):
        cols, _ = _rule(Plain32, cur, one, two, both, np.where(W > 0, W, 1.0), np.where(H > 0, H, 1.0))
    out = np.stack([np.where(hole | dead, np.float32(np.nan), q).astype(np.float32) for q, hole in cols], axis=1)
    return out.reshape(lm.shape[:2] + (NUM_FEATURES,))


def function_arguments(lm, detected=None, sizes=(640, 480)):
    """the f32 arguments the kernel's atan2f and sqrtf calls see on these clips, to float64 accuracy: (y [n], x [n], q [m])"""
    cur, one, two, both, W, H, dead, _, _ = _inputs(lm, detected, sizes, None, None)
    keep = ~dead
    collect = {"y": [], "x": [], "q": []}
    with np.errstate(all="ignore"):
        _rule(Bounded, cur[keep], one[keep], two[keep], both[keep], W[keep], H[keep], collect)
    y, x, q = (np.concatenate(collect[k]).astype(np.float32) for k in ("y", "x", "q"))
    ok = np.isfinite(y) & np.isfinite(x)
    return y[ok], x[ok], q[np.isfinite(q)]


def compare(got, ref, bound, what=""):
    """got: f32 [..., 443] from the kernel: NaNs where the reference has them, values within the bound, at most 1 % of the
    frames excluded (tests/_pose_ref.py::compare on the frames as rows).  Returns the largest error / bound."""
    return R.compare(np.asarray(got).reshape(-1, NUM_FEATURES), ref.reshape(-1, NUM_FEATURES),
                     bound.reshape(-1, NUM_FEATURES), what)


def reference_frames_per_second(lm, det, sizes=(640, 480), seconds=0.5):
    """`features` clip by clip, frame by frame with the history carried (the per-frame form of the reference's loop) on this
    host core: frames per second"""
    import time
    B, T = lm.shape[:2]
    done, t0 = 0, time.perf_counter()
    while True:
        b = (done // T) % B
        hist, count = None, None
        for t in range(T):
            _, _, _, hist, count = features(lm[b:b + 1, t:t + 1], det[b:b + 1, t:t + 1], sizes, hist, count)
            done += 1
        t = time.perf_counter() - t0
        if t >= seconds:
            return done / t
