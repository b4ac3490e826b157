"""Float64 statement of the pose-vector rule of include/qtcnn.h (qt_pose_features) and the error bound of the f32 kernel
that evaluates it (csrc/pose.hip), both vectorised over rows.

The reference is the header's rule evaluated in float64 on the f32 inputs: the joint angles as atan2(|ba x bc|, ba . bc),
everything else as experiment/test_on_video_cnn.py:126-202 writes it.  tests/golden/pose_features.npz holds what that
script's own function returns on the fixture rows (arccos form); tests/test_pose_cpu.py compares the two.

The bound follows the kernel operation by operation.  Every quantity is a pair (value in float64, bound on the distance of
the kernel's f32 value from it).  With u = 2^-24:
  a +- b, a b, a / b   correctly rounded (hipcc's default for f32 division and sqrtf): the operands' bounds carried through
                       the operation, plus u |result|.  A contracted multiply-add rounds once where the model rounds twice,
                       which the model covers.  A product that is not exactly zero also gets 2^-149 (underflow).
  sqrtf(a)             sqrt(a) - sqrt(a - e_a), plus ULP_SQRT ulp.
  atan2f(y, x)         the angle moves by at most asin(|(e_x, e_y)| / |(x, y)|), which is how an angle feature is
                       conditioned by |ba| |bc| (|(|ba x bc|, ba . bc)| = |ba| |bc|), plus ULP_ATAN2 ulp.
  a / b                (e_a + |a / b| e_b) / (|b| - e_b): the ratio through var(y), the distances through s.  Infinite when
                       e_b >= |b|.
  constants            180 / pi and pi / 2 are f32 constants in the kernel: u relative each.
Columns 41 and 42 end in `fold` (|d|, then 360 - d above 180), the distance of two directions on the circle: it moves by no
more than the directions do, on either side of 180 and of atan2's branch cut.

ULP_ATAN2, ULP_SQRT: no bound file here carried a constant for the device's atan2f or sqrtf (_loss_ref.py has exp, log1p,
expm1 and pow; _augment_ref.py none), so they were measured: scripts/measure_pose_ulp.py evaluates the device functions on
the arguments the rows of make_landmarks(4096, 1234) and of the fixture produce (function_arguments below) and compares
with float64.  The constant is twice the measured maximum, because one sample of arguments does not see the worst one.
    measured on the MI355X    atan2f 2.25 ulp (45,858 arguments)    sqrtf 0.50 ulp (54,196 arguments: correctly rounded)
    constant                  ULP_ATAN2 = 4.5                       ULP_SQRT = 1.0        (EXPERIMENTS.md, "Pose features")

Discontinuities of the rule: sw > 0, hw > 0, s > 0.05 (columns 43-45) and var(y) == 0 (column 46).  A row whose float64
value lies within its bound of one of them, without being exactly on it, is left out of the comparison of those columns
(`excluded`); the tests assert that this is at most 1 % of their rows.  The comparison at 0.65 is exact: for an f32 v,
v > 0.65f and double(v) > double(0.65f) agree.  Values that are exactly on a discontinuity in float64 (two equal shoulders,
four equal y) are exactly on it in f32 too, with one exception that the fixture avoids and the header's rule implies: the
f32 mean of THREE equal values y need not be y (3 y is not always an f32), so their f32 variance need not be 0.
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
MEASURED_ATAN2, MEASURED_SQRT = 2.25, 0.5     # ulp, largest seen on the MI355X (scripts/measure_pose_ulp.py)
ULP_ATAN2, ULP_SQRT = 2.0 * MEASURED_ATAN2, 2.0 * MEASURED_SQRT
R_ATAN2, R_SQRT = 2 * U * ULP_ATAN2, 2 * U * ULP_SQRT      # one ulp is at most 2^-23 of the value

NUM_LANDMARKS, NUM_FEATURES = 33, 47
FEATURE_NAMES = [f"LM{j}_visibility" for j in range(33)] + [
    "LEFT_ELBOW_ANGLE", "RIGHT_ELBOW_ANGLE", "LEFT_SHOULDER_ANGLE", "RIGHT_SHOULDER_ANGLE", "LEFT_KNEE_ANGLE",
    "RIGHT_KNEE_ANGLE", "LEFT_HIP_ANGLE", "RIGHT_HIP_ANGLE", "TORSO_VERTICAL_ANGLE", "TORSO_HORIZONTAL_ALIGNMENT",
    "DIST_LR_WRIST_NORM", "DIST_LR_ANKLE_NORM", "DIST_L_WRIST_HIP_NORM", "TORSO_VAR_XY_RATIO"]
ANGLE_TRIPLES = ((11, 13, 15), (12, 14, 16), (23, 11, 13), (24, 12, 14), (23, 25, 27), (24, 26, 28), (11, 23, 25), (12, 24, 26))
DIST_PAIRS = ((15, 16), (27, 28), (15, 23))
TORSO = (11, 12, 23, 24)
VIS_MIN = float(np.float32(0.65))
S_MIN = float(np.float32(0.05))
STD_MIN = float(np.float32(1e-6))
DEG = 180.0 / np.pi
RAW, ZERO, CLASS_MEAN, STANDARDIZE = 0, 1, 2, 3
SEED, ROWS = 1234, 4096      # the seeded random rows of the GPU bound test


def make_landmarks(rows, seed=SEED):
    """f32 [rows,33,4]: x, y ~ U(0,1), z ~ U(-0.5,0.5), visibility ~ U(0,1)"""
    rng = np.random.default_rng(seed)
    lm = rng.random((rows, NUM_LANDMARKS, 4), dtype=np.float32)
    lm[:, :, 2] -= np.float32(0.5)
    return lm


# ---- (value, bound) arithmetic ----------------------------------------------------------------------------------------------
class V:
    """value v (float64 array) and a bound e >= |kernel's f32 value - v|"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, dtype=np.float64)


def _rounded(v, e):
    return V(v, e + U * (np.abs(v) + e))


def add(a, b):
    return _rounded(a.v + b.v, a.e + b.e)


def sub(a, b):
    return _rounded(a.v - b.v, a.e + b.e)


def mul(a, b):
    v = a.v * b.v
    e = np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e
    r = _rounded(v, e)
    r.e = r.e + np.where((v != 0) | (e != 0), TINY, 0.0)
    return r


def half(a):          # exact
    return V(a.v * 0.5, a.e * 0.5)


def div(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        v = a.v / b.v
        room = np.abs(b.v) - b.e
        e = np.where(room > 0, (a.e + np.abs(v) * b.e) / np.where(room > 0, room, 1.0), np.inf)
    return _rounded(v, e)


def sqrt(a):
    with np.errstate(invalid="ignore"):
        v = np.sqrt(a.v)
        e = v - np.sqrt(np.maximum(a.v - a.e, 0.0))
    return V(v, e + R_SQRT * (v + e))


def atan2(y, x):
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.arctan2(y.v, x.v)
        r, d = np.hypot(x.v, y.v), np.hypot(x.e, y.e)
        e = np.where(d == 0, 0.0, np.where(d < r, np.arcsin(np.minimum(d / np.where(r > 0, r, 1.0), 1.0)), np.pi))
    return V(v, e + R_ATAN2 * (np.abs(v) + e))


def times_const(a, c):   # an f32 constant: u relative, then the product's rounding
    v = a.v * c
    return _rounded(v, a.e * abs(c) + U * np.abs(v))


def dot3(a, b):
    return add(add(mul(a[0], b[0]), mul(a[1], b[1])), mul(a[2], b[2]))


def dist3(p, q):
    d = [sub(p[k], q[k]) for k in range(3)]
    return sqrt(dot3(d, d))


def fold(d):
    v = np.abs(d.v)
    over = v > 180.0
    return V(np.where(over, 360.0 - v, v), d.e + np.where(over, U * (np.abs(360.0 - v) + d.e), 0.0))


# ---- the rule -------------------------------------------------------------------------------------------------------------
def _point(lm, j):
    return [V(lm[:, j, k].astype(np.float64)) for k in range(3)]


def _angle_args(lm, triple):
    """(|ba x bc|, ba . bc, zero-length flag) of one joint"""
    a, b, c = (_point(lm, j) for j in triple)
    ba = [sub(a[k], b[k]) for k in range(3)]
    bc = [sub(c[k], b[k]) for k in range(3)]
    cr = [sub(mul(ba[1], bc[2]), mul(ba[2], bc[1])), sub(mul(ba[2], bc[0]), mul(ba[0], bc[2])),
          sub(mul(ba[0], bc[1]), mul(ba[1], bc[0]))]
    nothing = np.all([x.v == 0 for x in ba], axis=0) | np.all([x.v == 0 for x in bc], axis=0)
    return dot3(cr, cr), dot3(ba, bc), nothing


def _torso_args(lm):
    """(t.y, t.x) of column 41 and the two (dy, dx) of column 42"""
    p = {j: _point(lm, j) for j in TORSO}
    t = [sub(half(add(p[11][k], p[12][k])), half(add(p[23][k], p[24][k]))) for k in range(2)]
    sh = [sub(p[12][k], p[11][k]) for k in range(2)]
    hp = [sub(p[24][k], p[23][k]) for k in range(2)]
    return (t[1], t[0]), (sh[1], sh[0]), (hp[1], hp[0])


def features(lm, detected=None):
    """lm: f32 [rows,33,4]; detected: None or [rows].  Returns (ref f64 [rows,47], bound f64 [rows,47], excluded bool
    [rows,47]): the raw features, the bound on the kernel's distance from them, and the elements next to a discontinuity."""
    lm = np.asarray(lm)
    assert lm.dtype == np.float32 and lm.shape[1:] == (NUM_LANDMARKS, 4)
    rows = lm.shape[0]
    ref = np.empty((rows, NUM_FEATURES))
    bound = np.zeros((rows, NUM_FEATURES))
    excluded = np.zeros((rows, NUM_FEATURES), dtype=bool)
    ref[:, :33] = lm[:, :, 3].astype(np.float64)
    nan = np.nan

    def put(col, val, also_nan=None):
        v = val.v if also_nan is None else np.where(also_nan, nan, val.v)
        ref[:, col] = v
        bound[:, col] = np.where(np.isnan(v), 0.0, val.e)

    for k, triple in enumerate(ANGLE_TRIPLES):
        sq, dt, nothing = _angle_args(lm, triple)
        put(33 + k, times_const(atan2(sqrt(sq), dt), DEG), nothing)
    (ty, tx), (sy, sx), (hy, hx) = _torso_args(lm)
    quarter = V(np.full(rows, np.pi / 2), np.full(rows, U * np.pi / 2))
    put(41, fold(times_const(sub(quarter, atan2(ty, tx)), DEG)))
    put(42, fold(sub(times_const(atan2(sy, sx), DEG), times_const(atan2(hy, hx), DEG))))

    p = {j: _point(lm, j) for j in (11, 12, 23, 24, 15, 16, 27, 28)}
    sw, hw = dist3(p[11], p[12]), dist3(p[23], p[24])
    both = (sw.v > 0) & (hw.v > 0)       # false for a NaN
    mid = half(add(sw, hw))
    s = V(np.where(both, mid.v, 1.0), np.where(both, mid.e, 0.0))
    small = ~(s.v > S_MIN)
    near = ((sw.v > 0) & (sw.v <= sw.e)) | ((hw.v > 0) & (hw.v <= hw.e)) | (np.abs(s.v - S_MIN) <= s.e)
    for k, (i, j) in enumerate(DIST_PAIRS):
        put(43 + k, div(dist3(p[i], p[j]), s), small)
        excluded[:, 43 + k] = near

    vis = np.stack([lm[:, j, 3].astype(np.float64) > VIS_MIN for j in TORSO], axis=1)      # [rows,4]; NaN: not visible
    n = vis.sum(axis=1)
    fn = V(np.maximum(n, 1).astype(np.float64))
    var = []
    for axis in (0, 1):
        vals = [V(lm[:, j, axis].astype(np.float64)) for j in TORSO]
        total = V(np.zeros(rows))
        for k in range(4):
            nxt = add(total, vals[k])
            total = V(np.where(vis[:, k], nxt.v, total.v), np.where(vis[:, k], nxt.e, total.e))
        mean = div(total, fn)
        q = V(np.zeros(rows))
        for k in range(4):
            dk = sub(vals[k], mean)
            nxt = add(q, mul(dk, dk))
            q = V(np.where(vis[:, k], nxt.v, q.v), np.where(vis[:, k], nxt.e, q.e))
        var.append(div(q, fn))
    vx, vy = var
    with np.errstate(invalid="ignore"):
        put(46, div(vx, vy), (n < 2) | (vy.v == 0))
        excluded[:, 46] = (n >= 2) & (vy.v > 0) & (vy.v <= vy.e)

    if detected is not None:
        off = np.asarray(detected).reshape(rows) == 0
        ref[off, :33] = 0.0
        ref[off, 33:] = nan
        bound[off] = 0.0
        excluded[off] = False
    bound[excluded] = np.inf
    return ref, bound, excluded


def function_arguments(lm):
    """the f32 arguments the kernel's atan2f and sqrtf calls see on these rows, to float64 accuracy: (y [n], x [n], q [m])"""
    ys, xs, qs = [], [], []
    for triple in ANGLE_TRIPLES:
        sq, dt, nothing = _angle_args(lm, triple)
        keep = ~nothing
        qs.append(sq.v[keep])
        ys.append(np.sqrt(sq.v[keep]))
        xs.append(dt.v[keep])
    for (y, x) in _torso_args(lm):
        ys.append(y.v)
        xs.append(x.v)
    for (i, j) in ((11, 12), (23, 24)) + DIST_PAIRS:
        d = [_point(lm, i)[k].v - _point(lm, j)[k].v for k in range(3)]
        qs.append(d[0] ** 2 + d[1] ** 2 + d[2] ** 2)
    f32 = lambda parts: np.concatenate(parts).astype(np.float32)
    y, x, q = f32(ys), f32(xs), f32(qs)
    ok = np.isfinite(y) & np.isfinite(x)
    return y[ok], x[ok], q[np.isfinite(q)]


def impute(ref, bound, mode, labels=None, means=None, stds=None, rows_per_label=1):
    """the imputation of include/qtcnn.h on (ref, bound) of `features` or on stored vectors (bound 0): (ref, bound)"""
    ref, bound = np.array(ref, dtype=np.float64), np.array(bound, dtype=np.float64)
    if mode == RAW:
        return ref, bound
    if mode == ZERO:
        hole = np.isnan(ref) & ~np.isinf(bound)      # (an excluded element stays excluded)
        return np.where(hole, 0.0, ref), np.where(hole, 0.0, bound)
    rows = ref.shape[0]
    lab = np.asarray(labels).reshape(-1)[np.arange(rows) // rows_per_label]
    K = means.shape[0]
    bad = (lab < 0) | (lab >= K)
    safe = np.where(bad, 0, lab)
    m = means.astype(np.float64)[safe]
    hole = np.isnan(ref)
    out, e = np.where(hole, m, ref), np.where(hole & ~np.isinf(bound), 0.0, bound)
    if mode == STANDARDIZE:
        sd32 = stds[safe]
        sd = sd32.astype(np.float64)
        flat = sd32 < np.float32(1e-6)
        with np.errstate(divide="ignore", invalid="ignore"):
            diff = out - m
            de = e + U * (np.abs(diff) + e)
            q = diff / sd
            qe = de / sd
            qe = qe + U * (np.abs(q) + qe)
        out, e = np.where(flat, 0.0, q), np.where(flat, 0.0, qe)
    out[bad] = np.nan
    e[bad] = 0.0
    return out, e


def restated(lm, detected=None):
    """The kernel's arithmetic restated in numpy f32, operation by operation (without the compiler's multiply-add
    contraction, numpy's float64 arctan2 rounded to f32 for atan2f): f32 [rows,47].  tests/test_pose_cpu.py holds it to the
    bound, so that a failure on the GPU is the kernel's and not the bound's."""
    f = np.float32
    lm = np.asarray(lm, dtype=f)
    rows = lm.shape[0]
    deg, quarter = f(DEG), f(np.pi / 2)
    pt = lambda j: [lm[:, j, k] for k in range(3)]
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    at2 = lambda y, x: np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(f)

    def dist(p, q):
        d = [p[k] - q[k] for k in range(3)]
        return np.sqrt(dot(d, d))

    def fold32(d):
        d = np.abs(d)
        return np.where(d > f(180), f(360) - d, d)

    out = np.empty((rows, NUM_FEATURES), f)
    out[:, :33] = lm[:, :, 3]
    with np.errstate(all="ignore"):
        for k, (a, b, c) in enumerate(ANGLE_TRIPLES):
            ba = [pt(a)[i] - pt(b)[i] for i in range(3)]
            bc = [pt(c)[i] - pt(b)[i] for i in range(3)]
            cr = [ba[1] * bc[2] - ba[2] * bc[1], ba[2] * bc[0] - ba[0] * bc[2], ba[0] * bc[1] - ba[1] * bc[0]]
            nothing = np.all([x == 0 for x in ba], axis=0) | np.all([x == 0 for x in bc], axis=0)
            out[:, 33 + k] = np.where(nothing, np.nan, at2(np.sqrt(dot(cr, cr)), dot(ba, bc)) * deg)
        ls, rs, lh, rh = (lm[:, j] for j in TORSO)
        t = [(ls[:, k] + rs[:, k]) * f(0.5) - (lh[:, k] + rh[:, k]) * f(0.5) for k in range(2)]
        out[:, 41] = fold32((quarter - at2(t[1], t[0])) * deg)
        out[:, 42] = fold32(at2(rs[:, 1] - ls[:, 1], rs[:, 0] - ls[:, 0]) * deg - at2(rh[:, 1] - lh[:, 1], rh[:, 0] - lh[:, 0]) * deg)
        sw, hw = dist(pt(11), pt(12)), dist(pt(23), pt(24))
        s = np.where((sw > 0) & (hw > 0), (sw + hw) * f(0.5), f(1))
        s = np.where(s == 0, f(1), s)
        for k, (i, j) in enumerate(DIST_PAIRS):
            out[:, 43 + k] = np.where(s > f(0.05), dist(pt(i), pt(j)) / s, np.nan)
        vis = np.stack([lm[:, j, 3] > f(0.65) for j in TORSO], axis=1)
        n = vis.sum(axis=1)
        fn = np.maximum(n, 1).astype(f)
        var = []
        for axis in (0, 1):
            vals = [lm[:, j, axis] for j in TORSO]
            total = np.zeros(rows, f)
            for k in range(4):
                total = np.where(vis[:, k], total + vals[k], total)
            mean = total / fn
            q = np.zeros(rows, f)
            for k in range(4):
                d = vals[k] - mean
                q = np.where(vis[:, k], q + d * d, q)
            var.append(q / fn)
        out[:, 46] = np.where((n < 2) | (var[1] == 0), np.nan, var[0] / var[1])
    if detected is not None:
        off = np.asarray(detected).reshape(rows) == 0
        out[off, :33] = 0
        out[off, 33:] = np.nan
    assert out.dtype == f
    return out


def compare(got, ref, bound, what=""):
    """got: f32 [rows,47] from the kernel.  NaNs where the reference has them (outside the excluded elements), values within
    the bound; asserts that at most 1 % of the rows have an excluded element.  Returns the largest error / bound."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    out = np.isinf(bound)
    share = float(out.any(axis=1).mean())
    assert share <= 0.01, f"{what}: {share:.2%} of the rows are next to a discontinuity"
    nan_ref, nan_got = np.isnan(ref) & ~out, np.isnan(got) & ~out
    assert np.array_equal(nan_ref, nan_got), (what, "NaN positions", np.argwhere(nan_ref != nan_got)[:8].tolist())
    live = ~np.isnan(ref) & ~out
    err = np.abs(got - ref)[live]
    b = bound[live]
    exact = b == 0
    assert (err[exact] == 0).all(), (what, "an exact element differs")
    worst = float((err[~exact] / b[~exact]).max()) if (~exact).any() else 0.0
    bad = np.argwhere(live & (np.abs(got - ref) > bound))
    assert bad.size == 0, (what, "beyond the bound at (row, col)", bad[:8].tolist(), worst)
    return worst


def reference_rows_per_second(lm, seconds=0.5):
    """`features` row by row (the per-sample form of a loader) on this host core: rows per second"""
    import time
    done, t0 = 0, time.perf_counter()
    while True:
        features(lm[done % lm.shape[0]][None])
        done += 1
        t = time.perf_counter() - t0
        if t >= seconds:
            return done / t
