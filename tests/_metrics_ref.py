"""numpy / float64 references and a DERIVED error bound for the evaluation report (csrc/metrics.hip), shared by
tests/test_metrics_gpu.py (the kernels on the GPU), tests/test_metrics_cpu.py (the references against the recorded outputs of
the reference's own evaluate_model and against scikit-learn, an f32 restatement of the softmax against the bound) and
tests/golden/make_metrics_golden.py.

Counting (`count`): the state of include/qtcnn.h by np.add.at: cm[label][pred], then rows counted / ignored / invalid /
update calls.  A label equal to ignore_index is ignored; a label or prediction outside [0, C) is invalid.
Report (`report`): the 4 C + 12 doubles from a matrix, by scikit-learn's rules (precision_recall_fscore_support with
zero_division=0, 'weighted' and 'macro' over the classes present in labels or predictions, accuracy_score, r2_score).

Probabilities (`softmax_ref`, `prob_bound`): float64 softmax and the bound of the kernel's documented f32 arithmetic
    m = z[argmax], d_k = fl(z_k - m), e_k = expf(d_k), s = f32 sum of the C e_k in any order, p_k = fl(e_k / s)
by tests/_bounds.py's rule, per element in float64:
    |err d_k| <= U |d_k|                                       the subtraction's rounding
    |err e_k| <= e_k (R_EXP + U |d_k|)                          expf at 3 ulp, and its argument's error times exp' = e_k
    |err s|   <= (C + 8) U s + sum_k |err e_k|                  sum_bound
    |err p_k| <= p_k (|err e_k| / e_k + |err s| / s + R_DIV) + TINY
The ulp table is the one tests/_loss_ref.py cites (OpenCL 3.0 C specification, section 7.4: exp <= 3 ulp, x / y <= 2.5 ulp;
one ulp is at most 2^-23 relative).  TINY = 2^-126, the smallest normal f32: below it a result may be flushed to zero or
kept as a subnormal with an absolute spacing of 2^-149, by the same table's rule for subnormals, and since s >= 1 (the
maximum's own e = 1) that much absolute error in e_k is at most that much in p_k.  The float64 reference's own rounding
(a few 2^-53 relative) is charged as 16 * 2^-53 p_k.  Nothing here is fitted to what a kernel returns."""
import numpy as np

from _bounds import U, UD, sum_bound
from _loss_ref import R_EXP

ULP_DIV = 2.5
R_DIV = 2 * U * ULP_DIV
TINY = 2.0 ** -126
IGNORE = -100
SCALARS = ("accuracy", "weighted_precision", "weighted_recall", "weighted_f1", "macro_precision", "macro_recall", "macro_f1",
           "r2", "samples", "ignored", "invalid", "classes_present")

# (rows, C) of the exact-count test: C = 1; C = 16 | 17 (thread -> 16-lane row) and 64 | 65 (-> wave, LDS histogram -> global
# atomics); row counts on both sides of one workgroup's tile (256 / 16 / 4 rows) and of a wave; the largest C; many tiles
SHAPES = [(1, 1), (1, 12), (7, 2), (63, 12), (64, 12), (65, 13), (257, 16), (300, 17), (129, 64), (130, 65), (33, 1024),
          (4099, 12)]


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def make_logits(rows, C, seed, scale=1.0, step=0.5):
    """seeded multiples of `step` in [-3, 3] * scale (f32): ties are frequent"""
    rng = np.random.default_rng(seed)
    n = int(round(3.0 / step))
    return (rng.integers(-n, n + 1, size=(rows, C)) * (step * scale)).astype(np.float32)


def make_labels(rows, C, seed):
    return np.random.default_rng(seed + 1).integers(0, C, size=rows).astype(np.int64)


def argmax_ref(z):
    """torch.max(z, 1)'s index on the CPU: the first maximum, a NaN wins"""
    import torch
    return torch.max(torch.from_numpy(np.ascontiguousarray(z)), 1).indices.numpy()


# ----------------------------------------------------------------------------------------------------------------------
# counting
# ----------------------------------------------------------------------------------------------------------------------
def count(labels, preds, C, ignore_index=IGNORE, state=None, calls=1):
    """the state after one update (added to `state` when given): int64 [C*C + 4]"""
    y = np.asarray(labels, np.int64)
    p = np.asarray(preds, np.int64)
    st = np.zeros(C * C + 4, np.int64) if state is None else state.copy()
    ignored = y == ignore_index
    invalid = ~ignored & ((y < 0) | (y >= C) | (p < 0) | (p >= C))
    ok = ~ignored & ~invalid
    np.add.at(st, y[ok] * C + p[ok], 1)
    st[C * C + 0] += int(ok.sum())
    st[C * C + 1] += int(ignored.sum())
    st[C * C + 2] += int(invalid.sum())
    st[C * C + 3] += calls
    return st


def present_classes(cm):
    return np.nonzero(cm.sum(0) + cm.sum(1))[0]


def present_submatrix(cm):
    """what sklearn.metrics.confusion_matrix(y, p) returns: only the classes that occur in y or p"""
    k = present_classes(cm)
    return cm[np.ix_(k, k)]


# ----------------------------------------------------------------------------------------------------------------------
# the report
# ----------------------------------------------------------------------------------------------------------------------
def _div0(a, b):
    return np.divide(a, b, out=np.zeros_like(a, dtype=np.float64), where=b != 0)


def report(state, C, macro_over_all_classes=False):
    """float64 [4C + 12] from a state (or from a bare C x C matrix).  macro_over_all_classes: the deliberately WRONG variant
    that averages the macro values over all C classes instead of the present ones."""
    st = np.asarray(state, np.int64).reshape(-1)
    cm = st[:C * C].reshape(C, C).astype(np.float64)
    extra = st[C * C:] if st.size > C * C else np.zeros(4, np.int64)
    tp, sup, prd = np.diag(cm).copy(), cm.sum(1), cm.sum(0)
    prec, rec, f1 = _div0(tp, prd), _div0(tp, sup), _div0(2.0 * tp, sup + prd)
    n = sup.sum()
    present = (sup + prd) > 0
    out = np.zeros(4 * C + 12)
    out[:C], out[C:2 * C], out[2 * C:3 * C], out[3 * C:4 * C] = prec, rec, f1, sup
    s = out[4 * C:]
    nan = float("nan")
    if n > 0:
        s[0] = tp.sum() / n
        s[1:4] = [(sup * v).sum() / n for v in (prec, rec, f1)]
        k = float(C) if macro_over_all_classes else float(present.sum())
        s[4:7] = [v[present].sum() / k for v in (prec, rec, f1)]
    else:
        s[0:7] = nan
    idx = np.arange(C, dtype=np.float64)
    if n >= 2:
        ss_res = (cm * (idx[:, None] - idx[None, :]) ** 2).sum()
        mean = (idx * sup).sum() / n
        ss_tot = (sup * (idx - mean) ** 2).sum()
        s[7] = 1.0 - ss_res / ss_tot if ss_tot != 0 else (1.0 if ss_res == 0 else 0.0)
    else:
        s[7] = nan
    s[8], s[9], s[10], s[11] = n, float(extra[1]), float(extra[2]), float(present.sum())
    return out


def scalars(rep, C):
    return dict(zip(SCALARS, np.asarray(rep)[4 * C:].tolist()))


def close(got, want, tol=1e-12):
    """|got - want| <= tol * max(1, |want|) elementwise, NaN only where NaN is wanted"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    m = ~np.isnan(want)
    return bool(np.all(np.abs(got[m] - want[m]) <= tol * np.maximum(1.0, np.abs(want[m]))))


# ----------------------------------------------------------------------------------------------------------------------
# probabilities
# ----------------------------------------------------------------------------------------------------------------------
def softmax_ref(z):
    """(p float64 [rows][C], bound float64 [rows][C]) for finite f32 logits"""
    zd = np.asarray(z, np.float64)
    C = zd.shape[1]
    d = zd - zd.max(1, keepdims=True)
    e = np.exp(d)
    s = e.sum(1, keepdims=True)
    p = e / s
    de_rel = R_EXP + U * np.abs(d)                       # |err e_k| / e_k
    ds = sum_bound(C, s) + (e * de_rel).sum(1, keepdims=True)
    bound = p * (de_rel + ds / s + R_DIV + 16 * UD) + TINY
    return p, bound


def ratio(got, ref, bound):
    """max |got - ref| / bound; inf for a non-finite result"""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / bound).max())


def softmax_f32(z, subtract_max=True):
    """the kernel's arithmetic restated in numpy f32; subtract_max=False is the deliberately WRONG variant"""
    z = np.asarray(z, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        d = z - z.max(1, keepdims=True) if subtract_max else z
        e = np.exp(d, dtype=np.float32)
        s = e.sum(1, keepdims=True, dtype=np.float32)
        return (e / s).astype(np.float32)


def nan_pattern(z):
    """torch.softmax(z, 1) on the CPU, as a NaN mask"""
    import torch
    return torch.isnan(torch.softmax(torch.from_numpy(np.ascontiguousarray(z, np.float32)), 1)).numpy()
