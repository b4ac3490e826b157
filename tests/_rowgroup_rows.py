"""Rows for the kernels that walk a [rows][C] matrix through csrc/qt_rowgroup.h (loss, metrics, scores, timeline): seeded
logits with the rows on which two argmax or softmax implementations part first, and the total order itself in numpy.
Used by tests/test_rowgroup_gpu.py and scripts/ab_rowgroup_bytes.py."""
import numpy as np

F32 = np.float32
KINDS = ("plain", "tie16", "tie1", "nan", "two_inf", "all_ninf", "times90")


def make_logits(rows, C, seed):
    """f32 [rows][C]; row i is of kind KINDS[(i + seed) % 7]:
      tie16     two exact maxima 16 columns apart (the same lane of a 16-lane group, two lanes of a wave); needs C > 16
      tie1      two exact maxima in neighbouring columns; needs C > 1
      nan       one NaN                        two_inf   two +inf (needs C > 1, else one)
      all_ninf  every logit -inf               times90   the row scaled by 90 (expf underflows off the maximum)
    a kind whose C is too small falls back to the next simpler one"""
    rng = np.random.default_rng(seed * 7919 + rows * 131 + C)
    z = rng.standard_normal((rows, C)).astype(F32)
    for i in range(rows):
        kind = KINDS[(i + seed) % len(KINDS)]
        top = F32(np.abs(z[i]).max() + 1.0)
        if kind == "tie16" and C <= 16:
            kind = "tie1"
        if kind == "tie16":
            a = int(rng.integers(0, C - 16))
            z[i, a] = z[i, a + 16] = top
        elif kind == "tie1" and C > 1:
            a = int(rng.integers(0, C - 1))
            z[i, a] = z[i, a + 1] = top
        elif kind == "nan":
            z[i, int(rng.integers(0, C))] = np.nan
        elif kind == "two_inf":
            z[i, rng.choice(C, size=min(2, C), replace=False)] = np.inf
        elif kind == "all_ninf":
            z[i] = -np.inf
        elif kind == "times90":
            z[i] *= F32(90.0)
    return z


def argmax_total_order(z):
    """the argmax of qt_arg_beats per row: a NaN beats every number (the first NaN wins), then the larger value, then the
    lower index"""
    z = np.asarray(z)
    out = np.empty(z.shape[0], np.int64)
    for i, r in enumerate(z):
        nan = np.isnan(r)
        out[i] = int(np.flatnonzero(nan)[0]) if nan.any() else int(np.flatnonzero(r == r.max())[0])
    return out
