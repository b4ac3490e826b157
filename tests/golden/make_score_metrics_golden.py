#!/usr/bin/env python3
"""Generate tests/golden/score_metrics.npz: what scikit-learn returns on the quantised scores q / K (developer aid; needs
scikit-learn, which no test needs: the tests read only the .npz).

    python tests/golden/make_score_metrics_golden.py

For five probability / label sets it records, per class, sklearn.metrics.roc_auc_score(y == k, q / K) (NaN where the class
or the rest has no sample) and average_precision_score(y == k, q / K) (NaN where the class has no sample), and
top_k_accuracy_score(y, p, k) for k = 1, 2, 3 on the unquantised rows, which hold no ties (scikit-learn breaks ties
differently; NaN for k >= C and for C = 2, where scikit-learn wants one score column).  The sets include absent classes, a
class whose scores all fall in one bin, and K = 16 and 4096.  Only data is written: probabilities, labels, bits, results.
"""
import os
import sys
import warnings

import numpy as np
from sklearn import metrics as M

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _scores_ref as R  # noqa: E402

# (C, rows, bits, absent classes, class with a constant score or None)
CASES = [(12, 1000, 12, (), None), (12, 300, 4, (3, 7), None), (2, 65, 12, (), None), (5, 64, 4, (0,), 4), (3, 7, 12, (1,), None)]


def make_case(C, n, absent, constant, seed):
    """probs f32 [n][C] (a softmax of peaked logits, so rows are trained-looking), labels int64 [n] without `absent`"""
    rng = np.random.default_rng(seed)
    allowed = np.array([c for c in range(C) if c not in absent], np.int64)
    z, _ = R.make_logits(n, C, seed, peak=0.0)
    y = allowed[rng.integers(0, len(allowed), size=n)]
    lift = rng.random(n) < 0.7
    z[np.arange(n)[lift], y[lift]] += np.float32(3.0)
    p = R.softmax_f32(z)
    if constant is not None:
        p[:, constant] = np.float32(0.40625)          # one bin at every K
    srt = np.sort(p, 1)
    assert not (srt[:, 1:] == srt[:, :-1]).any(), "rows must hold no ties"
    return p, y


def main():
    out = {"cases": np.array([f"C{c[0]}_n{c[1]}_b{c[2]}" for c in CASES]), "num_classes": np.array([c[0] for c in CASES], np.int64),
           "bits": np.array([c[2] for c in CASES], np.int64)}
    for i, (C, n, bits, absent, constant) in enumerate(CASES):
        p, y = make_case(C, n, absent, constant, seed=2000 + i)
        s = R.q_of(p, bits) / float(1 << bits)
        auc, ap = np.full(C, np.nan), np.full(C, np.nan)
        for k in range(C):
            t = y == k
            if t.any() and not t.all():
                auc[k] = M.roc_auc_score(t, s[:, k])
            if t.any():
                ap[k] = M.average_precision_score(t, s[:, k])
        topk = np.full(3, np.nan)
        if C > 2:
            for j, k in enumerate((1, 2, 3)):
                if k < C:
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        topk[j] = M.top_k_accuracy_score(y, p, k=k, labels=np.arange(C))
        out[f"probs{i}"], out[f"labels{i}"] = p, y
        out[f"auc{i}"], out[f"ap{i}"], out[f"topk{i}"] = auc, ap, topk
    dst = os.path.join(HERE, "score_metrics.npz")
    np.savez_compressed(dst, **out)
    print(f"{dst}: {len(CASES)} cases, {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main()
