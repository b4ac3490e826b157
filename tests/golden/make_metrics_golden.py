#!/usr/bin/env python3
"""Generate tests/golden/eval_metrics.npz by RUNNING THE REFERENCE's own evaluate_model on the CPU (developer aid; no test
and no GPU run reads the reference checkout; needs scikit-learn, which the reference script imports).

    python tests/golden/make_metrics_golden.py <path of the reference checkout>

Imports comparative analysis/analysis.py of the checkout by path.  Its sibling modules `model` and `dataloader` and
matplotlib are stubbed in sys.modules (every pyplot call is a no-op).  The "model" handed to evaluate_model returns preset
CPU logits batch by batch, the "loader" yields batches of 16 (the script's BATCH_SIZE) of dummy images and features and the
labels.  For each case the script records what evaluate_model itself returns: accuracy, weighted precision / recall / F1,
R^2 and the confusion matrix scikit-learn builds (present classes only).  Only data is written: logits, labels and those
outputs.  Logits are seeded multiples of 0.5, so ties are frequent; a class listed as absent occurs in no label and wins no
row.
"""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _metrics_ref as R  # noqa: E402

BATCH = 16
# (C, samples, absent classes)
CASES = [(12, 4099, ()), (12, 300, (3, 7)), (2, 65, ()), (5, 64, (0, 4)), (3, 7, (1,))]


def _stub_modules():
    mpl = types.ModuleType("matplotlib")
    plt = types.ModuleType("matplotlib.pyplot")
    plt.__getattr__ = lambda name: (lambda *a, **k: None)
    mpl.pyplot = plt
    sys.modules["matplotlib"], sys.modules["matplotlib.pyplot"] = mpl, plt
    model = types.ModuleType("model")
    model.get_model = None
    loader = types.ModuleType("dataloader")
    loader.get_dataloaders, loader.IMAGE_SIZE = None, 224
    sys.modules["model"], sys.modules["dataloader"] = model, loader


class _PresetModel:
    """returns the next batch of preset logits, whatever it is given"""

    def __init__(self, logits):
        self.batches = iter(torch.from_numpy(logits).split(BATCH))

    def eval(self):
        return self

    def __call__(self, images, numerical_features):
        return next(self.batches)


def make_case(C, n, absent, seed):
    """logits f32 [n][C] (multiples of 0.5; the label's column raised by 1.5 in about 70 % of the rows), labels int64 [n]"""
    rng = np.random.default_rng(seed)
    allowed = np.array([c for c in range(C) if c not in absent], np.int64)
    labels = allowed[rng.integers(0, len(allowed), size=n)]
    z = R.make_logits(n, C, seed)
    lift = rng.random(n) < 0.7
    z[np.arange(n)[lift], labels[lift]] += np.float32(1.5)
    z[:, list(absent)] = np.float32(-10.0)
    return z, labels


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    _stub_modules()
    path = os.path.join(sys.argv[1], "comparative analysis", "analysis.py")
    spec = importlib.util.spec_from_file_location("_reference_analysis_script", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    ref.device = torch.device("cpu")

    out = {"cases": np.array([f"C{C}_n{n}" for C, n, _ in CASES]), "num_classes": np.array([c[0] for c in CASES], np.int64)}
    for i, (C, n, absent) in enumerate(CASES):
        z, y = make_case(C, n, absent, seed=1000 + i)
        loader = [(torch.zeros(len(b), 1), torch.zeros(len(b), 1), b) for b in torch.from_numpy(y).split(BATCH)]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = ref.evaluate_model(_PresetModel(z), loader, [str(c) for c in range(C)], f"case{i}")
        pred = R.argmax_ref(z)
        seen = sorted(set(y.tolist()) | set(pred.tolist()))
        assert not set(seen) & set(absent) and got["confusion_matrix"].shape == (len(seen), len(seen)), (i, seen)
        out[f"logits{i}"], out[f"labels{i}"] = z, y
        out[f"scalars{i}"] = np.array([got[k] for k in ("accuracy", "precision", "recall", "f1", "r2")], np.float64)
        out[f"cm{i}"] = np.asarray(got["confusion_matrix"], np.int64)
    dst = os.path.join(HERE, "eval_metrics.npz")
    np.savez_compressed(dst, **out)
    print(f"{dst}: {len(CASES)} cases, {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main()
