"""The fused loss head, the parts that need no GPU: the derived bounds of tests/_loss_ref.py are met by a torch-f32
restatement of the kernels' arithmetic at every shape the GPU test uses (so a GPU failure is the kernel's, not the bound's) and
missed by three deliberately wrong restatements; the meter rule on a host model; the modules' constructor and device checks;
the C ABI's declarations and host-side argument checks."""
import ctypes
import os
import re

import pytest
import torch

import _loss_ref as R
from _util import PKG, ROOT, pkg

NEW_SYMBOLS = ["qt_loss_workspace_bytes", "qt_loss_forward", "qt_loss_backward"]
QT_ERR_INVALID_ARG, QT_ERR_UNSUPPORTED = -1, -3


def _check(name, got_loss, got_dz, ref):
    rl = R.ratio(got_loss.reshape(-1), ref["loss"].reshape(-1), ref["loss_bound"].reshape(-1))
    rg = R.ratio(got_dz, ref["dz"], ref["dz_bound"])
    return rl, rg


@pytest.mark.parametrize("rows,C", R.SHAPES)
def test_f32_restatement_of_cross_entropy_meets_the_bounds(rows, C):
    worst = (0.0, 0.0)
    i = 0
    for with_w in (False, True):
        for eps in (0.0, 0.1):
            for ignored in ("no", "some"):
                for red in (R.MEAN, R.SUM, R.NONE):
                    scale = R.SCALES[(i + rows + C) % 3]
                    i += 1
                    z = R.make_logits(rows, C, scale, seed=i)
                    y = R.make_labels(rows, C, ignored, seed=i)
                    if ignored == "some" and bool((y == R.IGNORE).all()):
                        continue   # (one row: 'some' would be 'all', which the GPU test checks for NaN)
                    w = R.make_weights(C, i) if with_w else None
                    g = R.make_grad_out(rows, red, i)
                    ref = R.ce_ref(z, y, w, eps, red, g)
                    loss, dz = R.restated(R.CE, z, y, w, eps, 0.0, red, g)
                    rl, rg = _check("ce", loss, dz, ref)
                    assert rl <= 1.0 and rg <= 1.0, (with_w, eps, ignored, red, scale, rl, rg)
                    worst = (max(worst[0], rl), max(worst[1], rg))
    print(f"cross-entropy {rows}x{C}: largest error / bound: loss {worst[0]:.3f}, dlogits {worst[1]:.3f}")


@pytest.mark.parametrize("rows,C", R.SHAPES)
def test_f32_restatement_of_focal_loss_meets_the_bounds(rows, C):
    i = 0
    for gamma in (0.0, 1.0, 2.0, 3.5):
        for red in (R.MEAN, R.SUM, R.NONE):
            scale = R.SCALES[(i + rows) % 3]
            i += 1
            z = R.make_logits(rows, C, scale, seed=100 + i)
            y = R.make_labels(rows, C, "no", seed=100 + i)
            alpha = R.make_weights(C, 100 + i)
            g = R.make_grad_out(rows, red, 100 + i)
            ref = R.focal_ref(z, y, alpha, gamma, red, g)
            loss, dz = R.restated(R.FOCAL, z, y, alpha, 0.0, gamma, red, g)
            rl, rg = _check("focal", loss, dz, ref)
            assert rl <= 1.0 and rg <= 1.0, (gamma, red, scale, rl, rg)


def _wrong_case():
    """7 x 5, non-uniform weights, rows 1 and 4 ignored: each mistake changes the result by far more than any rounding"""
    z = R.make_logits(7, 5, "x1", seed=900)
    y = R.make_labels(7, 5, "some", seed=900)
    assert int((y == R.IGNORE).sum()) >= 1
    w = torch.tensor([0.25, 2.0, 0.5, 1.5, 1.0])
    return z, y, w


def test_a_mean_that_counts_ignored_rows_misses_the_bound():
    z, y, w = _wrong_case()
    g = R.make_grad_out(7, R.MEAN, 900)
    ref = R.ce_ref(z, y, w, 0.0, R.MEAN, g)
    ok = _check("ce", *R.restated(R.CE, z, y, w, 0.0, 0.0, R.MEAN, g), ref)
    bad = _check("ce", *R.restated(R.CE, z, y, w, 0.0, 0.0, R.MEAN, g, wrong=R.WRONG[0]), ref)
    assert max(ok) <= 1.0 and bad[0] > 1.0 and bad[1] > 1.0, (ok, bad)


def test_a_smoothing_term_without_class_weights_misses_the_bound():
    z, y, w = _wrong_case()
    g = R.make_grad_out(7, R.MEAN, 900)
    ref = R.ce_ref(z, y, w, 0.1, R.MEAN, g)
    ok = _check("ce", *R.restated(R.CE, z, y, w, 0.1, 0.0, R.MEAN, g), ref)
    bad = _check("ce", *R.restated(R.CE, z, y, w, 0.1, 0.0, R.MEAN, g, wrong=R.WRONG[1]), ref)
    assert max(ok) <= 1.0 and bad[0] > 1.0 and bad[1] > 1.0, (ok, bad)


def test_a_focal_gradient_without_the_modulator_derivative_misses_the_bound():
    z, _, w = _wrong_case()
    y = R.make_labels(7, 5, "no", seed=900)
    g = R.make_grad_out(7, R.MEAN, 900)
    ref = R.focal_ref(z, y, w, 2.0, R.MEAN, g)
    ok = _check("focal", *R.restated(R.FOCAL, z, y, w, 0.0, 2.0, R.MEAN, g), ref)
    bad = _check("focal", *R.restated(R.FOCAL, z, y, w, 0.0, 2.0, R.MEAN, g, wrong=R.WRONG[2]), ref)
    assert max(ok) <= 1.0 and bad[0] <= 1.0 and bad[1] > 1.0, (ok, bad)   # the forward is untouched by this mistake


def test_focal_rows_with_p_next_to_one_and_next_to_zero():
    z = torch.zeros(4, 12)
    z[0, 3] = 17.0     # p_3 = 1 - 4.6e-7 ... and with 19 below 1 - 1e-7
    z[1, 3] = 19.0
    z[2, 5] = 17.0     # label 3: p_3 = 4e-8
    z[3, 5] = 30.0
    y = torch.tensor([3, 3, 3, 3])
    alpha = R.make_weights(12, 5)
    for gamma in (0.0, 1.0, 2.0, 3.5):
        g = R.make_grad_out(4, R.NONE, 5)
        ref = R.focal_ref(z, y, alpha, gamma, R.NONE, g)
        p = torch.softmax(z.double(), 1)[:, 3]
        assert float(1 - p[1]) < 1e-7 and float(p[2]) < 1e-7
        rl, rg = _check("focal", *R.restated(R.FOCAL, z, y, alpha, 0.0, gamma, R.NONE, g), ref)
        assert rl <= 1.0 and rg <= 1.0, (gamma, rl, rg)


def test_meter_rule_on_the_host_model():
    st = [0.0, 0, 0, 0]
    R.meter_step(st, 2.0, 4, 3)
    R.meter_step(st, float("nan"), 4, 1)
    R.meter_step(st, float("inf"), 4, 4)
    R.meter_step(st, 1.0, 2, 0)
    assert st == [10.0, 6, 3, 2]
    st = R.meter_step([0.0, 0, 0, 0], 6.0, 3, 1, reduction=R.SUM)
    assert st == [6.0, 3, 1, 0]


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    declared = set(re.findall(r"\b(qt_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(os.path.join(ROOT, PKG, "libqtcnn_hip.so"))
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
    assert "qt_loss_desc" in header


def test_host_side_argument_checks_need_no_device():
    M = pkg("loss")
    L = pkg("_lib").lib()
    assert L.qt_loss_workspace_bytes(256, 12) == 0 and L.qt_loss_workspace_bytes(257, 12) == 2 * 24
    assert L.qt_loss_workspace_bytes(16, 17) == 0 and L.qt_loss_workspace_bytes(17, 64) == 2 * 24
    assert L.qt_loss_workspace_bytes(4, 65) == 0 and L.qt_loss_workspace_bytes(5, 1024) == 2 * 24
    assert L.qt_loss_workspace_bytes(0, 12) == 0 and L.qt_loss_workspace_bytes(5, 1025) == 0
    z, y, out, st, rs = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000   # never dereferenced: every call is refused first

    def fwd(desc, rows=4, C=12, ld=12, ws=None, wsb=0, loss=out):
        return L.qt_loss_forward(ctypes.byref(desc), z, ld, y, rows, C, loss, rs, st, None, None, ws, wsb, None)

    good = M.LossDesc(0, 0, 0, -100, 0.0, 2.0, None)
    assert fwd(good, C=1025, ld=1025) == QT_ERR_UNSUPPORTED and b"1024" in L.qt_last_error()
    assert fwd(M.LossDesc(1, 0, 0, -100, 0.0, 0.0, None)) == QT_ERR_UNSUPPORTED      # bf16 logits
    assert fwd(M.LossDesc(0, 1, 0, -100, 0.0, 0.5, None)) == QT_ERR_UNSUPPORTED      # 0 < gamma < 1
    assert fwd(M.LossDesc(0, 1, 0, -100, 0.0, -1.0, None)) == QT_ERR_INVALID_ARG
    assert fwd(M.LossDesc(0, 2, 0, -100, 0.0, 0.0, None)) == QT_ERR_INVALID_ARG      # kind
    assert fwd(M.LossDesc(0, 0, 3, -100, 0.0, 0.0, None)) == QT_ERR_INVALID_ARG      # reduction
    assert fwd(M.LossDesc(0, 0, 0, -100, 1.5, 0.0, None)) == QT_ERR_INVALID_ARG      # label_smoothing
    assert fwd(good, rows=0) == QT_ERR_INVALID_ARG and fwd(good, C=0) == QT_ERR_INVALID_ARG
    assert fwd(good, ld=11) == QT_ERR_INVALID_ARG and b"stride" in L.qt_last_error()
    assert fwd(good, loss=None) == QT_ERR_INVALID_ARG
    assert fwd(good, rows=257) == QT_ERR_INVALID_ARG and b"workspace" in L.qt_last_error()
    assert fwd(good, rows=257, ws=0x60000, wsb=47) == QT_ERR_INVALID_ARG
    assert L.qt_loss_forward(None, z, 12, y, 4, 12, out, rs, st, None, None, None, 0, None) == QT_ERR_INVALID_ARG
    assert L.qt_loss_backward(ctypes.byref(good), z, 12, y, 4, 12, rs, st, None, out, 12, None) == QT_ERR_INVALID_ARG
    assert L.qt_loss_backward(ctypes.byref(good), z, 12, y, 4, 12, rs, st, out, out, 11, None) == QT_ERR_INVALID_ARG
    assert L.qt_loss_backward(ctypes.byref(good), z, 12, y, 4, 1025, rs, st, out, out, 1025, None) == QT_ERR_UNSUPPORTED


def test_module_constructors_and_device_checks():
    P = pkg()
    for bad in (dict(reduction="avg"), dict(label_smoothing=-0.1), dict(label_smoothing=1.5), dict(weight=torch.ones(2, 2))):
        with pytest.raises(ValueError):
            P.CrossEntropyLoss(**bad)
    ce = P.CrossEntropyLoss(weight=[1.0, 2.0, 3.0], ignore_index=7, reduction="sum", label_smoothing=0.1)
    assert "weight" in dict(ce.named_buffers()) and ce.weight.dtype == torch.float32 and ce.ignore_index == 7
    assert dict(P.CrossEntropyLoss().named_buffers()).get("weight", None) is None
    # the reference's FocalLoss fails with an unbound alpha_t for these; ours says so at construction
    for bad in (dict(alpha=0.25), dict(alpha=0.25, num_classes=12), dict(alpha=[0.5, 0.5], num_classes=3), dict(alpha=[0.5, 0.5]),
                dict(alpha=[[0.5, 0.5]], num_classes=2), dict(alpha=[1.0] * 3, num_classes=3, gamma=0.5),
                dict(alpha=[1.0] * 3, num_classes=3, gamma=-1.0), dict(alpha=[1.0] * 3, num_classes=3, reduction="avg")):
        with pytest.raises(ValueError):
            P.FocalLoss(**bad)
    fl = P.FocalLoss(alpha=0.25, num_classes=2)
    assert torch.equal(fl.alpha, torch.tensor([0.25, 0.75])) and fl.gamma == 2.0 and "alpha" in dict(fl.named_buffers())
    assert P.FocalLoss(alpha=[1.0, 2.0, 3.0], gamma=0, num_classes=3).gamma == 0.0
    # no torch fallback
    with pytest.raises(P.QtError):
        P.CrossEntropyLoss()(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(P.QtError):
        P.FocalLoss(alpha=[1.0, 2.0, 3.0], num_classes=3)(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(P.QtError):
        P.LossMeter("cpu")
    # the threed_cnn drop-in keeps its torch-level class
    assert pkg("threed_cnn.models").FocalLoss is not P.FocalLoss
