"""The image-gradient entry points (qt_stem_dgrad, qt_plan_backward_dx) are declared and exported, and refuse what they do
not cover before touching a device."""
import ctypes
import os

from _util import ROOT, PKG, pkg

QT_ERR_INVALID_ARG, QT_ERR_UNSUPPORTED = -1, -3


def _lib():
    if not os.path.exists(os.path.join(ROOT, PKG, "libqtcnn_hip.so")):
        import __graft_entry__ as g
        g.build()
    return pkg("_lib").lib()


def test_image_gradient_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    L = _lib()
    for name in ("qt_stem_dgrad", "qt_plan_backward_dx"):
        assert f"int {name}(" in header, name
        assert hasattr(L, name), name


def test_stem_dgrad_refuses_bad_arguments_without_a_device():
    L = _lib()
    fake = ctypes.c_void_p(1 << 20)   # never dereferenced: every call below returns before a launch
    assert L.qt_stem_dgrad(1, None, fake, fake, 2, None) == QT_ERR_INVALID_ARG
    assert L.qt_stem_dgrad(1, fake, fake, fake, 0, None) == QT_ERR_INVALID_ARG
    assert L.qt_stem_dgrad(7, fake, fake, fake, 2, None) == QT_ERR_UNSUPPORTED          # no such dtype
    assert L.qt_stem_dgrad(1, ctypes.c_void_p((1 << 20) + 8), fake, fake, 2, None) == QT_ERR_UNSUPPORTED  # dy alignment
    assert b"qt_stem_dgrad" in L.qt_last_error()


def test_plan_backward_dx_needs_a_recorded_forward():
    eng = pkg("engine")
    L = _lib()
    desc = eng.PlanDesc(0, 2, 12, 0, 0, 47, 0.5, 1e-5, 0.1, 0, 0)
    h = ctypes.c_void_p()
    assert L.qt_plan_create(ctypes.byref(desc), ctypes.byref(h)) == 0
    try:
        fake = ctypes.c_void_p(1 << 20)
        st = L.qt_plan_backward_dx(h, fake, fake, fake, fake, fake, 15, fake, None)
        assert st == QT_ERR_INVALID_ARG and b"no forward pass" in L.qt_last_error()
    finally:
        L.qt_plan_destroy(h)
