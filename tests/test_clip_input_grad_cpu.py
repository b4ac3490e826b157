"""The clip-gradient entry point (qt_conv3d_first_dgrad) is declared and exported, and refuses bad arguments and unknown
dtypes before touching a device."""
import ctypes
import os

from _util import ROOT, PKG, pkg

QT_ERR_INVALID_ARG, QT_ERR_UNSUPPORTED = -1, -3
QT_BF16, QT_F32 = 1, 0


def _lib():
    if not os.path.exists(os.path.join(ROOT, PKG, "libqtcnn_hip.so")):
        import __graft_entry__ as g
        g.build()
    L = pkg("_lib").lib()
    return L


def test_clip_gradient_entry_point_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    L = _lib()
    assert "int qt_conv3d_first_dgrad(" in header
    assert hasattr(L, "qt_conv3d_first_dgrad")
    assert (pkg("_lib").QT_BF16, pkg("_lib").QT_F32) == (QT_BF16, QT_F32)


def test_conv3d_first_dgrad_refuses_bad_arguments_without_a_device():
    L = _lib()
    fake = ctypes.c_void_p(1 << 20)   # never dereferenced: every call below returns before a launch
    for dtype in (QT_BF16, QT_F32):
        assert L.qt_conv3d_first_dgrad(dtype, None, fake, fake, 2, 3, 8, 16, None) == QT_ERR_INVALID_ARG
        assert L.qt_conv3d_first_dgrad(dtype, fake, None, fake, 2, 3, 8, 16, None) == QT_ERR_INVALID_ARG
        assert L.qt_conv3d_first_dgrad(dtype, fake, fake, None, 2, 3, 8, 16, None) == QT_ERR_INVALID_ARG
        assert b"qt_conv3d_first_dgrad" in L.qt_last_error()
        for bad in ((0, 3, 8, 16), (2, 0, 8, 16), (2, 3, 0, 16), (2, 3, 8, 0), (-1, 3, 8, 16), (2, 3, 8, -16)):
            assert L.qt_conv3d_first_dgrad(dtype, fake, fake, fake, *bad, None) == QT_ERR_INVALID_ARG, bad
    assert L.qt_conv3d_first_dgrad(7, fake, fake, fake, 2, 3, 8, 16, None) == QT_ERR_UNSUPPORTED   # no such dtype
    assert b"qt_conv3d_first_dgrad" in L.qt_last_error()
