"""Gradient clipping inside FusedAdam, the parts that need no GPU: the new C-ABI entry points are declared and exported,
they refuse bad arguments with QT_ERR_INVALID_ARG before any device work, and the optimizer's constructor option
validates, lives in `defaults` and survives state_dict() / load_state_dict()."""
import ctypes
import math
import os
import re

import pytest
import torch

from _util import PKG, ROOT, pkg

NEW_SYMBOLS = ["qt_grad_norm_workspace_bytes", "qt_grad_norm_multi", "qt_adam_multi_scaled",
               "qt_adam_pack_weights_batched_scaled", "qt_plan_adam_step_clipped"]
QT_ERR_INVALID_ARG = -1


def _lib():
    L = pkg("_lib").lib()
    return L


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    declared = set(re.findall(r"\b(qt_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(os.path.join(ROOT, PKG, "libqtcnn_hip.so"))
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s


def _items(numels, base=0x10000):
    """Items with made-up (never dereferenced) 16-byte aligned gradient addresses."""
    eng = pkg("engine")
    items = (eng.AdamItem * len(numels))()
    for j, n in enumerate(numels):
        items[j] = eng.AdamItem(None, base + j * (1 << 32), None, None, n)
    return items


def test_workspace_size_counts_one_float_per_chunk():
    L = _lib()
    eng = pkg("engine")
    assert L.qt_grad_norm_workspace_bytes(_items([1]), 1) == 4
    assert L.qt_grad_norm_workspace_bytes(_items([8192]), 1) == 4
    assert L.qt_grad_norm_workspace_bytes(_items([8193]), 1) == 8
    assert L.qt_grad_norm_workspace_bytes(_items([1, 3, 8192 * 3 + 1]), 3) == 4 * (1 + 1 + 4)
    # a pointer 4 bytes past a 16-byte boundary: three head elements go to the first chunk's workgroup
    one = (eng.AdamItem * 1)(eng.AdamItem(None, 0x10004, None, None, 8192 + 3))
    assert L.qt_grad_norm_workspace_bytes(one, 1) == 4
    one[0].numel = 8192 + 4
    assert L.qt_grad_norm_workspace_bytes(one, 1) == 8


def test_grad_norm_argument_checks():
    L = _lib()
    items = _items([100, 20000])
    need = L.qt_grad_norm_workspace_bytes(items, 2)
    assert need == 4 * 4
    ws, out = 0x2000000, 0x3000000   # never touched: every call below is refused before a launch
    call = L.qt_grad_norm_multi
    assert call(None, 2, 1.0, ws, need, out, None) == QT_ERR_INVALID_ARG
    assert call(items, 0, 1.0, ws, need, out, None) == QT_ERR_INVALID_ARG
    assert call(items, -1, 1.0, ws, need, out, None) == QT_ERR_INVALID_ARG
    for bad in (0.0, -1.0, float("nan")):
        assert call(items, 2, bad, ws, need, out, None) == QT_ERR_INVALID_ARG
        assert b"max_norm" in L.qt_last_error()
    assert call(items, 2, 1.0, ws, need - 1, out, None) == QT_ERR_INVALID_ARG
    assert b"workspace" in L.qt_last_error()
    assert call(items, 2, 1.0, None, need, out, None) == QT_ERR_INVALID_ARG
    assert call(items, 2, 1.0, ws, need, None, None) == QT_ERR_INVALID_ARG
    items[1].numel = 0
    assert call(items, 2, 1.0, ws, need, out, None) == QT_ERR_INVALID_ARG
    assert L.qt_grad_norm_workspace_bytes(items, 2) == 0
    assert L.qt_grad_norm_workspace_bytes(None, 2) == 0
    assert L.qt_grad_norm_workspace_bytes(_items([5]), 0) == 0


def test_scaled_adam_argument_checks():
    L = _lib()
    eng = pkg("engine")
    desc = eng.AdamDesc(1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1)
    assert L.qt_adam_multi_scaled(None, 1, ctypes.byref(desc), None, None) == QT_ERR_INVALID_ARG
    assert L.qt_adam_multi_scaled(_items([4]), 0, ctypes.byref(desc), None, None) == QT_ERR_INVALID_ARG
    bad = eng.AdamDesc(1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 0)   # step counts from 1
    assert L.qt_adam_multi_scaled(_items([4]), 1, ctypes.byref(bad), None, None) == QT_ERR_INVALID_ARG
    # the plan-level call refuses null arguments before it looks at anything else
    assert L.qt_plan_adam_step_clipped(None, None, None, None, None, None, ctypes.byref(desc), 1, 1.0, None, 0, None, 0,
                                       None, None) == QT_ERR_INVALID_ARG


def test_constructor_option():
    P = pkg()
    params = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]
    for bad in (0, -1, float("nan"), 0.0, -1e-3):
        with pytest.raises(ValueError):
            P.FusedAdam(params, max_grad_norm=bad)
    assert P.FusedAdam(params).defaults["max_grad_norm"] is None
    opt = P.FusedAdam(params, lr=1e-3, max_grad_norm=2)
    assert opt.defaults["max_grad_norm"] == 2.0 and isinstance(opt.defaults["max_grad_norm"], float)
    assert opt.param_groups[0]["max_grad_norm"] == 2.0
    assert opt.last_grad_norm is None and opt.last_clip_coef is None
    sd = opt.state_dict()
    assert sd["param_groups"][0]["max_grad_norm"] == 2.0
    other = P.FusedAdam(params, lr=1e-3)
    assert other._max_grad_norm() is None
    other.load_state_dict(sd)
    assert other._max_grad_norm() == 2.0
    back = P.FusedAdam(params, lr=1e-3, max_grad_norm=0.5)
    back.load_state_dict(P.FusedAdam(params, lr=1e-3).state_dict())
    assert back._max_grad_norm() is None
    assert math.isinf(P.FusedAdam(params, max_grad_norm=float("inf")).defaults["max_grad_norm"])
    assert callable(P.grad_norm)
