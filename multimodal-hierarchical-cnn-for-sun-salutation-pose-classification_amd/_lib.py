"""Loader of libqtcnn_hip.so (the C ABI declared in include/qtcnn.h; _abi.py holds its ctypes signatures and structs).

There is no CPU or PyTorch fallback: if the HIP library has not been built
(`python -c "import __graft_entry__ as g; g.build()"` or `make -C <pkg>/csrc`)
every product entry point raises.
"""
import ctypes
import os

# Side stream + RCCL streams need more than ROCm's default 4 hardware queues to really overlap
# (see bench.py); only effective if the HIP runtime has not been initialised yet.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import torch  # noqa: F401,E402  (loads the process-wide HIP runtime first)

from . import _abi  # noqa: E402
from ._abi import ConvDesc, ConvIO, ConvS2Desc, ConvS2IO, QtError  # noqa: F401,E402  (used as _lib.X everywhere)

_HERE = os.path.dirname(os.path.abspath(__file__))
# QTCNN_LIB_PATH: another build of the same ABI (A/B measurements of two kernel versions on one box)
LIB_PATH = os.environ.get("QTCNN_LIB_PATH") or os.path.join(_HERE, "libqtcnn_hip.so")

QT_F32, QT_BF16 = 0, 1
QT_CONV_FWD, QT_CONV_DGRAD = 0, 1


_lib = None


def lib():
    """The loaded library; raises QtError (never falls back) if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise QtError(
                f"{LIB_PATH} not found: the HIP extension is not built. "
                "Run __graft_entry__.build() (hipcc --offload-arch=gfx950). "
                "There is no CPU fallback for the product path.")
        _lib = _abi.bind(ctypes.CDLL(LIB_PATH))
    return _lib


def check(status, what=""):
    if status != 0:
        msg = lib().qt_last_error().decode(errors="replace")
        raise QtError(f"{what} failed with status {status}: {msg}")


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def qt_dtype(torch_dtype):
    if torch_dtype == torch.float32:
        return QT_F32
    if torch_dtype == torch.bfloat16:
        return QT_BF16
    raise QtError(f"unsupported activation dtype {torch_dtype}")
