"""qt_gemm_small (csrc/gemm_small.hip) against float64 at the smallest shapes that reach every branch of its dispatch: the
thread kernel (K <= 96), the wave kernel (K tails, k-strided operands, mixed dtypes, a misaligned pointer), the vectorised wave
kernel (fewer / more 8-element chunks than one 256-chunk trip) and the 32x32 tile kernel (M / N / K tile edges, all four
combinations of k-contiguous and k-strided staging), each with the epilogue options spread over them (tests/_bounds.GEMM_CASES).
Bound: (K + 3 + 8) * 2^-24 * (sum_k |a b| + |bias| + |C before|) + 2^-9 |ref| for a bf16 C.

Reference behaviour: nn.Linear forward / backward of the pose MLP and classifier.3 (Quadtree_from scratch/models.py:255-260,270)
and the LSTM input products (cnn+lstm/models.py:43-49)."""
import ctypes

import pytest
import torch

import _bounds as Bd
from _util import pkg

pytestmark = pytest.mark.gpu

QT_ERR_INVALID_ARG = -1


GemmSmallDesc = pkg("_abi").GemmSmallDesc   # qt_gemm_small_desc


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.mark.parametrize("case", Bd.GEMM_CASES, ids=[c[0] for c in Bd.GEMM_CASES])
def test_gemm_small_vs_float64(case):
    dev = _dev()
    L = pkg("_lib")
    lib = L.lib()
    name, M, N, K, adt, bdt, cdt, ak, bk, has_bias, relu, acc, cpad, aoff = case[:14]
    o = Bd.gemm_operands(case, dev)
    C = torch.full((M + 1, o["crs"]), float("nan"), dtype=cdt, device=dev)
    if acc:
        C[:M, :N] = o["cfill"]
    d = GemmSmallDesc(M, N, K, L.qt_dtype(adt), L.qt_dtype(bdt), L.qt_dtype(cdt), o["ars"], o["aks"], o["brs"], o["bks"], o["crs"],
                      relu, acc)
    assert o["a_ptr"].data_ptr() == o["a_keep"].data_ptr() + aoff * o["a_keep"].element_size()
    L.check(lib.qt_gemm_small(ctypes.byref(d), L.ptr(o["a_ptr"]), L.ptr(o["b_ptr"]), L.ptr(o["bias"]), L.ptr(C), L.stream_ptr()),
            "qt_gemm_small")
    torch.cuda.synchronize()
    assert bool(torch.isnan(C[M].float()).all()) and bool(torch.isnan(C[:M, N:].float()).all())   # row M, the row padding
    ref, bound = Bd.gemm_ref(o["A"], o["B"], o["bias"], o["cfill"], relu, cdt)
    r = Bd.ratio(C[:M, :N], ref, bound)
    print(f"  err/bound gemm_small {name}: {r:.3f}")
    assert r <= 1.0, (name, r)


def test_gemm_small_rejections():
    dev = _dev()
    L = pkg("_lib")
    lib = L.lib()
    A, B, C = torch.zeros(4, 8, device=dev), torch.zeros(4, 8, device=dev), torch.full((4, 4), 7.0, device=dev)

    def call(M=4, N=4, K=8, a=0, b=0, c=0, pa=A, pb=B, pc=C):
        d = GemmSmallDesc(M, N, K, a, b, c, 8, 1, 8, 1, 4, 0, 0)
        return lib.qt_gemm_small(ctypes.byref(d), L.ptr(pa), L.ptr(pb), None, L.ptr(pc), L.stream_ptr())

    for kw in (dict(a=7), dict(b=2), dict(c=-1), dict(K=0), dict(M=0), dict(pa=None), dict(pb=None), dict(pc=None)):
        assert call(**kw) == QT_ERR_INVALID_ARG, kw
    assert lib.qt_gemm_small(None, L.ptr(A), L.ptr(B), None, L.ptr(C), L.stream_ptr()) == QT_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert bool((C == 7.0).all())     # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((C == 0.0).all())
