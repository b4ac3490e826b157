"""The HBM-bound kernels around the convolutions (csrc/elementwise.hip and the one-liners of attention.hip / lstm.hip) against a
float64 restatement of the same operation on exactly the values the kernel reads, inside error bounds DERIVED from the kernel's
own f32 arithmetic (tests/_bounds.py; tests/test_kernel_bounds_cpu.py shows that correct f32 arithmetic meets them).  Shapes are
the smallest that reach every path: both reductions of the statistics (<= 1024 partial rows directly, above that an f32 fold of
64 rows first), both BatchNorm-backward apply kernels, a grid-stride loop that takes a second trip for some threads only
(bn_act, and bn_bwd_apply in bf16 without a mask, at M = 786433, C = 64; every other capped launch of these files takes its second
trip in tests/test_grid_caps_gpu.py, see the table of tests/_grid_caps.py), the 7-way unrolled average pool with a tail, the dropped
row / column and the tie rule of the quadrant pool.
Every test prints max(|err| / bound); output buffers are pre-filled with NaN and nothing outside the defined range may change.

Reference behaviour: nn.BatchNorm2d / nn.ReLU / nn.AdaptiveAvgPool2d / nn.MaxPool2d(2, 2) / nn.Dropout and their autograd as
wired by the reference's QuadtreeCNN (Quadtree_from scratch/models.py:222-294)."""
import functools

import pytest
import torch

import _bounds as Bd
from _util import pkg

pytestmark = pytest.mark.gpu

NAN = float("nan")
QT_ERR_INVALID_ARG = -1


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _env():
    dev = _dev()
    L = pkg("_lib")
    return dev, L, L.lib()


def _nan(shape, dt, dev):
    return torch.full(shape, NAN, dtype=dt, device=dev)


def _all_nan(t):
    return bool(torch.isnan(t.float()).all())


def _report(name, r):
    print(f"  err/bound {name}: {r:.3f}")
    assert r <= 1.0, (name, r)


BnEvalItem = pkg("_abi").BnEvalItem   # qt_bn_eval_item


# ---------------------------------------------------------------------------------------------------------------------
# 1. qt_bn_finalize
# ---------------------------------------------------------------------------------------------------------------------
def _run_finalize(L, lib, dev, partial, count, gamma, beta, rmean, rvar):
    rows, _, C = partial.shape
    cap = lib.qt_stats_capacity_rows(rows)
    assert cap >= rows and (cap == rows) == (rows <= 1024)
    buf = _nan((cap, 2, C), torch.float32, dev)
    buf[:rows] = partial
    outs = {k: _nan((C + 8,), torch.float32, dev) for k in ("mean", "invstd", "scale", "shift")}
    rm = rv = None
    if rmean is not None:
        rm, rv = _nan((C + 8,), torch.float32, dev), _nan((C + 8,), torch.float32, dev)
        rm[:C], rv[:C] = rmean, rvar
    nbt = torch.tensor([41, -7], dtype=torch.int64, device=dev)
    L.check(lib.qt_bn_finalize(L.ptr(buf), rows, C, count, L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), L.ptr(nbt),
                               0.1, 1e-5, L.ptr(outs["mean"]), L.ptr(outs["invstd"]), L.ptr(outs["scale"]),
                               L.ptr(outs["shift"]), L.stream_ptr()), "qt_bn_finalize")
    torch.cuda.synchronize()
    assert nbt.tolist() == [42, -7]
    assert torch.equal(buf[:rows], partial)            # the table itself is read only; the fold lives in the spare rows
    if rm is not None:
        outs["running_mean"], outs["running_var"] = rm, rv
    for k, v in outs.items():
        assert _all_nan(v[C:]), k                      # the c < C guards
    return {k: v[:C] for k, v in outs.items()}


@pytest.mark.parametrize("rows", Bd.FIN_ROWS_DIRECT + Bd.FIN_ROWS_FOLDED)
def test_bn_finalize_vs_float64(rows):
    dev, L, lib = _env()
    worst = {}
    for C in Bd.FIN_C:
        partial, count = Bd.fin_partial(rows, C, 100 + rows + C, dev)
        gamma, beta, rmean, rvar = Bd.fin_params(C, C, dev)
        got = _run_finalize(L, lib, dev, partial, count, gamma, beta, rmean, rvar)
        ref = Bd.bn_finalize_ref(partial, count, gamma, beta, rmean, rvar, folded=rows > 1024)
        assert set(got) == set(ref)
        for k, (r, b) in ref.items():
            worst[k] = max(worst.get(k, 0.0), Bd.ratio(got[k], r, b))
    for k, r in worst.items():
        _report(f"bn_finalize rows={rows} {k}", r)


@pytest.mark.parametrize("rows", [17, 1089])
@pytest.mark.parametrize("variant", ["no gamma/beta", "no running stats"])
def test_bn_finalize_null_operands(rows, variant):
    dev, L, lib = _env()
    C = 24
    partial, count = Bd.fin_partial(rows, C, 7 + rows, dev)
    gamma, beta, rmean, rvar = Bd.fin_params(C, 3, dev)
    if variant == "no gamma/beta":
        gamma = beta = None
    else:
        rmean = rvar = None
    got = _run_finalize(L, lib, dev, partial, count, gamma, beta, rmean, rvar)
    ref = Bd.bn_finalize_ref(partial, count, gamma, beta, rmean, rvar, folded=rows > 1024)
    assert set(got) == set(ref)
    for k, (r, b) in ref.items():
        _report(f"bn_finalize {variant} rows={rows} {k}", Bd.ratio(got[k], r, b))


def test_bn_finalize_count_one_uses_the_biased_variance():
    dev, L, lib = _env()
    C = 8
    partial, count = Bd.fin_partial(1, C, 5, dev, per=1)
    assert count == 1
    gamma, beta, rmean, rvar = Bd.fin_params(C, 4, dev)
    got = _run_finalize(L, lib, dev, partial, count, gamma, beta, rmean, rvar)
    for k, (r, b) in Bd.bn_finalize_ref(partial, count, gamma, beta, rmean, rvar, folded=False).items():
        _report(f"bn_finalize count=1 {k}", Bd.ratio(got[k], r, b))
    # a lone running statistic is refused
    st = lib.qt_bn_finalize(L.ptr(partial.clone()), 1, C, 1, None, None, L.ptr(rmean.clone()), None, None, 0.1, 1e-5,
                            L.ptr(got["mean"].clone()), L.ptr(got["invstd"].clone()), L.ptr(got["scale"].clone()),
                            L.ptr(got["shift"].clone()), L.stream_ptr())
    assert st == QT_ERR_INVALID_ARG


# ---------------------------------------------------------------------------------------------------------------------
# 2. qt_bn_act / qt_bn_act_mask
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _large_act(dt):
    """the one large case (786433 x 64), generated on the device once and left unchanged"""
    return Bd.act_inputs(Bd.LARGE_M, Bd.LARGE_C, dt, 77, torch.device("cuda:0"))


def _check_bn_act(L, lib, dev, dt, M, C, ins, residual, relu):
    y, res, sc, sh, rs, rb = ins
    if residual == "none":
        res = rs = rb = None
    elif residual == "plain":
        rs = rb = None
    out0 = _nan((M + 1, C), dt, dev)
    out1 = _nan((M + 1, C), dt, dev)
    bits = torch.full((M + 1, C // 8), 0xAA, dtype=torch.uint8, device=dev)
    st = L.stream_ptr()
    L.check(lib.qt_bn_act(L.qt_dtype(dt), L.ptr(y), L.ptr(sc), L.ptr(sh), L.ptr(res), L.ptr(rs), L.ptr(rb), relu, L.ptr(out0),
                          M, C, st), "qt_bn_act")
    L.check(lib.qt_bn_act_mask(L.qt_dtype(dt), L.ptr(y), L.ptr(sc), L.ptr(sh), L.ptr(res), L.ptr(rs), L.ptr(rb), relu,
                               L.ptr(out1), L.ptr(bits), M, C, st), "qt_bn_act_mask")
    torch.cuda.synchronize()
    assert _all_nan(out0[M]) and _all_nan(out1[M]) and bool((bits[M] == 0xAA).all())   # rows past M
    assert torch.equal(out0[:M], out1[:M])
    assert torch.equal(bits[:M], Bd.pack_bits(out1[:M].float() > 0))                   # the sign of the STORED output
    ref, bound = Bd.bn_act_ref(y, sc, sh, res, rs, rb, relu, dt)
    return Bd.ratio(out1[:M], ref, bound)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", Bd.ACT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bn_act_vs_float64(dt, shape):
    dev, L, lib = _env()
    M, C = shape
    ins = Bd.act_inputs(M, C, dt, 9 + M, dev)
    worst = 0.0
    for residual in ("none", "plain", "affine"):
        for relu in (0, 1):
            worst = max(worst, _check_bn_act(L, lib, dev, dt, M, C, ins, residual, relu))
    _report(f"bn_act {M}x{C} {dt}", worst)
    # half a pair of residual coefficients is refused
    o = _nan((M, C), dt, dev)
    assert lib.qt_bn_act(L.qt_dtype(dt), L.ptr(ins[0]), L.ptr(ins[2]), L.ptr(ins[3]), L.ptr(ins[1]), L.ptr(ins[4]), None, 1,
                         L.ptr(o), M, C, L.stream_ptr()) == QT_ERR_INVALID_ARG


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_bn_act_second_grid_pass(dt):
    """6.29 M eight-channel groups = 1.5 passes of the 16384 x 256 grid: the loop takes a second trip for half the threads"""
    dev, L, lib = _env()
    r = _check_bn_act(L, lib, dev, dt, Bd.LARGE_M, Bd.LARGE_C, _large_act(dt), "affine", 1)
    _report(f"bn_act {Bd.LARGE_M}x{Bd.LARGE_C} {dt}", r)


# ---------------------------------------------------------------------------------------------------------------------
# 3. BatchNorm backward
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _large_bwd():
    return Bd.bwd_inputs(Bd.LARGE_M, Bd.LARGE_C, torch.bfloat16, False, 78, torch.device("cuda:0"))


def _check_reduce(L, lib, dev, dt, M, C, ins, with_mask):
    g, mask, y, mean, invstd, _ = ins
    if not with_mask:
        mask = None
    rows = lib.qt_bn_bwd_partial_rows(M, C)
    assert 0 < rows <= 2048
    part = _nan((rows + 3, 2, C), torch.float32, dev)
    L.check(lib.qt_bn_bwd_reduce(L.qt_dtype(dt), L.ptr(g), L.ptr(mask), L.ptr(y), L.ptr(mean), L.ptr(invstd), L.ptr(part), M,
                                 C, L.stream_ptr()), "qt_bn_bwd_reduce")
    torch.cuda.synchronize()
    assert _all_nan(part[rows:])
    tot = part[:rows].double().sum(0)
    s1, s2, a1, a2 = Bd.bwd_sums_ref(g, mask, y, mean, invstd)
    n = -(-M // rows) + 40
    return max(Bd.ratio(tot[0], s1, Bd.sum_bound(n, a1)), Bd.ratio(tot[1], s2, Bd.sum_bound(n, a2)))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", Bd.BWD_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bn_bwd_reduce_vs_float64(dt, shape):
    dev, L, lib = _env()
    M, C = shape
    ins = Bd.bwd_inputs(M, C, dt, True, 31 + M, dev)
    r = max(_check_reduce(L, lib, dev, dt, M, C, ins, False), _check_reduce(L, lib, dev, dt, M, C, ins, True))
    _report(f"bn_bwd_reduce {M}x{C} {dt}", r)


def test_bn_bwd_reduce_large():
    dev, L, lib = _env()
    r = _check_reduce(L, lib, dev, torch.bfloat16, Bd.LARGE_M, Bd.LARGE_C, _large_bwd(), False)
    _report(f"bn_bwd_reduce {Bd.LARGE_M}x{Bd.LARGE_C} bf16", r)


@pytest.mark.parametrize("C", Bd.BWD_C_ACCEPT)
def test_bn_bwd_partial_rows_and_reduce_accept_the_same_channel_counts(C):
    dev, L, lib = _env()
    M = 64
    g, _, y, mean, invstd, _ = Bd.bwd_inputs(M, C, torch.float32, False, 3, dev)
    part = torch.zeros(64, 2, C, device=dev)
    rows = lib.qt_bn_bwd_partial_rows(M, C)
    st = lib.qt_bn_bwd_reduce(0, L.ptr(g), None, L.ptr(y), L.ptr(mean), L.ptr(invstd), L.ptr(part), M, C, L.stream_ptr())
    torch.cuda.synchronize()
    accepted = 256 % (C // 8) == 0
    assert (rows > 0) == accepted and (st == 0) == accepted
    if not accepted:
        assert rows == QT_ERR_INVALID_ARG and st == QT_ERR_INVALID_ARG


FINALIZE_CASES = [  # rows, C, accumulate, dgamma/dbeta given, gamma given, count
    (1, 8, 0, True, True, 5), (17, 24, 1, True, True, 1000), (129, 64, 0, False, True, 4096), (1024, 520, 1, True, False, 77),
    (16, 64, 0, True, True, 0), (1089, 64, 1, True, True, 9999)]


@pytest.mark.parametrize("case", FINALIZE_CASES, ids=lambda c: f"rows{c[0]}_C{c[1]}_acc{c[2]}_count{c[5]}")
def test_bn_bwd_finalize_vs_float64(case):
    dev, L, lib = _env()
    rows, C, acc, grads, has_gamma, count = case
    gen = torch.Generator().manual_seed(rows + C)
    partial = (torch.randn(rows, 2, C, generator=gen) + 0.3).to(dev)
    gamma = (0.5 + torch.rand(C, generator=gen)).to(dev) if has_gamma else None
    invstd = (0.5 + torch.rand(C, generator=gen)).to(dev)
    pre_g, pre_b = torch.randn(C, generator=gen).to(dev), torch.randn(C, generator=gen).to(dev)
    cap = lib.qt_stats_capacity_rows(rows)
    buf = _nan((cap, 2, C), torch.float32, dev)
    buf[:rows] = partial
    dgamma, dbeta = _nan((C + 8,), torch.float32, dev), _nan((C + 8,), torch.float32, dev)
    dgamma[:C], dbeta[:C] = pre_g, pre_b
    coef = _nan((3 * C + 8,), torch.float32, dev)
    L.check(lib.qt_bn_bwd_finalize(L.ptr(buf), rows, C, count, L.ptr(gamma), L.ptr(invstd), L.ptr(dgamma) if grads else None,
                                   L.ptr(dbeta) if grads else None, acc, L.ptr(coef), L.stream_ptr()), "qt_bn_bwd_finalize")
    torch.cuda.synchronize()
    assert torch.equal(buf[:rows], partial) and _all_nan(coef[3 * C:]) and _all_nan(dgamma[C:]) and _all_nan(dbeta[C:])
    ref = Bd.bwd_finalize_ref(partial, count, gamma, invstd, pre_g if acc else None, pre_b if acc else None, folded=rows > 1024)
    got = {"coef0": coef[:C], "coef1": coef[C:2 * C], "coef2": coef[2 * C:3 * C], "dgamma": dgamma[:C], "dbeta": dbeta[:C]}
    if not grads:
        assert torch.equal(dgamma[:C], pre_g) and torch.equal(dbeta[:C], pre_b)
    for k, (r, b) in ref.items():
        if k in ("dgamma", "dbeta") and not grads:
            continue
        _report(f"bn_bwd_finalize {k}", Bd.ratio(got[k], r, b))
    if count == 0:   # eval-mode BatchNorm: no batch-mean terms
        assert bool((coef[C:3 * C] == 0).all())


def _check_apply(L, lib, dev, dt, M, C, ins, with_mask, with_gout):
    g, mask, y, mean, invstd, gamma = ins
    if not with_mask:
        mask = None
    coef = Bd.bwd_coef(g, mask, y, mean, invstd, gamma)
    dy = _nan((M + 1, C), dt, dev)
    gout = _nan((M + 1, C), dt, dev) if with_gout else None
    L.check(lib.qt_bn_bwd_apply(L.qt_dtype(dt), L.ptr(g), L.ptr(mask), L.ptr(y), L.ptr(mean), L.ptr(invstd), L.ptr(coef), L.ptr(dy),
                                L.ptr(gout), M, C, L.stream_ptr()), "qt_bn_bwd_apply")
    torch.cuda.synchronize()
    light = Bd.light_route(M, C, dt, mask, gout)
    ref, bound, gm = Bd.bwd_apply_ref(g, mask, y, mean, invstd, coef, dt, light)
    assert _all_nan(dy[M])
    if with_gout:
        assert _all_nan(gout[M]) and torch.equal(gout[:M].double(), gm)
    return Bd.ratio(dy[:M], ref, bound), light


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", Bd.BWD_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bn_bwd_apply_vs_float64(dt, shape):
    dev, L, lib = _env()
    M, C = shape
    ins = Bd.bwd_inputs(M, C, dt, True, 57 + M, dev)
    routes = set()
    for with_mask, with_gout in ((False, False), (False, True), (True, False), (True, True)):
        r, light = _check_apply(L, lib, dev, dt, M, C, ins, with_mask, with_gout)
        routes.add(light)
        _report(f"bn_bwd_apply {M}x{C} {dt} mask={with_mask} g_out={with_gout} {'light' if light else 'general'}", r)
    assert routes == ({True, False} if dt == torch.bfloat16 else {False})   # bf16 took both kernels


@pytest.mark.parametrize("with_gout", [False, True], ids=["light", "general"])
def test_bn_bwd_apply_large(with_gout):
    """3 * stride + 16 four-channel groups: the pair loop and the single-element tail of the light kernel both run"""
    dev, L, lib = _env()
    r, light = _check_apply(L, lib, dev, torch.bfloat16, Bd.LARGE_M, Bd.LARGE_C, _large_bwd(), False, with_gout)
    assert light == (not with_gout)
    _report(f"bn_bwd_apply {Bd.LARGE_M}x{Bd.LARGE_C} bf16 {'light' if light else 'general'}", r)


@pytest.mark.parametrize("M,light", [(128, True), (1, False)])
def test_bn_bwd_apply_24_channels(M, light):
    """six four-channel groups per row: 768 groups = a grid of 3 blocks (a multiple of 6: light kernel with a group count that
    is no power of two); one row = one block of 256 threads (no multiple of 6: general kernel)"""
    dev, L, lib = _env()
    ins = Bd.bwd_inputs(M, 24, torch.bfloat16, False, 91, dev)
    r, took = _check_apply(L, lib, dev, torch.bfloat16, M, 24, ins, False, False)
    assert took == light
    _report(f"bn_bwd_apply {M}x24 bf16 {'light' if light else 'general'}", r)


# ---------------------------------------------------------------------------------------------------------------------
# 4. qt_bn_eval_affine(_batched)
# ---------------------------------------------------------------------------------------------------------------------
def _eval_items(n, dev):
    Cs = [(8, 24, 64, 520, 40, 512)[j % 6] for j in range(n)]
    return [(C, Bd.fin_params(C, 200 + j, dev), j % 2 == 0) for j, C in enumerate(Cs)]


@pytest.mark.parametrize("n", [1, 32])
def test_bn_eval_affine_vs_float64(n):
    dev, L, lib = _env()
    items = _eval_items(n, dev)
    arr = (BnEvalItem * 33)()
    keep, worst = [], 0.0
    for j, (C, (gamma, beta, rmean, rvar), pair) in enumerate(items):
        o = {k: _nan((C + 8,), torch.float32, dev) for k in ("scale", "shift", "mean", "invstd")}
        keep.append(o)
        arr[j] = BnEvalItem(gamma.data_ptr(), beta.data_ptr(), rmean.data_ptr(), rvar.data_ptr(), o["scale"].data_ptr(),
                            o["shift"].data_ptr(), C, o["mean"].data_ptr() if pair else None,
                            o["invstd"].data_ptr() if pair else None)
    L.check(lib.qt_bn_eval_affine_batched(arr, n, 1e-5, L.stream_ptr()), "qt_bn_eval_affine_batched")
    singles = []
    for C, (gamma, beta, rmean, rvar), _ in items[:3]:
        s, t = _nan((C + 8,), torch.float32, dev), _nan((C + 8,), torch.float32, dev)
        L.check(lib.qt_bn_eval_affine(L.ptr(gamma), L.ptr(beta), L.ptr(rmean), L.ptr(rvar), 1e-5, C, L.ptr(s), L.ptr(t),
                                      L.stream_ptr()), "qt_bn_eval_affine")
        singles.append((s, t))
    torch.cuda.synchronize()
    for j, (C, (gamma, beta, rmean, rvar), pair) in enumerate(items):
        ref = Bd.bn_eval_ref(gamma, beta, rmean, rvar)
        o = keep[j]
        for k in ("scale", "shift"):
            assert _all_nan(o[k][C:])
            worst = max(worst, Bd.ratio(o[k][:C], *ref[k]))
        if pair:
            assert torch.equal(o["mean"][:C], rmean) and _all_nan(o["mean"][C:]) and _all_nan(o["invstd"][C:])
            worst = max(worst, Bd.ratio(o["invstd"][:C], *ref["invstd"]))
        else:
            assert _all_nan(o["mean"]) and _all_nan(o["invstd"])
        if j < len(singles):
            s, t = singles[j]
            assert _all_nan(s[C:]) and _all_nan(t[C:])
            worst = max(worst, Bd.ratio(s[:C], *ref["scale"]), Bd.ratio(t[:C], *ref["shift"]))
    _report(f"bn_eval_affine n={n}", worst)


def test_bn_eval_affine_batched_rejections():
    dev, L, lib = _env()
    C = 8
    gamma, beta, rmean, rvar = Bd.fin_params(C, 1, dev)
    o = [torch.zeros(C, device=dev) for _ in range(4)]
    arr = (BnEvalItem * 33)()
    for j in range(33):
        arr[j] = BnEvalItem(gamma.data_ptr(), beta.data_ptr(), rmean.data_ptr(), rvar.data_ptr(), o[0].data_ptr(), o[1].data_ptr(),
                            C, None, None)
    assert lib.qt_bn_eval_affine_batched(arr, 33, 1e-5, L.stream_ptr()) == QT_ERR_INVALID_ARG
    arr[0].mean = o[2].data_ptr()   # mean without invstd
    assert lib.qt_bn_eval_affine_batched(arr, 1, 1e-5, L.stream_ptr()) == QT_ERR_INVALID_ARG
    arr[0].invstd = o[3].data_ptr()
    assert lib.qt_bn_eval_affine_batched(arr, 1, 1e-5, L.stream_ptr()) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 5. qt_avgpool / qt_avgpool_bwd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("hw", Bd.POOL_HW)
@pytest.mark.parametrize("C", Bd.POOL_C)
def test_avgpool_vs_float64(dt, hw, C):
    dev, L, lib = _env()
    worst_f = worst_b = 0.0
    for batch in Bd.POOL_BATCH:
        x, d = Bd.pool_inputs(batch, hw, C, dt, hw + C + batch, dev)
        for place in Bd.POOL_PLACE:
            ld, col0 = place or (C, 0)
            dst = _nan((batch + 1, ld), dt, dev)
            L.check(lib.qt_avgpool(L.qt_dtype(dt), L.ptr(x), L.ptr(dst), batch, hw, C, ld, col0, L.stream_ptr()), "qt_avgpool")
            dmat = torch.randn(batch, ld, device=dev).to(dt)     # a full gradient matrix; only [col0, col0 + C) is read
            dmat[:, col0:col0 + C] = d
            gx = _nan((batch * hw + 1, C), dt, dev)
            L.check(lib.qt_avgpool_bwd(L.qt_dtype(dt), L.ptr(dmat), L.ptr(x), L.ptr(gx), batch, hw, C, ld, col0, L.stream_ptr()),
                    "qt_avgpool_bwd")
            torch.cuda.synchronize()
            assert _all_nan(dst[batch]) and _all_nan(dst[:batch, :col0]) and _all_nan(dst[:batch, col0 + C:])
            worst_f = max(worst_f, Bd.ratio(dst[:batch, col0:col0 + C], *Bd.avgpool_ref(x, dt)))
            assert _all_nan(gx[batch * hw])
            got = gx[:batch * hw].view(batch, hw, C)
            assert bool((got[x.float() <= 0] == 0).all())        # zeros and negative zeros of x pass nothing
            worst_b = max(worst_b, Bd.ratio(got, *Bd.avgpool_bwd_ref(d, x, dt)))
    _report(f"avgpool hw={hw} C={C} {dt}", worst_f)
    _report(f"avgpool_bwd hw={hw} C={C} {dt}", worst_b)


def test_avgpool_rejects_bad_placement():
    dev, L, lib = _env()
    x = torch.zeros(2, 49, 64, device=dev)
    dst = torch.zeros(2, 128, device=dev)
    g = torch.zeros(2, 49, 64, device=dev)
    for ld, col0 in ((128, 4), (128, 72), (124, 0)):
        assert lib.qt_avgpool(0, L.ptr(x), L.ptr(dst), 2, 49, 64, ld, col0, L.stream_ptr()) == QT_ERR_INVALID_ARG
        assert lib.qt_avgpool_bwd(0, L.ptr(dst), L.ptr(x), L.ptr(g), 2, 49, 64, ld, col0, L.stream_ptr()) == QT_ERR_INVALID_ARG
    assert lib.qt_avgpool(0, L.ptr(x), L.ptr(dst), 2, 49, 64, 128, 64, L.stream_ptr()) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 6. qt_quad_pool / qt_quad_pool_bwd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("ld", [4608, 5376])
def test_quad_pool_bit_exact(dt, B, ld):
    dev, L, lib = _env()
    q, d = Bd.quad_inputs(B, dt)
    assert Bd.quad_tie_share(q) >= 0.05
    d = d[:, :ld].contiguous()
    pooled_ref, dq_ref = Bd.quad_pool_ref(q, d, B, ld, 0)
    qg, dg = q.to(dev), d.to(dev)
    dst = _nan((B + 1, ld), dt, dev)
    dq = _nan((B * 4 * 49 + 1, 128), dt, dev)
    L.check(lib.qt_quad_pool(L.qt_dtype(dt), L.ptr(qg), L.ptr(dst), B, ld, 0, L.stream_ptr()), "qt_quad_pool")
    L.check(lib.qt_quad_pool_bwd(L.qt_dtype(dt), L.ptr(dg), L.ptr(qg), L.ptr(dq), B, ld, 0, L.stream_ptr()), "qt_quad_pool_bwd")
    torch.cuda.synchronize()
    assert _all_nan(dst[B]) and _all_nan(dst[:B, 4608:]) and _all_nan(dq[B * 4 * 49])
    assert torch.equal(dst[:B, :4608].cpu(), pooled_ref.to(dt))
    got = dq[:B * 4 * 49].view(B * 4, 7, 7, 128).cpu()
    assert torch.equal(got.double(), dq_ref)        # d is stored in dt already: routing a value adds no rounding
    assert bool((got[:, 6] == 0).all()) and bool((got[:, :, 6] == 0).all())   # dropped pixels: zeros, not the prefill
    print("  quad_pool / quad_pool_bwd: bit-exact")


def test_quad_pool_rejects_a_short_row():
    dev, L, lib = _env()
    q = torch.zeros(4, 7, 7, 128, device=dev)
    dst = torch.zeros(1, 5376, device=dev)
    assert lib.qt_quad_pool(0, L.ptr(q), L.ptr(dst), 1, 4600, 0, L.stream_ptr()) == QT_ERR_INVALID_ARG
    assert lib.qt_quad_pool_bwd(0, L.ptr(dst), L.ptr(q), L.ptr(q.clone()), 1, 5376, 776, L.stream_ptr()) == QT_ERR_INVALID_ARG


# ---------------------------------------------------------------------------------------------------------------------
# 7. qt_dropout and its backward
# ---------------------------------------------------------------------------------------------------------------------
def _dropout(L, lib, dev, dt, p, seed, pad=0):
    rows, cols = Bd.DROP_ROWS, Bd.DROP_COLS
    x = _nan((rows, cols + pad), dt, dev)
    x[:, :cols] = 1.0
    L.check(lib.qt_dropout(L.qt_dtype(dt), L.ptr(x), rows, cols, cols + pad, seed, p, L.stream_ptr()),
            "qt_dropout")
    torch.cuda.synchronize()
    return x


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("p", Bd.DROP_P)
def test_dropout_follows_the_binomial_law(dt, p):
    dev, L, lib = _env()
    a, b = _dropout(L, lib, dev, dt, p, 1234), _dropout(L, lib, dev, dt, p, 99991)
    assert torch.equal(a, _dropout(L, lib, dev, dt, p, 1234))          # same seed, same bits
    kept = (torch.ones((), dtype=torch.float32) / (torch.ones((), dtype=torch.float32) - torch.tensor(p, dtype=torch.float32)))
    kept = kept.to(dt).to(dev)                                          # fl(1 / (1 - p)) in f32, then the storage rounding
    assert bool(((a == 0) | (a == kept)).all()) and bool(((b == 0) | (b == kept)).all())
    for name, v, lo, hi in Bd.dropout_conditions(a != 0, b != 0, p):
        print(f"  dropout p={p} {name}: {v:.5f} in [{lo:.5f}, {hi:.5f}]")
        assert lo <= v <= hi, name
    padded = _dropout(L, lib, dev, dt, p, 1234, pad=24)                # the mask depends on (seed, r * cols + c) only
    assert _all_nan(padded[:, Bd.DROP_COLS:]) and torch.equal(padded[:, :Bd.DROP_COLS], a)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_dropout_p0_is_the_identity(dt):
    dev, L, lib = _env()
    x = torch.randn(37, 50, device=dev).to(dt)
    y = x.clone()
    L.check(lib.qt_dropout(L.qt_dtype(dt), L.ptr(y), 37, 48, 50, 5, 0.0, L.stream_ptr()), "qt_dropout")
    torch.cuda.synchronize()
    assert torch.equal(x, y)
    assert lib.qt_dropout(L.qt_dtype(dt), L.ptr(y), 37, 48, 50, 5, 1.0, L.stream_ptr()) == QT_ERR_INVALID_ARG


def test_dropout_backward_pair_bit_exact():
    """qt_relu_mask_scale(g, act = the dropped ReLU output, 1 / (1 - p)) = g * mul where kept and positive, else 0"""
    dev, L, lib = _env()
    p, rows, cols = 0.5, 301, 47
    gen = torch.Generator().manual_seed(8)
    act = torch.relu(torch.randn(rows, cols, generator=gen)).to(dev)
    positive = act > 0
    L.check(lib.qt_dropout(0, L.ptr(act), rows, cols, cols, 77, p, L.stream_ptr()), "qt_dropout")
    g = torch.randn(rows * cols + 5, generator=gen).to(dev)
    g0 = g.clone()
    mul = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32)
    L.check(lib.qt_relu_mask_scale(0, L.ptr(g), L.ptr(act), rows * cols, float(mul), L.stream_ptr()), "qt_relu_mask_scale")
    torch.cuda.synchronize()
    kept = (act != 0).flatten()
    npos = int(positive.sum())
    assert bool((kept <= positive.flatten()).all()) and abs(int(kept.sum()) / npos - 0.5) <= 5 * (0.25 / npos) ** 0.5
    want = torch.where(kept, g0[:rows * cols] * mul.to(dev), torch.zeros((), device=dev))
    assert torch.equal(g[:rows * cols], want) and torch.equal(g[rows * cols:], g0[rows * cols:])


# ---------------------------------------------------------------------------------------------------------------------
# 8. one-liners
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [1, 255, 256, 1000])
def test_relu_mask_scale_and_cast_bit_exact(dt, n):
    dev, L, lib = _env()
    gen = torch.Generator().manual_seed(n)
    act = torch.randn(n + 3, generator=gen)
    act[::5] = 0.0
    act[1::7] = -0.0
    act, g = act.to(dev, dt), torch.randn(n + 3, generator=gen).to(dev, dt)
    g0 = g.clone()
    L.check(lib.qt_relu_mask_scale(L.qt_dtype(dt), L.ptr(g), L.ptr(act), n, 1.25, L.stream_ptr()), "qt_relu_mask_scale")
    out = _nan((n + 3,), torch.float32, dev)
    L.check(lib.qt_cast_f32(L.qt_dtype(dt), L.ptr(g0), L.ptr(out), n, L.stream_ptr()), "qt_cast_f32")
    torch.cuda.synchronize()
    want = torch.where(act[:n].float() > 0, g0[:n].float() * 1.25, torch.zeros((), device=dev)).to(dt)   # one f32 product, one store
    assert torch.equal(g[:n], want) and torch.equal(g[n:], g0[n:])
    assert torch.equal(out[:n], g0[:n].float()) and _all_nan(out[n:])


@pytest.mark.parametrize("n", [1, 255, 256, 1000])
def test_scale_by_nonzero_bit_exact(n):
    dev, L, lib = _env()
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n + 3, generator=gen)     # negative values count as non-zero
    x[::3] = 0.0
    x[1::9] = -0.0
    x, g = x.to(dev), torch.randn(n + 3, generator=gen).to(dev)
    g0 = g.clone()
    L.check(lib.qt_scale_by_nonzero(L.ptr(g), L.ptr(x), n, 2.0 / 3.0, L.stream_ptr()), "qt_scale_by_nonzero")
    torch.cuda.synchronize()
    mul = torch.tensor(2.0 / 3.0, dtype=torch.float32, device=dev)
    want = torch.where(x[:n] != 0, g0[:n] * mul, torch.zeros((), device=dev))
    assert n < 3 or bool(((x[:n] < 0) & (want != 0)).any())
    assert torch.equal(g[:n], want) and torch.equal(g[n:], g0[n:])


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 0), (5, 94, 5376, 5282), (3, 85, 100, 7), (4, 64, 64, 0)],
                         ids=lambda s: "x".join(map(str, s)))
def test_relu_mask_cols_bit_exact(dt, shape):
    dev, L, lib = _env()
    rows, cols, ld, col0 = shape
    gen = torch.Generator().manual_seed(rows + cols)
    act = torch.randn(rows, ld, generator=gen)
    act[:, ::4] = 0.0
    act, d = act.to(dev, dt), torch.randn(rows, ld, generator=gen).to(dev, dt)
    out = _nan((rows * cols + 3,), torch.float32, dev)
    L.check(lib.qt_relu_mask_cols(L.qt_dtype(dt), L.ptr(d), L.ptr(act), L.ptr(out), rows, cols, ld, col0, 1.5,
                                  L.stream_ptr()), "qt_relu_mask_cols")
    torch.cuda.synchronize()
    sl = slice(col0, col0 + cols)
    want = torch.where(act[:, sl].float() > 0, d[:, sl].float() * 1.5, torch.zeros((), device=dev))
    assert torch.equal(out[:rows * cols].view(rows, cols), want) and _all_nan(out[rows * cols:])
    assert lib.qt_relu_mask_cols(L.qt_dtype(dt), L.ptr(d), L.ptr(act), L.ptr(out), rows, cols, ld, ld - cols + 1, 1.5,
                                 L.stream_ptr()) == QT_ERR_INVALID_ARG
