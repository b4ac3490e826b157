"""The bounds and float64 references of tests/_bounds.py, checked WITHOUT a GPU: a plain torch-f32 (or bf16-output) restatement
of each operation stands in for the kernel, at the shapes of tests/test_elementwise_gpu.py and tests/test_gemm_small_gpu.py
(the one large case excepted), and must pass the same check.  So a GPU failure of those files is the kernel's, not the bound's
or the reference's.  Also here: the reference-only conditions (tie share of the quadrant-pool input, the dropout windows)."""
import math

import numpy as np
import pytest
import torch

import _bounds as Bd

CPU = torch.device("cpu")
DTS = [torch.float32, torch.bfloat16]


def _ok(name, got, ref, bound):
    r = Bd.ratio(got, ref, bound)
    assert r <= 1.0, (name, r)
    return r


@pytest.mark.parametrize("rows", Bd.FIN_ROWS_DIRECT + Bd.FIN_ROWS_FOLDED)
def test_bn_finalize_bounds(rows):
    for C in Bd.FIN_C:
        partial, count = Bd.fin_partial(rows, C, 100 + rows + C, CPU)
        gamma, beta, rmean, rvar = Bd.fin_params(C, C, CPU)
        folded = rows > 1024
        p = (Bd.fold_f32(partial) if folded else partial).double()     # the kernel: f32 fold above 1024 rows, then double
        m = p[:, 0].sum(0) / count
        var = (p[:, 1].sum(0) / count - m * m).clamp_min(0)
        inv = 1 / torch.sqrt(var + Bd.EPS)
        got = {"mean": m, "invstd": inv, "scale": gamma.double() * inv, "shift": beta.double() - m * gamma.double() * inv,
               "running_mean": (1 - Bd.MOMENTUM) * rmean.double() + Bd.MOMENTUM * m,
               "running_var": (1 - Bd.MOMENTUM) * rvar.double() + Bd.MOMENTUM * var * count / (count - 1)}
        ref = Bd.bn_finalize_ref(partial, count, gamma, beta, rmean, rvar, folded)
        assert set(ref) == set(got)
        for k, (r, b) in ref.items():
            assert bool((b > 0).all()) and bool((b <= 1e-3 * (r.abs() + 1)).all())      # a bound, and not a loose one
            _ok(k, got[k].float(), r, b)
            if folded and k == "invstd":   # the f32 fold really differs from the double sum, and the f32 rounding alone
                assert not torch.equal(p[:, 1].sum(0), partial.double()[:, 1].sum(0))   # would not cover a wrong fold:
                wrong = Bd.fold_f32(partial[:-1]).double()                               # (a fold that loses its last row)
                mw = wrong[:, 0].sum(0) / count
                iw = 1 / torch.sqrt((wrong[:, 1].sum(0) / count - mw * mw).clamp_min(0) + Bd.EPS)
                assert Bd.ratio(iw.float(), r, b) > 1.0


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", Bd.ACT_SHAPES)
def test_bn_act_bounds(dt, shape):
    M, C = shape
    y, res, sc, sh, rs, rb = Bd.act_inputs(M, C, dt, 9 + M, CPU)
    for residual in ("none", "plain", "affine"):
        for relu in (0, 1):
            r_, rs_, rb_ = (None, None, None) if residual == "none" else (res, None, None) if residual == "plain" else (res, rs, rb)
            v = y.float() * sc + sh
            if r_ is not None:
                v = v + (r_.float() * rs_ + rb_ if rs_ is not None else r_.float())
            if relu:
                v = torch.relu(v)
            ref, bound = Bd.bn_act_ref(y, sc, sh, r_, rs_, rb_, relu, dt)
            _ok("bn_act", v.to(dt), ref, bound)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", Bd.BWD_SHAPES + [(128, 24), (1, 24)])
def test_bn_bwd_bounds(dt, shape):
    M, C = shape
    g, mask, y, mean, invstd, gamma = Bd.bwd_inputs(M, C, dt, True, 31 + M, CPU)
    for mk in (None, mask):
        gm = g.float() if mk is None else torch.where(mk.float() > 0, g.float(), torch.zeros(()))
        if 256 % (C // 8) == 0:
            rows = Bd.bwd_partial_rows(M, C)
            n = -(-M // rows) + 40
            s1, s2, a1, a2 = Bd.bwd_sums_ref(g, mk, y, mean, invstd)
            _ok("sum g", gm.sum(0, dtype=torch.float32), s1, Bd.sum_bound(n, a1))
            _ok("sum g xhat", (gm * (y.float() - mean) * invstd).sum(0, dtype=torch.float32), s2, Bd.sum_bound(n, a2))
        coef = Bd.bwd_coef(g, mk, y, mean, invstd, gamma)
        ca, cb, cc = coef
        general = ca * (gm - cb - (y.float() - mean) * invstd * cc)
        ref, bound, _ = Bd.bwd_apply_ref(g, mk, y, mean, invstd, coef, dt, False)
        _ok("apply, general form", general.to(dt), ref, bound)
        Q = -ca * cc * invstd
        R = -ca * cb - Q * mean
        ref, bound, _ = Bd.bwd_apply_ref(g, mk, y, mean, invstd, coef, dt, True)
        _ok("apply, folded form", (ca * gm + Q * y.float() + R).to(dt), ref, bound)
        if M > 1:   # the sign of R matters at these inputs: the bound would catch it
            assert Bd.ratio((ca * gm + Q * y.float() - R).to(dt), ref, bound) > 1.0


def test_bn_bwd_apply_dispatch_restated():
    for (M, C), light in (((128, 24), True), ((1, 24), False), ((Bd.LARGE_M, Bd.LARGE_C), True)):
        assert Bd.light_route(M, C, torch.bfloat16, None, None) == light
        assert not Bd.light_route(M, C, torch.bfloat16, None, object()) and not Bd.light_route(M, C, torch.float32, None, None)
    for M, C in Bd.BWD_SHAPES:
        assert Bd.light_route(M, C, torch.bfloat16, None, None)
    cgs, stride = Bd.LARGE_C // 4, 16384 * 256
    assert Bd.LARGE_M * cgs == 3 * stride + 16              # pair loop, then the single-element tail
    assert 16384 * 256 < Bd.LARGE_M * (Bd.LARGE_C // 8) < 2 * 16384 * 256   # a second trip for some threads only


@pytest.mark.parametrize("rows,C,acc,count", [(1, 8, 0, 5), (17, 24, 1, 1000), (1024, 520, 1, 77), (16, 64, 0, 0), (1089, 64, 1, 9999)])
def test_bn_bwd_finalize_bounds(rows, C, acc, count):
    gen = torch.Generator().manual_seed(rows + C)
    partial = torch.randn(rows, 2, C, generator=gen) + 0.3
    gamma, invstd = 0.5 + torch.rand(C, generator=gen), 0.5 + torch.rand(C, generator=gen)
    pre_g, pre_b = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    folded = rows > 1024
    p = (Bd.fold_f32(partial) if folded else partial).double()
    s1, s2 = p[:, 0].sum(0), p[:, 1].sum(0)
    got = {"coef0": gamma * invstd, "dgamma": pre_g + s2.float() if acc else s2.float(), "dbeta": pre_b + s1.float() if acc else s1.float(),
           "coef1": (s1 / count).float() if count else torch.zeros(C), "coef2": (s2 / count).float() if count else torch.zeros(C)}
    for k, (r, b) in Bd.bwd_finalize_ref(partial, count, gamma, invstd, pre_g if acc else None, pre_b if acc else None, folded).items():
        _ok(k, got[k], r, b)


def test_bn_eval_bounds():
    for C in (8, 24, 64, 520):
        gamma, beta, rmean, rvar = Bd.fin_params(C, 200, CPU)
        inv = 1.0 / torch.sqrt(rvar + torch.tensor(1e-5))
        s = gamma * inv
        ref = Bd.bn_eval_ref(gamma, beta, rmean, rvar)
        _ok("scale", s, *ref["scale"]), _ok("invstd", inv, *ref["invstd"]), _ok("shift", beta - rmean * s, *ref["shift"])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("hw", Bd.POOL_HW)
@pytest.mark.parametrize("C", Bd.POOL_C)
def test_avgpool_bounds(dt, hw, C):
    for batch in Bd.POOL_BATCH:
        x, d = Bd.pool_inputs(batch, hw, C, dt, hw + C + batch, CPU)
        assert hw < 3 or (bool((x.float() == 0).any()) and bool(torch.signbit(x.float()[x.float() == 0]).any()))
        inv = torch.tensor(1.0, dtype=torch.float32) / hw
        _ok("avgpool", (x.float().sum(1, dtype=torch.float32) * inv).to(dt), *Bd.avgpool_ref(x, dt))
        gx = torch.where(x.float() > 0, d.float().unsqueeze(1) * inv, torch.zeros(()))
        _ok("avgpool_bwd", gx.to(dt), *Bd.avgpool_bwd_ref(d, x, dt))


def _quad_standin(q, d, B, ld, col0):
    """index arithmetic of the kernels: window (ph, pw) of region image b*4 + quad, first maximum in scan order, destination
    col0 + quad*1152 + c*9 + ph*3 + pw"""
    w = q.float()[:, :6, :6, :].reshape(B * 4, 3, 2, 3, 2, 128).permute(0, 1, 3, 5, 2, 4).reshape(B * 4, 3, 3, 128, 4)
    mx, am = w.max(-1)                                          # (ties: the first index)
    dst = mx.permute(0, 3, 1, 2).reshape(B, 4 * 1152)           # [img][c][ph][pw]
    gd = d.float()[:, col0:col0 + 4608].reshape(B * 4, 128, 3, 3).permute(0, 2, 3, 1)
    gd = torch.where(mx > 0, gd, torch.zeros(()))
    o = torch.zeros(B * 4, 3, 3, 128, 4).scatter_(-1, am.unsqueeze(-1), gd.unsqueeze(-1))
    dq = torch.zeros(B * 4, 7, 7, 128)
    dq[:, :6, :6, :] = o.view(B * 4, 3, 3, 128, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B * 4, 6, 6, 128)
    return dst, dq


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B", [1, 3])
def test_quad_pool_reference(dt, B):
    q, d = Bd.quad_inputs(B, dt)
    assert torch.equal(q, Bd.quad_inputs(B, dt)[0])             # fixed seed
    share = Bd.quad_tie_share(q)
    print(f"  positive ties in {share:.1%} of the windows")
    assert share >= 0.05
    # the largest value of every map lies in the dropped row and in the dropped column only
    top = q.float().amax((1, 2))
    assert bool((q.float()[:, 6].amax(1) == top).all()) and bool((q.float()[:, :, 6].amax(1) == top).all())
    assert bool((q.float()[:, :6, :6].amax((1, 2)) < top).all())
    for ld in (4608, 5376):
        pooled, dq = Bd.quad_pool_ref(q, d[:, :ld], B, ld, 0)
        dst, dq_s = _quad_standin(q, d[:, :ld], B, ld, 0)
        assert torch.equal(dst.double(), pooled) and torch.equal(dq_s.double(), dq)
        assert bool((dq[:, 6] == 0).all()) and bool((dq[:, :, 6] == 0).all()) and bool((dq != 0).any())


def _hash_keep(seed, n, p):
    """the counter hash of the dropout kernel (the splitmix64 finaliser over seed + i * golden ratio), upper 32 bits >= p * 2^32"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    thr = np.uint64(int(float(np.float32(p)) * 4294967296.0))
    return torch.from_numpy((z >> np.uint64(32)) >= thr)


@pytest.mark.parametrize("p", Bd.DROP_P)
def test_dropout_windows(p):
    n = Bd.DROP_ROWS * Bd.DROP_COLS
    assert n == 1 << 20
    masks = {"counter hash": (_hash_keep(1234, n, p), _hash_keep(99991, n, p))}
    g = torch.Generator().manual_seed(3)
    masks["bernoulli"] = tuple(torch.rand(n, generator=g) >= p for _ in range(2))
    for name, (a, b) in masks.items():
        for what, v, lo, hi in Bd.dropout_conditions(a.view(Bd.DROP_ROWS, Bd.DROP_COLS), b.view(Bd.DROP_ROWS, Bd.DROP_COLS), p):
            assert lo < hi and lo <= v <= hi, (name, what, v, lo, hi)
    pk = 1 - float(np.float32(p))
    lo, hi = [c for c in Bd.dropout_conditions(a.view(Bd.DROP_ROWS, -1), b.view(Bd.DROP_ROWS, -1), p) if c[0] == "kept share"][0][2:]
    assert math.ceil(lo * n) < math.floor(hi * n) and hi - lo < 0.01 and lo < pk < hi      # non-empty, and a real constraint
    # the kept value: fl(1 / (1 - p)) in f32, and its bf16 rounding
    kept = torch.ones((), dtype=torch.float32) / (torch.ones((), dtype=torch.float32) - torch.tensor(p, dtype=torch.float32))
    assert abs(float(kept) - 1 / (1 - p)) <= 4 * Bd.U / (1 - p) and abs(float(kept.bfloat16()) - float(kept)) <= Bd.UB * float(kept)


@pytest.mark.parametrize("case", Bd.GEMM_CASES, ids=[c[0] for c in Bd.GEMM_CASES])
def test_gemm_small_bounds(case):
    name, M, N, K, adt, bdt, cdt, ak, bk, has_bias, relu, acc, cpad, aoff = case[:14]
    o = Bd.gemm_operands(case, CPU)
    assert o["A"].shape == (M, K) and o["B"].shape == (N, K)
    assert o["A"].stride() == (o["ars"], o["aks"]) and o["B"].stride() == (o["brs"], o["bks"])
    v = o["A"].float() @ o["B"].float().t()
    if has_bias:
        v = v + o["bias"]
    if acc:
        v = v + o["cfill"].float()
    if relu:
        v = torch.relu(v)
    ref, bound = Bd.gemm_ref(o["A"], o["B"], o["bias"], o["cfill"], relu, cdt)
    _ok(name, v.to(cdt), ref, bound)


def test_gemm_small_cases_reach_every_kernel():
    """the dispatch of qt_gemm_small restated: every kernel, both staging orders of the tile kernel, every epilogue option"""
    seen, epi = set(), set()
    for name, M, N, K, adt, bdt, cdt, ak, bk, has_bias, relu, acc, cpad, aoff in (c[:14] for c in Bd.GEMM_CASES):
        ea, eb = (2 if adt == Bd.BF16 else 4), (2 if bdt == Bd.BF16 else 4)
        if K > 96 and M >= 32 and N >= 32:
            kind = f"tile a{ak} b{bk}"
        elif K <= 96:
            kind = "thread"
        else:
            vec = (not ak and not bk and K % 8 == 0 and (aoff * ea) % (8 * ea) == 0
                   and not (adt == Bd.F32 and bdt == Bd.BF16))
            kind = f"vec {ea}{eb}" if vec else "wave"
        assert name.split()[0] == kind.split()[0], (name, kind)
        seen.add(kind)
        epi |= {("bias", has_bias), ("relu", relu), ("acc", acc), ("bf16 C", cdt == Bd.BF16), ("padded C", cpad > 0)}
    assert seen == {"thread", "wave", "vec 22", "vec 24", "vec 44", "tile a0 b0", "tile a0 b1", "tile a1 b0", "tile a1 b1"}
    assert len(epi) == 10
