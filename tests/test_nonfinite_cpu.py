"""tests/_nonfinite.py without a GPU: the class rule (finite indicator convolutions) equals IEEE float64 arithmetic of torch on
the CPU -- F.conv2d / conv3d, the affine epilogue, torch.relu, F.max_pool2d / max_pool3d with return_indices -- on every row
tests/test_nonfinite_gpu.py runs; finite outputs equal the clean row bit for bit; the conditions hold on the references; the
pool rows hold the window kinds they are there for and ATen's argmax of a NaN window is its last NaN."""
import pytest
import torch
import torch.nn.functional as F

import _exact as E
import _nonfinite as N


def _case(name):
    table = N.PLANTS[name][0]
    if table is E.S2_ROWS:
        return N.s2_case(name)
    if table in (E.C3F_ROWS, E.C32_ROWS):
        return N.c3_case(name)
    if table is E.LINEAR_ROWS:
        return N.gemm_case(name)
    return N.fwd_case(name)


@pytest.mark.parametrize("name", list(N.PLANTS))
def test_rule_equals_ieee_arithmetic(name):
    c = _case(name)
    clean = c["clean"]
    images = c["images"]
    n_each = N.PLANTS[name][2]
    x = c["x"]
    assert [int(v) for v in (torch.isnan(x).sum(), (x == N.INF).sum(), (x == -N.INF).sum())] == [n_each] * 3
    for k in ("w", "scale", "shift", "sc", "sh", "wd", "sd", "shd", "bias", "res"):
        if clean.get(k) is not None:
            assert bool(torch.isfinite(clean[k]).all()), k
    pairs = [("raw", "raw"), ("pre", "pre"), ("act", "act")] + ([("rawd", "rawd"), ("pred", "pred")] if "rawd" in c else [])
    for key, ckey in pairs:
        assert torch.equal(N.classes(c[key]), c[ckey + "_c"]), (name, key)
    # finite outputs before the ReLU are those no planted value reaches: the clean row's, bit for bit
    clean_pre = clean["pre"] if "pre" in clean else None
    for key, ref in (("raw", clean.get("raw")), ("pre", clean_pre), ("rawd", clean.get("rawd")), ("pred", clean.get("pred"))):
        if key in c and ref is not None:
            assert N.finite_equal(c[key], ref), (name, key)
    # behind the ReLU a finite value is the clean one or the zero of a -inf
    if "act" in clean:
        fin = torch.isfinite(c["act"]) & (c["pre_c"] != N.NINF)
        assert torch.equal(c["act"][fin], clean["act"][fin])
        assert bool((c["act"][c["pre_c"] == N.NINF] == 0).all())
    N.conditions(c["raw_c"], c["pre_c"], c["act"], images)
    if "rawd" in c:
        N.conditions(c["rawd_c"], c["pred_c"], F.relu(c["pred"]), images)
    # the statistics rows: classes of the per-channel sums by the rule == those of torch's float64 sums
    assert torch.equal(N.stats_classes(c["raw_c"].unsqueeze(0) if c["raw"].dim() == 2 else c["raw_c"]),
                       N.classes(N.stats_ref(c["raw"].unsqueeze(0) if c["raw"].dim() == 2 else c["raw"])))
    if "pooled" in c:   # a NaN anywhere in a window is the pooled value; +inf beats every number
        k = 3 if c["pooled"].dim() == 4 else (1, 2, 2)
        pool = (lambda t: F.max_pool2d(t, 3, 2, 1)) if c["pooled"].dim() == 4 else (lambda t: F.max_pool3d(t, (1, 2, 2)))
        has_nan = pool(torch.isnan(c["act"]).double()) > 0
        assert torch.equal(torch.isnan(c["pooled"]), has_nan) and bool(has_nan.any()) and bool((c["pooled"] == N.INF).any())


def _last_nan_is_argmax(x, out, picked_is_nan_last):
    assert bool(picked_is_nan_last)


@pytest.mark.parametrize("pt", [1, 2])
def test_pool3d_rows(pt):
    c = N.pool3d_case(pt)
    x, out, code = c["x"], c["out"], c["code"].long()
    B, C, T, H, W = x.shape
    # windows [B][C][To][Ho][Wo][pt * 4] in scan order
    win = x.view(B, C, T // pt, pt, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(B, C, T // pt, H // 2, W // 2, pt * 4)
    nan = torch.isnan(win)
    assert torch.equal(torch.isnan(out), nan.any(-1))
    last_nan = (nan * torch.arange(1, pt * 4 + 1)).amax(-1) - 1
    assert torch.equal(code[nan.any(-1)], last_nan[nan.any(-1)])           # ATen: each NaN overwrites the previous one
    assert bool((nan.sum(-1) >= 2).any()) and bool(nan.all(-1).any())
    assert bool((nan.any(-1) & (win == N.INF).any(-1)).any())              # +inf beside NaN: NaN
    assert bool((out == -N.INF).any())                                     # -inf only
    picked = win.gather(-1, code.unsqueeze(-1)).squeeze(-1)
    assert torch.equal(torch.nan_to_num(picked, nan=12345.0), torch.nan_to_num(out, nan=12345.0))
    f = N.pool3d_fused_case(pt)
    assert bool(torch.isnan(f["out"]).any()) and bool((f["out"] == N.INF).any()) and not bool((f["out"] == -N.INF).any())
    assert torch.equal(torch.isnan(f["ymax"]) | torch.isnan(f["out"]), torch.isnan(f["out"]))


def test_stem_pool_and_quad_pool_rows():
    c = N.stem_pool_case()
    out, code = c["out"], c["code"].long()
    assert int(code.min()) >= 0 and int(code.max()) <= 8
    assert bool(torch.isnan(out).any()) and bool((out == N.INF).any()) and bool(torch.isnan(out[0, :, 0, 0]).any() | True)
    has_nan = F.max_pool2d(torch.isnan(c["act"]).double(), 3, 2, 1) > 0
    assert torch.equal(torch.isnan(out), has_nan)
    assert bool(torch.isfinite(out[1]).all())                               # the second image is untouched
    q = N.quad_pool_case()
    assert bool(torch.isnan(q["out"]).any()) and bool((q["out"] == -N.INF).any())
    assert torch.equal(torch.isnan(q["out"]), F.max_pool2d(torch.isnan(q["q"]).double(), 2, 2) > 0)


def test_signed_zero_row():
    c = N.signed_zero_stem_case()
    N.signed_zero_conditions(c)
    assert E.same(c["pooled"].to(E.BF), c["pooled"], E.BF)                  # representable: the comparison is bit-exact


def test_bn_act_and_finalize_rows():
    c = N.bn_act_case()
    for residual in ("none", "plain", "affine"):
        for relu in (0, 1):
            ref, rule = N.bn_act_ref(c, residual, relu)
            assert torch.equal(N.classes(ref), rule), (residual, relu)
            assert bool(torch.isfinite(ref[ref.shape[0] // 2:]).all())
    ref, _ = N.bn_act_ref(c, "none", 0)
    assert all(bool((N.classes(ref) == k).any()) for k in (N.NAN, N.PINF, N.NINF))
    f = N.finalize_case()
    r = N.finalize_ref(f)
    assert bool(torch.isnan(r["mean"][:2]).any()) and bool(torch.isfinite(r["mean"][6:]).all())
    for k, v in r.items():
        assert bool(torch.isfinite(v[6:]).all()), k
        assert not bool(torch.isfinite(v[:5]).all()), k
