"""The float64 reference, the input classes, the bounds and the path table of tests/_pool3d_bounds.py, checked WITHOUT a GPU: the
hand-written reference against F.max_pool3d / F.batch_norm and their autograd in float64, a plain torch-f32 restatement of every
kernel of csrc/video3d.hip that tests/test_pool3d_gpu.py runs, passed through the very comparisons the kernels go through, the
conditions the classes promise, and which kernel / which loop path every shape takes, re-derived from the launchers' formulas.
So a failure of tests/test_pool3d_gpu.py is the kernel's, not the bound's or the reference's.  The restatements are also damaged
on purpose, one way a kernel could be subtly wrong at a time; every damage must be caught by at least one case."""
import pytest
import torch
import torch.nn.functional as F

import _bounds as Bd
import _pool3d_bounds as Pb

F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")
KINDS = ["grid", "random"]
POOL_RUNS = [("c1", 1, "f32"), ("c1", 1, "bf16"), ("c1", 2, "f32"), ("c1", 2, "bf16"), ("c2", 1, "bf16"), ("c2", 2, "f32"),
             ("c3", 1, "f32"), ("c3", 2, "bf16")]


@pytest.fixture(scope="module", autouse=True)
def _drop_references():
    yield
    Pb.clear_caches()


def _ncthw(t):
    """[T][B][H][W][C] -> [B][C][T][H][W]"""
    return t.permute(1, 4, 0, 2, 3).contiguous()


def _tb(t):
    return t.permute(2, 0, 3, 4, 1).contiguous()


# ----------------------------------------------------------------------------------------------------------------------
# the reference is right
# ----------------------------------------------------------------------------------------------------------------------
def _codes_from_flat(idx, pt, H, W):
    """torch's flat (t * H + h) * W + w indices [B][C][To][Ho][Wo] -> tap codes (dt * 2 + dh) * 2 + dw, time-major NHWC"""
    t, h, w = idx // (H * W), (idx // W) % H, idx % W
    to = torch.arange(idx.shape[2]).view(1, 1, -1, 1, 1)
    ho = torch.arange(idx.shape[3]).view(1, 1, 1, -1, 1)
    wo = torch.arange(idx.shape[4]).view(1, 1, 1, 1, -1)
    dt, dh, dw = t - to * pt, h - ho * 2, w - wo * 2
    assert bool(((dt >= 0) & (dt < pt) & (dh >= 0) & (dh < 2) & (dw >= 0) & (dw < 2)).all())
    return _tb((dt * 2 + dh) * 2 + dw).to(torch.uint8)


@pytest.mark.parametrize("name,pt,dtn", POOL_RUNS)
@pytest.mark.parametrize("kind", KINDS)
def test_reference_equals_torch_float64(kind, name, pt, dtn):
    """ties included: ATen's CPU kernel keeps the first maximum in scan order, and so does the reference"""
    c = Pb.case(kind, name, pt, dtn)
    T, B, H, W, C = c["shape"]
    a = _ncthw(c["act"]).requires_grad_(True)
    out, idx = F.max_pool3d(a, (pt, 2, 2), (pt, 2, 2), return_indices=True)
    assert torch.equal(_tb(out.detach()), c["pooled"])
    assert torch.equal(_codes_from_flat(idx, pt, H, W), c["code"])
    ymax = _ncthw(c["y"]).flatten(2).gather(2, idx.flatten(2)).view_as(idx)
    assert torch.equal(_tb(ymax), c["ymax"])
    # g: the pool's gradient, then the ReLU's (zero where the maximum is zero; torch puts the pool's gradient there first)
    out.backward(_ncthw(torch.where(c["pooled"] > 0, c["d"], torch.zeros((), dtype=torch.float64))))
    assert torch.equal(_tb(a.grad), c["g"])
    x = _ncthw(c["x"]).requires_grad_(True)
    out, idx = F.max_pool3d(x, (pt, 2, 2), (pt, 2, 2), return_indices=True)
    out.backward(_ncthw(c["d"]))
    assert torch.equal(_tb(out.detach()), c["xpooled"]) and torch.equal(_codes_from_flat(idx, pt, H, W), c["xcode"])
    assert torch.equal(_tb(x.grad), c["dx"])


@pytest.mark.parametrize("pt", [1, 2])
def test_reference_equals_autograd_on_tie_free_data(pt):
    """BatchNorm3d (batch statistics) -> ReLU -> MaxPool3d and autograd, float64, continuous data (no two taps equal)"""
    T, B, H, W, C = Pb.shape("c1", pt)
    g = torch.Generator().manual_seed(40 + pt)
    y = torch.randn((T, B, H, W, C), generator=g, dtype=torch.float64) * 1.5 + torch.randn(C, generator=g, dtype=torch.float64)
    gamma = (0.5 + torch.rand(C, generator=g, dtype=torch.float64)) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)
    beta = torch.randn(C, generator=g, dtype=torch.float64) * 0.5
    d = torch.randn(Pb.pooled_shape(T, B, H, W, C, pt), generator=g, dtype=torch.float64)
    yr = _ncthw(y).requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    out = F.max_pool3d(F.relu(F.batch_norm(yr, None, None, gr, br, True, 0.1, Bd.EPS)), (pt, 2, 2), (pt, 2, 2))
    out.backward(_ncthw(d))
    mean = y.mean((0, 1, 2, 3))
    invstd = 1.0 / torch.sqrt(((y - mean) ** 2).mean((0, 1, 2, 3)) + Bd.EPS)
    scale = gamma * invstd
    shift = beta - mean * scale
    pooled, code, ymax = Pb.window_max(Pb.activation(y, scale, shift, F32), y, pt)
    gg = Pb.scatter(torch.where(pooled > 0, d, torch.zeros((), dtype=torch.float64)), code, pt, (T, B, H, W, C))
    S = Pb.sums_ref(gg, y, mean, invstd)
    M = T * B * H * W
    dy = Pb.dy_ref(gg, y, mean, invstd, torch.stack([scale, S["s1"] / M, S["s2"] / M]))
    # the pooled-side identity: every pooled cell sends its gradient to exactly one position
    gc = torch.where(pooled > 0, d, torch.zeros((), dtype=torch.float64))
    cell_s2 = (gc * (ymax - mean) * invstd).sum((0, 1, 2, 3))

    def rel(a, b):
        return float((a - b).abs().max() / b.abs().max())

    assert rel(_tb(out.detach()), pooled) <= 1e-12 and rel(dy, _tb(yr.grad)) <= 1e-12
    assert rel(S["s2"], gr.grad) <= 1e-12 and rel(S["s1"], br.grad) <= 1e-12
    assert rel(cell_s2, gr.grad) <= 1e-12 and rel(gc.sum((0, 1, 2, 3)), br.grad) <= 1e-12


# ----------------------------------------------------------------------------------------------------------------------
# the input classes keep their promises
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pt", [1, 2])
@pytest.mark.parametrize("dtn", ["f32", "bf16"])
def test_grid_class_conditions(dtn, pt):
    c = Pb.case("grid", "c1", pt, dtn)
    C = c["shape"][4]
    ties, masked, rounding = c["shares"]
    print(f"  grid c1 pool_t={pt} {dtn}: positive ties {ties:.3f}, masked {masked:.3f}, winner changed by rounding {rounding}")
    assert ties >= Pb.MIN_TIES and masked >= Pb.MIN_MASKED
    assert (rounding is not None and rounding >= Pb.MIN_ROUNDING) if dtn == "bf16" else rounding is None
    zero = torch.nonzero(c["scale"] == 0).flatten().tolist()
    assert len(zero) >= 2
    for ch in zero:   # all taps tie at 0.5: the first one is recorded; or everything is masked: code 0, no gradient
        assert bool((c["code"][..., ch] == 0).all())
        if float(c["shift"][ch]) > 0:
            assert bool((c["pooled"][..., ch] == 0.5).all())
        else:
            assert bool((c["pooled"][..., ch] == 0).all()) and bool((c["g"][..., ch] == 0).all())
    assert {float(c["shift"][ch]) for ch in zero} == {0.5, -0.5}
    assert sorted(torch.unique(c["code"]).tolist()) == list(range(4 * pt)) == sorted(torch.unique(c["xcode"]).tolist())
    assert set(c["scale"].tolist()) == set(Pb.SCALES)
    for k, grid in (("mean", 8), ("d", 8), ("y", 256 if c["tie"] else 8)):
        assert torch.equal(torch.round(c[k] * grid), c[k] * grid)
    assert torch.equal(torch.frexp(c["invstd"])[0], torch.full((C,), 0.5, dtype=torch.float64)) and float(c["d"].abs().max()) <= 4
    ca, cb, cc = c["coef"]
    assert set(ca.tolist()) == {1.0, 0.5} and set(cc.tolist()) == {1.0, 2.0} and torch.equal(torch.round(cb * 8), cb * 8)
    if pt == 2:   # the floor-mode remainder: no gradient, but dy = a (-b - xhat c) is not zero there
        T, B, H, W, _ = c["shape"]
        for rem in (c["g"][T - 1], c["g"][:, :, H - 1], c["g"][:, :, :, W - 1], c["dx"][T - 1]):
            assert bool((rem == 0).all())
        assert float((c["dy"][T - 1] != 0).double().mean()) > 0.5
    if c["tie"]:
        yt = c["y"][..., Pb.TIE_CH]
        assert float(yt.min()) >= 0.5 and float(yt.max()) < 1.0 and len(torch.unique(yt)) == 128
        v = yt + 8.0
        assert torch.equal(v.float().double(), v) and not torch.equal(v.to(BF16).double(), v)


@pytest.mark.parametrize("dtn", ["f32", "bf16"])
def test_random_class_conditions(dtn):
    c = Pb.case("random", "c1", 2, dtn)
    red = (0, 1, 2, 3)
    m, sd = c["y"].mean(red), c["y"].std(red, unbiased=False)
    assert torch.equal(c["y"].to(BF16).double(), c["y"]) and float(c["y"].abs().max()) < 8.0
    assert float(m.abs().max()) > 4.0 and float(sd.min()) < 0.5
    assert bool((c["gamma"] > 0).any()) and bool((c["gamma"] < 0).any())
    for k in ("mean", "invstd", "coef", "gamma"):                 # f32 values, the same for kernel and reference
        assert torch.equal(c[k].float().double(), c[k])
    assert c["shares"][1] >= Pb.MIN_MASKED
    b = Pb.dy_bound(c["dy"], c["g"], c["y"], c["mean"], c["invstd"], c["coef"], c["dt"])
    assert bool((b <= 2.0 ** -7 * c["dy"].abs() + 1e-4).all())     # not loose: half a bf16 unit in the last place + 14 U of the terms


def test_paths():
    S = Pb.LIGHT_THREADS
    assert S == 327680 and Pb.LIGHT_MIN_DEFAULT == 2 ** 20
    n = {name: Pb.apply_groups(*Pb.shape(name, pt)) for name, pt in Pb.LIGHT_CASES}
    assert n == {"L1": 47520, "L2": 460672, "L3": 691008}
    assert n["L1"] < S < n["L2"] < 2 * S < n["L3"] < 3 * S
    p1, p2, p3 = (Pb.light_paths(n[k]) for k in ("L1", "L2", "L3"))
    assert p1 == dict(idle_threads=True, second_row_live=False, second_row_mixed=False, trips=1, later_trip_second_row_dead=False)
    assert p2 == dict(idle_threads=False, second_row_live=True, second_row_mixed=True, trips=1, later_trip_second_row_dead=False)
    assert p3 == dict(idle_threads=False, second_row_live=True, second_row_mixed=False, trips=2, later_trip_second_row_dead=True)
    # what the existing op-level test reaches with the threshold at 1: one row per thread, one trip
    old = Pb.light_paths(Pb.apply_groups(5, 2, 9, 11, 16))
    assert not old["second_row_live"] and old["trips"] == 1
    # dispatch: bf16 only, full-width rows only, a group count that divides 256, the threshold
    for name, pt in Pb.LIGHT_CASES:
        T, B, H, W, C = Pb.shape(name, pt)
        assert Pb.light_taken(BF16, C, C, C, n[name], 1) and not Pb.light_taken(BF16, C, C, C, n[name], n[name] + 1)
        assert not Pb.light_taken(BF16, C, C, C, n[name]) and not Pb.light_taken(F32, C, C, C, n[name], 1)
        assert T * B * H * W * C * 2 <= 11.1e6                                    # the largest map: 11 MB
    T, B, H, W, C = Pb.shape("c3", 1)
    assert C // 8 == 3 and not Pb.light_taken(BF16, C, C, C, Pb.apply_groups(T, B, H, W, C), 1)
    T, B, H, W, C = Pb.shape("c1", 1)
    assert Pb.light_taken(BF16, C, C, C, Pb.apply_groups(T, B, H, W, C), 1)
    assert not Pb.light_taken(BF16, C, 32, C, Pb.apply_groups(T, B, H, W, C), 1)
    assert not Pb.light_taken(BF16, C, 32, 32, Pb.apply_groups(T, B, H, W, 32), 1)
    # no pool launch here reaches the 65 536-block cap; c1 takes more than one block, c2 a single thread group per channel group
    for name in Pb.SHAPES:
        for pt in (1, 2):
            T, B, H, W, C = Pb.shape(name, pt)
            assert -(-Pb.apply_groups(T, B, H, W, C) // 256) < Pb.POOL_GRID_CAP
    assert Pb.pool_grid(Pb.apply_groups(*Pb.shape("c1", 1))) > 1
    To, B, Ho, Wo, C = Pb.pooled_shape(*Pb.shape("c2", 2), 2)
    assert To * B * Ho * Wo * (C // 8) == 1
    # the packers
    for O, Op, I, Ip in Pb.PACK_TILE:
        assert Pb.pack_kernel(O, Op, I, Ip, 0) == "tile" and Pb.pack_kernel(O, Op, I, Ip, 0, aligned=False) == "element"
        assert not Pb.grid_strided(Pb.pack_total(Op, Ip, 0))
    assert [Pb.pack_kernel(O, Op, I, Ip, 0) for O, Op, I, Ip in Pb.PACK_ELEMENT] == ["element", "element"]
    assert [Pb.pack_kernel(O, Op, I, 0, 1) for O, Op, I in Pb.PACK_FIRST] == ["element", "element"]
    (O, Op, I, Ip), = [s for s in Pb.PACK_ELEMENT if s[0] == 256]
    assert Op * 27 * Ip == 1327104 and Pb.grid_strided(Pb.pack_total(Op, Ip, 0)) and O * I * 27 == 1271808 and Pb.grid_strided(O * I * 27)
    assert not Pb.grid_strided(Pb.pack_total(*Pb.PACK_ELEMENT[0][1::2], 0))
    # tiles of the LDS kernel: (64, 64, 32, 64): half the input-channel tiles are padding; (40, 64, 48, 64): 8 live rows
    O, Op, I, Ip = Pb.PACK_TILE[0]
    assert sum(c0 >= I for c0 in range(0, Ip, Pb.PK3_TI)) * 2 == Ip // Pb.PK3_TI
    O, Op, I, Ip = Pb.PACK_TILE[1]
    assert O - Pb.PK3_TO == 8 and Op // Pb.PK3_TO == 2 and I < Ip
    assert all(27 * I <= 128 for _, _, I in Pb.PACK_FIRST) and 27 * 5 > 128


# ----------------------------------------------------------------------------------------------------------------------
# torch-f32 restatements of the kernels (with the damage they can be given)
# ----------------------------------------------------------------------------------------------------------------------
def _store(v, dt, truncate=False):
    """an f32 value into the activation type: round-to-nearest-even, as the kernels' (T) conversion"""
    if dt == F32:
        return v.float()
    if truncate:
        return (v.float().contiguous().view(torch.int32) & -65536).view(F32).to(BF16)
    return v.float().to(BF16)


def _swapped(dt, dh, dw):
    return (dt * 2 + dw) * 2 + dh


def k_pool(c, wins=torch.gt, code=Pb.tap_code):
    """pool3d_max_kernel on the case's x"""
    x = c["x"].to(c["dt"]).float()
    best, idx, _ = Pb.window_max(x, x, c["pt"], wins, code)
    return _store(best, c["dt"]), idx


def k_pool_bwd(c, remainder=True):
    """pool3d_max_bwd_kernel: dx = dout where the code names the position, zero elsewhere and in the floor-mode remainder"""
    T, B, H, W, C = c["shape"]
    pt = c["pt"]
    dx = torch.full((T, B, H, W, C), NAN, dtype=c["dt"])
    body = Pb.scatter(c["d"].to(c["dt"]).float(), c["xcode"], pt, (T, B, H, W, C)).to(c["dt"])
    if remainder:
        dx.copy_(body)
    else:
        To, Ho, Wo = T // pt, H // 2, W // 2
        dx[:To * pt, :, :Ho * 2, :Wo * 2] = body[:To * pt, :, :Ho * 2, :Wo * 2]
    return dx


def k_fused(c, Cy=None, wins=torch.gt, code=Pb.tap_code, round_act=True, padding=True):
    """pool3d_bn_relu_max_kernel: the affine + ReLU in f32, rounded to the activation type before the comparison"""
    dt, C = c["dt"], c["shape"][4]
    Cy = C if Cy is None else Cy
    y = c["y"][..., :Cy].to(dt).float()
    a = (y * c["scale"][:Cy].float() + c["shift"][:Cy].float()).clamp_min(0.0)
    if round_act:
        a = _store(a, dt).float()
    best, idx, raw = Pb.window_max(a, y, c["pt"], wins, code)
    shape = tuple(best.shape[:4]) + (C,)
    pooled, ymax = torch.full(shape, NAN, dtype=dt), torch.full(shape, NAN, dtype=dt)
    arg = torch.full(shape, 0xFF, dtype=torch.uint8)
    pooled[..., :Cy], arg[..., :Cy], ymax[..., :Cy] = _store(best, dt), idx, _store(raw, dt)
    if padding:
        pooled[..., Cy:], arg[..., Cy:], ymax[..., Cy:] = 0, 0, 0
    return pooled, arg, ymax


def k_apply(c, Cy=None, Cd=None, gate=torch.gt, remainder="formula", padding=True, truncate=False):
    """pool3d_bn_bwd_apply_kernel on the REFERENCE's pooled map and codes: g = dout at the argmax where pooled > 0, zero elsewhere
    and in the remainder; dy = ca * (g - cb - (y - mean) * invstd * cc) in f32; zeros in the channels from Cy up"""
    dt, (T, B, H, W, C), pt = c["dt"], c["shape"], c["pt"]
    Cy = C if Cy is None else Cy
    Cd = C if Cd is None else Cd
    d, pooled = c["d"][..., :Cy].to(dt).float(), c["pooled"][..., :Cy].to(dt).float()
    g = Pb.scatter(torch.where(gate(pooled, torch.zeros(())), d, torch.zeros(())), c["code"][..., :Cy], pt, (T, B, H, W, Cy))
    ca, cb, cc = c["coef"][:, :Cy].float()
    y, mu, inv = c["y"][..., :Cy].to(dt).float(), c["mean"][:Cy].float(), c["invstd"][:Cy].float()
    o = ca * (g - cb - (y - mu) * inv * cc)
    if remainder == "zero":
        To, Ho, Wo = T // pt, H // 2, W // 2
        keep = torch.zeros((T, 1, H, W, 1), dtype=torch.bool)
        keep[:To * pt, :, :Ho * 2, :Wo * 2] = True
        o = torch.where(keep, o, torch.zeros(()))
    dy = torch.full((T, B, H, W, Cd), NAN, dtype=dt)
    dy[..., :Cy] = _store(o, dt, truncate)
    if padding:
        dy[..., Cy:] = 0
    return dy, g


def k_apply_light(c, second_row=True):
    """pool3d_bn_bwd_apply_light_kernel: the same arithmetic per 8-channel group; S resident threads, two groups per trip at
    i and i + S, `for (i = i0; i < n; i += 2 * S)`"""
    T, B, H, W, C = c["shape"]
    every, _ = k_apply(c)
    src = every.view(-1, 8)
    n, S = src.shape[0], Pb.LIGHT_THREADS
    assert n == Pb.apply_groups(T, B, H, W, C)
    out = torch.full_like(src, NAN)
    i0 = torch.arange(S)
    trip = 0
    while bool((i0 + 2 * trip * S < n).any()):
        for u in ((0, 1) if second_row else (0,)):
            i = i0 + (2 * trip + u) * S
            i = i[i < n]
            out[i] = src[i]
        trip += 1
    return out.view(T, B, H, W, C)


# ----------------------------------------------------------------------------------------------------------------------
# the restatements pass every comparison; each damage is caught
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pt,dtn", POOL_RUNS)
@pytest.mark.parametrize("kind", KINDS)
def test_kernels_restated_in_f32(kind, name, pt, dtn):
    c = Pb.case(kind, name, pt, dtn)
    assert Pb.pool_failures(c, *k_pool(c)) == []
    assert Pb.same(k_pool_bwd(c), c["dx"])
    assert Pb.forward_failures(c, *k_fused(c)) == []
    dy, g = k_apply(c)
    assert g.dtype == F32 and Pb.same(g, c["g"])
    bad, r = Pb.dy_check(c, dy)
    assert bad == []
    if r is not None:
        print(f"  err/bound dy (f32 restatement) {name} pool_t={pt} {dtn}: {r:.3f}")


@pytest.mark.parametrize("pt", [1, 2])
@pytest.mark.parametrize("dtn", ["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_narrow_rows_restated_in_f32(kind, dtn, pt):
    c = Pb.case(kind, "c1", pt, dtn)
    assert Pb.forward_failures(c, *k_fused(c, Cy=32), Cy=32) == []
    for Cd in (32, 64):
        assert Pb.dy_check(c, k_apply(c, Cy=32, Cd=Cd)[0], Cy=32, Cd=Cd)[0] == []
    # damage: the padding channels left unwritten
    assert "pooled padding" in Pb.forward_failures(c, *k_fused(c, Cy=32, padding=False), Cy=32)
    assert Pb.dy_check(c, k_apply(c, Cy=32, Cd=64, padding=False)[0], Cy=32, Cd=64)[0] == ["dy padding"]


@pytest.mark.parametrize("pt", [1, 2])
@pytest.mark.parametrize("dtn", ["f32", "bf16"])
def test_damaged_decisions_are_caught(dtn, pt):
    c = Pb.case("grid", "c1", pt, dtn)
    # last maximum wins
    assert Pb.pool_failures(c, *k_pool(c, wins=torch.ge)) == ["argmax"]
    assert Pb.forward_failures(c, *k_fused(c, wins=torch.ge)) == ["argmax", "y_at_max"]
    # the (dh, dw) bits of the code swapped
    assert Pb.pool_failures(c, *k_pool(c, code=_swapped)) == ["argmax"]
    assert Pb.forward_failures(c, *k_fused(c, code=_swapped)) == ["argmax"]
    # the gate pooled >= 0: the masked windows pass their gradient on
    dy, g = k_apply(c, gate=torch.ge)
    assert not Pb.same(g, c["g"]) and Pb.dy_check(c, dy)[0] == ["dy"]
    # comparison on the unrounded activation: seen in bf16 (the rounding-tie channels), invisible in f32
    bad = Pb.forward_failures(c, *k_fused(c, round_act=False))
    assert bad == (["argmax", "y_at_max"] if dtn == "bf16" else [])
    # a truncating bf16 store of dy
    if dtn == "bf16":
        assert Pb.dy_check(c, k_apply(c, truncate=True)[0])[0] == ["dy"]
    if pt == 2:
        # the floor-mode remainder left unwritten; dy of the remainder zero in place of a (-b - xhat c)
        assert not Pb.same(k_pool_bwd(c, remainder=False), c["dx"])
        assert Pb.dy_check(c, k_apply(c, remainder="zero")[0])[0] == ["dy"]


@pytest.mark.parametrize("dtn", ["f32", "bf16"])
def test_damage_is_outside_the_random_class_bounds(dtn):
    c = Pb.case("random", "c1", 2, dtn)
    assert Pb.dy_check(c, k_apply(c, gate=torch.ge)[0])[0] != []
    assert Pb.dy_check(c, k_apply(c, remainder="zero")[0])[0] != []
    wrong = c["coef"].clone()
    worst = int(c["dy"].abs().amax((0, 1, 2, 3)).argmax())
    wrong[0, worst] *= 1.0 + 2.0 ** -6        # gamma * invstd of one channel off by 1.6 %: inside 2e-2 of the maximum
    d = dict(c, coef=wrong)
    dy = k_apply(d)[0]
    assert float((dy.double() - c["dy"]).abs().max() / c["dy"].abs().max()) < 2e-2 and Pb.dy_check(c, dy)[0] != []
    if dtn == "bf16":
        assert Pb.dy_check(c, k_apply(c, truncate=True)[0])[0] != []


@pytest.mark.parametrize("name,pt", Pb.LIGHT_CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_resident_grid_loop_restated(kind, name, pt):
    c = Pb.build(kind, name, pt, "bf16")
    dy = k_apply_light(c)
    assert torch.equal(dy.view(torch.int16), k_apply(c)[0].view(torch.int16))          # the general kernel, bit for bit
    bad, r = Pb.dy_check(c, dy)
    assert bad == []
    if r is not None:
        print(f"  err/bound dy (f32 restatement, resident grid) {name} pool_t={pt}: {r:.3f}")
    # damage: the second row of a two-row trip skipped -- seen wherever a second row is live
    paths = Pb.light_paths(Pb.apply_groups(*c["shape"]))
    assert (Pb.dy_check(c, k_apply_light(c, second_row=False))[0] != []) == paths["second_row_live"]
    assert name == "L1" or paths["second_row_live"]


@pytest.mark.parametrize("dtn", ["f32", "bf16"])
@pytest.mark.parametrize("name,pt", [("c1", 1), ("c1", 2), ("c2", 2)])
def test_bn_sums_from_the_pooled_side_restated_in_f32(name, pt, dtn):
    """qt_bn_bwd_reduce's arithmetic on the pooled side (g = dout where pooled > 0, xhat from y_at_max) in f32, rows of 64 cells,
    the finalize step in float64 rounded to f32 once"""
    c = Pb.case("random", name, pt, dtn)
    dt, C = c["dt"], c["shape"][4]
    d, pooled, ymax = (c[k].to(dt).float().reshape(-1, C) for k in ("d", "pooled", "ymax"))
    cells = d.shape[0]
    g = torch.where(pooled > 0, d, torch.zeros(()))
    t = g * (ymax - c["mean"].float()) * c["invstd"].float()
    pad = (-cells) % 64
    rows = torch.stack([torch.cat([v, v.new_zeros(pad, C)]).view(-1, 64, C).sum(1) for v in (g, t)], 1)
    assert rows.dtype == F32
    s = rows.double().sum(0)
    M = c["y"].numel() // C
    coef = torch.stack([c["gamma"] * c["invstd"], s[0] / M, s[1] / M]).float()
    r = Pb.bn_sums_ratios(c, rows, cells, s[1].float(), s[0].float(), coef)
    print(f"  err/bound (f32 restatement) {name} pool_t={pt} {dtn}: " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0
    lost = rows.clone()
    lost[0] = 0                                # one row of cells dropped
    r = Pb.bn_sums_ratios(c, lost, cells, lost.double().sum(0)[1].float(), lost.double().sum(0)[0].float(), coef)
    assert max(r.values()) > 1.0


# ----------------------------------------------------------------------------------------------------------------------
# the packers
# ----------------------------------------------------------------------------------------------------------------------
def k_pack_element(w, Op, Ip, first, vecs, dt, with_wd, swap_wd=False, zero_pads=False, truncate=False):
    """pack_conv3d_block_kernel: one element of wf per index, its copy scattered into wd, then the five vectors"""
    O, I, _ = w.shape
    nf = Op * 128 if first else Op * 27 * Ip
    i = torch.arange(nf)
    if first:
        o, k = i >> 7, i & 127
        tap = k // I
        ch = k - tap * I
        ok = (o < O) & (k < 27 * I)
    else:
        ch, q = i % Ip, i // Ip
        tap, o = q % 27, q // 27
        ok = (o < O) & (ch < I)
    val = torch.where(ok, w[o.clamp(max=O - 1), ch.clamp(max=I - 1), tap.clamp(max=26)], torch.zeros(()))
    wf = _store(val, dt, truncate)
    wd = None
    if with_wd and not first:
        wd = torch.full((nf,), NAN, dtype=dt)
        wd[(o * 27 + tap) * Ip + ch if swap_wd else (ch * 27 + tap) * Op + o] = wf
    return wf, wd, _vectors(O, Op, vecs, zero_pads)


def _vectors(O, Op, vecs, zero_pads=False):
    vec = torch.full((5, Op), NAN)
    for v in range(5):
        cidx = torch.arange(Op)
        pad = 0.0 if zero_pads else (1.0 if v in (1, 4) else 0.0)
        src = vecs[v]
        vec[v] = torch.where(cidx < O, src[cidx.clamp(max=O - 1)], torch.full((), pad)) if src is not None else pad
    return vec


def k_pack_tile(w, Op, Ip, vecs, dt, with_wd, skip=None):
    """pack_conv3d_tile_kernel: a workgroup per 32 output x 16 input channels x 27 taps; rows past O and input-channel tiles
    past I are zeros; the last workgroup writes the vectors"""
    O, I, _ = w.shape
    assert Op % Pb.PK3_TO == 0 and Ip % Pb.PK3_TI == 0 and I % Pb.PK3_TI == 0
    wf = torch.full((Op, 27, Ip), NAN, dtype=dt)
    wd = torch.full((Ip, 27, Op), NAN, dtype=dt) if with_wd else None
    for o0 in range(0, Op, Pb.PK3_TO):
        for c0 in range(0, Ip, Pb.PK3_TI):
            if (o0, c0) == skip:
                continue
            tile = torch.zeros(Pb.PK3_TO, Pb.PK3_TI, 27)
            live = max(0, min(Pb.PK3_TO, O - o0))
            if c0 < I and live:
                tile[:live] = w[o0:o0 + live, c0:c0 + Pb.PK3_TI]
            wf[o0:o0 + Pb.PK3_TO, :, c0:c0 + Pb.PK3_TI] = _store(tile.permute(0, 2, 1), dt)
            if with_wd:
                wd[c0:c0 + Pb.PK3_TI, :, o0:o0 + Pb.PK3_TO] = _store(tile.permute(1, 2, 0), dt)
    return wf.flatten(), (wd.flatten() if with_wd else None), _vectors(O, Op, vecs)


def _pack_failures(got, w, Op, Ip, first, vecs, dt):
    wf, wd, vec = got
    rf, rd, rv = Pb.pack_ref(w, Op, Ip, first, vecs)
    bad = [] if Pb.same(wf, rf.to(dt).flatten()) else ["wf"]
    if wd is not None and not Pb.same(wd, rd.to(dt).flatten()):
        bad.append("wd")
    return bad if Pb.same(vec, rv) else bad + ["vec"]


@pytest.mark.parametrize("dt", [F32, BF16])
def test_pack_restated(dt):
    seen = set()
    for O, Op, I, Ip, first in [s + (0,) for s in Pb.PACK_TILE + Pb.PACK_ELEMENT] + [(O, Op, I, 0, 1) for O, Op, I in Pb.PACK_FIRST]:
        w, vecs = Pb.pack_weights(O, I, O + I), Pb.pack_vectors(O, O)
        assert Pb.bf16_tie_share(w) >= 0.01
        for with_wd in (True, False):
            args = (w, Op, Ip, first, vecs, dt)
            assert _pack_failures(k_pack_element(w, Op, Ip, first, vecs, dt, with_wd), *args) == []
            if Pb.pack_kernel(O, Op, I, Ip, first) == "tile":
                assert _pack_failures(k_pack_tile(w, Op, Ip, vecs, dt, with_wd), *args) == []
        # damage
        if not first:
            bad = _pack_failures(k_pack_element(w, Op, Ip, first, vecs, dt, True, swap_wd=True), *args)
            assert bad == (["wd"] if (O, Op) != (I, Ip) or O != I else bad)
            seen.update(bad)
        assert _pack_failures(k_pack_element(w, Op, Ip, first, vecs, dt, True, zero_pads=True), *args) == (["vec"] if Op > O else [])
        if dt == BF16:
            assert "wf" in _pack_failures(k_pack_element(w, Op, Ip, first, vecs, dt, True, truncate=True), *args)
        if Pb.pack_kernel(O, Op, I, Ip, first) == "tile":   # one 32 x 16 tile skipped: a live one, an all-padding one
            for skip in ((0, 0), (Op - Pb.PK3_TO, Ip - Pb.PK3_TI)):
                assert _pack_failures(k_pack_tile(w, Op, Ip, vecs, dt, True, skip=skip), *args) == ["wf", "wd"]
    assert "wd" in seen


def test_unpack_and_round_trip_restated():
    for O, Op, I, Ip, first in [s + (0,) for s in Pb.PACK_TILE + Pb.PACK_ELEMENT] + [(O, Op, I, 0, 1) for O, Op, I in Pb.PACK_FIRST]:
        w = Pb.pack_weights(O, I, 3 * O + I, integer=True)
        wf, _, _ = Pb.pack_ref(w, Op, Ip, first, [None] * 5)
        dw = Pb.forward_operand_as_wgrad(wf, Op, Ip, first)
        assert torch.equal(Pb.unpack_ref(dw, O, I, Op, Ip, first), w)
        # the kernel's own index arithmetic on distinct integers (padding included)
        n = Op * 128 if first else 3 * Op * 9 * Ip
        assert n < 2 ** 24
        dw = torch.arange(n, dtype=F32)
        i = torch.arange(O * I * 27)
        tap, q = i % 27, i // 27
        ch, o = q % I, q // I
        src = o * 128 + tap * I + ch if first else (((tap // 9) * Op + o) * 9 + tap % 9) * Ip + ch
        assert torch.equal(dw[src].view(O, I, 27), Pb.unpack_ref(dw, O, I, Op, Ip, first))


def test_clip27_restated():
    for B, T, H, W in Pb.CLIP_SHAPES:
        clips = torch.randint(-8, 9, (B, T, 3, H, W), generator=torch.Generator().manual_seed(B + T)).float()
        ref = Pb.clip27_ref(clips)
        assert bool((ref[..., 81:] == 0).all())
        # against unfold-free torch: a 3x3x3 convolution with a one-hot filter per K index
        x = clips.permute(0, 2, 1, 3, 4)
        eye = torch.zeros(81, 3, 3, 3, 3)
        for k in range(81):
            c, tap = k % 3, k // 3
            eye[k, c, tap // 9, (tap // 3) % 3, tap % 3] = 1.0
        got = F.conv3d(x, eye, padding=1).permute(2, 0, 3, 4, 1)
        assert torch.equal(got, ref[..., :81])
