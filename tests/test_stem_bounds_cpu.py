"""The float64 reference, the input classes and the bounds of tests/_stem_bounds.py, checked WITHOUT a GPU: the hand-written
reference against torch's own pooling / autograd in float64, a plain torch-f32 restatement of every stem-tail kernel (in the
kernel's place, with the kernel's grouping of the sums) inside every bound or, on the grid class, equal bit for bit, the
conditions the grid class promises, and the table of kernel paths each batch reaches.  So a failure of
tests/test_stem_tail_gpu.py is the kernel's, not the bound's or the reference's.  The restatements are also damaged on purpose
(a `>=` tie rule, a skipped tail, a tile dropped or read twice, a stale pooled row): each must be caught."""
import pytest
import torch
import torch.nn.functional as F

import _bounds as Bd
import _stem_bounds as Sb

H, W, P, C = Sb.H, Sb.W, Sb.P, Sb.C
F32, BF16 = torch.float32, torch.bfloat16
KINDS = ["grid", "random"]


@pytest.fixture(scope="module", autouse=True)
def _drop_references():
    yield
    Sb.clear_caches()


def _ok(name, got, ref, bound):
    r = Bd.ratio(got, ref, bound)
    assert r <= 1.0, (name, r)
    return r


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _codes_from_flat(idx):
    """torch's flat h * 112 + w indices [B][C][56][56] -> tap codes kh * 3 + kw, NHWC"""
    ph = torch.arange(P).view(1, 1, P, 1)
    pw = torch.arange(P).view(1, 1, 1, P)
    kh = idx // W - (2 * ph - 1)
    kw = idx % W - (2 * pw - 1)
    assert bool(((kh >= 0) & (kh < 3) & (kw >= 0) & (kw < 3)).all())
    return _nhwc(kh * 3 + kw).to(torch.uint8)


# ----------------------------------------------------------------------------------------------------------------------
# the reference is right
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_reference_equals_torch_float64(kind, B):
    c = Sb.case(kind, B)
    v = (Sb.to_nchw(c["y"]) * c["scale"].view(1, C, 1, 1) + c["shift"].view(1, C, 1, 1)).requires_grad_(True)
    out, idx = F.max_pool2d(F.relu(v), 3, 2, 1, return_indices=True)
    assert torch.equal(_nhwc(out.detach()), c["pooled"])
    assert torch.equal(_codes_from_flat(idx), c["code"])          # ATen keeps the first maximum in scan order
    ymax = Sb.to_nchw(c["y"]).flatten(2).gather(2, idx.flatten(2)).view_as(idx)
    assert torch.equal(_nhwc(ymax), c["ymax"])
    out.backward(Sb.to_nchw(c["d"]))
    assert torch.equal(_nhwc(v.grad), c["g"])                     # sums of <= 4 dyadic (grid) / bf16 values: exact in float64
    assert bool((c["gabs"] >= c["g"].abs()).all())


@pytest.mark.parametrize("B", [1, 3])
def test_reference_equals_autograd_with_consistent_statistics(B):
    y, d, gamma, beta, mean, invstd = Sb.consistent_case(B)
    yr = Sb.to_nchw(y).requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    out = F.max_pool2d(F.relu(F.batch_norm(yr, None, None, gr, br, True, 0.1, Bd.EPS)), 3, 2, 1)
    out.backward(Sb.to_nchw(d))
    scale = gamma * invstd
    shift = beta - mean * scale
    act, pooled, code, _ = Sb.forward_ref(y, scale, shift)
    g, _ = Sb.gather_ref(d, code, act)
    S = Sb.sums_ref(g, y, mean, invstd)
    M = B * H * W
    dy = Sb.dy_ref(g, y, mean, invstd, torch.stack([scale, S["s1"] / M, S["s2"] / M]))

    def rel(a, b):
        return float((a - b).abs().max() / b.abs().max())

    assert rel(_nhwc(out.detach()), pooled) <= 1e-12
    assert rel(dy, _nhwc(yr.grad)) <= 1e-12
    assert rel(S["s2"], gr.grad) <= 1e-12 and rel(S["s1"], br.grad) <= 1e-12


# ----------------------------------------------------------------------------------------------------------------------
# the input classes keep their promises
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", Sb.BATCHES)
def test_grid_class_conditions(B):
    c = Sb.case("grid", B)
    in_f32, in_bf16 = Sb.affine_exact(c["y"], c["scale"], c["shift"])
    assert in_f32 and in_bf16 and c["exact_bf16"]
    assert float(c["act"].max()) <= 18.0
    ties, positive, zero = Sb.grid_shares(c)
    print(f"  grid B={B}: positive ties {ties:.3f}, positive maximum {positive:.3f}, maximum 0 {zero:.3f}")
    assert ties >= 0.05 and positive >= 0.25 and zero >= 0.10
    assert set(c["scale"].tolist()) == set(Sb.SCALES)
    # all nine taps tie: the first VALID tap is recorded, in the absolute numbering kh * 3 + kw
    for ch, val in ((Sb.ZERO_POS, 0.5), (Sb.ZERO_NEG, 0.0)):
        k = c["code"][..., ch]
        assert bool((c["pooled"][..., ch] == val).all())
        assert bool((k[:, 1:, 1:] == Sb.FIRST_VALID_TAP["interior"]).all()) and bool((k[:, 0, 1:] == Sb.FIRST_VALID_TAP["top"]).all())
        assert bool((k[:, 1:, 0] == Sb.FIRST_VALID_TAP["left"]).all()) and bool((k[:, 0, 0] == Sb.FIRST_VALID_TAP["corner"]).all())
    assert bool((c["g"][..., Sb.ZERO_NEG] == 0).all()) and float(c["S"]["a1"][Sb.ZERO_NEG]) == 0.0
    assert float(c["S"]["a1"][Sb.ZERO_POS]) > 0
    # every tap code occurs, and cells with a maximum of 0 still record one (their gradient is masked, not lost track of)
    assert sorted(torch.unique(c["code"]).tolist()) == list(range(9))
    # the cancellation of the light sums kernel: channels that sit 5 standard deviations off zero and carry a gradient
    sd = c["y"].std((0, 1, 2), unbiased=False)
    far = ((c["y"].mean((0, 1, 2)).abs() / sd) >= 5.0) & (c["S"]["a1"] > 0)
    assert int(far.sum()) >= 4
    # mean a multiple of 1/8, invstd a power of two, d(pooled) a multiple of 1/8 within +-4
    assert torch.equal(torch.round(c["mean"] * 8), c["mean"] * 8)
    assert torch.equal(torch.frexp(c["invstd"])[0], torch.full((C,), 0.5, dtype=torch.float64))
    assert torch.equal(torch.round(c["d"] * 8), c["d"] * 8) and float(c["d"].abs().max()) <= 4.0


@pytest.mark.parametrize("B", Sb.BATCHES)
def test_random_class_conditions(B):
    c = Sb.case("random", B)
    in_f32, _ = Sb.affine_exact(c["y"], c["scale"], c["shift"])
    assert in_f32                                                 # for EVERY element: nothing is excluded later
    assert torch.equal(c["y"].to(BF16).double(), c["y"]) and float(c["y"].abs().max()) < 8.0
    m, sd = c["y"].mean((0, 1, 2)), c["y"].std((0, 1, 2), unbiased=False)
    assert float(m.abs().max()) > 4.0 and float(sd.min()) < 0.5 and float((m.abs() / sd).max()) > 5.0
    assert bool((c["gamma"] > 0).any()) and bool((c["gamma"] < 0).any())
    for k in ("mean", "invstd", "coef"):                          # f32 values, the same for kernel and reference
        assert torch.equal(c[k].float().double(), c[k])
    assert float((c["pooled"] > 0).double().mean()) >= 0.25


def test_paths_per_batch():
    at11, at3, at1 = Sb.paths(11), Sb.paths(3), Sb.paths(1)
    assert all(at11.values()), at11
    assert not any(at3.values()), at3                             # (why 11 is there)
    assert not any(at1.values()), at1
    r = Sb.tile_ranges(11)
    assert len(r) == 256 and r[0][0] == 0 and r[-1][1] == 616 and all(a[1] == b[0] for a, b in zip(r, r[1:]))
    assert r[23] == (55, 57) and r[162] == (389, 392) and 391 % 56 == 55
    assert Sb.wgrad_chain(11) == 3 * 224 + 256 and Sb.wgrad_chain(3) == 224 + 256
    assert (Sb.reduce_rows(3), Sb.reduce_rows(11), Sb.sums_rows(3), Sb.sums_rows(11)) == (1176, 2048, 294, 1024)
    assert min(b for b in range(1, 64) if all(Sb.paths(b).values())) == 11


# ----------------------------------------------------------------------------------------------------------------------
# f32 restatements of the kernels (their grouping of the sums included) stay inside the bounds
# ----------------------------------------------------------------------------------------------------------------------
def _seq_sum(t):
    """t[k][...] added in f32 one after the other, the way a thread's accumulator does"""
    acc = torch.zeros_like(t[0])
    for row in t:
        acc = acc + row
    return acc


def _by_thread(t, slots):
    """[items][64] -> [trips][slots][64]: item i belongs to thread slot i % slots (a grid-stride loop), zero padded"""
    n = t.shape[0]
    pad = (-n) % slots
    if pad:
        t = torch.cat([t, t.new_zeros((pad, C))])
    return t.view(-1, slots, C)


def _general_rows(g, y, mean, invstd, rows):
    """stem_bn_bwd_sums_kernel / stem_pool_bwd_kernel<T, 1>: 32 items x 8 channel groups per block and trip"""
    gf, yf = g.float().reshape(-1, C), y.float().reshape(-1, C)
    t2 = gf * (yf - mean.float()) * invstd.float()
    out = []
    for t in (gf, t2):
        per = _seq_sum(_by_thread(t, rows * 32))                  # [rows * 32][64]
        out.append(_seq_sum(per.view(rows, 32, C).transpose(0, 1)))
    return out


def _light_rows(d, ymax, scale, shift, mean, invstd, rows, skip_tail=False):
    """stem_bn_bwd_sums_light_kernel: 16 cells x 16 four-channel groups per block and trip, the correction by mean / invstd
    per thread, two butterfly steps over the four cells of a wave, four waves"""
    df, vf = d.float().reshape(-1, C), ymax.float().reshape(-1, C)
    on = vf * scale.float() + shift.float() > 0
    gf = torch.where(on, df, torch.zeros(()))
    slots = rows * 16
    a, b = _by_thread(gf, slots), _by_thread(gf * vf, slots)
    if skip_tail and a.shape[0] % 2 == 1:
        a, b = a[:-1], b[:-1]
    s1, s2 = _seq_sum(a), _seq_sum(b)
    s2 = (s2 - mean.float() * s1) * invstd.float()
    out = []
    for s in (s1, s2):
        w = s.view(rows, 4, 4, C)                                 # block, wave, cell of the wave
        w = (w[:, :, 0] + w[:, :, 1]) + (w[:, :, 2] + w[:, :, 3])
        out.append(((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3])
    return out


@pytest.mark.parametrize("B", Sb.BATCHES)
@pytest.mark.parametrize("kind", KINDS)
def test_sums_restated_in_f32(kind, B):
    c = Sb.case(kind, B)
    S, mean, invstd = c["S"], c["mean"], c["invstd"]
    on = c["ymax"] * c["scale"] + c["shift"] > 0
    gcell = torch.where(on, c["d"], torch.zeros((), dtype=torch.float64))
    forms = {
        "reduce": (_general_rows(c["g"], c["y"], mean, invstd, Sb.reduce_rows(B)), Sb.sums_bound(S, Sb.chain_reduce(B))),
        "sums": (_general_rows(gcell, c["ymax"], mean, invstd, Sb.sums_rows(B)), Sb.sums_bound(S, Sb.chain_sums(B))),
        "light": (_light_rows(c["d"], c["ymax"], c["scale"], c["shift"], mean, invstd, Sb.sums_rows(B)),
                  Sb.light_bound(S, Sb.chain_light(B), mean, invstd)),
    }
    for name, ((r1, r2), (b1, b2)) in forms.items():
        assert r1.dtype == F32 and r2.dtype == F32
        s1, s2 = r1.double().sum(0), r2.double().sum(0)
        if kind == "grid":                                        # exact: one dropped or doubled element shows
            assert torch.equal(s1, S["s1"]) and torch.equal(s2, S["s2"]), name
        else:
            print(f"  err/bound {name} B={B}: {_ok(name, s1, S['s1'], b1):.3f} {_ok(name, s2, S['s2'], b2):.3f}")
            assert bool((b1 <= 1e-3 * S["a1"] + 1e-30).all()) and bool((b2 <= 1e-2 * S["a2"] + 1e-30).all())   # not loose
    if kind == "grid" and Sb.paths(B)["light_tail"]:              # damage: the tail of the two-element loop skipped
        r1, r2 = _light_rows(c["d"], c["ymax"], c["scale"], c["shift"], mean, invstd, Sb.sums_rows(B), skip_tail=True)
        assert not torch.equal(r1.double().sum(0), S["s1"]) and not torch.equal(r2.double().sum(0), S["s2"])


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_gather_and_apply_restated_in_f32(kind, B, dt):
    c = Sb.case(kind, B)
    g32, _ = Sb.gather_ref(c["d"].float(), c["code"], c["act"])
    assert g32.dtype == F32
    gb = Sb.g_bound(c["g"], c["gabs"], dt)
    _ok("g", g32.to(dt), c["g"], gb)
    if kind == "grid":
        assert torch.equal(g32.to(dt).double(), c["g"])
    ca, cb, cc = c["coef"].float()
    yf, mu, inv = c["y"].float(), c["mean"].float(), c["invstd"].float()
    dy = ca * (g32 - cb - (yf - mu) * inv * cc)
    bound = Sb.dy_bound(c["dy"], c["g"], c["y"], c["mean"], c["invstd"], c["coef"], dt)
    print(f"  err/bound dy {kind} B={B}: {_ok('dy', dy.to(dt), c['dy'], bound):.3f}")
    assert bool((bound <= 2.0 ** -7 * c["dy"].abs() + 1e-3).all())
    # one pooled cell routed to the neighbouring position is outside the bound
    wrong = dy.clone()
    n, h, w, ch = [int(v) for v in torch.nonzero(c["g"].abs() >= 0.5)[0]]
    wrong[n, h, w, ch] = (ca * (0 - cb - (yf - mu) * inv * cc))[n, h, w, ch]
    if float(ca[ch].abs()) > 0:
        assert Bd.ratio(wrong.to(dt), c["dy"], bound) > 1.0


def _folded_dy(c, coef, g32):
    """the one-launch backward's gradient tile: k1 g - k3 y + k4 in f32, stored as bf16"""
    ca, cb, cc = coef.float()
    mu, inv = c["mean"].float(), c["invstd"].float()
    k3 = ca * inv * cc
    k4 = k3 * mu - ca * cb
    return (ca * g32 + (k4 - k3 * c["y"].float())).to(BF16)


@pytest.mark.parametrize("B", [1, 3])
def test_fused_backward_restated_in_f32(B):
    c = Sb.case("random", B)
    image, dw, bound = Sb.dense_wgrad(B)
    g32, _ = Sb.gather_ref(c["d"].float(), c["code"], c["act"])
    dyb = _folded_dy(c, c["coef"], g32)
    _ok("folded dy", dyb, c["dy"], Sb.dy_bound_folded(c["dy"], c["g"], c["y"], c["mean"], c["invstd"], c["coef"], BF16))
    got = torch.nn.grad.conv2d_weight(image.float(), (C, 3, 7, 7), Sb.to_nchw(dyb.float()), stride=2, padding=3)
    assert got.dtype == F32
    print(f"  err/bound dw B={B}: {_ok('dw', got, dw, bound):.3f}")
    lost = dyb.float().clone()
    lost[0, 2:4] = 0                                              # (one tile of 2 x 112 positions dropped)
    got = torch.nn.grad.conv2d_weight(image.float(), (C, 3, 7, 7), Sb.to_nchw(lost), stride=2, padding=3)
    print(f"  err/bound dw with one tile dropped B={B}: {Bd.ratio(got, dw, bound):.3f}   (the sparse probe is the test for that)")


@pytest.mark.parametrize("B", Sb.BATCHES)
def test_sparse_probe(B):
    c = Sb.case("grid", B)
    d, coef, image, dw, cells = Sb.sparse_probe(B)
    assert len(cells) == B * 56 and int((d != 0).sum()) == B * 56
    assert len({(n, rp) for n, rp, *_ in cells}) == B * 56
    assert len({b for _, _, _, b, _, _ in cells}) >= 40 and len({ch for *_, ch, _ in cells}) >= 8
    assert all(float(c["scale"][ch]) > 0 and float(c["pooled"][n, row, b, ch]) > 0 for n, _, row, b, ch, _ in cells)
    assert all((row == rp + 1 and k < 3) or (row == rp and k >= 3) for _, rp, row, _, _, k in cells)
    assert torch.equal(torch.round(image * 8), image * 8) and float(image.abs().max()) <= 4.0
    # exact in f32 in any order: sum |terms| far below 2^24 units of 1/16
    g, _ = Sb.gather_ref(d, c["code"], c["act"])
    assert float(Sb.wgrad_ref(image.abs(), g.abs()).max()) * 16 < 2.0 ** 24
    dyb = _folded_dy(c, coef, g.float())
    assert torch.equal(dyb.double(), g)                           # coef (1, 0, 0): the gradient tile IS g
    got = torch.nn.grad.conv2d_weight(image.float(), (C, 3, 7, 7), Sb.to_nchw(dyb.float()), stride=2, padding=3)
    assert torch.equal(got.double(), dw)
    assert float((dw != 0).double().mean()) > 0.2

    def damaged(gd):
        return torch.nn.grad.conv2d_weight(image.float(), (C, 3, 7, 7), Sb.to_nchw(gd.float()), stride=2, padding=3).double()

    # every single tile matters: dropped, or taken from the tile before it (the wrong LDS buffer)
    for n, rp in ((0, 0), (B - 1, 55), (B // 2, 54)) + (((6, 53), (0, 55), (1, 0)) if B == 11 else ()):
        gd = g.clone()
        gd[n, 2 * rp:2 * rp + 2] = 0
        assert not torch.equal(damaged(gd), dw), (n, rp)
        t = n * 56 + rp
        if t > 0:
            gd[n, 2 * rp:2 * rp + 2] = g[(t - 1) // 56, 2 * ((t - 1) % 56):2 * ((t - 1) % 56) + 2]
            assert not torch.equal(damaged(gd), dw), (n, rp)
    # the rp == 55 tile reading a stale copy of pooled row 54 as its second row: row 54's cell (a tap of window row 0) lands
    # four conv rows further down as well, where the activation is positive by construction
    for n in range(B):
        (_, _, row, b, ch, k), = [x for x in cells if x[0] == n and x[1] == 53]
        assert row == 54 and k < 3
        hh, ww = 2 * 56 - 1, 2 * b - 1 + k
        assert float(c["act"][n, hh, ww, ch]) > 0
        gd = g.clone()
        gd[n, hh, ww, ch] += d[n, row, b, ch]
        assert not torch.equal(damaged(gd), dw)


# ----------------------------------------------------------------------------------------------------------------------
# the tie rule is observable
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_last_maximum_wins_is_caught(kind):
    c = Sb.case(kind, 1)
    _, pooled, code, ymax = Sb.forward_ref(c["y"], c["scale"], c["shift"], wins=torch.ge)
    assert torch.equal(pooled, c["pooled"])                       # the maximum is the same,
    assert not torch.equal(code, c["code"])                       # the recorded tap is not
    if kind == "grid":
        assert float((code != c["code"]).double().mean()) > 0.05
