"""The integer-grid cases of tests/_exact.py without a GPU: every table row meets its conditions on the float64 reference
alone; a torch-f32 computation in the kernel's place (two memory formats: two summation orders) passes the same torch.equal
checks tests/test_conv_exact_gpu.py applies to the HIP kernels; and each listed kind of damage to that stand-in is caught."""
import pytest
import torch
import torch.nn.functional as F

import _exact as E
from _exact import BF, F32


def _formats(x):
    fmt = torch.channels_last if x.dim() == 4 else torch.channels_last_3d
    return [x.contiguous(), x.contiguous(memory_format=fmt)]


def _conv32(x, w, s, p):
    """f32 convolution of f64-held integers, once per memory format of the input"""
    return [E._conv(xf, w.float(), s, p) for xf in _formats(x.float())]


FWD, FWD_IDS = E.expand(E.FWD_ROWS)


@pytest.mark.parametrize("row,dt", FWD, ids=FWD_IDS)
def test_forward_rows(row, dt):
    c = E.fwd_data(row)
    E.fwd_conditions(c, dt)
    mode = row["mode"]
    _, _, _, _, _, s, p = row["cfg"]
    for raw in _conv32(c["x"], c["w"], s, p):
        assert torch.equal(raw.double(), c["raw"])                       # f32 in any order == float64
        assert E.same(raw.to(dt), c["raw"], dt)
        act = F.relu(raw * E.bcast(c["scale"].float(), raw) + E.bcast(c["shift"].float(), raw) + c["res"].float())
        assert E.same(act.to(dt), c["act"], dt)
        if mode == "A":
            rows = raw.movedim(1, -1).reshape(-1, raw.shape[1])              # [M][C] as the kernels see it
            part = torch.stack([torch.stack([t.sum(0), (t * t).sum(0)]) for t in rows.split(128)])
            assert E.stats_equal(part, c["raw"])


S2, S2_IDS = E.expand(E.S2_ROWS)


@pytest.mark.parametrize("row,dt", S2, ids=S2_IDS)
def test_stride2_pair_rows(row, dt):
    c = E.s2_data(row)
    E.s2_conditions(c, dt)
    mode = row["mode"]
    for raw, rawd in zip(_conv32(c["x"], c["w"], 2, 1), _conv32(c["x"], c["wd"], 2, 0)):
        assert E.same(raw.to(dt), c["raw"], dt) and E.same(rawd.to(dt), c["rawd"], dt)
        act = F.relu(raw * E.bcast(c["sc"].float(), raw) + E.bcast(c["sh"].float(), raw))
        assert E.same(act.to(dt), c["act"], dt)
        assert E.same((rawd * E.bcast(c["sd"].float(), raw) + E.bcast(c["shd"].float(), raw)).to(dt), c["pred"], dt)


@pytest.mark.parametrize("row", E.STEM_ROWS, ids=E.ids(E.STEM_ROWS))
def test_stem_rows(row):
    c = E.stem_data(row)
    mode = row["mode"]
    E.conditions(c["raw"], c["araw"], BF, mode, w=c["w"], acts=[c["x"]], stats=(mode == "A"))
    E.conditions(c["pre"], c["apre"], BF, mode, zeros=False)
    for raw in _conv32(c["x"], c["w"], 2, 3):
        assert E.same(raw.to(BF), c["raw"], BF)
        act = F.relu(raw * E.bcast(c["scale"].float(), raw) + E.bcast(c["shift"].float(), raw)).to(BF)
        assert E.same(act, c["act"], BF)
        assert E.same(F.max_pool2d(act.float(), 3, 2, 1).to(BF), c["pooled"], BF)


DG, DG_IDS = E.expand(E.DGRAD_ROWS + E.S2D_ROWS)


@pytest.mark.parametrize("row,dt", DG, ids=DG_IDS)
def test_data_gradient_rows(row, dt):
    c = E.s2d_data(row) if "form" in row else E.dgrad_data(row)
    E.dgrad_conditions(c, dt)
    B, Cin, Cout, H, k, s, p = row["cfg"]
    for dyf in _formats(c["dy"].float()):
        dx = torch.nn.grad.conv2d_input((B, Cin, H, H), c["w"].float(), dyf, s, p)
        if "wd" in c:
            dx = dx + torch.nn.grad.conv2d_input((B, Cin, H, H), c["wd"].float(), c["dyd"].float(), 2, 0)
        out = torch.where(c["act"].to(dt).float() > 0, dx + c["other"].float(), torch.zeros(()))
        assert E.same(out.to(dt), c["out"], dt)


WG, WG_IDS = E.expand(E.WGRAD_ROWS)


@pytest.mark.parametrize("row,dt", WG, ids=WG_IDS)
def test_weight_gradient_rows(row, dt):
    c = E.wgrad_data(row)
    E.wgrad_conditions(c)
    _, _, _, _, _, s, p = row["cfg"]
    for xf in _formats(c["x"].float()):
        dw = torch.nn.grad.conv2d_weight(xf, tuple(c["dw"].shape), c["dy"].float(), s, p)
        assert E.same(dw, c["dw"], F32)


@pytest.mark.parametrize("row", E.LWGRAD_ROWS, ids=E.ids(E.LWGRAD_ROWS))
def test_linear_weight_gradient_rows(row):
    c = E.lwgrad_data(row)
    E.lwgrad_conditions(c)
    assert E.same(c["dy"].float().t() @ c["x"].float(), c["dw"], F32)
    assert E.same((c["x"].float().t() @ c["dy"].float()).t().contiguous(), c["dw"], F32)


@pytest.mark.parametrize("row", E.LINEAR_ROWS, ids=E.ids(E.LINEAR_ROWS))
def test_linear_rows(row):
    c = E.gemm_data(row)
    E.gemm_conditions(c, BF)
    b = c["bias"].float() if c["bias"] is not None else None
    for y in (F.linear(c["x"].float(), c["w"].float(), b), (c["w"].float() @ c["x"].float().t()).t() + (b if b is not None else 0)):
        y = F.relu(y) if row["relu"] else y
        assert E.same(y.to(BF), c["out"], BF)


SD, SD_IDS = E.expand(E.STEMD_ROWS)


@pytest.mark.parametrize("row,dt", SD, ids=SD_IDS)
def test_stem_data_gradient_rows(row, dt):
    """qt_stem_dgrad writes the f32 image gradient whatever the type of the gradient map"""
    c = E.dgrad_data(row)
    E.dgrad_conditions(c, F32)
    for dyf in _formats(c["dy"].float()):
        assert E.same(torch.nn.grad.conv2d_input((row["cfg"][0], 3, 224, 224), c["w"].float(), dyf, 2, 3), c["dx"], F32)


SW, SW_IDS = E.expand(E.STEMW_ROWS)


@pytest.mark.parametrize("row,dt", SW, ids=SW_IDS)
def test_stem_weight_gradient_rows(row, dt):
    c = E.wgrad_data(row)
    E.wgrad_conditions(c)
    for xf in _formats(c["x"].float()):
        assert E.same(torch.nn.grad.conv2d_weight(xf, (64, 3, 7, 7), c["dy"].float(), 2, 3), c["dw"], F32)


C3 = [(r, dt, ci, co) for rows, ci, co in ((E.C3F_ROWS, 3, 32), (E.C32_ROWS, 32, 64)) for r in rows for dt in r["dts"]]
C3_IDS = [f"{r['name']}-{'bf16' if dt == BF else 'f32'}" for r, dt, _, _ in C3]


@pytest.mark.parametrize("row,dt,cin,cout", C3, ids=C3_IDS)
def test_conv3d_rows(row, dt, cin, cout):
    c = E.c3_data(row, cin, cout)
    first = cin == 3
    if "fwd" in row["only"]:
        E.c3_conditions(c, dt, "fwd")
        for raw in _conv32(c["x"], c["w"], 1, 1):
            assert E.same(raw.to(dt), c["raw"], dt)
            act = F.relu(raw * E.bcast(c["scale"].float(), raw) + E.bcast(c["shift"].float(), raw)).to(dt)
            assert E.same(act, c["act"], dt)
            assert E.same(F.max_pool3d(act.float(), (1, 2, 2)).to(dt), c["pooled"], dt)
    if "dgrad" in row["only"]:
        ddt = F32 if first else dt          # the first convolution's data gradient is the f32 clip gradient
        E.c3_conditions(c, ddt, "dgrad")
        for dyf in _formats(c["dyf"].float()):
            assert E.same(torch.nn.grad.conv3d_input(c["x1"].shape, c["wg"].float(), dyf, 1, 1).to(ddt), c["dx"], ddt)
    if "wgrad" in row["only"]:
        E.c3_conditions(c, F32, "wgrad")
        for xf in _formats(c["x1"].float()):
            assert E.same(torch.nn.grad.conv3d_weight(xf, c["w"].shape, c["dy"].float(), 1, 1), c["dw"], F32)


FUSED = [(r, cp) for r in E.C3F_ROWS if "fused" in r["only"] for cp in (32, 64)]


def _fused_dy32(f, gate_ge=False):
    """the kernel's own form in f32: dy = ka g + kb - y kc with ka = a, kc = a invstd c, kb = a (mean invstd c - b), as bf16"""
    y = f["y"].float()
    a, b, c = (E.bcast(f["coef"][j, :32].float(), y) for j in range(3))
    mu, inv = E.bcast(f["mean"].float(), y), E.bcast(f["invstd"].float(), y)
    pre = y * E.bcast(f["scale"].float(), y) + E.bcast(f["shift"].float(), y)
    up = f["dout"][:, :32].float().repeat_interleave(2, 3).repeat_interleave(2, 4)
    on = (pre >= 0) if gate_ge else (pre > 0)
    g = torch.where(f["gate"] & on, up, torch.zeros(()))
    return (a * g + a * (mu * inv * c - b) - y * (a * inv * c)).to(BF)


@pytest.mark.parametrize("row,cp", FUSED, ids=[f"{r['name']}-cp{cp}" for r, cp in FUSED])
def test_fused_first_conv3d_weight_gradient_rows(row, cp):
    f = E.c3_fused_data(E.c3_data(row, 3, 32), cp)
    E.c3_fused_conditions(f)
    dy = _fused_dy32(f)
    assert E.same(dy, f["dy"], BF)
    for xf in _formats(f["x1"].float()):
        assert E.same(torch.nn.grad.conv3d_weight(xf, f["w"].shape, dy.float(), 1, 1), f["dw"], F32)
    # a gate that lets y * scale + shift == 0 through is caught
    bad = _fused_dy32(f, gate_ge=True)
    assert not E.same(torch.nn.grad.conv3d_weight(f["x1"].float(), f["w"].shape, bad.float(), 1, 1), f["dw"], F32)


# ----------------------------------------------------------------------------------------------------------------------
# damage: each of these must make the comparison fail
# ----------------------------------------------------------------------------------------------------------------------
def _row(rows, name):
    return next(r for r in rows if r["name"] == name)


DAMAGE_ROWS = [_row(E.FWD_ROWS, "generic_3x3"), _row(E.FWD_ROWS, "ring_b1"), _row(E.FWD_ROWS, "generic_m49")]


@pytest.mark.parametrize("row", DAMAGE_ROWS, ids=E.ids(DAMAGE_ROWS))
def test_a_skipped_tap_a_dropped_k_element_and_a_missing_tile_are_caught(row):
    c = E.fwd_data(row)
    dt = BF
    _, _, Cout, _, k, s, p = row["cfg"]
    x, w = c["x"].float(), c["w"].float()
    raw = F.conv2d(x, w, None, s, p)
    assert E.same(raw.to(dt), c["raw"], dt)
    # the centre tap skipped at the first output column of one channel
    ch = Cout // 3
    only = torch.zeros_like(w)
    only[ch, :, k // 2, k // 2] = w[ch, :, k // 2, k // 2]
    hurt = raw.clone()
    hurt[:, ch, :, 0] -= F.conv2d(x, only, None, s, p)[:, ch, :, 0]
    assert not E.same(hurt.to(dt), c["raw"], dt)
    assert E.first_mismatch(hurt.to(dt), c["raw"], dt)[0][1] == ch
    # one k element dropped
    o, i, a, b = (int(v) for v in (w != 0).nonzero()[len((w != 0).nonzero()) // 2])
    w2 = w.clone()
    w2[o, i, a, b] = 0
    assert not E.same(F.conv2d(x, w2, None, s, p).to(dt), c["raw"], dt)
    # the last (ragged) 128-row tile left out of the statistics
    rows = raw.movedim(1, -1).reshape(-1, Cout)
    tiles = rows.split(128)
    part = torch.stack([torch.stack([t.sum(0), (t * t).sum(0)]) for t in tiles])
    assert E.stats_equal(part, c["raw"])
    assert tiles[-1].shape[0] <= 128 and not E.stats_equal(part[:-1], c["raw"])


# ----------------------------------------------------------------------------------------------------------------------
# damage to the walk of a persistent kernel: a stand-in with a capped grid (workgroup k takes items k, k + grid, ...)
# ----------------------------------------------------------------------------------------------------------------------
FAULTS = ("stale_slab", "round_skipped", "last_item_only", "frame_slot_left")


def _slabs(x, R):
    """[B][C][T][H][W] -> the input of every (clip, R-row slab) item with its row halo: [items][C][T][R + 2][W]"""
    B, C, T, H, W = x.shape
    u = F.pad(x, (0, 0, 1, 1)).unfold(3, R + 2, R)                  # [B][C][T][H / R][W][R + 2]
    return u.permute(0, 3, 1, 2, 5, 4).reshape(B * (H // R), C, T, R + 2, W)


def _walked_conv3d(x, w, R, cap, fault=None, dy=None):
    """3x3x3 / pad 1 convolution of x [B][C][T][H][W] (f32) the way the slab kernels walk it: item = (clip, R output rows), its
    input the frame slabs with a row halo and a zero frame on either side of the clip; workgroup k of min(items, cap) takes
    items k, k + grid, ...  Returns (y [B][O][T][H][W], statistics rows [grid][2][O], the weight gradient for `dy` or None).
    fault (each is invisible when every workgroup has one item):
      stale_slab       a workgroup's second item is computed from its first item's slabs (ring not refilled / stale prefetch)
      round_skipped    the loop runs the full rounds only: the items of the last, partial round are never computed
      last_item_only   a workgroup's statistics row and partial filter hold its last item alone (overwritten, not accumulated)
      frame_slot_left  the frame before the clip (t - 1 at t = 0) of a later item is the previous item's last frame slab, not zeros"""
    B, _, T, H, W = x.shape
    O = w.shape[0]
    xi = _slabs(x, R)
    items = xi.shape[0]
    grid, wg, trip = E.walk_items(items, cap)
    i = torch.arange(items)
    if fault == "stale_slab":
        xi = xi[torch.where(trip == 1, i - grid, i)]
    xp = F.pad(xi, (0, 0, 0, 0, 1, 1))                               # a zero frame before and after the clip
    if fault == "frame_slot_left":
        later = trip >= 1
        xp[later, :, 0] = xi[i[later] - grid, :, T - 1]
    yi = F.conv3d(xp, w, None, 1, (0, 0, 1))                         # [items][O][T][R][W]
    done = i < (items // grid) * grid if fault == "round_skipped" else torch.ones(items, dtype=torch.bool)
    yi = yi * done.view(-1, 1, 1, 1, 1)                              # (what a skipped item leaves behind: anything but the result)
    y = yi.view(B, H // R, O, T, R, W).permute(0, 2, 3, 1, 4, 5).reshape(B, O, T, H, W)
    counted = done & (i + grid >= items) if fault == "last_item_only" else done
    per_item = torch.stack([yi.sum((2, 3, 4)), (yi * yi).sum((2, 3, 4))], 1) * counted.view(-1, 1, 1)
    part = torch.zeros(grid, 2, O).index_add_(0, wg, per_item)
    dw = None
    if dy is not None:
        dyi = dy.view(B, O, T, H // R, R, W).permute(0, 3, 1, 2, 4, 5).reshape(items, O, T, R, W)
        dw = torch.nn.grad.conv3d_weight(xp[counted], w.shape, dyi[counted], 1, (0, 0, 1))
    return y, part, dw


def _walked_stem_dgrad(dy, w, ty, cap, fault=None):
    """conv1's data gradient the way stem_dgrad.hip walks it: item = a tile of ty x 16 blocks of 2 x 2 image pixels, its input
    the dy rows and columns of the tile with a halo of 1 before and 2 after; the same capped grid and the faults of
    _walked_conv3d that a kernel without frames and partial rows can have"""
    B = dy.shape[0]
    u = F.pad(dy, (1, 2, 1, 2)).unfold(2, ty + 3, ty).unfold(3, 19, 16)      # [B][64][112 / ty][7][ty + 3][19]
    ny = 112 // ty
    di = u.permute(0, 2, 3, 1, 4, 5).reshape(B * ny * 7, 64, ty + 3, 19)
    items = di.shape[0]
    grid, wg, trip = E.walk_items(items, cap)
    i = torch.arange(items)
    if fault == "stale_slab":
        di = di[torch.where(trip == 1, i - grid, i)]
    # halo pixel j of a tile is conv1 output y0 - 1 + j: it reaches image row 2 (y0 - 1 + j) + k - 3, the transposed
    # convolution's row 2 j + k: the tile's image rows 2 y0 .. 2 y0 + 2 ty - 1 are its rows 5 .. 5 + 2 ty - 1
    full = F.conv_transpose2d(di, w, None, 2)
    out = full[:, :, 5:5 + 2 * ty, 5:5 + 32]
    if fault == "round_skipped":
        out = out * (i < (items // grid) * grid).view(-1, 1, 1, 1)
    return out.reshape(B, ny, 7, 3, 2 * ty, 32).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, 224, 224)


def _caught(ok, walking, what):
    """a fault shows exactly where workgroups take more than one item"""
    assert ok == (not walking), (what, "caught" if not ok else "not caught", "walking" if walking else "one item per workgroup")


WALK3D = [(r, 3, 32, 4, 512) for r in E.C3F_ROWS if r.get("walk")] + [(r, 32, 64, 2, 256) for r in E.C32_ROWS if r.get("walk")]


@pytest.mark.parametrize("row,cin,cout,R,cap", WALK3D, ids=[r["name"] for r, *_ in WALK3D])
def test_a_stale_slab_a_skipped_round_an_overwritten_partial_and_a_left_frame_slot_are_caught(row, cin, cout, R, cap):
    """R, cap: output rows per item and the grid cap of the kernels of the row (conv3d_first.hip: 4 rows, 2 x 256 CUs;
    conv3d_slab.hip: 2 rows, 256 CUs).  Every fault fails the GPU test's comparisons on the walk rows at that cap, and none
    does on the same data when the grid has a workgroup per item -- the state of every earlier row."""
    dt = BF
    c = E.c3_data(row, cin, cout)
    B, T, H, W = row["cfg"]
    items = B * (H // R)
    assert items >= row["walk"] * cap + 1
    x, w = c["x"].float(), c["w"].float()
    wflip = c["wg"].float().transpose(0, 1).flip(2, 3, 4).contiguous()        # conv3d_input(dy, wg) = conv3d(dy, wflip)
    ddt = F32 if cin == 3 else dt
    grads = [("wgrad", c["x1"].float(), c["dy"].float(), c["dw"])]
    if "fused" in row["only"]:
        f = E.c3_fused_data(c, 32)
        grads.append(("fused", f["x1"].float(), f["dy"].float(), f["dw"]))
    for walking in (True, False):
        g = cap if walking else items
        y, part, _ = _walked_conv3d(x, w, R, g)
        assert part.shape[0] == min(items, g)
        assert E.same(y.to(dt), c["raw"], dt) and E.stats_equal(part, c["raw"])
        assert E.same(_walked_conv3d(c["dyf"].float(), wflip, R, g)[0].to(ddt), c["dx"], ddt)
        for _, x1, dy, dw in grads:
            assert E.same(_walked_conv3d(x1, w, R, g, dy=dy)[2], dw, F32)
        for fault in FAULTS:
            y, part, _ = _walked_conv3d(x, w, R, g, fault)
            if fault != "last_item_only":                                  # (that one leaves the map alone)
                _caught(E.same(y.to(dt), c["raw"], dt), walking, (fault, "forward"))
                dx = _walked_conv3d(c["dyf"].float(), wflip, R, g, fault)[0]
                _caught(E.same(dx.to(ddt), c["dx"], ddt), walking, (fault, "data gradient"))
            if fault in ("round_skipped", "last_item_only"):
                _caught(E.stats_equal(part, c["raw"]), walking, (fault, "statistics"))
            for name, x1, dy, dw in grads:
                _caught(E.same(_walked_conv3d(x1, w, R, g, fault, dy=dy)[2], dw, F32), walking, (fault, name))


WALK_STEM, WALK_STEM_IDS = E.expand([r for r in E.STEMD_ROWS if r.get("walk")])


@pytest.mark.parametrize("row,dt", WALK_STEM, ids=WALK_STEM_IDS)
def test_a_stale_tile_prefetch_and_a_skipped_round_of_the_stem_data_gradient_are_caught(row, dt):
    """stem_dgrad.hip: tiles of 16 x 16 blocks (bf16) / 8 x 16 blocks (f32) on a grid of at most 256 workgroups, the next tile's
    rows loaded into registers under the current tile's MFMAs"""
    c = E.dgrad_data(row)
    B = row["cfg"][0]
    ty, cap = (16 if dt == BF else 8), 256
    items = B * (112 // ty) * 7
    assert items >= row["walk"] * cap + 1
    dy, w = c["dy"].float(), c["w"].float()
    for walking in (True, False):
        g = cap if walking else items
        assert E.same(_walked_stem_dgrad(dy, w, ty, g), c["dx"], F32)
        for fault in ("stale_slab", "round_skipped"):
            _caught(E.same(_walked_stem_dgrad(dy, w, ty, g, fault), c["dx"], F32), walking, fault)


# ----------------------------------------------------------------------------------------------------------------------
# damage to the walk of the stem and layer-1 ring kernels: a capped grid of CONTIGUOUS shares (E.share_items)
# ----------------------------------------------------------------------------------------------------------------------
def test_the_walk_rows_reach_what_they_are_there_for():
    """the recorded facts are those of the split, and 39 / 21 are the smallest batches at which conv_stem_kernel (512
    workgroups) / the fused stem (256) reach all of E.stem_walk_reaches()"""
    rows = {r["name"]: r for r in E.FWD_ROWS + E.STEM_ROWS + E.STEMW_ROWS}
    for name, (per, cap, want) in E.WALKS.items():
        B, H = rows[name]["cfg"][0], rows[name]["cfg"][3]
        items = per * B if per else E.ring_tiles(B, H)
        f = E.share_facts(items, cap, per)
        assert {k: f[k] for k in want} == want, (name, f)
        assert f["least"] >= rows[name]["walk"] and items >= rows[name]["walk"] * f["grid"] + 1
    for cap, smallest in ((512, 39), (256, 21)):
        assert [B for B in range(1, smallest + 1) if E.stem_walk_reaches(E.share_facts(28 * B, cap, 28))] == [smallest]
    # the ring kernel's window: a share of n tiles reads window indices up to 256 n - 1 + 2 * 58 + 2.  Two tiles stay inside
    # the 640 rows; the fifth tile of a share reads past 1280, the second wrap
    last_index = lambda n: 256 * n - 1 + 2 * 58 + 2
    assert last_index(2) == 629 < 640 <= last_index(3) and last_index(E.WALKS["ring_walk"][2]["most"]) >= 1280


def _share(items, cap):
    grid, wg, trip = E.share_items(items, cap)
    return grid, wg, trip, torch.bincount(wg, minlength=grid)[wg]      # (.. and the length of the share an item lies in)


def _stem_slabs(x, top, rows, step):
    """[B][3][224][224] -> per tile the `rows` packed input rows from packed row step * k - top on: [B * 28 or 56][3][rows][230]"""
    u = F.pad(x, (3, 3, 3 + top, 3)).unfold(2, rows, step)               # [B][3][tiles][230][rows]
    return u.permute(0, 2, 1, 4, 3).reshape(-1, 3, rows, 230)


def _stale(slabs, trip):
    """a workgroup's third tile is computed from the input rows of its first: the buffer was reused without a refill"""
    i = torch.arange(slabs.shape[0])
    return slabs[torch.where(trip == 2, i - 2, i)]


def _walked_stem_conv(x, w, cap, fault=None):
    """conv1 the way conv_stem_kernel walks it: tile = (image, 4 output rows) from 13 packed rows, contiguous shares on
    min(tiles, cap) workgroups, one statistics row per workgroup.  Returns (y [B][64][112][112], rows [grid][2][64])"""
    B = x.shape[0]
    xi = _stem_slabs(x, 0, 13, 8)
    grid, wg, trip, n = _share(xi.shape[0], cap)
    if fault == "stale_input":
        xi = _stale(xi, trip)
    yi = F.conv2d(xi, w, None, 2)                                        # [tiles][64][4][112]
    counted = trip == n - 1 if fault == "last_item_only" else torch.ones_like(trip, dtype=torch.bool)
    per_item = torch.stack([yi.sum((2, 3)), (yi * yi).sum((2, 3))], 1) * counted.view(-1, 1, 1)
    part = torch.zeros(grid, 2, 64).index_add_(0, wg, per_item)
    return yi.view(B, 28, 64, 4, 112).permute(0, 2, 1, 3, 4).reshape(B, 64, 112, 112), part


def _walked_stem_pool(x, w, scale, shift, cap, fault=None):
    """the fused eval stem the way conv_stem_pool_kernel walks it: tile = (image, k), conv rows 4k - 1 .. 4k + 3 from 15 packed
    rows as a bf16 ReLU tile of five rows, two pooled rows from it; conv row -1 of a first tile (k = 0) is not computed and
    not read (0 never beats a ReLU output).  fault top_row_left: a first tile that is not its workgroup's first reads the row
    the previous tile left in that place"""
    B = x.shape[0]
    xi = _stem_slabs(x, 2, 15, 8)
    grid, wg, trip, n = _share(xi.shape[0], cap)
    if fault == "stale_input":
        xi = _stale(xi, trip)
    raw = F.conv2d(xi, w, None, 2)                                       # [tiles][64][5][112]
    tile = F.relu(raw * E.bcast(scale, raw) + E.bcast(shift, raw)).to(BF).float()
    first = torch.arange(xi.shape[0]) % 28 == 0
    top = torch.zeros_like(tile[:, :, 0])
    if fault == "top_row_left":
        later = first & (trip >= 1)
        top[later] = tile[later.nonzero().flatten() - 1, :, 0]
    tile[first, :, 0] = top[first]
    pooled = F.max_pool2d(F.pad(tile, (1, 0)), 3, 2)                     # [tiles][64][2][56]
    return pooled.view(B, 28, 64, 2, 56).permute(0, 2, 1, 3, 4).reshape(B, 64, 56, 56)


@pytest.mark.parametrize("row", E.STEM_ROWS, ids=E.ids(E.STEM_ROWS))
def test_a_stale_input_buffer_a_left_top_row_and_overwritten_statistics_of_the_stem_are_caught(row):
    """Every fault fails the GPU test's comparisons on the walk rows and none does on the one-image rows, where a workgroup
    has one tile: those rows could not see them"""
    c = E.stem_data(row)
    only = row.get("only", ("conv", "pool"))
    walking = bool(row.get("walk"))
    x, w, sc, sh = (c[n].float() for n in ("x", "w", "scale", "shift"))
    if "conv" in only:
        y, part = _walked_stem_conv(x, w, 512)
        assert E.same(y.to(BF), c["raw"], BF)
        assert row["mode"] == "B" or E.stats_equal(part, c["raw"])
        y, _ = _walked_stem_conv(x, w, 512, "stale_input")
        _caught(E.same(y.to(BF), c["raw"], BF), walking, "stale_input")
        if row["mode"] == "A":
            _, part = _walked_stem_conv(x, w, 512, "last_item_only")
            _caught(E.stats_equal(part, c["raw"]), walking, "last_item_only")
    if "pool" in only:
        assert E.same(_walked_stem_pool(x, w, sc, sh, 256).to(BF), c["pooled"], BF)
        for fault in ("stale_input", "top_row_left"):
            _caught(E.same(_walked_stem_pool(x, w, sc, sh, 256, fault).to(BF), c["pooled"], BF), walking, fault)


@pytest.mark.parametrize("row", E.STEMW_ROWS, ids=E.ids(E.STEMW_ROWS))
def test_a_stale_input_buffer_and_an_overwritten_partial_filter_of_the_stem_weight_gradient_are_caught(row):
    """stem_wgrad_rows_kernel: tile = (image, 2 rows of dy) with 9 packed input rows, contiguous shares on min(tiles, 256)
    workgroups, a partial filter per workgroup summed over its share"""
    c = E.wgrad_data(row)
    B = row["cfg"][0]
    walking = bool(row.get("walk"))
    xi = _stem_slabs(c["x"].float(), 0, 9, 4)
    dyi = c["dy"].float().view(B, 64, 56, 2, 112).permute(0, 2, 1, 3, 4).reshape(B * 56, 64, 2, 112)
    grid, wg, trip, n = _share(B * 56, 256)
    assert (n.min() >= 2 and n.max() >= 3) == walking
    assert bool((dyi != 0).flatten(1).any(1).all())                      # every tile holds a non-zero dy
    every = torch.ones_like(trip, dtype=torch.bool)
    for fault, xs, counted in ((None, xi, every), ("stale_input", _stale(xi, trip), every), ("last_item_only", xi, trip == n - 1)):
        dw = torch.nn.grad.conv2d_weight(xs[counted], (64, 3, 7, 7), dyi[counted], 2, 0)
        if fault is None:
            assert E.same(dw, c["dw"], F32)
        else:
            _caught(E.same(dw, c["dw"], F32), walking, fault)


def _walked_ring(x, w, cap, fault=None):
    """3x3 / pad 1 convolution of x [B][C][H][H] (f32) the way conv_l1_ring_kernel walks it: the padded grid [B][H + 2][H + 2]
    as one sequence of positions, tiles of 256 of them in contiguous shares on min(tiles, cap) workgroups; a workgroup
    reads position q + (kh - 1)(H + 2) + (kw - 1) at window index u = (q - first position of its share) + kh (H + 2) + kw,
    kept in ring row u mod 640; a lane reads its four 16-row fragments of a tap at rr0, rr0 + 16, rr0 + 32, rr0 + 48 with
    rr0 = (256 k + 64 wm + frow + shift) mod 640, so rows 640 .. 687 are a mirror of rows 0 .. 47.
    Returns (y [B][O][H][H], statistics rows [grid][2][O]).  fault:
      unfolded_row     window indices >= 640 are not folded: the data of the position 640 earlier is read
      mirror_left      the mirror keeps the first window: a read through it gets window index u mod 640 of the share's start
      last_item_only   the workgroup's statistics row holds its last tile alone"""
    B, C, H, _ = x.shape
    O = w.shape[0]
    PW = H + 2
    Q, M = B * PW * PW, PW + 1
    tiles = E.ring_tiles(B, H)
    grid, wg, trip, n = _share(tiles, cap)
    src = torch.zeros(M + tiles * 256 + M, C)
    src[M:M + Q] = F.pad(x, (1, 1, 1, 1)).permute(0, 2, 3, 1).reshape(Q, C)
    i = torch.arange(256).view(1, -1)
    q = torch.arange(tiles).view(-1, 1) * 256 + i
    start = (torch.arange(tiles) - trip).view(-1, 1) * 256              # first position of the share a tile lies in
    u0 = trip.view(-1, 1) * 256 + i
    j16 = (i % 64) // 16 * 16
    out = torch.zeros(tiles * 256, O)
    for kh in range(3):
        for kw in range(3):
            shift = kh * PW + kw
            u, pos = u0 + shift, q - M + shift
            if fault == "unfolded_row":
                pos = torch.where(u >= 640, pos - 640, pos)
            if fault == "mirror_left":
                through_mirror = (u0 - j16 + shift) % 640 + j16 >= 640
                pos = torch.where(through_mirror, start - M + u % 640, pos)
            out += src[(pos + M).flatten()] @ w[:, :, kh, kw].t()
    qq = q.flatten()
    hp, wp = qq % (PW * PW) // PW, qq % PW
    live = (qq < Q) & (hp >= 1) & (hp <= H) & (wp >= 1) & (wp <= H)
    counted = (trip == n - 1) if fault == "last_item_only" else torch.ones_like(trip, dtype=torch.bool)
    lv = out * (live & counted.repeat_interleave(256)).view(-1, 1)
    part = torch.zeros(grid, 2, O).index_add_(0, wg, torch.stack([lv.view(tiles, 256, O).sum(1), (lv * lv).view(tiles, 256, O).sum(1)], 1))
    y = out[:Q].view(B, PW, PW, O)[:, 1:-1, 1:-1].permute(0, 3, 1, 2)
    return y, part


RING_FWD = [r for r in E.FWD_ROWS if r.get("path") == "ring" and r["name"] != "ring_walk_rounded"]
RING_DG = [r for r in E.DGRAD_ROWS if r.get("path") == "ring"]
RING = [("fwd", r) for r in RING_FWD] + [("dgrad", r) for r in RING_DG]


@pytest.mark.parametrize("kind,row", RING, ids=[f"{k}-{r['name']}" for k, r in RING])
def test_an_unfolded_ring_row_a_left_mirror_and_overwritten_statistics_of_the_ring_kernel_are_caught(kind, row):
    """An unfolded row and a mirror that is not refreshed show only from a share's third tile on (window index 640): caught on
    ring_walk (4-5 tiles per workgroup), invisible on every other ring row (two tiles at the most)"""
    walking = bool(row.get("walk"))
    B, H = row["cfg"][0], row["cfg"][3]
    assert (E.share_facts(E.ring_tiles(B, H), 256)["least"] >= 3) == walking
    if kind == "fwd":
        c = E.fwd_data(row)
        x, w, ref = c["x"].float(), c["w"].float(), c["raw"]
    else:
        c = E.dgrad_data(row)
        x, w, ref = c["dy"].float(), c["w"].float().transpose(0, 1).flip(2, 3).contiguous(), c["dx"]   # conv2d_input as a conv
    y, part = _walked_ring(x, w, 256)
    assert E.same(y.to(BF), ref, BF)
    for fault in ("unfolded_row", "mirror_left"):
        _caught(E.same(_walked_ring(x, w, 256, fault)[0].to(BF), ref, BF), walking, fault)
    if kind == "fwd" and row["mode"] == "A":
        assert E.stats_equal(part, ref)
        _caught(E.stats_equal(_walked_ring(x, w, 256, "last_item_only")[1], ref), walking, "last_item_only")


ROUNDED = [_row(E.FWD_ROWS, "generic_3x3_rounded"), _row(E.FWD_ROWS, "ring_rounded"), _row(E.FWD_ROWS, "pt_14_rounded")]


@pytest.mark.parametrize("row", ROUNDED, ids=E.ids(ROUNDED))
def test_a_truncating_store_is_caught(row):
    c = E.fwd_data(row)
    _, _, _, _, _, s, p = row["cfg"]
    raw = F.conv2d(c["x"].float(), c["w"].float(), None, s, p)
    assert E.same(raw.to(BF), c["raw"], BF)
    trunc = (raw.view(torch.int32) & ~0xFFFF).view(torch.float32).to(BF)
    assert not E.same(trunc, c["raw"], BF)
    # round-half-up instead of round-half-to-even
    up = ((raw.view(torch.int32) + 0x8000) & ~0xFFFF).view(torch.float32).to(BF)
    assert not E.same(up, c["raw"], BF)


MASKED = [_row(E.DGRAD_ROWS, "generic_3x3"), _row(E.DGRAD_ROWS, "pt_7_ragged"), _row(E.S2D_ROWS, "merged5_small")]


@pytest.mark.parametrize("row", MASKED, ids=E.ids(MASKED))
def test_a_mask_that_lets_zeros_through_is_caught(row):
    c = E.s2d_data(row) if "form" in row else E.dgrad_data(row)
    pre = c["pre"].float()
    act = c["act"].to(BF).float()
    zero = torch.zeros(())
    assert E.same(torch.where(act > 0, pre, zero).to(BF), c["out"], BF)
    assert not E.same(torch.where(act >= 0, pre, zero).to(BF), c["out"], BF)
    # a mask read from the sign bit alone: +0 passes, -0 masks
    assert not E.same(torch.where(~torch.signbit(act), pre, zero).to(BF), c["out"], BF)
