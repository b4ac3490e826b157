"""The kernel route of every conv block of Quadtree3DCNN (video3d._ConvBlock.route) at the shapes where the routes come apart.
No device is needed: the shape queries behind the routes fall back to 256 compute units without one.

The five blocks see, for a clip [B, T, 3, H, H]: (T, H), (T, H/2), (T/2, H/4), (T/4, H/8), (T/4, H/16) -- the pools are
(1,2,2), (2,2,2), (2,2,2), (1,2,2), none.
"""
import pytest
import torch

from _util import pkg

B, T = 2, 4
SWITCHES = ("FUSED_POOL", "LSTM_SIDE", "WGRAD_SIDE", "PACK_CACHE", "SLAB_C32", "FIRST_WGRAD_FUSED", "POOLED32")


@pytest.fixture
def v3d(monkeypatch):
    v = pkg("video3d")
    for s in SWITCHES:   # the defaults, whatever the environment of this run sets
        monkeypatch.setattr(v, s, True)
    monkeypatch.delenv("QTCNN_CONV3D_FIRST", raising=False)
    return v


@pytest.fixture(scope="module")
def blocks():
    return pkg("video3d").Quadtree3DCNN(12, sequence_length=T)._conv_blocks()


def _routes(blocks, dt, HW, training=True, keep=True, aligned=True):
    out, t, h = [], T, HW
    for blk in blocks:
        out.append(blk.route(dt, B, t, h, h, training, keep, aligned))
        if blk.pool_t:
            t, h = t // blk.pool_t, h // 2
    return out


def test_routes_of_the_three_configurations(v3d, blocks):
    bf, f32 = torch.bfloat16, torch.float32
    # 64 x 64, bf16: the first layer from the clip, block 2 slab-resident at 32 x 32, 32-channel rows between them
    r = _routes(blocks, bf, 64)
    assert [x.kernel for x in r] == [v3d.RAW, v3d.SLAB, v3d.GEMM, v3d.GEMM, v3d.GEMM]
    assert [x.width for x in r] == [32, 64, 128, 256, 1024]
    assert [x.fused_pool for x in r] == [True, True, True, True, False] and not any(x.fused_eval for x in r)
    assert all(x.prow > 0 for x in r)
    # 48 x 48: W % 16 == 0, so the first layer still reads the clip; the pooled width 24 is no slab shape: rows padded to 64
    r = _routes(blocks, bf, 48)
    assert [x.kernel for x in r] == [v3d.RAW, v3d.GEMM, v3d.GEMM, v3d.GEMM, v3d.GEMM]
    assert [x.width for x in r] == [64, 64, 128, 256, 1024]
    # f32: packed first layer, the implicit GEMM everywhere
    r = _routes(blocks, f32, 32)
    assert [x.kernel for x in r] == [v3d.PACKED, v3d.GEMM, v3d.GEMM, v3d.GEMM, v3d.GEMM]
    assert [x.width for x in r] == [64, 64, 128, 256, 1024]
    assert all(x.prow > 0 for x in r)


def test_eval_routes(v3d, blocks):
    r = _routes(blocks, torch.bfloat16, 32, training=False, keep=False)
    assert [x.kernel for x in r] == [v3d.RAW, v3d.SLAB, v3d.GEMM, v3d.GEMM, v3d.GEMM]
    assert all(x.fused_eval and not x.fused_pool for x in r) and r[0].width == 32
    r = _routes(blocks, torch.bfloat16, 32, training=False, keep=True)   # eval with a backward to come: nothing fused away
    assert not any(x.fused_eval for x in r) and [x.fused_pool for x in r] == [True, True, True, True, False]
    assert all(x.prow == 0 for x in r[1:])   # (running statistics: no partial sums)


def test_switches_change_exactly_their_fields(v3d, blocks, monkeypatch):
    bf = torch.bfloat16
    base = _routes(blocks, bf, 64)
    monkeypatch.setattr(v3d, "POOLED32", False)
    off = _routes(blocks, bf, 64)
    assert off[0] == base[0]._replace(width=64) and off[1:] == base[1:]
    monkeypatch.setattr(v3d, "POOLED32", True)
    monkeypatch.setattr(v3d, "SLAB_C32", False)
    off = _routes(blocks, bf, 64)
    assert off[0] == base[0]._replace(width=64)
    assert off[1].kernel == v3d.GEMM and off[1] == base[1]._replace(kernel=v3d.GEMM, prow=off[1].prow) and off[1].prow > 0
    assert off[2:] == base[2:]
    monkeypatch.setattr(v3d, "SLAB_C32", True)
    monkeypatch.setattr(v3d, "FUSED_POOL", False)
    off = _routes(blocks, bf, 64)
    assert off[0].kernel == v3d.PACKED and off[0].width == 64 and off[1].kernel == v3d.SLAB
    assert not any(x.fused_pool for x in off)
    monkeypatch.setattr(v3d, "FUSED_POOL", True)
    monkeypatch.setenv("QTCNN_CONV3D_FIRST", "0")   # consulted per call
    assert _routes(blocks, bf, 64)[0].kernel == v3d.PACKED
    monkeypatch.delenv("QTCNN_CONV3D_FIRST")
    assert _routes(blocks, bf, 64) == base
    # an input that does not start on a 16-byte boundary takes neither the raw nor the slab kernel
    assert [x.kernel for x in _routes(blocks, bf, 64, aligned=False)[:2]] == [v3d.PACKED, v3d.GEMM]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("HW", [32, 48, 64, 96, 256])
def test_block1_rows_are_32_wide_iff_block2_is_slab(v3d, blocks, dt, HW):
    """block 1 writes 32-channel pooled rows exactly where block 2 reads them: on the slab route at the pooled shape"""
    for training, keep in ((True, True), (False, True), (False, False)):
        r = _routes(blocks, dt, HW, training, keep)
        assert (r[0].width == 32) == (r[1].kernel == v3d.SLAB), (training, keep, r[:2])
        assert r[0].width in (32, 64) and (r[0].kernel == v3d.RAW or r[0].width == 64)
