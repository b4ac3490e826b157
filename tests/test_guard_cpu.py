"""tests/_guard.py on CPU tensors: each kind of damage is reported with its buffer, side and offset; a clean run passes."""
import pytest
import torch

import _guard
from _guard import Guard, POISON, band_bytes

CPU = torch.device("cpu")


def _buf(g, t):
    return next(b for b in g.bufs if b.t is t)


def test_band_size():
    assert band_bytes(0) == 64 << 10
    assert band_bytes(128 * 2) == 64 << 10           # 256 rows of 256 bytes = 64 KiB
    assert band_bytes(512 * 4) == 256 * 2048
    assert band_bytes(257) == -(-256 * 257 // 256) * 256 and band_bytes(257) % 256 == 0
    assert band_bytes(3 * 4) == 64 << 10


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.uint8])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_layout_alignment_and_offsets(dt, offset):
    g = Guard(CPU)
    y = g.output("y", (5, 7), dt, offset=offset)
    ws = g.workspace("ws", 1000)
    x = g.input("x", torch.arange(35, dtype=torch.float32).to(dt).view(5, 7), offset=offset)
    es = y.element_size()
    assert y.data_ptr() % 256 == offset * es and x.data_ptr() % 256 == offset * es and ws.data_ptr() % 256 == 0
    assert ws.numel() == 1000 and ws.dtype == torch.uint8
    for t in (y, ws, x):
        b = _buf(g, t)
        # the bands adjoin the payload byte for byte and hold 0xFF; the front band starts 256-byte aligned
        assert b.payload.data_ptr() == t.data_ptr() and b.payload.numel() == t.numel() * t.element_size()
        assert b.front.data_ptr() + b.front.numel() == t.data_ptr() and b.front.data_ptr() % 256 == 0
        assert b.back.data_ptr() == t.data_ptr() + b.nbytes
        assert b.front.numel() >= 64 << 10 and b.back.numel() >= 64 << 10 and b.back.numel() % 256 == 0
        assert bool((b.front == POISON).all()) and bool((b.back == POISON).all())
    assert bool((_buf(g, y).payload == POISON).all()) and bool((ws == POISON).all())
    if dt != torch.uint8:
        assert bool(torch.isnan(y).all())
    assert torch.equal(x, torch.arange(35, dtype=torch.float32).to(dt).view(5, 7))


def test_band_follows_the_row_length():
    g = Guard(CPU)
    y = g.output("y", (3, 512), torch.float32)
    assert _buf(g, y).back.numel() == 256 * 512 * 4 == _buf(g, y).front.numel()


def test_clean_run_passes():
    g = Guard(CPU)
    y = g.output("y", (4, 8), torch.float32)
    acc = g.output("acc", (8,), torch.float32, fill=0)
    code = g.output("code", (4, 8), torch.uint8)
    g.workspace("ws", 96)
    x = g.input("x", torch.randn(4, 8))
    assert g.input("none", None) is None
    y.copy_(x * 2)
    acc += x.sum(0)
    code.fill_(255)            # byte outputs may hold 0xFF
    g.check()
    g.check()                  # checking changes nothing


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("where", ["before", "after", "far_front", "far_back"])
def test_a_store_outside_the_payload_is_reported(dt, where):
    g = Guard(CPU)
    y = g.output("y", (6, 16), dt)
    y.zero_()
    b = _buf(g, y)
    es, n = y.element_size(), y.numel()
    flat = b.whole[b.lo - b.band_front:b.lo + b.nbytes + b.band].view(dt)   # front band + payload + back band, as elements
    first = b.band_front // es
    idx = {"before": first - 1, "after": first + n, "far_front": 0, "far_back": flat.numel() - 1}[where]
    flat[idx] = 1.0
    side = "front" if where in ("before", "far_front") else "back"
    off = (idx - first) * es
    # (1.0 is 00 00 80 3F as f32 and 80 3F as bf16, little endian: every byte of the element differs from 0xFF)
    with pytest.raises(AssertionError, match=rf"output 'y': {side} band changed, first at byte offset {off} relative"):
        g.check()


def test_a_single_byte_at_either_end_is_reported():
    g = Guard(CPU)
    ws = g.workspace("ws", 100)
    b = _buf(g, ws)
    b.whole[b.lo + 100] = 0
    with pytest.raises(AssertionError, match=r"workspace 'ws': back band changed, first at byte offset 100 relative"):
        g.check()
    b.whole[b.lo + 100] = POISON
    b.whole[b.lo - 1] = 7
    with pytest.raises(AssertionError, match=r"workspace 'ws': front band changed, first at byte offset -1 relative"):
        g.check()
    b.whole[b.lo - 1] = POISON
    g.check()


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_an_unwritten_element_is_reported(dt):
    g = Guard(CPU)
    y = g.output("y", (6, 16), dt)
    y.zero_()
    y.view(-1)[37] = float("nan")
    y.view(-1)[80] = float("nan")
    with pytest.raises(AssertionError, match=r"output 'y': element 37 of 96 was never written \(2 in all\)"):
        g.check()


def test_zero_filled_and_byte_outputs_are_not_asked_to_be_written():
    g = Guard(CPU)
    g.output("acc", (8,), torch.float32, fill=0)
    g.output("partial", (8,), torch.float32, fill=0, written=False)
    g.output("bits", (8,), torch.uint8)
    g.check()
    with pytest.raises(AssertionError):
        g.output("bad", (8,), torch.float32, fill=0, written=True)


def test_a_modified_input_is_reported():
    g = Guard(CPU)
    x = g.input("x", torch.ones(4, 8))
    g.check()
    x[1, 2] = 3.0
    with pytest.raises(AssertionError, match=r"input 'x' was modified, first at byte offset 4[0-3]$"):
        g.check()


def test_a_view_keeps_its_enclosing_tensor():
    wide = torch.arange(2 * 5 * 12, dtype=torch.float32).view(2, 5, 12)
    sl = wide[..., 4:8]
    g = Guard(CPU)
    x = g.input("x", sl)
    assert torch.equal(x, sl) and x.stride() == sl.stride() and x.storage_offset() - _buf(g, x).payload.view(
        torch.float32).storage_offset() == 4
    b = _buf(g, x)
    assert b.nbytes == wide.numel() * 4 and torch.equal(b.payload.view(torch.float32).view(2, 5, 12), wide)
    # the neighbours of the slice are the enclosing tensor's data, the bands start where that tensor ends
    assert x.data_ptr() - 16 == b.payload.data_ptr()
    flat = wide.view(-1)[4:]
    f = g.input("flat", flat)
    assert torch.equal(f, flat) and _buf(g, f).nbytes == wide.numel() * 4
    g.check()


def test_out_of_range_read_meets_nan():
    g = Guard(CPU)
    x = g.input("x", torch.ones(3, 4))
    b = _buf(g, x)
    around = b.whole[b.lo - 4:b.lo + b.nbytes + 4].view(torch.float32)
    assert bool(torch.isnan(around[0])) and bool(torch.isnan(around[-1])) and float(around[1:-1].sum()) == 12.0
    assert _guard.POISON == 0xFF
