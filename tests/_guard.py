"""Guard bands for buffers handed to a kernel: what value parity cannot see.

Every buffer is ONE uint8 allocation, laid out as  [front band | payload | back band].  The bands hold byte 0xFF (NaN as f32
and as bf16, 255 as a byte) and adjoin the payload byte for byte, so a store one element before or behind it lands in a
band.  Three kinds of buffer:

  output     the payload is poison too (or zeros where the contract in include/qtcnn.h has the caller provide zeros: a
             packer that writes the real taps only, a kernel that accumulates); after the call no float element may still
             be NaN.  Byte outputs legitimately hold 0xFF: run those cases with fill=0xFF and fill=0x00 and compare.
  workspace  the payload is exactly the byte count the size query returned, NaN-filled.
  input      the payload is the data (the whole storage behind a strided view, so a slice keeps its enclosing tensor and
             that tensor gets the bands); it must be byte-identical after the call.  A halo or tail load that leaves the
             tensor reads NaN, which reaches the result and fails the case's own value check.

Payload sizes are what the entry point is documented to write.  A partial-statistics output of a convolution is
[qt_conv2d_stats_rows][2][C] (its sentence in qtcnn.h), not the qt_stats_capacity_rows(rows) rows a caller reserves: the spare
rows belong to qt_bn_finalize's folding, the convolution must not touch them, and here they would lie in the back band.

Guard.check() asserts all of it.  Each band is the larger of 64 KiB and 256 payload rows (the tallest pixel tile any kernel
here writes), rounded up to 256 bytes.  A store farther out than a band stays invisible, and so does one internal buffer of
a workspace running into the next: the bands sit at the two ends only (the plan workspace: tests/_plan_gaps.py).
"""
import math

import torch

POISON = 0xFF
ALIGN = 256
BAND_MIN_BYTES = 64 << 10
BAND_ROWS = 256


def band_bytes(row_bytes):
    """bytes of one band next to a payload whose rows are `row_bytes` long"""
    n = max(BAND_MIN_BYTES, BAND_ROWS * int(row_bytes))
    return -(-n // ALIGN) * ALIGN


def _esize(dt):
    return torch.empty(0, dtype=dt).element_size()


def _storage_bytes(t):
    """the whole storage behind `t` as a uint8 tensor (no copy)"""
    return torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())


class _Buf:
    def __init__(self, name, kind, whole, lo, nbytes, band, band_front):
        self.name, self.kind, self.whole = name, kind, whole
        self.lo, self.nbytes, self.band = lo, nbytes, band    # payload = whole[lo : lo + nbytes]
        self.band_front = band_front                          # the front band + the gap an element offset leaves
        self.t = None            # what the kernel is given
        self.snapshot = None     # inputs: the uploaded bytes
        self.written = False     # outputs: every float element must be overwritten

    @property
    def front(self):
        return self.whole[self.lo - self.band_front:self.lo]

    @property
    def back(self):
        return self.whole[self.lo + self.nbytes:self.lo + self.nbytes + self.band]

    @property
    def payload(self):
        return self.whole[self.lo:self.lo + self.nbytes]


class Guard:
    """the guarded buffers of one kernel call (or of a few calls that share them)"""

    def __init__(self, dev):
        self.dev = torch.device(dev)
        self.bufs = []

    # ---- allocation -------------------------------------------------------------------------------------------------------
    def _alloc(self, name, kind, nbytes, row_bytes, off_bytes, fill):
        band = band_bytes(row_bytes)
        whole = torch.full((ALIGN + band + off_bytes + nbytes + band,), POISON, dtype=torch.uint8, device=self.dev)
        start = -whole.data_ptr() % ALIGN          # the front band starts 256-byte aligned, and so does an unshifted payload
        b = _Buf(name, kind, whole, start + band + off_bytes, nbytes, band, band + off_bytes)
        if fill != POISON:
            b.payload.fill_(fill)
        self.bufs.append(b)
        return b

    def output(self, name, shape, dt, fill=POISON, offset=0, written=None):
        """An output of `shape` (the documented capacity, not the logical size).  fill: POISON, or 0 where the caller must
        provide zeros.  offset: payload shifted by 1..3 elements off the 256-byte boundary.  written: every float element
        must be overwritten (default: when the fill is poison)."""
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        es = _esize(dt)
        b = self._alloc(name, "output", math.prod(shape) * es, (shape[-1] if shape else 1) * es, offset * es, fill)
        b.t = b.payload.view(dt).view(shape)
        b.written = (fill == POISON) if written is None else bool(written)
        assert not b.written or fill == POISON, "only a poisoned payload can show an unwritten element"
        return b.t

    def workspace(self, name, nbytes):
        """exactly `nbytes` (what the size query returned) of NaN between two bands, as uint8"""
        b = self._alloc(name, "workspace", int(nbytes), 0, 0, POISON)
        b.t = b.payload
        return b.t

    def input(self, name, t, offset=0):
        """A copy of `t` on the guard's device with poison around it; a view comes back as the same view of a copy of its
        whole storage.  None stays None (optional operands)."""
        if t is None:
            return None
        src = _storage_bytes(t)
        es = t.element_size()
        row = (t.shape[-1] if t.dim() else 1) * es
        b = self._alloc(name, "input", src.numel(), row, offset * es, POISON)
        b.payload.copy_(src)
        b.snapshot = b.payload.clone()
        base = b.payload[:src.numel() // es * es].view(t.dtype)
        b.t = torch.as_strided(base, t.size(), t.stride(), base.storage_offset() + t.storage_offset())
        return b.t

    # ---- the assertions ---------------------------------------------------------------------------------------------------
    def check(self):
        """bands intact, float outputs fully written, inputs unchanged"""
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)
        for b in self.bufs:
            for side, band in (("front", b.front), ("back", b.back)):
                if not bool((band == POISON).all()):
                    first = int((band != POISON).nonzero()[0])
                    off = first - band.numel() if side == "front" else b.nbytes + first
                    raise AssertionError(f"guard: {b.kind} '{b.name}': {side} band changed, first at byte offset {off} "
                                         f"relative to the payload ({b.nbytes} bytes)")
            if b.kind == "output" and b.written and b.t.is_floating_point():
                nan = torch.isnan(b.t).reshape(-1)
                if bool(nan.any()):
                    raise AssertionError(f"guard: output '{b.name}': element {int(nan.nonzero()[0])} of {nan.numel()} was "
                                         f"never written ({int(nan.sum())} in all)")
            if b.kind == "input" and not torch.equal(b.payload, b.snapshot):
                first = int((b.payload != b.snapshot).nonzero()[0])
                raise AssertionError(f"guard: input '{b.name}' was modified, first at byte offset {first}")
