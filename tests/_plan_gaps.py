"""Poisoned gaps between the internal buffers of the plan workspace: what the guard bands at its two ends cannot see.

csrc/plan.hip carves every buffer of a train step out of ONE allocation, each sized by a formula written by hand in
layout_workspace().  A launch that runs over its buffer lands in the next one, which is valid memory.  Under
qt_set_plan_guard_gap(GAP_BYTES) every region of a plan created afterwards is followed by GAP_BYTES nobody owns;
qt_plan_region lists the regions.  Here the engine of such a plan is moved onto a Guard.workspace (tests/_guard.py) of exactly
qt_plan_workspace_bytes, every byte 0xFF, and check() asserts that every byte of every gap still is:

  gap i = [offset_i + bytes_i, offset_{i+1})       (the last one ends with the workspace)

so the rounding of a payload to 256 bytes belongs to the gap behind it and a store ONE element past a buffer is seen.  The
payloads start as NaN as well: a kernel that READS past its buffer, or reads what nothing wrote, gets NaN, which the value
comparison with the plain twin shows.

GAP_BYTES = 1 MiB: the tallest tile any kernel writes is 256 rows (_guard.BAND_ROWS), the widest activation row a tiled
kernel writes is 512 channels of f32 = 2 KiB (layer4's maps; the BatchNorm partial tables of `stats` have [2][512] f32 =
4 KiB rows, 256 of them are the 1 MiB), which gives 512 KiB, doubled.  The rows of `fused` / `dfused` are wider (5376
elements) but thin kernels write them row by row, no 256-row tile.  As with the bands of _guard.py, a store farther out than
one gap stays invisible: it lands in the region behind, or in a later gap, which is seen but reported against the wrong
neighbour.  The caller's stream workspace (qt_plan_stream_workspace_bytes) has no regions and is not covered.

plan_run() is the call sequence tests/test_guard_gpu.py and tests/test_plan_gaps_gpu.py drive two twins through, and
compare_twins() what both assert about the recorded tensors.
"""
import contextlib
import ctypes

import torch
import torch.nn.functional as F

from _guard import POISON
from _util import pkg, rel_err

GAP_BYTES = 1 << 20
# f32 twins: two runs of the f32 backward differ in the order in which atomics add partial tiles, nothing else; each is held to
# 1e-3 of max|ref| against the oracle (the f32 build's tolerance for the train step), so that is what two of
# them may differ by at the very most.  Everything that is not a gradient or a stepped parameter: 1e-5.
F32_GRAD_TOL = 1e-3
F32_VALUE_TOL = 1e-5
END = "the end of the workspace"


# ---- the region table ---------------------------------------------------------------------------------------------------
def bound_lib():
    L = pkg("_lib").lib()
    return L


def region_table(L, handle):
    """[(name, offset, bytes)] of a plan, in the library's order"""
    n = L.qt_plan_num_regions(handle)
    assert n > 0, n
    name, off, size = ctypes.c_char_p(), ctypes.c_size_t(), ctypes.c_size_t()
    table = []
    for i in range(n):
        assert L.qt_plan_region(handle, i, ctypes.byref(name), ctypes.byref(off), ctypes.byref(size)) == 0, i
        table.append((name.value.decode(), off.value, size.value))
    return table


def gap_table(table, total):
    """[(region in front, region behind, first byte, end)] for the gaps of a region table in a workspace of `total` bytes"""
    gaps = []
    for i, (name, off, size) in enumerate(table):
        behind, end = (table[i + 1][0], table[i + 1][1]) if i + 1 < len(table) else (END, total)
        assert off + size <= end, (name, behind)
        gaps.append((name, behind, off + size, end))
    return gaps


def check_gaps(ws, gaps):
    """every byte of every gap of the uint8 tensor `ws` (CPU or GPU) is still POISON"""
    assert ws.dtype == torch.uint8 and ws.dim() == 1
    views = [(g, ws[g[2]:g[3]]) for g in gaps if g[3] > g[2]]
    changed = torch.stack([(v != POISON).any() for _, v in views]).cpu()    # one transfer, not one per gap
    if not bool(changed.any()):
        return
    (front, behind, lo, hi), v = views[int(changed.nonzero()[0])]
    first = int((v != POISON).nonzero()[0])
    raise AssertionError(f"plan workspace: the gap between '{front}' and '{behind}' changed, first at byte +{first} behind the "
                         f"end of '{front}' (gap of {hi - lo} bytes, {int((v != POISON).sum())} changed)")


# ---- an engine on a guarded workspace --------------------------------------------------------------------------------------
@contextlib.contextmanager
def plan_guard_gap(nbytes):
    """plans created inside leave `nbytes` unused behind every region"""
    L = bound_lib()
    assert L.qt_set_plan_guard_gap(nbytes) == 0
    try:
        yield
    finally:
        L.qt_set_plan_guard_gap(0)


def rehome(eng, guard):
    """Move a PlanEngine onto guard.workspace: exactly qt_plan_workspace_bytes of 0xFF (NaN) between two bands.  csrc/plan.hip
    keeps offsets, never a pointer into a workspace (every entry point takes the workspace as an argument), so the engine's own
    attributes are enough to move it."""
    L = pkg("_lib")
    ws = guard.workspace("plan workspace", eng.workspace_bytes)
    assert ws.data_ptr() % 256 == 0 and ws.numel() == eng.L.qt_plan_workspace_bytes(eng.handle)
    eng.workspace = ws
    eng.ws_ptr = ctypes.c_void_p(ws.data_ptr())
    L.check(eng.L.qt_plan_init_workspace(eng.handle, eng.ws_ptr, L.stream_ptr()), "qt_plan_init_workspace")
    eng._packed_version = None
    eng._weights_stale = True
    return ws


class PlanGaps:
    """the engine of `model` (built under plan_guard_gap) on a guarded workspace; check(): the guard's bands, the gaps, and
    that the model still runs on this engine and this workspace"""

    def __init__(self, model, guard):
        self.model, self.guard, self.eng = model, guard, model._engine
        self.table = region_table(self.eng.L, self.eng.handle)
        self.ws = rehome(self.eng, guard)
        self.gaps = gap_table(self.table, self.ws.numel())

    def check(self):
        eng = self.model._engine
        assert eng is self.eng and eng.workspace is self.ws and eng.ws_ptr.value == self.ws.data_ptr()
        assert eng.L.qt_plan_num_regions(eng.handle) == len(self.table)
        self.guard.check()          # (synchronizes)
        check_gaps(self.ws, self.gaps)


# ---- the call sequence and the comparison of two twins ---------------------------------------------------------------------
def plan_run(models, checks, share_grads, data, small, image_grad=False):
    """Both twins in step: eval forward on data = (x, f, y) and on its first `small` rows, a train step without and one with
    max_grad_norm, a forward on the re-packed operands; checks[i]() after every call of twin i.  share_grads: twin 1 steps
    twin 0's gradients -- the f32 backward is not bit-reproducible from run to run, and Adam turns a last-bit difference of a
    near-zero gradient into a visible one (tests/test_clip_adam_gpu.py::_compare_twins).  image_grad: the train steps ask for
    d(loss)/d(image) as well."""
    P = pkg()
    x, f, y = data
    outs = [{} for _ in models]

    def forward(tag, xb, fb):
        for m, check, out in zip(models, checks, outs):
            m.eval()
            with torch.no_grad():
                out[tag] = m(xb, fb).float().clone()
            check()
            m.train()

    forward("eval", x, f)
    forward("eval_small", x[:small], f[:small])
    for tag, max_norm in (("plain", None), ("clipped", 0.05)):
        opts = [P.FusedAdam(m.parameters(), lr=1e-3, weight_decay=1e-4, model=m, max_grad_norm=max_norm) for m in models]
        for m, opt, check, out in zip(models, opts, checks, outs):
            opt.zero_grad(set_to_none=True)
            xi = x.clone().requires_grad_(True) if image_grad else x
            logits = m(xi, f)
            check()
            F.cross_entropy(logits, y).backward()
            check()
            out[tag + "/logits"] = logits.detach().float().clone()
            if image_grad:
                out[tag + "/grad/image"] = xi.grad.clone()
            for n, p in m.named_parameters():
                if p.grad is not None:
                    out[f"{tag}/grad/{n}"] = p.grad.clone()
        if share_grads:
            for p, q in zip(models[0].parameters(), models[1].parameters()):
                assert (p.grad is None) == (q.grad is None)
                if p.grad is not None:
                    q.grad.copy_(p.grad)
        for m, opt, check, out in zip(models, opts, checks, outs):
            opt.step()
            check()
            for n, p in m.named_parameters():
                out[f"{tag}/param/{n}"] = p.detach().clone()
    forward("after", x, f)
    return outs


def compare_twins(want, got, dt):
    """what plan_run recorded for the plain twin and for the guarded one"""
    from test_clip_adam_gpu import ADAM_TOL
    assert want.keys() == got.keys() and any("/grad/" in k for k in want)
    for k in want:
        assert bool(torch.isfinite(got[k]).all()), k
        if dt == torch.bfloat16:   # the bf16 build is bit-reproducible (tests/test_clip_adam_gpu.py)
            assert torch.equal(want[k], got[k]), k
        elif "/param/" in k:       # f32: the bounds tests/test_clip_adam_gpu.py uses for twins
            assert float((want[k] - got[k]).abs().max()) <= ADAM_TOL * float(want[k].abs().max()), k
        elif "/grad/" in k:        # recorded before twin 0's gradients are copied over
            assert rel_err(got[k].cpu(), want[k].cpu()) <= F32_GRAD_TOL, k
        else:
            assert rel_err(got[k].cpu(), want[k].cpu()) <= F32_VALUE_TOL, k
