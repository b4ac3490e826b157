"""CPU: the gap check of tests/_plan_gaps.py finds what it is there to find.  A uint8 tensor is laid out from the region table
of a real plan (qt_plan_create is host-only) and damaged on purpose in three places; each must be reported with the right
pair of regions and the right offset.  The mistakes made on purpose stay here: nothing under-sized ever runs on the GPU.

The plan is QuadtreeCNN numerical_only, bf16, batch 1 (no activation buffers: 90 MB of packed weights and scratch) under a
gap of 4 KiB: check_gaps() takes the table as it comes, and the 1 MiB of the GPU runs would only make the tensor larger."""
import ctypes
import os

import pytest
import torch

from _guard import POISON
from _plan_gaps import END, bound_lib, check_gaps, gap_table, plan_guard_gap, region_table
from _util import ROOT, PKG, pkg

GAP = 4096


@pytest.fixture(scope="module")
def layout():
    """(region table, gaps, workspace bytes)"""
    if not os.path.exists(os.path.join(ROOT, PKG, "libqtcnn_hip.so")):
        import __graft_entry__ as g
        g.build()
    L = bound_lib()
    desc = pkg("engine").PlanDesc(1, 1, 12, 0, 2, 47, 0.5, 1e-5, 0.1, 0, 0)     # bf16, batch 1, QuadtreeCNN, numerical_only
    h = ctypes.c_void_p()
    with plan_guard_gap(GAP):
        assert L.qt_plan_create(ctypes.byref(desc), ctypes.byref(h)) == 0
    try:
        table, total = region_table(L, h), L.qt_plan_workspace_bytes(h)
    finally:
        L.qt_plan_destroy(h)
    return table, gap_table(table, total), total


def _workspace(total):
    return torch.full((total,), POISON, dtype=torch.uint8)


def test_untouched_workspace_passes(layout):
    table, gaps, total = layout
    assert len(gaps) == len(table) and gaps[-1][1] == END and gaps[-1][3] == total
    assert all(hi - lo >= GAP for _, _, lo, hi in gaps)
    ws = _workspace(total)
    check_gaps(ws, gaps)
    for _, off, size in table:      # whatever the launches do inside their regions
        ws[off:off + size] = 0
    check_gaps(ws, gaps)


def _damaged(layout, front, at):
    """check_gaps' message for one changed byte, `at(lo, hi)` bytes behind the end of region `front`"""
    table, gaps, total = layout
    (name, behind, lo, hi), = [g for g in gaps if g[0] == front]
    rel = at(lo, hi)
    ws = _workspace(total)
    ws[lo + rel] = 0
    with pytest.raises(AssertionError) as e:
        check_gaps(ws, gaps)
    return str(e.value), behind, rel, hi - lo


def test_one_byte_behind_a_batchnorm_vector(layout):
    """bn0.mean is 64 f32 = 256 bytes: the byte right behind it is the first of the gap, one element past the vector"""
    table = layout[0]
    assert dict((n, b) for n, _, b in table)["bn0.mean"] == 256
    msg, behind, rel, size = _damaged(layout, "bn0.mean", lambda lo, hi: 0)
    assert behind == "bn0.invstd" and size == GAP
    assert "between 'bn0.mean' and 'bn0.invstd'" in msg and "byte +0 behind the end of 'bn0.mean'" in msg


def test_one_byte_in_the_rounding_behind_a_payload(layout):
    """lin_ws is not a multiple of 256 bytes here (or the next region whose size is not): the slack up to the next 256-byte
    boundary belongs to the gap, so one element past the payload is seen"""
    table, gaps, _ = layout
    front = next(n for n, _, b in table if b % 256)
    (_, behind, lo, hi), = [g for g in gaps if g[0] == front]
    assert hi - lo > GAP
    msg, behind, rel, size = _damaged(layout, front, lambda lo, hi: 0)
    assert f"between '{front}' and '{behind}'" in msg and f"byte +0 behind the end of '{front}'" in msg


def test_one_byte_in_the_middle_of_a_gap(layout):
    msg, behind, rel, size = _damaged(layout, "stats", lambda lo, hi: (hi - lo) // 2)
    assert behind == "stats_bn2" and rel == GAP // 2
    assert "between 'stats' and 'stats_bn2'" in msg and f"byte +{GAP // 2} behind the end of 'stats'" in msg


def test_the_last_byte_of_a_gap(layout):
    msg, behind, rel, size = _damaged(layout, "conv3.w_dgrad", lambda lo, hi: hi - lo - 1)
    assert behind == "conv4.w_fwd" and rel == GAP - 1
    assert "between 'conv3.w_dgrad' and 'conv4.w_fwd'" in msg and f"byte +{GAP - 1} behind the end of 'conv3.w_dgrad'" in msg
    # ... and of the last gap, which ends with the workspace
    last = layout[0][-1][0]
    msg, behind, rel, size = _damaged(layout, last, lambda lo, hi: hi - lo - 1)
    assert behind == END and f"between '{last}' and '{END}'" in msg and f"byte +{rel} behind" in msg


def test_the_first_damaged_gap_is_the_one_reported(layout):
    table, gaps, total = layout
    ws = _workspace(total)
    for front in ("wgrad_part", "bn7.coef"):
        lo = next(g[2] for g in gaps if g[0] == front)
        ws[lo + 3] = 1
    with pytest.raises(AssertionError, match="between 'bn7.coef' and 'bn8.mean'.*byte \\+3 behind"):
        check_gaps(ws, gaps)
