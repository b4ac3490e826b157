"""CPU: the plan's graph and workspace layout (qt_plan_create and the introspection entry points are host-only) are
exactly the recorded ones -- tests/golden/plan_layout.json holds, for the four plan models x {f32, bf16} at batch 256
(CnnLstm: 16 sequences x 16 frames, hidden 256), the tensor table, the workspace size and the offset of every buffer name
qt_plan_find_buffer knows, under the default QTCNN_* switches.  The values are the same with and without a visible GPU.

The recorded offsets prove that the layout did not change.  The region table (qt_plan_region) is checked for its shape here:
ascending, disjoint, aligned, the same with and without the guard gap of qt_set_plan_guard_gap but for the gap; whether every
region is LARGE enough for what the kernels write is the business of tests/test_plan_gaps_gpu.py."""
import ctypes
import json
import os

import pytest

from _plan_gaps import GAP_BYTES, plan_guard_gap, region_table
from _util import ROOT, PKG, pkg

GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_layout.json")
MODELS = (("quadtree", 0), ("standard_resnet", 1), ("attention", 2), ("cnn_lstm", 3))
DTYPES = (("f32", 0), ("bf16", 1))


def _lib():
    if not os.path.exists(os.path.join(ROOT, PKG, "libqtcnn_hip.so")):
        import __graft_entry__ as g
        g.build()
    return pkg("_lib").lib()


def buffer_names(num_convs, attention):
    names = ["fused", "dfused", "hidden", "stem.pooled", "stem.gpooled"]
    for b in range(8):
        names += [f"block{b}.out", f"block{b}.gout", f"block{b}.a1"]
    for c in range(num_convs):
        names += [f"conv{c}.y", f"conv{c}.gy"]
    if attention:
        names += ["attention.vectors", "attention.weights"]
    return names


def plan_layout(L):
    """{"<model>/<dtype>": {"tensors": [[name, kind, [dims]]...], "workspace_bytes": n, "buffers": {name: offset}}}"""
    eng = pkg("engine")
    out = {}
    for mname, model in MODELS:
        for dname, dtype in DTYPES:
            desc = eng.PlanDesc(dtype, 256, 12, model, 0, 47, 0.5, 1e-5, 0.1, 16 if model == 3 else 0, 256 if model == 3 else 0)
            h = ctypes.c_void_p()
            assert L.qt_plan_create(ctypes.byref(desc), ctypes.byref(h)) == 0, (mname, dname)
            try:
                dims = (ctypes.c_int * 4)()
                tensors = []
                for i in range(L.qt_plan_num_tensors(h)):
                    nd = L.qt_plan_tensor_shape(h, i, dims)
                    tensors.append([L.qt_plan_tensor_name(h, i).decode(), L.qt_plan_tensor_kind(h, i), [dims[k] for k in range(nd)]])
                # 20 backbone convolutions (stem, 16 in the blocks, 3 downsamples) + the region heads
                num_convs = 20 + (2 if model == 2 else 1 if model == 0 else 0)
                buffers = {}
                for name in buffer_names(num_convs, model == 2):
                    off = ctypes.c_size_t()
                    assert L.qt_plan_find_buffer(h, name.encode(), ctypes.byref(off)) == 0, (mname, dname, name)
                    buffers[name] = off.value
                off = ctypes.c_size_t()
                assert L.qt_plan_find_buffer(h, f"conv{num_convs}.y".encode(), ctypes.byref(off)) != 0
                out[f"{mname}/{dname}"] = {"tensors": tensors, "workspace_bytes": L.qt_plan_workspace_bytes(h),
                                           "buffers": buffers}
            finally:
                L.qt_plan_destroy(h)
    return out


def test_plan_graph_and_workspace_layout_match_the_recorded_ones():
    got = plan_layout(_lib())
    want = json.load(open(GOLDEN))
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key]["tensors"] == want[key]["tensors"], key
        assert got[key]["workspace_bytes"] == want[key]["workspace_bytes"], key
        assert got[key]["buffers"] == want[key]["buffers"], key


# ---- the region table -----------------------------------------------------------------------------------------------------
def _create(L, model, dtype, batch):
    eng = pkg("engine")
    seq = {256: 16, 18: 3}[batch] if model == 3 else 0      # CnnLstm: whole sequences
    desc = eng.PlanDesc(dtype, batch, 12, model, 0, 47, 0.5, 1e-5, 0.1, seq, 256 if model == 3 else 0)
    h = ctypes.c_void_p()
    assert L.qt_plan_create(ctypes.byref(desc), ctypes.byref(h)) == 0
    return h


def _tensors(L, h):
    dims = (ctypes.c_int * 4)()
    out = {}
    for i in range(L.qt_plan_num_tensors(h)):
        nd = L.qt_plan_tensor_shape(h, i, dims)
        out[L.qt_plan_tensor_name(h, i).decode()] = [dims[k] for k in range(nd)]
    return out


def _dw_slices(L, h, num_convs):
    """[(offset, bytes)] of the convolutions that own a slice of the f32 weight-gradient scratch, in layout order.  Conv i is
    the i-th 4-d tensor of the table (build_graph appends both in the same order); its slice is [O][kh][kw][I] f32, the
    stem's the packed [64][8 taps][32]."""
    weights = [shape for shape in _tensors(L, h).values() if len(shape) == 4]
    assert len(weights) == num_convs
    slices = []
    for i, (o, c, kh, kw) in enumerate(weights):
        off = ctypes.c_size_t()
        if L.qt_plan_find_buffer(h, f"conv{i}.dw".encode(), ctypes.byref(off)) == 0:
            slices.append((off.value, 4 * (64 * 8 * 32 if i == 0 else o * c * kh * kw)))
    return slices


@pytest.mark.parametrize("batch", [256, 18])
@pytest.mark.parametrize("dname,dtype", DTYPES)
@pytest.mark.parametrize("mname,model", MODELS)
def test_region_table_with_and_without_the_guard_gap(mname, model, dname, dtype, batch):
    L = _lib()
    tables = {}
    for gap in (0, GAP_BYTES):
        with plan_guard_gap(gap):
            h = _create(L, model, dtype, batch)
        try:
            table = region_table(L, h)
            total = L.qt_plan_workspace_bytes(h)
            names = [n for n, _, _ in table]
            assert len(set(names)) == len(names)
            end = 0
            for i, (name, off, size) in enumerate(table):
                assert off % 256 == 0 and size > 0, name
                assert off >= end, name                                 # ascending and disjoint
                if i:
                    prev = table[i - 1]
                    assert off - (prev[1] + prev[2]) >= gap, name         # (the rounding belongs to the gap)
                    assert off == -(-(prev[1] + prev[2]) // 256) * 256 + gap, name
                end = off + size
            assert table[0][1] == 0
            assert total == -(-end // 256) * 256 + gap
            # every buffer qt_plan_find_buffer knows is the region of that name
            starts = {n: o for n, o, _ in table}
            num_convs = 20 + (2 if model == 2 else 1 if model == 0 else 0)
            for name in buffer_names(num_convs, model == 2):
                off = ctypes.c_size_t()
                assert L.qt_plan_find_buffer(h, name.encode(), ctypes.byref(off)) == 0, name
                assert starts[name] == off.value, name
            # the weight-gradient scratch is ONE region,
            # ... the slices of its owners back to back, no gap inside: one memset zeroes it (csrc/plan.hip, backward())
            dw = [t for t in table if t[0] == "dw"]
            slices = _dw_slices(L, h, num_convs)
            assert len(dw) == 1 and slices and slices[0][0] == dw[0][1]
            assert all(a[0] + a[1] == b[0] for a, b in zip(slices, slices[1:]))
            assert dw[0][2] == sum(size for _, size in slices)
            assert dtype == 1 or len(slices) >= 17     # f32: the stem and the sixteen 3x3 convs of the blocks at least
            # out of range
            name, off, size = ctypes.c_char_p(), ctypes.c_size_t(), ctypes.c_size_t()
            for i in (-1, len(table)):
                assert L.qt_plan_region(h, i, ctypes.byref(name), ctypes.byref(off), ctypes.byref(size)) != 0
            tables[gap] = table
        finally:
            L.qt_plan_destroy(h)
    assert [(n, b) for n, _, b in tables[0]] == [(n, b) for n, _, b in tables[GAP_BYTES]]


def test_guard_gap_setter_takes_multiples_of_256_and_resets():
    L = _lib()
    assert L.qt_set_plan_guard_gap(100) != 0 and L.qt_set_plan_guard_gap(257) != 0
    with plan_guard_gap(GAP_BYTES):
        h = _create(L, 0, 1, 18)
        gapped = L.qt_plan_workspace_bytes(h)
        regions = L.qt_plan_num_regions(h)
        L.qt_plan_destroy(h)
    h = _create(L, 0, 1, 18)
    try:
        assert gapped == L.qt_plan_workspace_bytes(h) + regions * GAP_BYTES
    finally:
        L.qt_plan_destroy(h)
    # back at 0 the layout is the recorded one
    got, want = plan_layout(L), json.load(open(GOLDEN))
    assert got == want
