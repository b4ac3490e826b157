"""CPU: the plan's graph and workspace layout (qt_plan_create and the introspection entry points are host-only) are
exactly the recorded ones -- tests/golden/plan_layout.json holds, for the four plan models x {f32, bf16} at batch 256
(CnnLstm: 16 sequences x 16 frames, hidden 256), the tensor table, the workspace size and the offset of every buffer name
qt_plan_find_buffer knows, under the default QTCNN_* switches.  The values are the same with and without a visible GPU."""
import ctypes
import json
import os

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
    eng._bind_api(L)
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
