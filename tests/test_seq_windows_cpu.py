"""Sequence windows, the parts that need no GPU: the plain loops of tests/_seq_windows_ref.py against what the reference's own
two scripts produced (tests/golden/seq_windows.npz), a Python walk of the kernel's three launches against the plain loops
around every tile size, the C ABI's declaration and host-side argument checks, the module's refusals, the exports."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _seq_windows_ref as W
from _util import PKG, ROOT, pkg

QT_ERR_INVALID_ARG, QT_ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "seq_windows.npz"))
    return {k: g[k] for k in g.files}


def _source():
    return open(os.path.join(ROOT, PKG, "csrc", "seq_windows.hip")).read()


@pytest.mark.parametrize("rule", ["uniform", "last"])
def test_plain_loops_reproduce_the_reference_on_the_fixture(fixture, rule):
    g = {k[len(rule) + 1:]: v for k, v in fixture.items() if k.startswith(rule + "_")}
    T, stride, K = int(g["T"]), int(g["stride"]), int(g["num_classes"])
    starts, labels, count = W.windows(g["labels"], g["lengths"], T, stride, K, W.RULES[rule])
    assert count == len(g["starts"]) >= 10
    assert starts.tolist() == g["starts"].tolist() and labels.tolist() == g["window_labels"].tolist()
    assert (np.diff(starts) > 0).all()                      # the reference's order is ascending frame order
    # what the reference stored per window is the T consecutive rows at its start
    assert W.gather_rows(g["rows"], starts, T).tobytes() == g["stored"].tobytes()
    assert np.isnan(g["stored"]).any()


def test_fixture_clips_are_what_they_claim_to_be(fixture):
    clips = [str(c) for c in fixture["clips"]]
    for what in ("shorter_than_T", "exactly_T", "T_plus_1", "label_change_mid_clip", "unlabelled_frames_bridged",
                 "no_labelled_frame", "odd_remainder", "last_frame_of_unknown_class"):
        assert any(what in c for c in clips), what
    T = int(fixture["uniform_T"])
    assert T == int(fixture["last_T"]) == 4 and int(fixture["uniform_stride"]) == 1 and int(fixture["last_stride"]) == 2
    lengths = fixture["uniform_lengths"].tolist()
    begin = np.concatenate([[0], np.cumsum(lengths)])
    starts = fixture["uniform_starts"]
    rel = lambda c: (starts[(starts >= begin[c]) & (starts < begin[c + 1])] - begin[c]).tolist()
    assert lengths[0] == T - 1 and rel(0) == []
    assert lengths[1] == T and rel(1) == [0]
    assert lengths[2] == T + 1 and rel(2) == [0, 1]
    assert lengths[3] == 10 and rel(3) == [0, 1, 5, 6]      # A x 5, B x 5
    # frames without a label: eight given, six left, and the windows bridge the gap
    assert fixture["uniform_lengths_given"][4] == 8 and lengths[4] == 6 and rel(4) == [0, 1, 2]
    assert fixture["uniform_lengths_given"][6] == 4 and lengths[6] == 0
    # the caller's filter gives the reference's table: labels, rows and lengths counted over the mask
    given, keep = fixture["uniform_labels_given"], fixture["uniform_labels_given"] >= 0
    assert given[keep].tolist() == fixture["uniform_labels"].tolist()
    assert fixture["uniform_rows_given"][keep].tobytes() == fixture["uniform_rows"].tobytes()
    bounds = np.concatenate([[0], np.cumsum(fixture["uniform_lengths_given"])])
    assert [int(keep[a:b].sum()) for a, b in zip(bounds[:-1], bounds[1:])] == lengths
    # and without the filter the kernel's rule ("no label" = out of range) gives other windows: no bridge
    unfiltered, _, _ = W.windows(given, fixture["uniform_lengths_given"], T, 1, 3, W.UNIFORM)
    assert len(unfiltered) < len(starts)
    # last rule: stride 2 with an odd remainder, an unknown class in the last frame
    lengths = fixture["last_lengths"].tolist()
    begin = np.concatenate([[0], np.cumsum(lengths)])
    starts = fixture["last_starts"]
    assert lengths[3] == 7 and rel(3) == [0, 2]
    assert lengths[4] == 10 and rel(4) == [0, 2, 4, 6]
    assert (fixture["last_labels"][begin[5]:begin[6]] == -1).sum() == 2 and rel(5) == [4]


def test_tile_constants_are_the_kernels():
    src = _source()
    const = lambda name: int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))
    assert (const("SW_SPAN"), const("SW_THREADS"), const("SW_SCAN"), const("SW_MAX_SEQ")) == (W.SPAN, W.THREADS, W.SCAN, W.MAX_SEQ)
    assert const("SW_TRIPS") * W.THREADS == W.SPAN
    assert re.search(r"#define QT_WAVE (\d+)", open(os.path.join(ROOT, PKG, "csrc", "qt_common.h")).read()).group(1) == str(W.WAVE)


@pytest.mark.parametrize("rule", [W.UNIFORM, W.LAST])
def test_kernel_walk_equals_the_plain_loop(rule):
    """counts, scan and scatter in Python, at the kernel's tile sizes and at small ones that make every boundary cheap"""
    K = 5
    sizes = [1, 3, 4, 5, W.SPAN - 1, W.SPAN, W.SPAN + 1, 2 * W.SPAN + 1]
    for n, frames in enumerate(sizes):
        for T, stride in ((1, 1), (4, 2), (10, 3)):
            for clips in (1, 7):
                labels, lengths = W.random_case(100 + n, frames, clips, K)
                want = W.windows(labels, lengths, T, stride, K, rule)
                got = W.kernel_walk(labels, lengths, T, stride, K, rule)
                assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and got[2] == want[2], \
                    (frames, T, stride, clips)
                fast = W.windows_vectorised(labels, lengths, T, stride, K, rule)
                assert fast[0].tolist() == want[0].tolist() and fast[1].tolist() == want[1].tolist() and fast[2] == want[2]
    # small tiles: several spans, several scan trips, a window that reaches over two span edges
    for frames in (1, 15, 16, 17, 33, 16 * 4, 16 * 4 + 1, 16 * 8 + 1, 300):
        for T, stride in ((1, 1), (4, 1), (4, 2), (10, 3), (20, 1)):
            labels, lengths = W.random_case(7 * frames + T, frames, 1 + frames // 40, K, run=12)
            want = W.windows(labels, lengths, T, stride, K, rule)
            got = W.kernel_walk(labels, lengths, T, stride, K, rule, span=16, threads=8, scan=4, wave=4)
            assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and got[2] == want[2], (frames, T)
            assert got[3] == -(-(-(-frames // 16)) // 4)
    # capacity below the count: the first `capacity` windows, the count is the total
    labels, lengths = W.random_case(5, 300, 3, K, run=30, unknown=0.0)
    want = W.windows(labels, lengths, 4, 1, K, rule)
    assert want[2] > 40
    got = W.kernel_walk(labels, lengths, 4, 1, K, rule, capacity=40, span=16, threads=8, scan=4, wave=4)
    assert got[2] == want[2] and got[0].tolist() == want[0][:40].tolist() and got[1].tolist() == want[1][:40].tolist()
    # many one-frame clips, empty clips in between
    lengths = np.array([1, 0] * 50 + [0, 0, 4])
    labels = np.arange(int(lengths.sum())) % K
    labels[-4:] = 2
    for T in (1, 4):
        want = W.windows(labels, lengths, T, 1, K, rule)
        got = W.kernel_walk(labels, lengths, T, 1, K, rule, span=16, threads=8, scan=4, wave=4)
        assert got[0].tolist() == want[0].tolist() and want[2] == (54 if T == 1 else 1)


def test_the_scan_takes_a_second_trip_where_the_gpu_test_says():
    frames = W.SCAN * W.SPAN + 1
    assert -(-frames // W.SPAN) == W.SCAN + 1 and -(-(frames - 1) // W.SPAN) == W.SCAN and frames < (1 << 22)


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    declared = set(re.findall(r"\b(qt_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(os.path.join(ROOT, PKG, "libqtcnn_hip.so"))
    for symbol in ("qt_seq_windows_workspace_bytes", "qt_seq_windows_plan", "qt_seq_gather_rows", "qt_seq_gather_features"):
        assert symbol in declared and hasattr(lib, symbol), symbol
    M = pkg("sequence_windows")
    for struct, cls in (("qt_seq_windows_desc", M.SeqWindowsDesc), ("qt_seq_gather_desc", M.SeqGatherDesc),
                        ("qt_seq_features_desc", M.SeqFeaturesDesc)):
        fields = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", header, re.S).group(1)
        fields = re.sub(r"/\*.*?\*/", "", fields)
        names = re.findall(r"\b(\w+)\s*[,;]", fields)
        assert names == [n for n, _ in cls._fields_], struct
        ctype = {"int": ctypes.c_int, "long long": ctypes.c_longlong}
        types = [ctype[t] for t, _ in re.findall(r"^\s*(int|long long)\s+(\w+);", fields, re.M)]
        assert types == [t for _, t in cls._fields_], struct
    assert "enum { QT_SEQ_LABEL_UNIFORM = 0, QT_SEQ_LABEL_LAST = 1 };" in header
    assert (M.QT_SEQ_LABEL_UNIFORM, M.QT_SEQ_LABEL_LAST) == (W.UNIFORM, W.LAST) == (0, 1)
    P = pkg()
    assert P.SequenceWindows is M.SequenceWindows and P.WindowPlan is M.WindowPlan and P.fit_class_stats is M.fit_class_stats
    assert {"SequenceWindows", "WindowPlan", "fit_class_stats"} <= set(P.__all__)
    for doc in ("INTEGRATION.md", os.path.join(PKG, "pose_sequence.py")):
        assert "Not built: class-mean and standardize imputation" not in re.sub(r"\s+", " ", open(os.path.join(ROOT, doc)).read())


def _lib():
    M = pkg("sequence_windows")
    L = pkg("_lib").lib()
    return M, L


def test_plan_argument_checks_need_no_device():
    """every refusal below comes before the first device call: the pointers are never dereferenced"""
    M, L = _lib()
    D = M.SeqWindowsDesc
    labels, offsets, starts, out, count, ws = (0x10000 * k for k in range(1, 7))

    def call(desc, labels=labels, offsets=offsets, starts=starts, out=out, count=count, ws=ws, ws_bytes=1 << 20):
        return L.qt_seq_windows_plan(ctypes.byref(desc), labels, offsets, starts, out, count, ws, ws_bytes, None)

    good = D(5000, 3, 4, 2, 12, 100, W.LAST)
    assert L.qt_seq_windows_workspace_bytes(ctypes.byref(good)) == 4 * 5
    assert L.qt_seq_windows_workspace_bytes(ctypes.byref(D(W.SPAN, 1, 4, 1, 2, 1, 0))) == 4
    assert L.qt_seq_windows_workspace_bytes(ctypes.byref(D(W.SPAN + 1, 1, 4, 1, 2, 1, 0))) == 8
    assert L.qt_seq_windows_plan(None, labels, offsets, starts, out, count, ws, 64, None) == QT_ERR_INVALID_ARG
    for bad in (D(0, 3, 4, 2, 12, 100, 1), D(-5, 3, 4, 2, 12, 100, 1), D(5000, 0, 4, 2, 12, 100, 1), D(5000, 3, 4, 2, 0, 100, 1),
                D(5000, 3, 4, 2, 12, 0, 1), D(5000, 3, 4, 2, 12, -1, 1)):
        assert call(bad) == QT_ERR_INVALID_ARG and b"positive" in L.qt_last_error()
        assert L.qt_seq_windows_workspace_bytes(ctypes.byref(bad)) == 0
    for T in (0, -1, 65, 1000):
        assert call(D(5000, 3, T, 2, 12, 100, 1)) == QT_ERR_INVALID_ARG and b"seq_len" in L.qt_last_error()
    for stride in (0, -2):
        assert call(D(5000, 3, 4, stride, 12, 100, 1)) == QT_ERR_INVALID_ARG and b"stride" in L.qt_last_error()
    for rule in (-1, 2, 7):
        assert call(D(5000, 3, 4, 2, 12, 100, rule)) == QT_ERR_INVALID_ARG and b"rule" in L.qt_last_error()
    assert call(D((1 << 22) + 1, 3, 4, 2, 12, 100, 1)) == QT_ERR_UNSUPPORTED and b"frames" in L.qt_last_error()
    assert L.qt_seq_windows_workspace_bytes(ctypes.byref(D((1 << 22) + 1, 3, 4, 2, 12, 100, 1))) == 0
    assert L.qt_seq_windows_workspace_bytes(ctypes.byref(D(1 << 22, 3, 4, 2, 12, 100, 1))) == 4 * 4096
    for name in ("labels", "offsets", "starts", "out", "count", "ws"):
        assert call(good, **{name: None}) == QT_ERR_INVALID_ARG and b"null" in L.qt_last_error(), name
    for name, off in (("labels", 4), ("out", 4), ("offsets", 2), ("starts", 1), ("count", 2), ("ws", 3)):
        assert call(good, **{name: 0x10000 + off}) == QT_ERR_INVALID_ARG and b"aligned" in L.qt_last_error(), name
    assert call(good, ws_bytes=4 * 5 - 1) == QT_ERR_INVALID_ARG and b"workspace" in L.qt_last_error()
    assert call(good, ws_bytes=0) == QT_ERR_INVALID_ARG


def test_gather_argument_checks_need_no_device():
    M, L = _lib()
    R, F = M.SeqGatherDesc, M.SeqFeaturesDesc
    src, starts, dst, labels, means, stds = (0x10000000 * k for k in range(1, 7))

    def rows(desc, src=src, starts=starts, dst=dst):
        return L.qt_seq_gather_rows(ctypes.byref(desc), src, starts, dst, None)

    good = R(100, 188, 8, 4)
    assert L.qt_seq_gather_rows(None, src, starts, dst, None) == QT_ERR_INVALID_ARG
    for bad in (R(0, 188, 8, 4), R(100, 0, 8, 4), R(100, -3, 8, 4), R(100, 188, 0, 4), R(-1, 188, 8, 4)):
        assert rows(bad) == QT_ERR_INVALID_ARG and b"positive" in L.qt_last_error()
    for T in (0, 65):
        assert rows(R(100, 188, 8, T)) == QT_ERR_INVALID_ARG and b"seq_len" in L.qt_last_error()
    assert rows(R(1 << 31, 188, 8, 4)) == QT_ERR_UNSUPPORTED
    for name in ("src", "starts", "dst"):
        assert rows(good, **{name: None}) == QT_ERR_INVALID_ARG and b"null" in L.qt_last_error()
    assert rows(good, starts=starts + 2) == QT_ERR_INVALID_ARG and b"4-byte" in L.qt_last_error()
    assert rows(good, dst=src + 100 * 188 - 1) == QT_ERR_INVALID_ARG and b"overlap" in L.qt_last_error()
    assert rows(good, dst=src - 8 * 4 * 188 + 1) == QT_ERR_INVALID_ARG and b"overlap" in L.qt_last_error()

    def feats(desc, raw=src, starts=starts, labels=labels, means=means, stds=stds, out=dst):
        return L.qt_seq_gather_features(ctypes.byref(desc), raw, starts, labels, means, stds, out, None)

    good = F(100, 47, 8, 4, 3, 12)
    assert L.qt_seq_gather_features(None, src, starts, labels, means, stds, dst, None) == QT_ERR_INVALID_ARG
    for bad in (F(0, 47, 8, 4, 3, 12), F(100, 47, 0, 4, 3, 12)):
        assert feats(bad) == QT_ERR_INVALID_ARG and b"positive" in L.qt_last_error()
    for width in (0, -1, 1025):
        assert feats(F(100, width, 8, 4, 3, 12)) == QT_ERR_INVALID_ARG and b"features" in L.qt_last_error()
    for T in (0, 65):
        assert feats(F(100, 47, 8, T, 3, 12)) == QT_ERR_INVALID_ARG and b"seq_len" in L.qt_last_error()
    for mode in (-1, 4, 9):
        assert feats(F(100, 47, 8, 4, mode, 12)) == QT_ERR_INVALID_ARG and b"mode" in L.qt_last_error()
    assert feats(F(1 << 31, 47, 8, 4, 3, 12)) == QT_ERR_UNSUPPORTED
    for name in ("raw", "starts", "out"):
        assert feats(good, **{name: None}) == QT_ERR_INVALID_ARG and b"null" in L.qt_last_error()
    for name, off in (("raw", 2), ("starts", 1), ("out", 3), ("means", 2), ("stds", 1), ("labels", 4)):
        base = dict(raw=src, starts=starts, out=dst, means=means, stds=stds, labels=labels)[name]
        assert feats(good, **{name: base + off}) == QT_ERR_INVALID_ARG and b"aligned" in L.qt_last_error(), name
    # a class mode without its tables
    for mode, missing in ((2, "labels"), (2, "means"), (3, "means"), (3, "stds"), (3, "labels")):
        assert feats(F(100, 47, 8, 4, mode, 12), **{missing: None}) == QT_ERR_INVALID_ARG, (mode, missing)
        assert b"needs" in L.qt_last_error()
    assert feats(F(100, 47, 8, 4, 3, 0)) == QT_ERR_INVALID_ARG and b"num_classes" in L.qt_last_error()
    assert feats(good, out=src + 4 * 47) == QT_ERR_INVALID_ARG and b"overlap" in L.qt_last_error()


def test_module_refusals_need_no_device():
    P = pkg()
    for bad in (dict(seq_len=0), dict(seq_len=65), dict(seq_len=4, stride=0), dict(seq_len=4, label="first"),
                dict(seq_len=4, num_classes=None), dict(seq_len=4, num_classes=0)):
        with pytest.raises(ValueError):
            P.SequenceWindows(**{"num_classes": 3, **bad})
    win = P.SequenceWindows(seq_len=4, stride=2, label="last", num_classes=3)
    assert (win.seq_len, win.stride, win.label, win.num_classes) == (4, 2, "last", 3)
    labels = torch.zeros(10, dtype=torch.int64)
    for lengths in ([4, 5], [11], [12, -2], [], torch.tensor([4.0, 6.0]), torch.tensor([[4, 6]])):
        with pytest.raises(ValueError):
            win.plan(labels, lengths)
    # no torch fallback
    with pytest.raises(P.QtError, match="AMD GPU"):
        win.plan(labels, [4, 6])
    with pytest.raises(P.QtError, match="AMD GPU"):
        win.plan(labels, torch.tensor([4, 6]))
    with pytest.raises(P.QtError, match="int64"):
        win.plan(labels.int(), [4, 6])
    with pytest.raises(P.QtError, match="tensor"):
        win.plan(np.zeros(10, np.int64), [4, 6])
    with pytest.raises(P.QtError, match="AMD GPU"):
        win.gather(torch.zeros(10, 3, dtype=torch.uint8), None, None)
    with pytest.raises(P.QtError, match="AMD GPU"):
        win.gather_features(torch.zeros(10, 47), None, None)
    with pytest.raises(P.QtError, match="float32"):
        win.gather_features(torch.zeros(10, 47, dtype=torch.float64), None, None)
    with pytest.raises(ValueError, match="mode"):
        win.gather_features(torch.zeros(10, 47), None, None, mode="mean")
    with pytest.raises(ValueError, match="means"):
        win.gather_features(torch.zeros(10, 47), None, None, mode="class_mean")
    with pytest.raises(ValueError, match="stds"):
        win.gather_features(torch.zeros(10, 47), None, None, mode="standardize", means=torch.zeros(3, 47))
    with pytest.raises(P.QtError, match="AMD GPU"):
        P.fit_class_stats(torch.zeros(10, 443), labels, 3)
    with pytest.raises(P.QtError, match="AMD GPU"):
        P.PoseFeatures.fit(torch.zeros(10, 47), labels, 3)
    M = pkg("sequence_windows")
    assert M.candidate_count([3, 4, 5, 7, 0], 4, 2) == W.candidate_count([3, 4, 5, 7, 0], 4, 2) == 0 + 1 + 1 + 2 + 0
