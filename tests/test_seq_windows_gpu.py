"""Sequence windows on the GPU (csrc/seq_windows.hip, <pkg>/sequence_windows.py): qt_seq_windows_plan against the plain loops
of tests/_seq_windows_ref.py on the fixture and on seeded random clips at the sizes where the spans, the scan's trips and the
capacity can go wrong; qt_seq_gather_rows byte for byte against numpy at every alignment of source and destination;
qt_seq_gather_features against the bound of tests/_pose_ref.py::impute and bit for bit against qt_pose_features; the Python
class end to end into CnnLstm.  Every buffer sits between poisoned guard bands (tests/_guard.py)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import _pose_ref as R
import _seq_windows_ref as W
from _guard import POISON, Guard
from _util import ROOT, pkg

pytestmark = pytest.mark.gpu
K = 5              # classes of the seeded cases


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "seq_windows.npz"))
    return {k: g[k] for k in g.files}


def _api():
    M, Lm = pkg("sequence_windows"), pkg("_lib")
    return M, Lm, Lm.lib()


# ---- the plan -------------------------------------------------------------------------------------------------------------------
def run_plan(dev, labels, lengths, T, stride, num_classes, rule, capacity=None):
    """qt_seq_windows_plan through ctypes, every buffer guarded, the workspace exactly what the query says.  Returns (starts,
    labels, count, the bytes of both output payloads); asserts that elements at and behind min(count, capacity) were not
    written."""
    M, Lm, L = _api()
    labels = np.ascontiguousarray(labels, dtype=np.int64)
    capacity = W.candidate_count(lengths, T, stride) if capacity is None else capacity
    assert capacity >= 1
    G = Guard(dev)
    # ([n,1]: the guard sizes its bands from the last dimension, and 64 KiB on either side is what these need)
    d_labels = G.input("labels", torch.from_numpy(labels).reshape(-1, 1))
    d_offsets = G.input("clip_offsets", torch.from_numpy(W.offsets_of(lengths)).reshape(-1, 1))
    starts = G.output("starts", (capacity, 1), torch.int32)
    out = G.output("window_labels", (capacity, 1), torch.int64)
    count = G.output("count", (1,), torch.int32)
    desc = M.SeqWindowsDesc(len(labels), len(lengths), T, stride, num_classes, capacity, rule)
    nbytes = L.qt_seq_windows_workspace_bytes(ctypes.byref(desc))
    assert nbytes == 4 * -(-len(labels) // W.SPAN)
    ws = G.workspace("workspace", nbytes)
    Lm.check(L.qt_seq_windows_plan(ctypes.byref(desc), Lm.ptr(d_labels), Lm.ptr(d_offsets), Lm.ptr(starts), Lm.ptr(out),
                                   Lm.ptr(count), Lm.ptr(ws), nbytes, Lm.stream_ptr()), "qt_seq_windows_plan")
    G.check()
    n = int(count.item())
    keep = min(n, capacity)
    s_bytes, l_bytes = starts.view(torch.uint8).cpu().numpy(), out.view(torch.uint8).cpu().numpy()
    assert (s_bytes[4 * keep:] == POISON).all() and (l_bytes[8 * keep:] == POISON).all(), "written at or behind count"
    return starts[:keep, 0].cpu().numpy(), out[:keep, 0].cpu().numpy(), n, s_bytes.tobytes() + l_bytes.tobytes()


def _reference(labels, lengths, T, stride, rule, capacity=None):
    """the plain loop; its vectorised form (held equal to it by tests/test_seq_windows_cpu.py) where the loop takes seconds"""
    f = W.windows if len(labels) <= 4096 else W.windows_vectorised
    return f(labels, lengths, T, stride, K, rule, capacity)


def _same(got, want, what):
    assert got[2] == want[2], (what, "count", got[2], want[2])
    assert got[0].dtype == np.int32 and got[1].dtype == np.int64
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what


@pytest.mark.parametrize("rule", ["uniform", "last"])
def test_plan_gives_the_fixture_back(rule):
    dev = _dev()
    g = {k[len(rule) + 1:]: v for k, v in fixture().items() if k.startswith(rule + "_")}
    got = run_plan(dev, g["labels"], g["lengths"], int(g["T"]), int(g["stride"]), int(g["num_classes"]), W.RULES[rule])
    assert got[2] == len(g["starts"]) and np.array_equal(got[0], g["starts"]) and np.array_equal(got[1], g["window_labels"])


# 1, T - 1, T, T + 1 for T in {1, 4, 10}; one span - 1 / exact / + 1; two spans + 1; the scan's second trip
FRAMES = [1, 3, 4, 5, 9, 10, 11, W.SPAN - 1, W.SPAN, W.SPAN + 1, 2 * W.SPAN + 1, W.SCAN * W.SPAN + 1]


@pytest.mark.parametrize("frames", FRAMES)
def test_plan_random_clips(frames):
    """both rules, stride 1, 2, 3 and T 1, 4, 10 at every size; clips of about 37 frames, some empty"""
    dev = _dev()
    labels, lengths = W.random_case(1000 + frames, frames, max(1, frames // 37), K)
    second_trip = frames == W.SCAN * W.SPAN + 1
    if second_trip:        # the one frame of the last span, partial[SW_SCAN], is a kept start at T = 1 under every stride
        _, lengths = W.random_case(1000 + frames, frames - 13, frames // 37, K)
        lengths = np.concatenate([lengths, [13]])
        labels[-13:] = 2
    ran = 0
    for rule in (W.UNIFORM, W.LAST):
        for stride in (1, 2, 3):
            for T in (1, 4, 10):
                if W.candidate_count(lengths, T, stride) == 0:
                    continue                   # no clip reaches T frames: capacity 0 is the module's case, not the kernel's
                want = _reference(labels, lengths, T, stride, rule)
                _same(run_plan(dev, labels, lengths, T, stride, K, rule), want, (frames, rule, stride, T))
                assert not (second_trip and T == 1) or want[0][-1] == frames - 1
                ran += 1
    assert ran >= (6 if frames < 10 else 18)


def test_plan_single_clip_one_frame_clips_and_capacity():
    dev = _dev()
    frames = 2 * W.SPAN + 1
    labels, _ = W.random_case(77, frames, 1, K, run=40, unknown=0.02)
    for rule in (W.UNIFORM, W.LAST):
        one = [frames]
        want = _reference(labels, one, 4, 1, rule)
        got = run_plan(dev, labels, one, 4, 1, K, rule)
        _same(got, want, "single clip")
        assert want[2] > 1000
        again = run_plan(dev, labels, one, 4, 1, K, rule)
        assert again[3] == got[3]              # the same bytes on every run, unwritten elements included
        # capacity below the count: the first `capacity` windows, the total in count, bands and the rest untouched
        for capacity in (1, 1000, want[2] - 1):
            _same(run_plan(dev, labels, one, 4, 1, K, rule, capacity=capacity), _reference(labels, one, 4, 1, rule, capacity),
                  ("capacity", capacity))
        # many one-frame clips: every frame is a window at T = 1, none at T = 4 (one candidate in a last clip of four)
        ones = [1] * (frames - 4) + [4]
        _same(run_plan(dev, labels, ones, 1, 1, K, rule), _reference(labels, ones, 1, 1, rule), "one-frame clips, T 1")
        _same(run_plan(dev, labels, ones, 4, 1, K, rule), _reference(labels, ones, 4, 1, rule), "one-frame clips, T 4")
        # empty clips between the others
        gaps = [0, 700, 0, 0, frames - 700, 0]
        _same(run_plan(dev, labels, gaps, 10, 3, K, rule), _reference(labels, gaps, 10, 3, rule), "empty clips")


# ---- gather_rows ----------------------------------------------------------------------------------------------------------------
def run_rows(dev, src, starts, T, src_shift=0, dst_shift=0, fill=POISON):
    """qt_seq_gather_rows through ctypes on a uint8 source [N,row_bytes]; source and destination start `shift` bytes off a
    256-byte boundary.  Returns uint8 [B,T,row_bytes]."""
    M, Lm, L = _api()
    N, row_bytes = src.shape
    G = Guard(dev)
    d_src = G.input("src", torch.from_numpy(np.array(src)).reshape(-1, 1), offset=src_shift)
    d_starts = G.input("starts", torch.from_numpy(np.array(starts, dtype=np.int32)))
    dst = G.output("dst", (len(starts) * T * row_bytes, 1), torch.uint8, fill=fill, offset=dst_shift)
    assert d_src.data_ptr() % 256 == src_shift and dst.data_ptr() % 256 == dst_shift
    desc = M.SeqGatherDesc(N, row_bytes, len(starts), T)
    Lm.check(L.qt_seq_gather_rows(ctypes.byref(desc), Lm.ptr(d_src), Lm.ptr(d_starts), Lm.ptr(dst), Lm.stream_ptr()),
             "qt_seq_gather_rows")
    G.check()                                  # bands intact, the source unchanged
    return dst.cpu().numpy().reshape(len(starts), T, row_bytes)


@functools.lru_cache(maxsize=None)
def byte_rows(row_bytes, N=7):
    rows = np.random.default_rng(row_bytes).integers(0, 255, (N, row_bytes), dtype=np.uint8)     # (no 0xFF: a fill shows)
    rows.setflags(write=False)
    return rows


@pytest.mark.parametrize("row_bytes", [1, 3, 4, 16, 188, 1772, 150528, 150529])
def test_gather_rows_every_alignment(row_bytes):
    """source and destination 0 .. 3 bytes off a 256-byte boundary each: units of 16 bytes (equal shifts, 16-byte rows), of 4
    bytes (equal shifts, rows of 4, 188, 1772 bytes at starts that are no multiple of 4 rows) and single bytes, every head and
    tail length; the first and the last possible start, duplicates"""
    dev = _dev()
    src = byte_rows(row_bytes)
    N = src.shape[0]
    for T in (1, 4):
        starts = [0, N - T, 1, 1, N - T, 2]
        want = W.gather_rows(src, starts, T)
        for s in range(4):
            for d in range(4):
                got = run_rows(dev, src, starts, T, s, d)
                assert got.tobytes() == want.tobytes(), (T, s, d)


@pytest.mark.parametrize("row_bytes", [3, 188, 150529])
def test_gather_rows_start_out_of_range(row_bytes):
    """-1 and src_rows - T + 1 give 0xFF windows between untouched neighbours, whatever the output held before"""
    dev = _dev()
    src = byte_rows(row_bytes)
    N, T = src.shape[0], 4
    starts = [1, -1, 0, N - T + 1, N - T, -(1 << 31), (1 << 31) - 1, 2]
    want = W.gather_rows(src, starts, T)
    assert (want[[1, 3, 5, 6]] == 0xFF).all() and (want[[0, 2, 4, 7]] != 0xFF).all()
    for fill in (POISON, 0x00):
        for d in (0, 1, 3):
            assert run_rows(dev, src, starts, T, 0, d, fill).tobytes() == want.tobytes(), (fill, d)


# ---- gather_features ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def feature_case(F, N=41, T=4):
    """seeded rows with about 20 % NaNs, tables with one flat column (std < 1e-6) per class, windows with the first and last
    start and a duplicate, one out-of-range start, one out-of-range label"""
    rng = np.random.default_rng(500 + F)
    raw = (rng.standard_normal((N, F)) * 3).astype(np.float32)
    raw[rng.random((N, F)) < 0.2] = np.nan
    means = rng.standard_normal((K, F)).astype(np.float32)
    stds = (0.5 + rng.random((K, F))).astype(np.float32)
    stds[np.arange(K), rng.integers(0, F, K)] = np.float32(5e-7)
    stds[0, 0] = np.float32(0)
    starts = np.array([0, N - T, 3, 3, 17, N - T + 1, 9, 30], dtype=np.int32)
    labels = np.array([0, 1, 2, 3, 4, 1, K, 0], dtype=np.int64)       # window 5: no rows; window 6: no class
    for a in (raw, means, stds, starts, labels):
        a.setflags(write=False)
    return raw, means, stds, starts, labels


def run_features(dev, raw, starts, T, mode, labels=None, means=None, stds=None, shift=0):
    M, Lm, L = _api()
    N, F = raw.shape
    G = Guard(dev)
    t = lambda name, a: None if a is None else G.input(name, torch.from_numpy(np.array(a)))
    d_raw, d_starts, d_labels, d_means, d_stds = t("raw", raw), t("starts", starts), t("labels", labels), t("means", means), t("stds", stds)
    out = G.output("out", (len(starts), T, F), torch.float32, offset=shift, written=False)
    desc = M.SeqFeaturesDesc(N, F, len(starts), T, mode, 0 if means is None else means.shape[0])
    Lm.check(L.qt_seq_gather_features(ctypes.byref(desc), Lm.ptr(d_raw), Lm.ptr(d_starts), Lm.ptr(d_labels), Lm.ptr(d_means),
                                      Lm.ptr(d_stds), Lm.ptr(out), Lm.stream_ptr()), "qt_seq_gather_features")
    G.check()
    return out.cpu().numpy()


def _tables(mode, labels, means, stds):
    return (labels if mode >= R.CLASS_MEAN else None, means if mode >= R.CLASS_MEAN else None,
            stds if mode == R.STANDARDIZE else None)


@pytest.mark.parametrize("F", [1, 5, 47, 443])
def test_gather_features_within_the_bound_of_impute(F):
    dev = _dev()
    raw, means, stds, starts, labels = feature_case(F)
    T = 4
    rows = W.gather_rows(raw, starts, T)                                  # [B,T,F], window 5 NaN (0xFF bytes)
    B = len(starts)
    for mode in (R.RAW, R.ZERO, R.CLASS_MEAN, R.STANDARDIZE):
        want, bound = R.impute(rows.reshape(B * T, F), np.zeros((B * T, F)), mode, labels, means, stds, rows_per_label=T)
        want, bound = want.reshape(B, T, F), bound.reshape(B, T, F)
        want[5] = np.nan                                                  # an out-of-range start is NaN in every mode
        bound[5] = 0
        for shift in range(4):
            got = run_features(dev, raw, starts, T, mode, *_tables(mode, labels, means, stds), shift=shift)
            assert np.array_equal(np.isnan(got), np.isnan(want)), (mode, shift, "NaN positions")
            live = ~np.isnan(want)
            err = np.abs(got.astype(np.float64) - want)[live]
            assert (err <= bound[live]).all(), (mode, shift, float((err - bound[live]).max()))
            if shift == 0:
                first = got
            assert got.tobytes() == first.tobytes(), (mode, shift)        # the bits do not depend on the alignment
        if mode >= R.CLASS_MEAN:
            assert np.isnan(got[6]).all() and not np.isnan(got[[0, 1, 2, 3, 4, 7]]).any()
        if mode == R.STANDARDIZE:
            flat = stds[labels[0]] < np.float32(1e-6)
            assert flat.any() and (got[0][:, flat] == 0).all()
        if mode == R.RAW:                                                 # the same bytes as qt_seq_gather_rows
            as_rows = run_rows(dev, np.ascontiguousarray(raw).view(np.uint8).reshape(raw.shape[0], 4 * F), starts, T)
            assert got.tobytes() == as_rows.tobytes() and np.isnan(got).mean() > 0.15
        assert (got[5].view(np.uint32) == 0xFFFFFFFF).all()


def test_gather_features_47_is_bitwise_qt_pose_features():
    """every mode against qt_pose_features (stored vectors, rows_per_label = T) on the host-gathered rows; the window without
    rows is left out (there is nothing to hand to qt_pose_features for it), the one without a class is in"""
    dev = _dev()
    P = pkg()
    raw, means, stds, starts, labels = feature_case(47)
    T = 4
    keep = [0, 1, 2, 3, 4, 6, 7]
    rows = torch.from_numpy(W.gather_rows(raw, starts[keep], T)).to(dev)
    d_means, d_stds, d_labels = (torch.from_numpy(np.array(a)).to(dev) for a in (means, stds, labels[keep]))
    for mode, name in ((R.RAW, "raw"), (R.ZERO, "zero"), (R.CLASS_MEAN, "class_mean"), (R.STANDARDIZE, "standardize")):
        want = P.PoseFeatures(name, d_means if mode >= R.CLASS_MEAN else None,
                              d_stds if mode == R.STANDARDIZE else None).impute(rows, d_labels)
        got = run_features(dev, raw, starts, T, mode, *_tables(mode, labels, means, stds))
        assert got[keep].tobytes() == want.cpu().numpy().tobytes(), name


def test_fit_class_stats():
    dev = _dev()
    P = pkg()
    rng = np.random.default_rng(9)
    N = 300
    labels = rng.integers(-1, K + 1, N)                                   # some outside [0, K)
    labels[labels == 3] = 2                                               # class 3 has no row: mean 0, std 1
    d_labels = torch.from_numpy(labels).to(dev)
    for F in (47, 443):
        raw = (rng.standard_normal((N, F)) * 2 + 1).astype(np.float32)
        raw[rng.random((N, F)) < 0.2] = np.nan
        raw[labels == 1, 0] = np.nan                                      # a cell without a value
        mean, std = P.fit_class_stats(torch.from_numpy(raw).to(dev), d_labels, K)
        assert mean.dtype == std.dtype == torch.float32 and tuple(mean.shape) == tuple(std.shape) == (K, F)
        if F == 47:
            m47, s47 = P.PoseFeatures.fit(torch.from_numpy(raw).to(dev), d_labels, K)
            assert torch.equal(mean, m47) and torch.equal(std, s47)
        # float64 restatement.  The module's float64 result, before it is rounded to f32, must lie within 1e-12 relative of
        # this one; what is compared is its f32 rounding, half an ulp (2^-24 relative) further away at the most.
        want_m, want_s = np.zeros((K, F)), np.ones((K, F))
        for k in range(K):
            v = raw[labels == k].astype(np.float64)
            for c in range(F):
                col = v[:, c][~np.isnan(v[:, c])]
                if len(col):
                    want_m[k, c] = col.mean()
                    want_s[k, c] = np.sqrt(((col - col.mean()) ** 2).mean()) + 1e-6
        for got, want in ((mean, want_m), (std, want_s)):
            err = np.abs(got.cpu().numpy().astype(np.float64) - want)
            assert (err <= (2.0 ** -24 + 1e-12) * np.abs(want) + 1e-300).all(), (F, float(err.max()))
        assert want_m[3].tolist() == [0.0] * F and want_m[1, 0] == 0 and want_s[1, 0] == 1


# ---- the Python class -----------------------------------------------------------------------------------------------------------
def test_the_python_class_on_the_fixture():
    dev = _dev()
    P = pkg()
    g = fixture()
    for rule in ("uniform", "last"):
        T, stride, C = int(g[f"{rule}_T"]), int(g[f"{rule}_stride"]), int(g[f"{rule}_num_classes"])
        win = P.SequenceWindows(seq_len=T, stride=stride, label=rule, num_classes=C)
        labels = torch.from_numpy(g[f"{rule}_labels"]).to(dev)
        lengths = g[f"{rule}_lengths"].tolist()
        plan = win.plan(labels, lengths if rule == "uniform" else torch.tensor(lengths))
        assert plan.capacity == W.candidate_count(lengths, T, stride)
        assert plan.count == len(plan) == len(g[f"{rule}_starts"])
        assert plan.starts.dtype == torch.int32 and plan.labels.dtype == torch.int64 and plan.starts.device == dev
        assert plan.starts.tolist() == g[f"{rule}_starts"].tolist() and plan.labels.tolist() == g[f"{rule}_window_labels"].tolist()
        # what the reference stored per window: all windows, then the loader's shuffle; no host synchronisation in a gather
        rows = torch.from_numpy(g[f"{rule}_rows"]).to(dev)                # f64 [N,5] / f32 [N,47]
        idx = torch.randperm(plan.count, device=dev, generator=torch.Generator(dev).manual_seed(3))[:5]
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            everything = win.gather(rows, plan, torch.arange(plan.count, device=dev))
            some = win.gather(rows, plan, idx)
            into = torch.empty_like(some)
            assert win.gather(rows, plan, idx.int(), out=into) is into
            if rule == "last":
                raw = win.gather_features(rows, plan, idx, mode="raw")
                zero = win.gather_features(rows, plan, idx, mode="zero")
        finally:
            torch.cuda.set_sync_debug_mode("default")
        stored = g[f"{rule}_stored"]
        assert everything.cpu().numpy().tobytes() == stored.tobytes() and everything.dtype == rows.dtype
        assert some.cpu().numpy().tobytes() == stored[idx.cpu().numpy()].tobytes() and torch.equal(into.view(torch.uint8), some.view(torch.uint8))
        if rule == "last":
            assert raw.cpu().numpy().tobytes() == some.cpu().numpy().tobytes()
            assert torch.equal(zero, torch.nan_to_num(some, nan=0.0)) and bool(torch.isnan(some).any())
            means, stds = P.fit_class_stats(rows, labels, C)
            got = win.gather_features(rows, plan, idx, mode="standardize", means=means, stds=stds)
            want = P.PoseFeatures("standardize", means, stds).impute(some, plan.labels[idx])
            assert torch.equal(got, want) and tuple(got.shape) == (5, T, 47)
            # errors
            with pytest.raises(P.QtError, match="frames"):
                win.gather(rows[:-1], plan, idx)
            with pytest.raises(P.QtError, match="contiguous"):
                win.gather(rows.t().contiguous().t(), plan, idx)
            with pytest.raises(P.QtError, match="out must be"):
                win.gather(rows, plan, idx, out=torch.empty(5, T, 46, device=dev))
            with pytest.raises(P.QtError, match="idx"):
                win.gather(rows, plan, idx.float())
            with pytest.raises(P.QtError, match="cuda"):
                win.gather(rows, plan, idx.cpu())
            with pytest.raises(P.QtError, match="seq_len"):
                P.SequenceWindows(seq_len=3, num_classes=C).gather(rows, plan, idx)
            with pytest.raises(P.QtError, match="means must be"):
                win.gather_features(rows, plan, idx, mode="class_mean", means=means[:, :40].contiguous())
            with pytest.raises(P.QtError, match="one shape"):
                win.gather_features(rows, plan, idx, mode="standardize", means=means, stds=stds[:1])
    # a dataset without a window: no device call, an empty plan
    win = P.SequenceWindows(seq_len=10, num_classes=3)
    empty = win.plan(torch.zeros(12, dtype=torch.int64, device=dev), [4, 4, 4])
    assert empty.count == 0 and tuple(empty.starts.shape) == (0,) and empty.labels.dtype == torch.int64
    with pytest.raises(P.QtError, match="no windows"):
        win.gather(torch.zeros(12, 3, device=dev), empty, torch.zeros(1, dtype=torch.int64, device=dev))
    with pytest.raises(P.QtError, match="frames"):
        win.plan(torch.zeros((1 << 22) + 1, dtype=torch.int64, device=dev), [(1 << 22) + 1])


def test_end_to_end_into_the_sequence_models():
    """three clips of 64 x 48 uint8 frames, T 4, stride 2: gather -> FramePreprocessor -> CnnLstm in eval() gives the logits of
    the same windows assembled on the host, bit for bit; Quadtree3DCNN takes the batch as it is"""
    dev = _dev()
    P, synth = pkg(), pkg("synth")
    T, C = 4, 12
    lengths = [7, 4, 10]
    N = sum(lengths)
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (N, 48, 64, 3), dtype=np.uint8)
    pose = synth.synth_pose_features(N, salt=5).numpy().astype(np.float32)
    pose[rng.random(pose.shape) < 0.1] = np.nan
    labels = rng.integers(0, C, N)
    win = P.SequenceWindows(seq_len=T, stride=2, label="last", num_classes=C)
    plan = win.plan(torch.from_numpy(labels).to(dev), lengths)
    want_starts, want_labels, count = W.windows(labels, lengths, T, 2, C, W.LAST)
    assert plan.count == count == 2 + 1 + 4 and plan.starts.tolist() == want_starts.tolist()
    idx = torch.tensor([5, 0, 3, 3, 6, 1], device=dev)
    clips = win.gather(torch.from_numpy(frames).to(dev), plan, idx)
    numer = win.gather_features(torch.from_numpy(pose).to(dev), plan, idx, mode="zero")
    assert tuple(clips.shape) == (6, T, 48, 64, 3) and clips.dtype == torch.uint8 and tuple(numer.shape) == (6, T, 47)
    assert plan.labels[idx].tolist() == want_labels[idx.cpu().numpy()].tolist()
    host = want_starts[idx.cpu().numpy()]
    host_clips = torch.from_numpy(W.gather_rows(frames, host, T)).to(dev)
    host_numer = torch.from_numpy(np.nan_to_num(W.gather_rows(pose, host, T), nan=0.0)).to(dev)
    assert torch.equal(clips, host_clips) and torch.equal(numer, host_numer)
    pre = P.FramePreprocessor()
    model = P.CnnLstm(C, sequence_length=T, dropout_rate=0.0, pretrained=False)
    model.load_state_dict(synth.synth_state_dict(model))
    model = model.to(dev).eval()
    with torch.no_grad():
        got = model(pre(clips), numer)
        want = model(pre(host_clips), host_numer)
    assert tuple(got.shape) == (6, C) and bool(torch.isfinite(got).all()) and torch.equal(got, want)
    clip_model = P.Quadtree3DCNN(C, sequence_length=T, dropout_rate=0.0)
    clip_model.load_state_dict(synth.synth_state_dict(clip_model))
    clip_model = clip_model.to(dev).eval()
    with torch.no_grad():
        out = clip_model(pre(clips[:2]), numer[:2])
    assert tuple(out.shape) == (2, C) and bool(torch.isfinite(out).all())
