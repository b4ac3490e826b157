"""Sequence pose features on the GPU (csrc/pose_seq.hip, <pkg>/pose_sequence.py): qt_pose_sequence_features against the float64
rule and the derived bound of tests/_pose_seq_ref.py on the fixture and on seeded random clips, at the sizes where the tiling,
the backward search for the predecessors, the history carried between calls and the heads and tails of the 1772-byte rows
can go wrong.  Every buffer sits between poisoned guard bands (tests/_guard.py)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import _pose_seq_ref as S
from _guard import Guard
from _util import ROOT, pkg, rel_err

pytestmark = pytest.mark.gpu
R = S.TILE         # frames per workgroup


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "pose_seq.npz"))
    return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def random_clips(batch, frames, size=(640, 480)):
    """seeded random clips with about 30 % of the frames undetected and their reference, computed once and shared (never
    written)"""
    lm, det = S.make_clips(batch, frames, seed=S.SEED + 100 * batch + frames, undetected=0.3)
    ref, bound, excluded, end, end_count = S.features(lm, det, size)
    for a in (lm, det, ref, bound, excluded, end, end_count):
        a.setflags(write=False)
    return lm, det, ref, bound, excluded, end, end_count


def run(dev, lm, det=None, size=(640, 480), sizes=None, mode=S.RAW, hist=None, carry=False, shift=0):
    """qt_pose_sequence_features through ctypes.  lm: f32 [B,T,33,4]; hist: None or (frames [B,2,33,4], counts [B]); carry:
    ask for the history after the call.  The output starts `shift` floats off a 256-byte boundary (shift 1, 2, 3: a head of
    3, 2, 1 single floats); outputs lie between poisoned bands that must stay as they are, the inputs (hist_in included) must
    not be written, and in mode zero every output element must have been written.  Returns (out [B,T,443], history or
    None)."""
    M, Lm = pkg("pose_sequence"), pkg("_lib")
    L = Lm.lib()
    B, T = lm.shape[:2]
    G = Guard(dev)
    t = lambda name, a, dt=None: None if a is None else G.input(name, torch.from_numpy(np.array(a, dtype=dt)))
    d_lm, d_det, d_sizes = t("landmarks", lm), t("detected", det, np.uint8), t("sizes", sizes, np.int32)
    d_hin, d_cin = (None, None) if hist is None else (t("hist_in", hist[0]), t("hist_count_in", hist[1], np.uint8))
    out = G.output("out", (B, T, 443), torch.float32, offset=shift, written=(mode == S.ZERO))
    d_hout = G.output("hist_out", (B, 2, 33, 4), torch.float32) if carry else None
    d_cout = G.output("hist_count_out", (B,), torch.uint8) if carry else None
    w, h = (0, 0) if sizes is not None else size
    desc = M.PoseSeqDesc(B, T, w, h, mode)
    Lm.check(L.qt_pose_sequence_features(ctypes.byref(desc), Lm.ptr(d_lm), Lm.ptr(d_det), Lm.ptr(d_sizes), Lm.ptr(d_hin),
                                         Lm.ptr(d_cin), Lm.ptr(d_hout), Lm.ptr(d_cout), Lm.ptr(out), Lm.stream_ptr()),
             "qt_pose_sequence_features")
    G.check()
    return out.cpu().numpy(), ((d_hout.cpu().numpy(), d_cout.cpu().numpy()) if carry else None)


def test_fixture_clips_within_bound():
    dev = _dev()
    g = fixture()
    ref, bound, excluded, _, _ = S.features(g["landmarks"], g["detected"], g["sizes"])
    got, _ = run(dev, g["landmarks"], g["detected"], sizes=g["sizes"])
    assert not excluded.any()
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN positions"
    assert np.array_equal(np.isnan(got), np.isnan(g["features64"])), "NaN positions of the reference's own output"
    worst = S.compare(got, ref, bound, "fixture")
    print(f"fixture: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("frames", [1, 2, 3, R - 1, R, R + 1, 2 * R + 1])
@pytest.mark.parametrize("batch", [1, 3])
def test_random_clips_within_bound(batch, frames):
    """1, 2, 3 frames (no, one, two predecessors); one tile, one frame fewer, one more; 2 R + 1 (a last tile of one frame)"""
    dev = _dev()
    lm, det, ref, bound, excluded, end, end_count = random_clips(batch, frames)
    assert excluded.reshape(-1, 443).any(axis=1).mean() <= 0.01
    got, hist = run(dev, lm, det, carry=True)
    worst = S.compare(got, ref, bound, f"{batch} x {frames}")
    print(f"{batch} x {frames}: largest error / bound {worst:.3f}")
    assert hist[1].tobytes() == end_count.tobytes() and hist[0].tobytes() == end.tobytes()
    again, _ = run(dev, lm, det)
    assert again.tobytes() == got.tobytes()                    # the same bits on every run, with or without hist_out


def test_predecessors_far_behind_the_tile():
    """clip 0: poses in frames 2 and 5, none up to frame 40: the predecessors of frame 41 (third tile) lie two tiles back,
    and the second tile has no pose at all.  clip 1: none up to frame 90: the backward walk takes two ballots.  clip 2: one
    pose before a long gap: a single predecessor, so the motion stays NaN one frame longer."""
    dev = _dev()
    T = 100
    lm, _ = S.make_clips(3, T, seed=77)
    lm[..., 3] = np.float32(0.9)
    det = np.zeros((3, T), np.uint8)
    det[0, [2, 5]] = det[1, [2, 5]] = 1
    det[0, 41:] = det[1, 91:] = 1
    det[2, 3] = 1
    det[2, 70:] = 1
    ref, bound, excluded, end, end_count = S.features(lm, det)
    got, hist = run(dev, lm, det, carry=True)
    S.compare(got, ref, bound, "long gaps")
    dyn = slice(S.COL_DYN, S.COL_VAR)
    assert np.isnan(got[0, 16:32]).all() and np.isfinite(got[0, 41, dyn]).all() and np.isfinite(got[1, 91, dyn]).all()
    assert np.isnan(got[2, 70, dyn]).all() and np.isfinite(got[2, 70, :S.COL_DYN]).all() and np.isfinite(got[2, 71, dyn]).all()
    assert hist[0].tobytes() == end.tobytes() and hist[1].tolist() == [2, 2, 2]


def test_zero_mode_is_raw_with_the_nans_zeroed():
    dev = _dev()
    lm, det, ref, bound, _, _, _ = random_clips(3, 2 * R + 1)
    raw, _ = run(dev, lm, det)
    zero, _ = run(dev, lm, det, mode=S.ZERO, shift=1)
    assert np.isnan(raw).any() and not np.isnan(zero).any()
    want = np.where(np.isnan(raw), np.float32(0), raw)
    assert zero.tobytes() == want.tobytes()
    assert not zero[det == 0].any() and not np.signbit(zero[det == 0]).any()


def test_per_clip_sizes_equal_the_clips_one_at_a_time():
    dev = _dev()
    lm, det, _, _, _, _, _ = random_clips(3, R + 1)
    sizes = np.array([[640, 480], [1920, 1080], [224, 224]], np.int32)
    ref, bound, _, _, _ = S.features(lm, det, sizes)
    got, _ = run(dev, lm, det, sizes=sizes)
    S.compare(got, ref, bound, "per-clip sizes")
    for b in range(3):
        alone, _ = run(dev, lm[b:b + 1], det[b:b + 1], size=tuple(int(v) for v in sizes[b]))
        assert alone.tobytes() == got[b:b + 1].tobytes(), b    # and a clip alone has the bits it has in the batch
    # a non-positive entry makes that clip NaN and no other; its history is carried as usual
    broken = sizes.copy()
    broken[1] = (0, 1080)
    part, hist = run(dev, lm, det, sizes=broken, carry=True)
    assert np.isnan(part[1]).all() and part[[0, 2]].tobytes() == got[[0, 2]].tobytes()
    _, _, _, end, end_count = S.features(lm, det, sizes)
    assert hist[0].tobytes() == end.tobytes() and hist[1].tobytes() == end_count.tobytes()


@pytest.mark.parametrize("cuts", [[1], [2 * R], [R], [R, 2 * R], [3, R + 5], list(range(1, 2 * R + 1))],
                         ids=["after_first_frame", "before_last_frame_and_tile_edge", "tile_edge", "every_tile_edge", "inside_tiles",
                              "single_frames"])
def test_chunks_give_the_bits_of_one_call(cuts):
    """T = 2 R + 1: the cut before the last frame, T - 1 = 2 R, is the second tile edge as well"""
    dev = _dev()
    T = 2 * R + 1
    lm, det, _, _, _, end, end_count = random_clips(2, T)
    whole, _ = run(dev, lm, det)
    hist, parts = None, []
    for a, b in zip([0] + cuts, cuts + [T]):
        part, hist = run(dev, lm[:, a:b], det[:, a:b], hist=hist, carry=True)
        parts.append(part)
    assert np.concatenate(parts, axis=1).tobytes() == whole.tobytes()
    assert hist[0].tobytes() == end.tobytes() and hist[1].tobytes() == end_count.tobytes()      # the last two detected frames


def test_history_counts_and_slots():
    """a count above 2 is 2; a count of 1 reads slot 0 only (slot 1 is poison); slots beyond the count come back as zeros"""
    dev = _dev()
    lm, _ = S.make_clips(2, 3, seed=91)
    lm[..., 3] = np.float32(0.9)
    det = np.array([[1, 1, 1], [0, 0, 1]], np.uint8)
    prior, _ = S.make_clips(2, 2, seed=92)
    prior[..., 3] = np.float32(0.9)
    for counts, model in (([7, 2], [2, 2]), ([1, 0], [1, 0])):
        frames = prior.copy()
        for b, c in enumerate(model):
            frames[b, c:] = np.nan
        ref, bound, _, end, end_count = S.features(lm, det, hist=np.nan_to_num(frames), hist_count=np.array(model, np.uint8))
        got, hist = run(dev, lm, det, hist=(frames, np.array(counts, np.uint8)), carry=True)
        S.compare(got, ref, bound, f"counts {counts}")
        assert hist[1].tobytes() == end_count.tobytes() and hist[0].tobytes() == end.tobytes()
    assert end_count.tolist() == [2, 1] and not end[1, 1].any()


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_output_alignments(shift):
    """`out` at every address modulo 16, T = R + 1 with three clips: clips 1 and 2 start at other addresses modulo 16 again"""
    dev = _dev()
    lm, det, ref, bound, _, _, _ = random_clips(3, R + 1)
    base, _ = run(dev, lm, det)
    got, _ = run(dev, lm, det, shift=shift)
    assert got.tobytes() == base.tobytes()
    zero, _ = run(dev, lm, det, mode=S.ZERO, shift=shift)       # mode zero: the guard also sees an element left unwritten
    assert zero.tobytes() == np.where(np.isnan(base), np.float32(0), base).tobytes()
    alone, _ = run(dev, lm[:1, :1])                             # 443 floats: head, vectors and tail in one row
    one, _ = run(dev, lm[:1, :1], shift=shift, mode=S.ZERO)
    assert one.tobytes() == np.where(np.isnan(alone), np.float32(0), alone).tobytes()


def test_undetected_frames_and_nan_visibility():
    dev = _dev()
    lm, det = S.make_clips(1, 6, seed=12)
    lm, det = lm.copy(), np.ones((1, 6), np.uint8)
    lm[..., 3] = np.float32(0.9)
    clean, _ = run(dev, lm, det)
    det[0, 2] = 0
    lm[0, 2] = np.nan                          # not used where nothing was detected
    lm[0, 4, 12, 3] = np.nan                   # a NaN visibility is not visible
    ref, bound, _, _, _ = S.features(lm, det)
    got, _ = run(dev, lm, det)
    S.compare(got, ref, bound, "NaN inputs")
    col = {n: i for i, n in enumerate(S.FEATURE_NAMES)}
    assert np.isnan(got[0, 2]).all() and np.isfinite(got[0, 3, :S.COL_DYN]).all()
    assert np.isnan(got[0, 4, [col["LM12_visibility"], col["RIGHT_ELBOW_ANGLE"], col["LM12_rel_x_norm"], col["LM12_vx_px"]]]).all()
    assert np.isfinite(got[0, 4, [col["LEFT_ELBOW_ANGLE"], col["LM11_vx_px"], col["TORSO_VAR_XY_RATIO"]]]).all()
    assert got[0, :2].tobytes() == clean[0, :2].tobytes()


def test_cnn_lstm_takes_the_443_columns_as_they_are():
    """CnnLstm(numerical_feature_dim=443) is the reference's sequence model on these features; no model changes for it"""
    dev = _dev()
    P, synth = pkg(), pkg("synth")
    B, T = 2, 3
    lm, det = S.make_clips(B, T, seed=9)
    numerical = P.SequencePoseFeatures("zero", frame_size=(640, 480)).from_landmarks(torch.from_numpy(lm).to(dev),
                                                                                      torch.from_numpy(det).to(dev))
    assert tuple(numerical.shape) == (B, T, 443) and numerical.is_contiguous() and bool(torch.isfinite(numerical).all())
    model = P.CnnLstm(12, sequence_length=T, numerical_feature_dim=443, dropout_rate=0.0, compute_dtype=torch.float32)
    model.load_state_dict(synth.synth_state_dict(model))
    model = model.to(dev).eval()
    images = synth.synth_images(B * T, salt=9).view(B, T, 3, 224, 224).to(dev)
    ref, _, _, _, _ = S.features(lm, det, mode=S.ZERO)
    with torch.no_grad():
        got = model(images, numerical).cpu()
        want = model(images, torch.from_numpy(ref.astype(np.float32)).to(dev)).cpu()
    assert tuple(got.shape) == (B, 12) and torch.isfinite(got).all()
    assert rel_err(got, want) <= 1e-3             # LOGIT_TOL of tests/test_model_gpu.py for the f32 build


def test_the_python_class():
    dev = _dev()
    P = pkg()
    lm, det, ref, bound, _, end, end_count = random_clips(3, 2 * R + 1)
    want, _ = run(dev, lm, det, mode=S.ZERO)
    d_lm, d_det = torch.from_numpy(np.array(lm)).to(dev), torch.from_numpy(np.array(det)).to(dev)
    seq = P.SequencePoseFeatures("zero", frame_size=(640, 480))
    got = seq.from_landmarks(d_lm, d_det)
    assert tuple(got.shape) == (3, 2 * R + 1, 443) and got.dtype == torch.float32 and got.device == d_lm.device
    assert got.is_contiguous() and got.cpu().numpy().tobytes() == want.tobytes()
    assert seq.from_landmarks(d_lm, d_det.bool()).cpu().numpy().tobytes() == want.tobytes()
    one = seq.from_landmarks(d_lm[1], d_det[1])                # [T,33,4]: one clip
    assert tuple(one.shape) == (2 * R + 1, 443) and torch.equal(one, got[1])
    sizes = torch.tensor([[640, 480]] * 3, dtype=torch.int32, device=dev)
    assert torch.equal(P.SequencePoseFeatures("zero").from_landmarks(d_lm, d_det, sizes=sizes), got)
    raw = P.SequencePoseFeatures("raw", frame_size=(640, 480)).from_landmarks(d_lm, d_det)
    assert torch.equal(torch.nan_to_num(raw, nan=0.0), got) and bool(torch.isnan(raw).any())
    # the history: chunks through the two swapped buffers, under "no host synchronisation"
    hist = seq.history(3, dev)
    assert hist.counts.tolist() == [0, 0, 0]
    chunks = [(0, 5), (5, R), (R, R + 1), (R + 1, 2 * R + 1)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        parts = [seq.from_landmarks(d_lm[:, a:b], d_det[:, a:b], history=hist) for a, b in chunks]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(torch.cat(parts, dim=1), got)
    assert hist.counts.cpu().numpy().tobytes() == end_count.tobytes() and hist.frames.cpu().numpy().tobytes() == end.tobytes()
    # reset(mask): clip 1 starts anew, the others go on
    hist.reset(torch.tensor([False, True, False], device=dev))
    assert hist.counts.tolist() == [int(end_count[0]), 0, int(end_count[2])]
    more = seq.from_landmarks(d_lm[:, :3], d_det[:, :3], history=hist)
    fresh, fb, _, _, _ = S.features(lm[:, :3], det[:, :3], mode=S.ZERO)
    carried, cb, _, _, _ = S.features(lm[:, :3], det[:, :3], hist=end, hist_count=end_count, mode=S.ZERO)
    S.compare(more[1:2].cpu().numpy(), fresh[1:2], fb[1:2], "after reset")
    S.compare(more[[0, 2]].cpu().numpy(), carried[[0, 2]], cb[[0, 2]], "carried on")
    hist.reset()
    assert hist.counts.tolist() == [0, 0, 0]
    # errors
    with pytest.raises(P.QtError, match="AMD GPU"):
        seq.from_landmarks(d_lm.cpu(), d_det)
    with pytest.raises(P.QtError, match="cuda"):
        seq.from_landmarks(d_lm, d_det.cpu())
    with pytest.raises(P.QtError, match="float32"):
        seq.from_landmarks(d_lm.double(), d_det)
    with pytest.raises(P.QtError, match="landmarks must be"):
        seq.from_landmarks(d_lm[..., :3], d_det)
    with pytest.raises(P.QtError, match="detected must have shape"):
        seq.from_landmarks(d_lm, d_det[:, :5])
    with pytest.raises(P.QtError, match="sizes must have shape"):
        seq.from_landmarks(d_lm, d_det, sizes=sizes[:2])
    with pytest.raises(P.QtError, match="int32"):
        seq.from_landmarks(d_lm, d_det, sizes=sizes.long())
    with pytest.raises(P.QtError, match="no frame size"):
        P.SequencePoseFeatures("zero").from_landmarks(d_lm, d_det)
    with pytest.raises(P.QtError, match="history"):
        seq.from_landmarks(d_lm, d_det, history=seq.history(2, dev))
    with pytest.raises(P.QtError, match="mask"):
        hist.reset(torch.zeros(2, dtype=torch.bool, device=dev))
