"""Sequence pose features, the parts that need no GPU: tests/_pose_seq_ref.py against what the reference's own pipeline wrote
for the fixture clips, its bound against an f32 restatement of the kernel, a Python walk of the kernel's tiling and backward
search against the plain per-clip loop, the chunk contract on the host model, the C ABI's declaration and host-side
argument checks, the exports."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _pose_ref as R
import _pose_seq_ref as S
from _util import PKG, ROOT, pkg

QT_ERR_INVALID_ARG, QT_ERR_UNSUPPORTED = -1, -3
EPS64 = 2.0 ** -53


@pytest.fixture(scope="module")
def fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "pose_seq.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def fixture_ref(fixture):
    return S.features(fixture["landmarks"], fixture["detected"], fixture["sizes"])


def _arccos_tolerance(deg):
    """How far two float64 evaluations of one joint angle may lie apart, in degrees, where one is the reference's
    arccos(clip(v1 . v2 / (|v1| |v2|))) and the other atan2(|v1 x v2|, v1 . v2).
    The reference's cosine c carries: the dot product, three products and two sums, at most 3 eps |v1| |v2| absolute, that is
    3 eps in c; each norm 2 eps relative (sum of squares, square root), their product and the quotient one eps each: at most
    delta = 9 eps in c, eps = 2^-53.  arccos is not Lipschitz at +-1, so its share is taken as it is:
    max |arccos(clip(c +- delta)) - arccos(c)|.  The atan2 form is well conditioned everywhere: its arguments carry at most
    6 eps |v1| |v2| (cross and dot products of rounded differences), which turn the angle by at most 6 eps rad; both library
    functions and both conversions to degrees add a few eps of the angle.  Together: the arccos term + 16 eps rad + 8 eps
    of 180 degrees."""
    theta = np.deg2rad(deg)
    c = np.cos(theta)
    delta = 9 * EPS64
    moved = np.maximum(np.abs(np.arccos(np.clip(c - delta, -1, 1)) - theta), np.abs(np.arccos(np.clip(c + delta, -1, 1)) - theta))
    return np.rad2deg(moved + 16 * EPS64) + 8 * EPS64 * 180.0


def test_float64_rule_reproduces_the_reference_on_the_fixture(fixture, fixture_ref):
    ref, bound, excluded, _, _ = fixture_ref
    want = fixture["features64"]
    assert want.shape == ref.shape == (12, 12, 443) and int(fixture["lengths"].sum()) >= 100
    assert np.array_equal(np.isnan(ref), np.isnan(want))
    assert not excluded.any()                      # no fixture frame sits next to a discontinuity
    live = ~np.isnan(ref)
    angle = np.zeros(443, dtype=bool)
    angle[S.COL_ANGLE:S.COL_DIST] = True
    plain = live & ~angle
    rel = np.abs(ref - want)[plain] / np.maximum(np.abs(want[plain]), 1e-300)
    print(f"largest relative distance from the reference outside the angles: {rel.max():.2e}")
    assert rel.max() <= 1e-9
    a_ref, a_want = ref[..., angle][live[..., angle]], want[..., angle][live[..., angle]]
    ratio = np.abs(a_ref - a_want) / _arccos_tolerance(a_want)
    print(f"angles: largest distance {np.abs(a_ref - a_want).max():.2e} degrees, largest distance / tolerance {ratio.max():.3f}")
    assert a_ref.size > 300 and (ratio <= 1).all()
    assert _arccos_tolerance(np.array([90.0])).max() < 1e-12 and _arccos_tolerance(np.array([0.0])).max() < 1e-5


def test_fixture_clips_are_what_they_claim_to_be(fixture, fixture_ref):
    ref = fixture_ref[0]
    want = fixture["features64"]
    clip = {str(n): i for i, n in enumerate(fixture["clips"])}
    col = {n: i for i, n in enumerate(S.FEATURE_NAMES)}
    det, lengths = fixture["detected"], fixture["lengths"]
    dyn = slice(S.COL_DYN, S.COL_VAR)
    assert set(clip) >= {"random", "undetected_first_frame", "undetected_run_of_1", "undetected_run_of_2", "undetected_run_of_5",
                         "landmark_drops_in_one_frame_of_three", "visibility_exactly_0.65f", "both_hips_invisible",
                         "shoulders_below_scale_hips_above", "shoulders_and_hips_below_scale", "wrist_on_elbow", "non_square_frame"}
    assert lengths.max() <= 12 and all(not det[i, n:].any() for i, n in enumerate(lengths))
    c = clip["undetected_first_frame"]
    assert det[c, 0] == 0 and np.isnan(want[c, 0]).all()
    assert np.isnan(want[c, 1:3, dyn]).all() and np.isfinite(want[c, 3, dyn]).any()       # frames 1, 2 have < 2 predecessors
    for run in (1, 2, 5):
        c = clip[f"undetected_run_of_{run}"]
        assert not det[c, 3:3 + run].any() and det[c, 3 + run] and np.isnan(want[c, 3:3 + run]).all()
        after = want[c, 3 + run]                   # every landmark visible: the history survived the gap
        assert np.isfinite(after[dyn]).all()
        lm = fixture["landmarks"][c].astype(np.float64)
        w = float(fixture["sizes"][c, 0])
        assert after[col["LM5_vx_px"]] == lm[3 + run, 5, 0] * w - lm[2, 5, 0] * w          # against frame 2, not the gap
    c = clip["landmark_drops_in_one_frame_of_three"]
    wrist = [col[f"LM15_{k}_px"] for k in ("vx", "vy", "vz", "ax", "ay", "az")]
    for t in range(2, 10):
        assert np.isnan(want[c, t, wrist]).all() == (t in (4, 5, 6)), t
    c = clip["visibility_exactly_0.65f"]
    assert np.isnan(want[c, :6, col["LM13_rel_x_norm"]]).all() and np.isfinite(want[c, :6, col["LM14_rel_x_norm"]]).all()
    assert np.isnan(want[c, :6, col["LEFT_ELBOW_ANGLE"]]).all() and np.isfinite(want[c, :6, col["RIGHT_ELBOW_ANGLE"]]).all()
    c = clip["both_hips_invisible"]
    lm = fixture["landmarks"][c].astype(np.float64)
    assert (want[c, :6, col["LM0_rel_x_norm"]] == lm[:6, 0, 0] - 0.5).all() and (want[c, :6, col["LM0_rel_z_norm"]] == lm[:6, 0, 2]).all()
    for name, scale in (("shoulders_below_scale_hips_above", "hw"), ("shoulders_and_hips_below_scale", "third")):
        c = clip[name]
        lm = fixture["landmarks"][c].astype(np.float64)
        w, h = (float(v) for v in fixture["sizes"][c])
        px = lambda j: lm[:6, j, :3] * np.array([w, h, w])
        s = np.linalg.norm(px(23) - px(24), axis=1) if scale == "hw" else h / 3.0
        assert np.allclose(want[c, :6, col["DIST_LR_WRIST_NORM"]], np.linalg.norm(px(15) - px(16), axis=1) / s, rtol=1e-12)
    assert (want[clip["wrist_on_elbow"], :6, col["LEFT_ELBOW_ANGLE"]] == 0.0).all()
    assert (ref[clip["wrist_on_elbow"], :6, col["LEFT_ELBOW_ANGLE"]] == 0.0).all()
    assert tuple(fixture["sizes"][clip["non_square_frame"]]) == (1920, 1080)


def test_feature_names_are_the_fixtures(fixture):
    M = pkg("pose_sequence")
    assert list(M.SEQUENCE_FEATURE_NAMES) == [str(c) for c in fixture["columns"]] == S.FEATURE_NAMES
    P = pkg()
    assert P.SEQUENCE_FEATURE_NAMES is M.SEQUENCE_FEATURE_NAMES and P.NUM_SEQUENCE_FEATURES == M.NUM_SEQUENCE_FEATURES == 443
    assert P.SequencePoseFeatures is M.SequencePoseFeatures
    assert {"SequencePoseFeatures", "SEQUENCE_FEATURE_NAMES", "NUM_SEQUENCE_FEATURES"} <= set(P.__all__)


def test_f32_restatement_of_the_kernel_meets_the_bound(fixture, fixture_ref):
    ref, bound, excluded, _, _ = fixture_ref
    worst = S.compare(S.restated(fixture["landmarks"], fixture["detected"], fixture["sizes"]), ref, bound, "fixture")
    print(f"fixture: largest error / bound {worst:.3f}")
    for size in ((640, 480), (1920, 1080), (224, 224)):
        lm, det = S.make_clips(3, 2 * S.TILE + 1, undetected=0.3)
        ref, bound, excluded, _, _ = S.features(lm, det, size)
        assert not excluded.any()
        worst = S.compare(S.restated(lm, det, size), ref, bound, str(size))
        finite = np.isfinite(bound)
        print(f"{size}: largest error / bound {worst:.3f}; largest bounds: angle {bound[..., 132:142][finite[..., 132:142]].max():.2e} "
              f"degrees, motion {bound[..., 244:442].max():.2e} px, ratio {bound[..., 442].max():.2e}")
        assert bound[..., 132:142].max() < 1e-2 and bound[..., 244:442].max() < 1e-2      # the bound is not vacuous
        assert np.isfinite(ref[..., 244:442]).mean() > 0.1                                # and the motion columns are exercised
    # mistakes the bound must see: W and H exchanged; the previous frame taken whether a pose was found in it or not
    lm, det = S.make_clips(2, 20, seed=3, undetected=0.3)
    ref, bound, _, _, _ = S.features(lm, det)
    with pytest.raises(AssertionError):
        S.compare(S.restated(lm, det, (480, 640)), ref, bound, "wrong")
    naive = S.restated(lm, np.ones_like(det))
    naive[det == 0] = np.nan
    with pytest.raises(AssertionError):
        S.compare(naive, ref, bound, "wrong")


def test_no_seeded_row_is_next_to_a_scale_threshold():
    """the 4096 seeded rows of the 47-vector's tests as 256 clips of 16 frames, at three frame sizes"""
    lm = R.make_landmarks(4096, 1234).reshape(256, 16, 33, 4)
    lm[..., 3] = np.float32(0.9)            # every landmark visible: sw and hw are both in play
    for size in ((640, 480), (1920, 1080), (224, 224)):
        _, _, excluded, _, _ = S.features(lm, None, size)
        assert not excluded.any(), size


def test_near_threshold_frames_are_excluded_and_counted():
    lm, det = S.make_clips(1, 8, seed=5)
    lm[..., 3] = np.float32(0.9)
    lm[0, 2, 12, :3] = lm[0, 2, 11, :3] + np.array([0.05, 0, 0], np.float32)     # sw within rounding of 0.05f W
    lm[0, 5, [11, 12], 3] = np.float32(0.3)                                       # shoulders unseen: hw decides
    lm[0, 5, 24, :3] = lm[0, 5, 23, :3] + np.array([0.05, 0, 0], np.float32)
    ref, bound, excluded, _, _ = S.features(lm, det)
    assert excluded[0, 2, 142:145].all() and excluded[0, 5, 142:145].all() and excluded.sum() == 6
    assert np.isinf(bound[excluded]).all()
    with pytest.raises(AssertionError, match="discontinuity"):
        S.compare(S.restated(lm, det), ref, bound, "two of eight frames")


@pytest.mark.parametrize("count", [0, 1, 2])
def test_kernel_walk_finds_the_plain_loops_predecessors(count):
    """the tiling, the ballots of the backward walk and the pass over the tile's flags, in Python, against the deque"""
    rng = np.random.default_rng(40 + count)
    patterns = []
    for T in (1, 2, 3, S.TILE - 1, S.TILE, S.TILE + 1, 2 * S.TILE + 1, 100, 200):
        for share in (0.0, 0.3, 0.9, 1.0):
            patterns.append((rng.random(T) >= share).astype(np.uint8))
    gap = np.zeros(200, np.uint8)             # predecessors more than two ballots back
    gap[[1, 4]] = 1
    gap[170:] = 1
    patterns.append(gap)
    one = np.zeros(150, np.uint8)             # a single detected frame far back: the second comes from the history
    one[3] = 1
    one[149] = 1
    patterns.append(one)
    most = 0
    for det in patterns:
        want, want_last = S.plain_predecessors(det, count)
        got, got_last, ballots = S.kernel_predecessors(det, count)
        assert got == want and got_last == want_last, (len(det), det.tolist())
        most = max(most, ballots)
        for t, (s1, s2) in enumerate(want):   # nothing outside the clip, nothing at or after the frame itself
            assert all(s is None or -2 <= s < t for s in (s1, s2))
    assert most >= 3                          # the long gaps made the walk take several steps
    assert S.kernel_predecessors(gap, count, tile=S.TILE, wave=64)[0] == S.kernel_predecessors(gap, count, tile=5, wave=8)[0]


def test_chunks_carry_the_history_on_the_host_model():
    lm, det = S.make_clips(2, 23, seed=8, undetected=0.3)
    whole, _, _, end, end_count = S.features(lm, det)
    for cuts in ([1], [22], [16], [5, 6, 7, 20], list(range(1, 23))):
        hist, count, parts = None, None, []
        for a, b in zip([0] + cuts, cuts + [23]):
            part, _, _, hist, count = S.features(lm[:, a:b], det[:, a:b], hist=hist, hist_count=count)
            parts.append(part)
        assert np.concatenate(parts, axis=1).tobytes() == whole.tobytes(), cuts
        assert hist.tobytes() == end.tobytes() and count.tobytes() == end_count.tobytes()
    for b in range(2):                        # the final history is the last two detected frames
        found = np.flatnonzero(det[b])[::-1][:2]
        assert end_count[b] == len(found) and all((end[b, k] == lm[b, t]).all() for k, t in enumerate(found))


def test_new_symbol_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    declared = set(re.findall(r"\b(qt_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(os.path.join(ROOT, PKG, "libqtcnn_hip.so"))
    assert "qt_pose_sequence_features" in declared and hasattr(lib, "qt_pose_sequence_features")
    assert "qt_pose_seq_desc" in header and "#define QT_POSE_SEQ_FEATURES 443" in header
    M = pkg("pose_sequence")
    fields = re.search(r"typedef struct qt_pose_seq_desc \{(.*?)\} qt_pose_seq_desc;", header, re.S).group(1)
    names = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields))
    assert names == [n for n, _ in M.PoseSeqDesc._fields_]
    assert (S.RAW, S.ZERO) == (M.QT_POSE_RAW, M.QT_POSE_ZERO) == (0, 1) and S.TILE == 16
    source = open(os.path.join(ROOT, PKG, "csrc", "pose_seq.hip")).read()
    assert re.search(r"PS_ROWS = (\d+);", source).group(1) == str(S.TILE)


def test_host_side_argument_checks_need_no_device():
    """every refusal below comes before the first device call: the pointers are never dereferenced"""
    M = pkg("pose_sequence")
    L = pkg("_lib").lib()
    lm, det, sz, hin, cin, hout, cout, out = (0x10000 * k for k in range(1, 9))

    def call(desc, landmarks=lm, detected=det, sizes=None, hist_in=None, count_in=None, hist_out=None, count_out=None, dst=out):
        return L.qt_pose_sequence_features(ctypes.byref(desc), landmarks, detected, sizes, hist_in, count_in, hist_out, count_out,
                                           dst, None)

    D = M.PoseSeqDesc
    good = D(2, 5, 640, 480, M.QT_POSE_ZERO)
    assert L.qt_pose_sequence_features(None, lm, det, None, None, None, None, None, out, None) == QT_ERR_INVALID_ARG
    for bad in (D(0, 5, 640, 480, 1), D(-1, 5, 640, 480, 1), D(2, 0, 640, 480, 1), D(2, -7, 640, 480, 1)):
        assert call(bad) == QT_ERR_INVALID_ARG and b"positive" in L.qt_last_error()
    for mode in (-1, 2, 3, 4):                # the class-table modes of the 47-vector do not exist here
        assert call(D(2, 5, 640, 480, mode)) == QT_ERR_INVALID_ARG and b"mode" in L.qt_last_error()
    assert call(D(1 << 11, (1 << 11) + 1, 640, 480, 1)) == QT_ERR_UNSUPPORTED and b"frames" in L.qt_last_error()
    assert call(D(1, (1 << 22) + 1, 640, 480, 1)) == QT_ERR_UNSUPPORTED
    assert call(good, landmarks=None) == QT_ERR_INVALID_ARG and call(good, dst=None) == QT_ERR_INVALID_ARG
    assert call(good, landmarks=lm + 4) == QT_ERR_INVALID_ARG and b"16-byte" in L.qt_last_error()
    assert call(good, dst=out + 2) == QT_ERR_INVALID_ARG and b"4-byte" in L.qt_last_error()
    assert call(good, sizes=sz + 1) == QT_ERR_INVALID_ARG
    for w, h in ((0, 480), (640, 0), (-640, 480), (640, -1)):
        assert call(D(2, 5, w, h, 1)) == QT_ERR_INVALID_ARG and b"frame size" in L.qt_last_error()
    # half a history pair
    assert call(good, hist_in=hin) == QT_ERR_INVALID_ARG and b"half" in L.qt_last_error()
    assert call(good, count_in=cin) == QT_ERR_INVALID_ARG
    assert call(good, hist_out=hout) == QT_ERR_INVALID_ARG
    assert call(good, hist_in=hin, count_in=cin, count_out=cout) == QT_ERR_INVALID_ARG
    assert call(good, hist_in=hin + 8, count_in=cin) == QT_ERR_INVALID_ARG and b"16-byte" in L.qt_last_error()
    assert call(good, hist_out=hout + 4, count_out=cout) == QT_ERR_INVALID_ARG
    # aliased histories: the same buffer, an overlapping one (2 clips x 2 x 528 bytes), the same counts
    assert call(good, hist_in=hin, count_in=cin, hist_out=hin, count_out=cout) == QT_ERR_INVALID_ARG and b"overlap" in L.qt_last_error()
    assert call(good, hist_in=hin, count_in=cin, hist_out=hin + 2 * 2 * 528 - 16, count_out=cout) == QT_ERR_INVALID_ARG
    assert call(good, hist_in=hin, count_in=cin, hist_out=hout, count_out=cin + 1) == QT_ERR_INVALID_ARG


def test_module_constructor_and_device_checks():
    P = pkg()
    for bad in (dict(mode="mean"), dict(mode="class_mean"), dict(mode="standardize"), dict(frame_size=(0, 480)),
                dict(frame_size=(640, -1))):
        with pytest.raises(ValueError):
            P.SequencePoseFeatures(**bad)
    seq = P.SequencePoseFeatures()
    assert seq.mode == "zero" and seq.frame_size is None
    assert P.SequencePoseFeatures("raw", frame_size=(640, 480)).frame_size == (640, 480)
    # no torch fallback
    with pytest.raises(P.QtError, match="AMD GPU"):
        seq.from_landmarks(torch.zeros(2, 3, 33, 4))
    with pytest.raises(P.QtError, match="AMD GPU"):
        seq.from_landmarks(torch.zeros(3, 33, 4))
    with pytest.raises(P.QtError, match="float32"):
        seq.from_landmarks(torch.zeros(2, 3, 33, 4, dtype=torch.float64))
    with pytest.raises(P.QtError, match="tensor"):
        seq.from_landmarks(np.zeros((2, 3, 33, 4), np.float32))
    with pytest.raises(P.QtError, match="AMD GPU"):
        seq.history(2, "cpu")
    with pytest.raises(ValueError):
        seq.history(0, "cuda:0")
