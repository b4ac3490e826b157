"""The pose vector, the parts that need no GPU: tests/_pose_ref.py against what the reference's own function returned on
the fixture rows, its bound against an f32 restatement of the kernel, the C ABI's declarations and host-side argument
checks, the class tables read by name, the exports."""
import ctypes
import json
import os
import random
import re

import numpy as np
import pytest
import torch

import _pose_ref as R
from _util import PKG, ROOT, pkg

NEW_SYMBOLS = ["qt_pose_features"]
QT_ERR_INVALID_ARG, QT_ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "pose_features.npz"))


def test_float64_rule_reproduces_the_reference_on_the_fixture(fixture):
    ref, bound, excluded = R.features(fixture["landmarks"], fixture["detected"])
    want = fixture["features64"]                   # the reference's values before its float32 cast
    assert want.shape == ref.shape == (len(fixture["cases"]), 47) and ref.shape[0] >= 70
    assert np.array_equal(np.isnan(ref), np.isnan(want))
    assert np.array_equal(np.isnan(ref), np.isnan(fixture["features"]))
    live = ~np.isnan(ref)
    rel = np.abs(ref - want)[live] / np.maximum(np.abs(want[live]), 1e-300)
    print(f"largest relative distance from the reference: {rel.max():.2e}")
    assert rel.max() <= 1e-9
    # the f32 array the reference returns is that, rounded
    got32 = fixture["features"][live].astype(np.float64)
    assert (np.abs(ref[live] - got32) <= np.spacing(np.abs(got32).astype(np.float32))).all()
    assert not excluded.any()                      # no fixture row sits next to a discontinuity
    # the structured cases are what they claim to be
    case = {str(n): i for i, n in enumerate(fixture["cases"])}
    col = {n: i for i, n in enumerate(R.FEATURE_NAMES)}
    no_pose = ref[case["no_pose"]]
    assert not no_pose[:33].any() and np.isnan(no_pose[33:]).all() and fixture["detected"][case["no_pose"]] == 0
    assert np.isnan(ref[case["zero_length_forearm"], col["LEFT_ELBOW_ANGLE"]])
    assert np.isnan(ref[case["body_scale_below_0.05"], 43:46]).all()
    assert np.isfinite(ref[case["shoulder_width_zero"], 43:46]).all()
    for n in (0, 1):
        assert np.isnan(ref[case[f"{n}_visible_torso_landmarks"], 46])
    assert np.isfinite(ref[case["2_visible_torso_landmarks"], 46])
    assert np.isnan(ref[case["visible_y_all_equal"], 46])
    assert ref[case["torso_on_branch_cut"], col["TORSO_VERTICAL_ANGLE"]] == 90.0
    if "elbow_179.99" in case:
        assert abs(ref[case["elbow_179.99"], col["LEFT_ELBOW_ANGLE"]] - 179.99) < 1e-4


def test_feature_names_are_the_fixtures(fixture):
    assert list(pkg("pose").FEATURE_NAMES) == [str(c) for c in fixture["columns"]] == R.FEATURE_NAMES
    assert pkg().FEATURE_NAMES is pkg("pose").FEATURE_NAMES


def test_f32_restatement_of_the_kernel_meets_the_bound(fixture):
    for what, lm, det in (("random", R.make_landmarks(R.ROWS, R.SEED), None),
                          ("fixture", fixture["landmarks"], fixture["detected"])):
        ref, bound, excluded = R.features(lm, det)
        assert not excluded.any(), what            # (checked for the issue: seed 1234 leaves out no row of 4096)
        worst = R.compare(R.restated(lm, det), ref, bound, what)
        print(f"{what}: largest error / bound {worst:.3f}; largest angle bound {bound[:, 33:41].max():.2e} degrees")
        assert bound[:, 33:43].max() < 1e-2        # the bound is not vacuous: a hundredth of a degree at the most
    # a mistake the bound must see: the elbow taken at the wrist
    lm = R.make_landmarks(64, seed=3)
    ref, bound, _ = R.features(lm)
    wrong = R.restated(lm[:, [0] * 13 + [15, 14, 13] + list(range(16, 33))])
    with pytest.raises(AssertionError):
        R.compare(wrong, ref, bound, "wrong")


def test_near_discontinuity_rows_are_excluded_and_counted():
    lm = R.make_landmarks(8, seed=5)
    lm[0, 12, :3] = lm[0, 11, :3] + np.array([0.05, 0, 0], np.float32)     # s within rounding of 0.05
    lm[0, 24, :3] = lm[0, 23, :3] + np.array([0.05, 0, 0], np.float32)
    lm[1, list(R.TORSO), 3] = 0.9
    lm[1, list(R.TORSO), 1] = np.float32(0.3) + np.arange(4, dtype=np.float32) * np.float32(2.0 ** -25)   # var(y) ~ rounding
    ref, bound, excluded = R.features(lm)
    assert excluded[0, 43:46].all() and not excluded[0, :43].any() and not excluded[2:].any()
    assert excluded[1, 46] or np.isnan(ref[1, 46])
    with pytest.raises(AssertionError, match="discontinuity"):
        R.compare(R.restated(lm), ref, bound, "two of eight rows")


def test_imputation_rule_on_the_host_model():
    raw = np.array([[1.0, np.nan, 3.0], [np.nan, 5.0, 6.0], [7.0, 8.0, np.nan]])
    raw = np.concatenate([raw, np.zeros((3, 44))], axis=1)
    zero = np.zeros_like(raw)
    means = np.arange(2 * 47, dtype=np.float32).reshape(2, 47) + 10
    stds = np.full((2, 47), 2.0, np.float32)
    stds[1, 0] = 1e-7
    labels = np.array([0, 1, 5])
    got, _ = R.impute(raw, zero, R.RAW)
    assert np.array_equal(np.isnan(got), np.isnan(raw))
    got, _ = R.impute(raw, zero, R.ZERO)
    assert got[0, 1] == 0 and got[1, 0] == 0 and got[0, 0] == 1 and not np.isnan(got).any()
    got, _ = R.impute(raw, zero, R.CLASS_MEAN, labels, means)
    assert got[0, 1] == 11 and got[1, 0] == 57 and got[1, 1] == 5 and np.isnan(got[2]).all()
    got, bound = R.impute(raw, zero, R.STANDARDIZE, labels, means, stds)
    assert got[0, 1] == 0 and got[0, 0] == (1 - 10) / 2 and got[1, 0] == 0 and got[1, 1] == (5 - 58) / 2
    assert np.isnan(got[2]).all() and (bound[2] == 0).all() and bound[0, 0] > 0
    got, _ = R.impute(raw[:2], zero[:2], R.CLASS_MEAN, np.array([1]), means, rows_per_label=2)
    assert got[0, 1] == 58 and got[1, 0] == 57


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    declared = set(re.findall(r"\b(qt_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(os.path.join(ROOT, PKG, "libqtcnn_hip.so"))
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
    assert "qt_pose_desc" in header and "#define QT_POSE_FEATURES 47" in header and "#define QT_POSE_LANDMARKS 33" in header
    M = pkg("pose")
    for name, value in (("QT_POSE_RAW", 0), ("QT_POSE_ZERO", 1), ("QT_POSE_CLASS_MEAN", 2), ("QT_POSE_STANDARDIZE", 3)):
        assert re.search(rf"\b{name} = {value}\b", header) and getattr(M, name) == value
    assert (R.RAW, R.ZERO, R.CLASS_MEAN, R.STANDARDIZE) == (0, 1, 2, 3)


def test_host_side_argument_checks_need_no_device():
    """every refusal below comes before the first device call: the pointers are never dereferenced"""
    M = pkg("pose")
    L = pkg("_lib").lib()
    lm, det, raw, lab, mean, std, out = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000

    def call(desc, landmarks=lm, detected=None, rawv=None, labels=None, means=None, stds=None, dst=out):
        return L.qt_pose_features(ctypes.byref(desc), landmarks, detected, rawv, labels, means, stds, dst, None)

    zero = M.PoseDesc(4, M.QT_POSE_ZERO, 1, 0)
    assert call(M.PoseDesc(0, M.QT_POSE_ZERO, 1, 0)) == QT_ERR_INVALID_ARG and b"rows" in L.qt_last_error()
    assert call(M.PoseDesc(-3, M.QT_POSE_ZERO, 1, 0)) == QT_ERR_INVALID_ARG
    assert call(M.PoseDesc((1 << 22) + 1, M.QT_POSE_ZERO, 1, 0)) == QT_ERR_UNSUPPORTED and b"rows" in L.qt_last_error()
    assert call(M.PoseDesc(4, 4, 1, 0)) == QT_ERR_INVALID_ARG and b"mode" in L.qt_last_error()
    assert call(M.PoseDesc(4, -1, 1, 0)) == QT_ERR_INVALID_ARG
    assert L.qt_pose_features(None, lm, None, None, None, None, None, out, None) == QT_ERR_INVALID_ARG
    assert call(zero, landmarks=None) == QT_ERR_INVALID_ARG and b"source" in L.qt_last_error()          # neither source
    assert call(zero, rawv=raw) == QT_ERR_INVALID_ARG and b"source" in L.qt_last_error()                # both
    assert call(zero, landmarks=None, rawv=raw, detected=det) == QT_ERR_INVALID_ARG
    assert call(zero, dst=None) == QT_ERR_INVALID_ARG
    assert call(zero, landmarks=lm + 4) == QT_ERR_INVALID_ARG and b"16-byte" in L.qt_last_error()
    assert call(zero, landmarks=None, rawv=raw + 2) == QT_ERR_INVALID_ARG
    assert call(zero, dst=out + 1) == QT_ERR_INVALID_ARG
    by_mean, by_std = M.PoseDesc(4, M.QT_POSE_CLASS_MEAN, 1, 3), M.PoseDesc(4, M.QT_POSE_STANDARDIZE, 1, 3)
    assert call(by_mean) == QT_ERR_INVALID_ARG and b"needs" in L.qt_last_error()                        # no labels, no table
    assert call(by_mean, labels=lab) == QT_ERR_INVALID_ARG
    assert call(by_mean, means=mean) == QT_ERR_INVALID_ARG
    assert call(by_mean, labels=lab + 4, means=mean) == QT_ERR_INVALID_ARG
    assert call(by_mean, labels=lab, means=mean + 2) == QT_ERR_INVALID_ARG
    assert call(M.PoseDesc(4, M.QT_POSE_CLASS_MEAN, 1, 0), labels=lab, means=mean) == QT_ERR_INVALID_ARG    # K = 0
    assert call(by_std, labels=lab, means=mean) == QT_ERR_INVALID_ARG and b"stds" in L.qt_last_error()
    assert call(M.PoseDesc(4, M.QT_POSE_STANDARDIZE, 0, 3), labels=lab, means=mean, stds=std) == QT_ERR_INVALID_ARG
    assert call(M.PoseDesc(4, M.QT_POSE_STANDARDIZE, 3, 3), labels=lab, means=mean, stds=std) == QT_ERR_INVALID_ARG
    assert b"rows_per_label" in L.qt_last_error()


def test_module_constructor_and_device_checks():
    P = pkg()
    assert P.PoseFeatures is pkg("pose").PoseFeatures and P.load_class_stats is pkg("pose").load_class_stats
    assert {"PoseFeatures", "FEATURE_NAMES", "load_class_stats"} <= set(P.__all__)
    table = torch.zeros(3, 47)
    for bad in (dict(mode="mean"), dict(mode="class_mean"), dict(mode="standardize", means=table),
                dict(mode="class_mean", means=torch.zeros(3, 46)), dict(mode="standardize", means=table, stds=torch.zeros(2, 47))):
        with pytest.raises(ValueError):
            P.PoseFeatures(**bad)
    assert P.PoseFeatures().mode == "zero"
    # no torch fallback
    pose = P.PoseFeatures("zero")
    with pytest.raises(P.QtError, match="AMD GPU"):
        pose.from_landmarks(torch.zeros(2, 33, 4))
    with pytest.raises(P.QtError, match="AMD GPU"):
        pose.impute(torch.zeros(2, 47))
    with pytest.raises(P.QtError, match="float32"):
        pose.from_landmarks(torch.zeros(2, 33, 4, dtype=torch.float64))
    with pytest.raises(P.QtError, match="float32"):
        pose.impute(torch.zeros(2, 47, dtype=torch.float16))
    with pytest.raises(P.QtError):
        P.PoseFeatures.fit(torch.zeros(2, 47), torch.zeros(2, dtype=torch.int64), 3)


def test_load_class_stats_matches_columns_by_name(tmp_path):
    M = pkg("pose")
    rnd = random.Random(7)
    classes = ["Warrior", "Cobra", "Mountain"]
    value = lambda cls, col, scale: scale * (classes.index(cls) * 100 + col + 0.25)

    def write(path, scale):
        data = {}
        for cls in classes:                              # classes unsorted, every class's keys in an order of its own
            cols = list(range(47))
            rnd.shuffle(cols)
            data[cls] = {M.FEATURE_NAMES[c]: value(cls, c, scale) for c in cols}
        with open(path, "w") as f:
            json.dump(data, f)

    mp, sp = str(tmp_path / "class_feature_means.json"), str(tmp_path / "class_feature_stds.json")
    write(mp, 1.0)
    write(sp, 0.5)
    means, stds = M.load_class_stats(mp, sp)
    assert means.dtype == stds.dtype == torch.float32 and tuple(means.shape) == tuple(stds.shape) == (3, 47)
    for k, cls in enumerate(sorted(classes)):            # the loaders' numbering
        for c in range(47):
            assert means[k, c] == np.float32(value(cls, c, 1.0)) and stds[k, c] == np.float32(value(cls, c, 0.5))
    only, none = M.load_class_stats(mp)
    assert none is None and torch.equal(only, means)
    picked, _ = M.load_class_stats(mp, class_names=["Warrior", "Cobra"])
    assert torch.equal(picked[0], means[2]) and torch.equal(picked[1], means[0])
    with pytest.raises(M.QtError, match="class"):
        M.load_class_stats(mp, class_names=["Tree"])
    data = json.load(open(mp))
    del data["Cobra"]["TORSO_VAR_XY_RATIO"]
    json.dump(data, open(mp, "w"))
    with pytest.raises(M.QtError, match="TORSO_VAR_XY_RATIO"):
        M.load_class_stats(mp)
