#!/usr/bin/env python3
"""Generate tests/golden/pose_features.npz by RUNNING THE REFERENCE's own feature function on the CPU (developer aid; no
test and no GPU run reads the reference checkout).

    python tests/golden/make_pose_golden.py <path of the reference checkout>

Imports experiment/test_on_video_cnn.py of the checkout by path.  The modules it imports at the top and this machine may
lack (mediapipe, cv2, torchvision, its sibling models_cnn) are stubbed in sys.modules: the stub's PoseLandmark is an enum
with MediaPipe's 33 names and indices, and its Pose().process returns the landmark objects this script made, or no pose.
For every fixture row the script records what extract_and_process_features returns (f32, `features`), and the same call
with the function's final float32 cast replaced by float64 (`features64`: the module's `np` is wrapped so that
np.float32 is np.float64 for that call; nothing else changes), which is what tests/_pose_ref.py is compared with at 1e-9.
Only data is written: the landmarks, the detected flags, the two feature arrays, the reference's column names and the
case names.  Rows: 64 seeded random frames, then the structured cases listed in CASES.
"""
import enum
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _pose_ref as R  # noqa: E402

LANDMARK_NAMES = ["NOSE", "LEFT_EYE_INNER", "LEFT_EYE", "LEFT_EYE_OUTER", "RIGHT_EYE_INNER", "RIGHT_EYE", "RIGHT_EYE_OUTER",
                  "LEFT_EAR", "RIGHT_EAR", "MOUTH_LEFT", "MOUTH_RIGHT", "LEFT_SHOULDER", "RIGHT_SHOULDER", "LEFT_ELBOW",
                  "RIGHT_ELBOW", "LEFT_WRIST", "RIGHT_WRIST", "LEFT_PINKY", "RIGHT_PINKY", "LEFT_INDEX", "RIGHT_INDEX",
                  "LEFT_THUMB", "RIGHT_THUMB", "LEFT_HIP", "RIGHT_HIP", "LEFT_KNEE", "RIGHT_KNEE", "LEFT_ANKLE", "RIGHT_ANKLE",
                  "LEFT_HEEL", "RIGHT_HEEL", "LEFT_FOOT_INDEX", "RIGHT_FOOT_INDEX"]
PoseLandmark = enum.IntEnum("PoseLandmark", {n: i for i, n in enumerate(LANDMARK_NAMES)})


class _Landmark:
    def __init__(self, row):
        # MediaPipe's fields are f32; Python reads them as floats
        self.x, self.y, self.z, self.visibility = (float(v) for v in row)


class _Results:
    def __init__(self, lm):
        self.pose_landmarks = None if lm is None else types.SimpleNamespace(landmark=[_Landmark(r) for r in lm])


class _Pose:
    def __init__(self, *a, **k):
        pass

    def process(self, frame):
        return _Results(frame)       # the "frame" handed in is the landmark array itself (or None: no pose)


def _stub_modules():
    mp = types.ModuleType("mediapipe")
    pose = types.SimpleNamespace(Pose=_Pose, PoseLandmark=PoseLandmark)
    mp.solutions = types.SimpleNamespace(pose=pose, drawing_utils=None, drawing_styles=None)
    sys.modules["mediapipe"] = mp
    sys.modules["cv2"] = types.ModuleType("cv2")
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tv.transforms
    mc = types.ModuleType("models_cnn")
    mc.QuadtreeCNN = mc.get_model = None
    sys.modules["models_cnn"] = mc


class _Float64Numpy:
    """numpy with float32 -> float64"""

    def __getattr__(self, name):
        return np.float64 if name == "float32" else getattr(np, name)


def _structured_cases():
    """(name, landmarks [33,4] or None)"""
    base = R.make_landmarks(16, seed=99)
    f = np.float32
    cases = [("no_pose", None)]
    lm = base[0].copy()
    lm[15, :3] = lm[13, :3]                                  # wrist on the elbow
    cases.append(("zero_length_forearm", lm))
    lm = base[1].copy()
    lm[12, :3] = lm[11, :3] + np.array([0.02, 0, 0], f)
    lm[24, :3] = lm[23, :3] + np.array([0, 0.03, 0], f)
    cases.append(("body_scale_below_0.05", lm))
    lm = base[2].copy()
    lm[12, :3] = lm[11, :3]
    cases.append(("shoulder_width_zero", lm))
    for n in (0, 1, 2):
        lm = base[3 + n].copy()
        lm[list(R.TORSO), 3] = [f(0.9) if k < n else f(0.3) for k in range(4)]
        cases.append((f"{n}_visible_torso_landmarks", lm))
    lm = base[6].copy()
    lm[list(R.TORSO), 3] = f(0.9)
    lm[list(R.TORSO), 1] = f(0.4375)
    cases.append(("visible_y_all_equal", lm))
    lm = base[7].copy()                                      # t = (-0.5, 0): on atan2's branch cut
    lm[11, :2], lm[12, :2], lm[23, :2], lm[24, :2] = (0.125, 0.25), (0.375, 0.75), (0.625, 0.75), (0.875, 0.25)
    cases.append(("torso_on_branch_cut", lm))
    lm = base[8].copy()                                      # an elbow at 179.99 degrees
    a = np.deg2rad(179.99)
    lm[13, :3] = (0.5, 0.5, 0.0)
    lm[11, :3] = (0.75, 0.5, 0.0)
    lm[15, :3] = (0.5 + 0.25 * np.cos(a), 0.5 + 0.25 * np.sin(a), 0.0)
    cases.append(("elbow_179.99", lm))
    return cases


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    _stub_modules()
    path = os.path.join(sys.argv[1], "experiment", "test_on_video_cnn.py")
    spec = importlib.util.spec_from_file_location("_reference_video_script", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    rows = [(f"random_{i}", lm) for i, lm in enumerate(R.make_landmarks(64, seed=7))] + _structured_cases()
    names, lms, det, f32s, f64s = [], [], [], [], []
    for name, lm in rows:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")      # the 0 / 0 of a zero-length limb
            got = ref.extract_and_process_features(lm, 0, 0)
            ref.np = _Float64Numpy()
            try:
                got64 = ref.extract_and_process_features(lm, 0, 0)
            finally:
                ref.np = np
        assert got.dtype == np.float32 and got64.dtype == np.float64 and got.shape == got64.shape == (47,)
        if name == "elbow_179.99" and np.isnan(got64[33]):
            continue                             # kept only if the reference's own arccos does not return NaN
        names.append(name)
        lms.append(np.zeros((33, 4), np.float32) if lm is None else lm)
        det.append(0 if lm is None else 1)
        f32s.append(got)
        f64s.append(got64)
    out = os.path.join(HERE, "pose_features.npz")
    np.savez_compressed(out, landmarks=np.stack(lms), detected=np.array(det, np.uint8), features=np.stack(f32s),
                        features64=np.stack(f64s), columns=np.array(ref.SELECTED_FEATURE_COLUMNS), cases=np.array(names))
    print(f"{out}: {len(names)} rows, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
