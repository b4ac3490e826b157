#!/usr/bin/env python3
"""Generate tests/golden/pose_seq.npz by RUNNING THE REFERENCE's own sequence pipeline on the CPU (developer aid; no test and
no GPU run reads the reference checkout).

    python tests/golden/make_pose_seq_golden.py <path of the reference checkout>

Imports "sqn process/processing_image_sequence.py" of the checkout by path and drives its process_image_sequences() itself,
so the reference's own loop and its deque decide every frame's history; nothing of that protocol is restated here.  What the
function touches and this machine may lack is stubbed in sys.modules:
  mediapipe   solutions.pose.Pose is a context manager whose process() returns the next landmark set this script made, or
              no pose; the frames are served in the order the function walks them (sorted clips, sorted files)
  cv2         imread returns a black image of the clip's (H, W) for the empty files of a temporary directory named as
              frames; cvtColor returns it; imwrite is a no-op
  pandas      DataFrame captures the list of per-frame dicts; to_csv is a no-op
and the module's drawing function is replaced by a no-op.  Only data is written: the landmarks, the detected flags, the
clips' lengths and frame sizes, the 443 values per frame as float64 (a key the reference did not write for a frame is NaN,
as pandas leaves it), the reference's column names (the key order of calculate_all_features) and the clip names.  Clips are
padded to 12 frames with undetected frames; `lengths` says how many are real.
"""
import importlib.util
import os
import sys
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _pose_seq_ref as S  # noqa: E402

FRAMES = 12
META = ("clip_id", "frame_index", "original_image_filename", "annotated_image_path")


def clips():
    """(name, landmarks f32 [t,33,4], detected [t], (W, H))"""
    f = np.float32
    out = []

    def walk(seed, t=FRAMES, steady=False):
        lm, _ = S.make_clips(1, t, seed=seed)
        lm = lm[0].copy()
        if steady:
            lm[:, :, 3] = f(0.9)
        return lm

    ones = lambda t=FRAMES: np.ones(t, np.uint8)
    out.append(("random", walk(101), ones(), (640, 480)))
    det = ones()
    det[0] = 0
    out.append(("undetected_first_frame", walk(102), det, (640, 480)))
    for run, t in ((1, 8), (2, 9), (5, 12)):
        det = ones(t)
        det[3:3 + run] = 0
        out.append((f"undetected_run_of_{run}", walk(110 + run, t, steady=True), det, (224, 224)))
    lm = walk(120, 10, steady=True)
    lm[4, 15, 3] = f(0.3)                                      # the left wrist, in frame 4 only: frames 4, 5, 6 lose its motion
    out.append(("landmark_drops_in_one_frame_of_three", lm, ones(10), (640, 480)))
    lm = walk(121, 6, steady=True)
    lm[:, 13, 3] = f(0.65)                                     # exactly 0.65f: not visible
    lm[:, 14, 3] = np.nextafter(f(0.65), f(1))                 # the next f32: visible
    out.append(("visibility_exactly_0.65f", lm, ones(6), (640, 480)))
    lm = walk(122, 6, steady=True)
    lm[:, [23, 24], 3] = f(0.3)
    out.append(("both_hips_invisible", lm, ones(6), (640, 480)))
    lm = walk(123, 6, steady=True)
    lm[:, 12, :3] = lm[:, 11, :3] + np.array([0.02, 0, 0], f)
    lm[:, 24, :3] = lm[:, 23, :3] + np.array([0.2, 0, 0], f)
    out.append(("shoulders_below_scale_hips_above", lm, ones(6), (640, 480)))
    lm = walk(124, 6, steady=True)
    lm[:, 12, :3] = lm[:, 11, :3] + np.array([0.02, 0, 0], f)
    lm[:, 24, :3] = lm[:, 23, :3] + np.array([0, 0.03, 0], f)
    out.append(("shoulders_and_hips_below_scale", lm, ones(6), (640, 480)))
    lm = walk(125, 6, steady=True)
    lm[:, 15, :3] = lm[:, 13, :3]
    out.append(("wrist_on_elbow", lm, ones(6), (640, 480)))
    det = ones()
    det[[2, 7]] = 0
    out.append(("non_square_frame", walk(126), det, (1920, 1080)))
    return out


class _Landmark:
    def __init__(self, row):
        # MediaPipe's fields are f32; Python reads them as floats
        self.x, self.y, self.z, self.visibility = (float(v) for v in row)


class _Feed:
    """what the stubs serve: the frames in the order the reference walks them"""

    def __init__(self, cases):
        self.by_dir = {f"clip_{i:02d}_{name}": (lm, det, size) for i, (name, lm, det, size) in enumerate(cases)}
        self.queue = [(lm[t] if det[t] else None) for _, (lm, det, _) in sorted(self.by_dir.items()) for t in range(len(det))]
        self.frames = []          # the captured DataFrames, one list of dicts per clip

    def install(self):
        feed = self

        class Pose:
            def __init__(self, *a, **k):
                pass

            def __enter__(self):
                return self

            def __exit__(self, *a):
                return False

            def process(self, frame):
                lm = feed.queue.pop(0)
                marks = None if lm is None else types.SimpleNamespace(landmark=[_Landmark(r) for r in lm])
                return types.SimpleNamespace(pose_landmarks=marks)

        mp = types.ModuleType("mediapipe")
        mp.solutions = types.SimpleNamespace(pose=types.SimpleNamespace(Pose=Pose, POSE_CONNECTIONS=frozenset()),
                                             drawing_utils=None, drawing_styles=None)
        cv2 = types.ModuleType("cv2")
        cv2.COLOR_BGR2RGB = 4

        def imread(path):
            w, h = feed.by_dir[os.path.basename(os.path.dirname(path))][2]
            return np.zeros((h, w, 3), np.uint8)

        cv2.imread = imread
        cv2.cvtColor = lambda image, code: image.copy()
        cv2.imwrite = lambda path, image: True
        cv2.line = cv2.circle = lambda *a, **k: None
        pd = types.ModuleType("pandas")

        class DataFrame:
            def __init__(self, rows):
                feed.frames.append(list(rows))

            def to_csv(self, *a, **k):
                pass

        pd.DataFrame = DataFrame
        sys.modules["mediapipe"], sys.modules["cv2"], sys.modules["pandas"] = mp, cv2, pd


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    cases = clips()
    assert all(len(det) <= FRAMES and len(det) == len(lm) for _, lm, det, _ in cases)
    feed = _Feed(cases)
    feed.install()
    path = os.path.join(sys.argv[1], "sqn process", "processing_image_sequence.py")
    spec = importlib.util.spec_from_file_location("_reference_sequence_script", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    ref.draw_enhanced_skeleton = lambda image, *a, **k: image
    ref.print = lambda *a, **k: None
    with tempfile.TemporaryDirectory() as tmp:
        raw, done = os.path.join(tmp, "raw"), os.path.join(tmp, "processed")
        for name, (lm, det, _) in feed.by_dir.items():
            os.makedirs(os.path.join(raw, "train", name))
            for t in range(len(det)):
                open(os.path.join(raw, "train", name, f"frame_{t:05d}.jpg"), "w").close()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref.process_image_sequences(raw, done)
    assert not feed.queue and len(feed.frames) == len(cases)

    columns = None
    for rows in feed.frames:
        for row in rows:
            keys = [k for k in row if k not in META]
            if "TORSO_VAR_XY_RATIO" in row and "LM0_visibility" in row:       # a frame with a pose: the real keys
                columns = columns or keys
                assert keys == columns
    assert columns is not None and len(columns) == S.NUM_FEATURES
    C = len(cases)
    lms = np.zeros((C, FRAMES, 33, 4), np.float32)
    dets = np.zeros((C, FRAMES), np.uint8)
    feats = np.full((C, FRAMES, S.NUM_FEATURES), np.nan)
    for i, ((name, lm, det, size), rows) in enumerate(zip(cases, feed.frames)):      # sorted directory order is case order
        assert len(rows) == len(det) and all(r["clip_id"].endswith(name) and r["frame_index"] == t for t, r in enumerate(rows))
        lms[i, :len(det)], dets[i, :len(det)] = lm, det
        for t, row in enumerate(rows):
            feats[i, t] = [float(row.get(k, np.nan)) for k in columns]
    out = os.path.join(HERE, "pose_seq.npz")
    np.savez_compressed(out, landmarks=lms, detected=dets, lengths=np.array([len(c[2]) for c in cases], np.int32),
                        sizes=np.array([c[3] for c in cases], np.int32), features64=feats, columns=np.array(columns),
                        clips=np.array([c[0] for c in cases]))
    print(f"{out}: {C} clips, {int(sum(len(c[2]) for c in cases))} frames, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
