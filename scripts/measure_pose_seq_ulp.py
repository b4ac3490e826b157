#!/usr/bin/env python
"""Largest ulp error of the device's atan2f and sqrtf on the arguments the sequence-feature kernel produces (developer aid;
the source of MEASURED_ATAN2 / MEASURED_SQRT in tests/_pose_seq_ref.py and of the figures in EXPERIMENTS.md, "Sequence pose
features").  scripts/measure_pose_ulp.py sampled the 47-vector's arguments, which are in normalised coordinates; the angles
and distances of csrc/pose_seq.hip are taken in pixel space, |ba x bc| and ba . bc up to W^2 times larger, so the
measurement is repeated on them.

The arguments are those of tests/_pose_seq_ref.py::function_arguments on make_clips(16, 64) at 640 x 480, 1920 x 1080 and
224 x 224 and on the clips of tests/golden/pose_seq.npz.  scripts/pose_ulp.hip (built with the flags of csrc/Makefile into
build/, unless build/pose_ulp is there already) evaluates the two functions on the GPU; the results are compared with
numpy's float64 ones, in units of the f32 spacing at the exact value.

    python scripts/measure_pose_seq_ulp.py [--out profiles/pose_seq_ulp.json]

Prints one JSON line.  No test runs this."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from measure_pose_ulp import FLAGS, ulp_error  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    args = ap.parse_args()
    import _pose_seq_ref as S
    build = os.path.join(ROOT, "build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "pose_ulp")
    if not os.path.exists(exe):
        subprocess.run([args.hipcc] + FLAGS + [os.path.join(ROOT, "scripts", "pose_ulp.hip"), "-o", exe], check=True)
    fixture = np.load(os.path.join(ROOT, "tests", "golden", "pose_seq.npz"))
    lm, det = S.make_clips(16, 64, undetected=0.1)
    parts = [S.function_arguments(lm, det, size) for size in ((640, 480), (1920, 1080), (224, 224))]
    parts.append(S.function_arguments(fixture["landmarks"], fixture["detected"], fixture["sizes"]))
    y, x, q = (np.concatenate([p[k] for p in parts]) for k in range(3))
    src, dst = os.path.join(build, "pose_seq_ulp_in.bin"), os.path.join(build, "pose_seq_ulp_out.bin")
    with open(src, "wb") as f:
        np.array([y.size, q.size], np.int32).tofile(f)
        for a in (y, x, q):
            a.astype(np.float32).tofile(f)
    subprocess.run([exe, src, dst], check=True)
    got = np.fromfile(dst, dtype=np.float32)
    assert got.size == y.size + q.size
    at = ulp_error(got[:y.size], np.arctan2(y.astype(np.float64), x.astype(np.float64)))
    sq = ulp_error(got[y.size:], np.sqrt(q.astype(np.float64)))
    rec = {"atan2f": {"arguments": int(y.size), "max_ulp": float(at.max()), "mean_ulp": float(at.mean()),
                      "largest_argument": float(max(np.abs(y).max(), np.abs(x).max()))},
           "sqrtf": {"arguments": int(q.size), "max_ulp": float(sq.max()), "mean_ulp": float(sq.mean()),
                     "largest_argument": float(q.max())}}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
