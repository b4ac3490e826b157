#!/usr/bin/env python
"""Largest ulp error of the device's atan2f and sqrtf on the arguments the pose kernel's tests produce (developer aid; the
source of MEASURED_ATAN2 / MEASURED_SQRT in tests/_pose_ref.py and of the figures in EXPERIMENTS.md, "Pose features").

The arguments are those of tests/_pose_ref.py::function_arguments on make_landmarks(4096, 1234) and on the rows of
tests/golden/pose_features.npz.  scripts/pose_ulp.hip, a stand-alone program built here with the flags of csrc/Makefile
(into build/, unless build/pose_ulp is there already), evaluates the two functions on the GPU; the results are compared
with numpy's float64 ones, in units of the f32 spacing at the exact value.

    python scripts/measure_pose_ulp.py [--out profiles/pose_ulp.json]

Prints one JSON line.  No test runs this."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=fast"]      # csrc/Makefile's


def ulp_error(got, exact):
    exact = np.asarray(exact, dtype=np.float64)
    spacing = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - exact) / spacing


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    args = ap.parse_args()
    import _pose_ref as R
    build = os.path.join(ROOT, "build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "pose_ulp")
    if not os.path.exists(exe):
        subprocess.run([args.hipcc] + FLAGS + [os.path.join(ROOT, "scripts", "pose_ulp.hip"), "-o", exe], check=True)
    fixture = np.load(os.path.join(ROOT, "tests", "golden", "pose_features.npz"))
    parts = [R.function_arguments(R.make_landmarks(R.ROWS, R.SEED)),
             R.function_arguments(fixture["landmarks"][fixture["detected"] != 0])]
    y, x, q = (np.concatenate([p[k] for p in parts]) for k in range(3))
    src, dst = os.path.join(build, "pose_ulp_in.bin"), os.path.join(build, "pose_ulp_out.bin")
    with open(src, "wb") as f:
        np.array([y.size, q.size], np.int32).tofile(f)
        for a in (y, x, q):
            a.astype(np.float32).tofile(f)
    subprocess.run([exe, src, dst], check=True)
    got = np.fromfile(dst, dtype=np.float32)
    assert got.size == y.size + q.size
    at = ulp_error(got[:y.size], np.arctan2(y.astype(np.float64), x.astype(np.float64)))
    sq = ulp_error(got[y.size:], np.sqrt(q.astype(np.float64)))
    rec = {"atan2f": {"arguments": int(y.size), "max_ulp": float(at.max()), "mean_ulp": float(at.mean())},
           "sqrtf": {"arguments": int(q.size), "max_ulp": float(sq.max()), "mean_ulp": float(sq.mean())}}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
