#!/usr/bin/env python
"""What the sequence pose features on the device cost (developer aid, not a test; not part of bench.py).

256 clips x 64 frames with 10 % of the frames undetected, 640 x 480, timed with device events, the variants alternating inside
every repeat:

  kernel       qt_pose_sequence_features through ctypes into a preallocated output, mode "zero", no history
               (csrc/pose_seq.hip): 528 B read and 1772 B written per frame
  wrapper      SequencePoseFeatures.from_landmarks with a history carried (allocates the output, swaps the history buffers)
  copy         a device-to-device copy of frames x 528 bytes followed by one of frames x 1772 bytes (the same arrays read
               AND written: twice the kernel's traffic, in two launches)
  copy_out     the copy of frames x 1772 bytes alone

and, on one host core, the float64 restatement of tests/_pose_seq_ref.py frame by frame with the history carried (the form
the reference's loop has), in frames per second.

    python scripts/bench_pose_seq.py --out profiles/pose_seq.json

Prints one JSON line.  No threshold rests on it."""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "multimodal-hierarchical-cnn-for-sun-salutation-pose-classification_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-seconds", type=float, default=1.0, help="length of the host-core measurement")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_seq.py measures on the GPU; there is none")
    import _pose_seq_ref as S
    P = importlib.import_module(PKG)
    M, Lm = importlib.import_module(PKG + ".pose_sequence"), importlib.import_module(PKG + "._lib")
    dev = torch.device("cuda:0")
    B, T = args.clips, args.frames
    lm_host, det_host = S.make_clips(B, T, seed=1, undetected=0.1)
    lm, det = torch.from_numpy(lm_host).to(dev), torch.from_numpy(det_host).to(dev)
    seq = P.SequencePoseFeatures("zero", frame_size=(640, 480))
    hist = seq.history(B, dev)
    out = seq.from_landmarks(lm, det)
    lm_sink, out_sink = torch.empty_like(lm), torch.empty_like(out)
    L = Lm.lib()
    desc = M.PoseSeqDesc(B, T, 640, 480, M.QT_POSE_ZERO)

    def kernel():
        Lm.check(L.qt_pose_sequence_features(ctypes.byref(desc), Lm.ptr(lm), Lm.ptr(det), None, None, None, None, None,
                                             Lm.ptr(out), Lm.stream_ptr()), "qt_pose_sequence_features")

    def copy():
        lm_sink.copy_(lm)
        out_sink.copy_(out)

    variants = {"kernel": kernel, "wrapper": lambda: seq.from_landmarks(lm, det, history=hist), "copy": copy,
                "copy_out": lambda: out_sink.copy_(out)}
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.iters * 1e3)     # microseconds per call
    rec = {"device": torch.cuda.get_device_name(0), "clips": B, "frames": T, "undetected": round(float(1 - det_host.mean()), 4),
           "iters": args.iters, "repeats": args.repeats, "bytes_read": B * T * 528, "bytes_written": B * T * 1772,
           "us_per_call": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                           for k, v in times.items()}}
    k = rec["us_per_call"]["kernel"]["median"]
    rec["kernel_gb_per_s"] = round(B * T * 2300 / k * 1e-3, 1)
    rec["kernel_frames_per_second"] = round(B * T / k * 1e6)
    rec["host_float64_frames_per_second"] = round(S.reference_frames_per_second(lm_host[:4], det_host[:4], (640, 480),
                                                                                args.host_seconds), 1)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
