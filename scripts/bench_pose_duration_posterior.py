#!/usr/bin/env python
"""What the pose-order posteriors with hold durations cost (developer aid, not a test; not part of bench.py).

Whole videos of 9,000 frames (five minutes at 30 frames a second), the shapes of scripts/bench_pose_duration.py, timed with
device events, the variants alternating inside every repeat, microseconds per call:

  one        S = C = 12, D = 64, one stream
  sixteen    S = C = 12, D = 64, sixteen streams, ragged lengths
  wide       S = C = 64, D = 128, one stream (the limits)

  posterior     qt_pose_duration_posterior through ctypes into preallocated buffers: posterior, class_posterior, begin and
                the evidence, dur_counts NULL
  counts        the same call with dur_counts too (the second launch included)
  counts_only   dur_counts alone, every other output NULL
  smooth        PoseDurationPosterior.smooth(by_class=True, begin=True, evidence=True): the launch, the allocations, the Python
  decoder       PoseDurationDecoder.decode(start=True, score=True) on the same inputs in the same process
  copy          a device-to-device copy of the probabilities' bytes

and per shape `us_per_frame` of posterior, counts and decoder (the call over the frames of its longest stream: one workgroup
walks each stream's frames in order, the streams side by side) and their ratios to the decoder.  Before timing, the device
results are held against the float64 loops of tests/_pose_duration_posterior_ref.py on the first 600 frames of the same data
(the figures are printed; --no-check skips it).

    python scripts/bench_pose_duration_posterior.py --out profiles/pose_duration_posterior.json

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
SHAPES = (("one", 1, 12, 64), ("sixteen", 16, 12, 64), ("wide", 1, 64, 128))      # name, streams, S = C, D
CHECK_FRAMES = 600


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=9000)
    ap.add_argument("--iters", type=int, default=5, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="one,sixteen,wide")
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_duration_posterior.py measures on the GPU; there is none")
    import _pose_duration_posterior_ref as PR
    import _pose_order_ref as R
    P = importlib.import_module(PKG)
    M, Lm = importlib.import_module(PKG + ".pose_order"), importlib.import_module(PKG + "._lib")
    L = Lm.lib()
    dev = torch.device("cuda:0")

    def timed(variants):
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
        return {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                for k, v in times.items()}

    T = args.frames
    rec = {"device": torch.cuda.get_device_name(0), "frames": T, "iters": args.iters, "repeats": args.repeats, "shapes": {}}
    for name, B, S, D in SHAPES:
        if name not in args.shapes.split(","):
            continue
        C = S
        sc, tr = M.cyclic_prior(range(S), stay=M.prob_score(0.9), advance=M.prob_score(0.1), skip=M.prob_score(0.01))
        dur = M.hold_prior(S, D, 4, min(D, 48), inside=M.prob_score(0.05), outside=M.prob_score(0.0005))
        dur_open = np.maximum.accumulate(dur[:, ::-1], axis=1)[:, ::-1].copy()
        probs_np = R.make_probs(7, B, T, C)
        lengths_np = None if B == 1 else np.maximum(T - 137 * np.arange(B), 1).astype(np.int32)
        probs = torch.from_numpy(probs_np).to(dev)
        t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d_sc, d_tr, d_dur, d_open, d_len = t(sc), t(tr), t(dur), t(dur_open), t(lengths_np)
        post = torch.empty(B, T, S, dtype=torch.float32, device=dev)
        cls = torch.empty(B, T, C, dtype=torch.float32, device=dev)
        begin = torch.empty(B, T, S, dtype=torch.float32, device=dev)
        ev = torch.empty(B, dtype=torch.float64, device=dev)
        counts = torch.zeros(S, D, dtype=torch.float64, device=dev)
        sink = torch.empty_like(probs)
        desc = M.PoseDurationDesc(B, T, C, S, D)
        need = L.qt_pose_duration_posterior_workspace_bytes(ctypes.byref(desc))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)

        def call(p, c, b, e, n):
            Lm.check(L.qt_pose_duration_posterior(ctypes.byref(desc), Lm.ptr(probs), C, Lm.ptr(d_sc), Lm.ptr(d_tr), None,
                                                  Lm.ptr(d_dur), Lm.ptr(d_open), Lm.ptr(d_len), Lm.ptr(p), Lm.ptr(c), Lm.ptr(b),
                                                  Lm.ptr(e), Lm.ptr(n), Lm.ptr(ws), need, Lm.stream_ptr()),
                     "qt_pose_duration_posterior")

        smoother = P.PoseDurationPosterior(sc, tr, dur, dev, streams=B)
        decoder = P.PoseDurationDecoder(sc, tr, dur, dev, streams=B)
        call(post, cls, begin, ev, None)
        got = smoother.smooth(probs, lengths=d_len, by_class=True, begin=True, evidence=True)
        assert all(torch.equal(g, w) for g, w in zip(got, (post, cls, begin, ev)))
        check = None
        if not args.no_check:
            n = min(T, CHECK_FRAMES)
            short = P.PoseDurationPosterior(sc, tr, dur, dev, streams=B)
            head = probs[:, :n].contiguous()
            head_len = None if d_len is None else d_len.clamp(max=n)
            g_post, g_begin, g_ev = short.smooth(head, lengths=head_len, begin=True, evidence=True)
            g_counts = short.expected_durations(head, head_len)
            want = PR.loops64(probs_np[:, :n], sc, tr, dur, None, dur_open, None if lengths_np is None else np.minimum(lengths_np, n))
            check = {"frames": n,
                     "posterior": float(np.abs(g_post.cpu().numpy() - want[0]).max()),
                     "begin": float(np.abs(g_begin.cpu().numpy() - want[2]).max()),
                     "evidence_rel": float((np.abs(g_ev.cpu().numpy() - want[3]) / np.maximum(1.0, np.abs(want[3]))).max()),
                     "dur_counts_rel": float((np.abs(g_counts.cpu().numpy() - want[4]) / np.maximum(1.0, want[4])).max())}
            assert max(check["posterior"], check["begin"], check["evidence_rel"], check["dur_counts_rel"]) < 1e-4, check
            del short
        us = timed({"posterior": lambda: call(post, cls, begin, ev, None), "counts": lambda: call(post, cls, begin, ev, counts),
                    "counts_only": lambda: call(None, None, None, None, counts),
                    "smooth": lambda: smoother.smooth(probs, lengths=d_len, by_class=True, begin=True, evidence=True),
                    "decoder": lambda: decoder.decode(probs, lengths=d_len, start=True, score=True),
                    "copy": lambda: sink.copy_(probs)})
        per = lambda k: round(us[k]["median"] / T, 4)
        rec["shapes"][name] = {"streams": B, "states": S, "max_duration": D, "workspace_bytes": need, "us_per_call": us,
                               "us_per_frame": {k: per(k) for k in ("posterior", "counts", "decoder")},
                               "over_decoder": {k: round(us[k]["median"] / us["decoder"]["median"], 2)
                                                for k in ("posterior", "counts", "counts_only")},
                               "check_against_float64": check}
        del smoother, decoder, probs, sink, ws
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
