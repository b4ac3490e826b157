#!/usr/bin/env python
"""What one E-step of the pose-order learner costs (developer aid, not a test; not part of bench.py).

The three shapes of scripts/bench_pose_posterior.py, S = C = 12 (a cycle over the twelve steps), timed with device events, the
variants alternating inside every repeat, microseconds per call:

  live      16 streams x 1 frame (short route; a learner never sees such a call, the shape is kept for the comparison)
  batch     64 videos x 256 frames (tiled route, four tiles per video)
  offline   one video of 65,536 frames in one call (tiled route, 1,024 tiles)

  expect        qt_pose_prior_expect alone, through ctypes, onto accumulators that are never zeroed (the values do not matter)
  posterior     qt_pose_posterior on the same input (posterior only), behind a carry.zero_() so that every call sees a whole video
  carry_zero    that carry.zero_() alone, to subtract
  accumulate    PoseOrderLearner.accumulate: the launches and the Python
  count_paths   qt_pose_prior_count_paths on a path of the same length
  update        qt_pose_prior_update alone

Before timing, the E-step's counts are measured against the float64 loops of tests/_pose_prior_ref.py (shapes of up to 2^14
frames; the host loops take a minute at 65,536).

    python scripts/bench_pose_prior.py --out profiles/pose_prior.json

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
SHAPES = (("live", 16, 1), ("batch", 64, 256), ("offline", 1, 1 << 16))
S = C = 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="live,batch,offline")
    ap.add_argument("--no-host", action="store_true", help="skip the host loops and the comparison with them (for a trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_prior.py measures on the GPU; there is none")
    import _pose_order_ref as O
    import _pose_prior_ref as R
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

    sc, tr = M.cyclic_prior(range(S), stay=M.prob_score(0.9), advance=M.prob_score(0.1), skip=M.prob_score(0.01))
    rec = {"device": torch.cuda.get_device_name(0), "states": S, "classes": C, "iters": args.iters, "repeats": args.repeats,
           "shapes": {}}
    for name, B, T in SHAPES:
        if name not in args.shapes.split(","):
            continue
        probs_np = O.make_probs(7, B, T, C)
        probs = torch.from_numpy(probs_np).to(dev)
        d_sc, d_tr = torch.from_numpy(sc).to(dev), torch.from_numpy(tr).to(dev)
        counts = torch.zeros(S, S, dtype=torch.float64, device=dev)
        start = torch.zeros(S, dtype=torch.float64, device=dev)
        totals = torch.zeros(2, dtype=torch.float64, device=dev)
        desc = M.PoseOrderDesc(B, T, C, S)
        need = L.qt_pose_prior_workspace_bytes(ctypes.byref(desc))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)

        def expect():
            Lm.check(L.qt_pose_prior_expect(ctypes.byref(desc), Lm.ptr(probs), C, Lm.ptr(d_sc), Lm.ptr(d_tr), None, Lm.ptr(counts),
                                            Lm.ptr(start), Lm.ptr(totals), Lm.ptr(ws), need, Lm.stream_ptr()), "qt_pose_prior_expect")

        carry = torch.zeros(B, S + 2, dtype=torch.float64, device=dev)
        post = torch.empty(B, T, S, dtype=torch.float32, device=dev)
        p_need = L.qt_pose_posterior_workspace_bytes(ctypes.byref(desc))
        p_ws = torch.empty(max(p_need, 8), dtype=torch.uint8, device=dev)

        def posterior():
            carry.zero_()
            Lm.check(L.qt_pose_posterior(ctypes.byref(desc), Lm.ptr(probs), C, Lm.ptr(d_sc), Lm.ptr(d_tr), None, Lm.ptr(carry),
                                         Lm.ptr(post), None, None, None, Lm.ptr(p_ws) if p_need else None, p_need,
                                         Lm.stream_ptr()), "qt_pose_posterior")

        path = torch.from_numpy((np.arange(B * T).reshape(B, T) // 5) % S).to(dev)

        def count_paths():
            Lm.check(L.qt_pose_prior_count_paths(ctypes.byref(desc), Lm.ptr(path), Lm.ptr(counts), Lm.ptr(start), Lm.ptr(totals),
                                                 Lm.ptr(ws), need, Lm.stream_ptr()), "qt_pose_prior_count_paths")

        allowed = torch.ones(S, S, dtype=torch.int32, device=dev)
        new_tr = torch.empty_like(d_tr)

        def update():
            Lm.check(L.qt_pose_prior_update(S, Lm.ptr(counts), Lm.ptr(start), Lm.ptr(allowed), 0.0, Lm.ptr(d_tr), None,
                                            Lm.ptr(new_tr), None, Lm.stream_ptr()), "qt_pose_prior_update")

        error = None
        if not args.no_host and B * T <= 1 << 14:
            counts.zero_(), start.zero_(), totals.zero_()
            expect()
            want = R.loops64(probs_np, sc, tr)
            got = [t.cpu().numpy() for t in (counts, start, totals)]
            error = {"counts_relative": float(max((np.abs(g - w) / np.maximum(1.0, w)).max() for g, w in zip(got[:2], want[:2]))),
                     "evidence_relative": float(abs(got[2][0] - want[2][0]) / max(1.0, abs(want[2][0])))}
            assert error["counts_relative"] <= 1e-4, f"{name}: the device result is not the rule's"
        learner = P.PoseOrderLearner(sc, tr, dev)
        us = timed({"expect": expect, "posterior": posterior, "carry_zero": lambda: carry.zero_(),
                    "accumulate": lambda: learner.accumulate(probs), "count_paths": count_paths, "update": update})
        net = us["posterior"]["median"] - us["carry_zero"]["median"]
        rec["shapes"][name] = {"streams": B, "frames": T, "workspace_bytes": need, "posterior_workspace_bytes": p_need,
                               "us_per_call": us, "expect_over_posterior": round(us["expect"]["median"] / net, 2),
                               "error": error}
        del learner, probs, ws, p_ws, post
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
