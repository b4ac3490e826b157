#!/usr/bin/env python
"""What the fixed-lag pose-order posteriors with hold durations cost (developer aid, not a test; not part of bench.py).

16 streams, S = C = 12, D = 64, lag = 16, timed with device events, the variants alternating inside every repeat,
microseconds per call:

  live      one push of 16 streams x 1 frame on a warm stream (the live loop's step)
    duration_lag_smooth   PoseDurationLagSmoother.push(rows)
    duration_lag_begin    PoseDurationLagSmoother.push(rows, by_class=True, begin=True, filtered=True, evidence=True)
    plain_lag_smooth      PoseLagSmoother.push(rows) on the same frames
    duration_lag_decode   PoseDurationLagDecoder.push(rows) on the same frames
    posterior_64          PoseDurationPosterior.smooth of the first 64 frames: what a loop without this class would pay
                          on every frame of a video that is 64 frames old
  catch_up  one push of 16 x 4096 frames with flush on a stream just reset (a recording, or a loop that fell behind)
    duration_lag_smooth   PoseDurationLagSmoother.push(rows, flush=True)
    posterior             PoseDurationPosterior.smooth(rows) of the same videos

The live pushes walk on through the same 4096 frames and start over at their end (`reset`), so a timed window holds the odd
warm-up call; it costs what any other call costs.  Before timing, the joined live outputs and the catch-up outputs are
compared with each other byte for byte, the newest lag + 1 rows with PoseDurationPosterior.smooth's byte for byte, and the
first --check-frames frames of stream 0 with the loops of tests/_pose_duration_lag_posterior_ref.py (--no-check skips that).

    python scripts/bench_pose_duration_lag_posterior.py --out profiles/pose_duration_lag_posterior.json

Prints one JSON line.  No threshold rests on it."""
import argparse
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
    ap.add_argument("--streams", type=int, default=16)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--states", type=int, default=12)
    ap.add_argument("--max-duration", type=int, default=64)
    ap.add_argument("--lag", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50, help="live pushes per timed window")
    ap.add_argument("--catch-up-iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--check-frames", type=int, default=120)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_duration_lag_posterior.py measures on the GPU; there is none")
    import _pose_duration_lag_posterior_ref as LS
    import _pose_order_ref as R
    P = importlib.import_module(PKG)
    M = importlib.import_module(PKG + ".pose_order")
    dev = torch.device("cuda:0")
    B, T, S, D, lag = args.streams, args.frames, args.states, args.max_duration, args.lag
    C = S

    def timed(variants, iters):
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
                for _ in range(iters):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) / iters * 1e3)     # microseconds per call
        return {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                for k, v in times.items()}

    sc, tr = M.cyclic_prior(range(S), stay=M.prob_score(0.9), advance=M.prob_score(0.1), skip=M.prob_score(0.01))
    dur = M.hold_prior(S, D, 4, min(D, 48), inside=M.prob_score(0.05), outside=M.prob_score(0.0005))
    probs_np = R.make_probs(7, B, T, C)
    probs = torch.from_numpy(probs_np).to(dev)
    frames = [probs[:, f:f + 1].contiguous() for f in range(T)]
    head = probs[:, :64].contiguous()
    live = P.PoseDurationLagSmoother(sc, tr, dur, dev, lag, streams=B)
    live_all = P.PoseDurationLagSmoother(sc, tr, dur, dev, lag, streams=B)
    batch = P.PoseDurationLagSmoother(sc, tr, dur, dev, lag, streams=B)
    whole = P.PoseDurationPosterior(sc, tr, dur, dev, streams=B)
    whole_64 = P.PoseDurationPosterior(sc, tr, dur, dev, streams=B)
    plain_live = P.PoseLagSmoother(sc, tr, dev, lag, streams=B)
    path_live = P.PoseDurationLagDecoder(sc, tr, dur, dev, lag, streams=B)
    extras = dict(by_class=True, begin=True, filtered=True, evidence=True)

    # the joined live pushes are the catch-up push; the newest lag + 1 rows are the whole-video posterior's
    parts = [live.push(frames[f], **extras)[1:] for f in range(T)] + [live.push(probs[:, :0], flush=True, **extras)[1:]]
    outs = batch.push(probs, flush=True, **extras)[1:]
    for i in range(5):
        assert torch.equal(torch.cat([p[i] for p in parts], dim=1), outs[i]), i
    w_post, w_cls, w_begin, w_ev = whole.smooth(probs, by_class=True, begin=True, evidence=True)
    for got, want in zip(outs[:3], (w_post, w_cls, w_begin)):
        assert torch.equal(got[:, T - lag - 1:], want[:, T - lag - 1:])
    assert torch.equal(outs[4][:, -1], w_ev)
    if not args.no_check:
        n = min(args.check_frames, T)
        dur_open = np.maximum.accumulate(dur[:, ::-1], axis=1)[:, ::-1].copy()
        ref = [LS.smooth(probs_np[:1, :n], sc, tr, dur, None, dur_open, lag=lag, flush=False, F=F)[1] for F in (np.float64, np.float32)]
        m = ref[0][0].shape[1]
        e_k = max(float(np.abs(outs[i][:1, :m].cpu().numpy().astype(np.float64) - ref[0][i]).max()) for i in range(3))
        e_m = max(float(np.abs(ref[1][i].astype(np.float64) - ref[0][i]).max()) for i in range(3))
        assert e_k <= 4 * e_m + 2.0 ** -20, ("the device result differs from the rule", e_k, e_m)
    live.reset()

    def stepper(obj, **kw):
        def step():
            if obj.seen == T:
                obj.reset()
            obj.push(frames[obj.seen], **kw)
        return step

    us_live = timed({"duration_lag_smooth": stepper(live), "duration_lag_begin": stepper(live_all, **extras),
                     "plain_lag_smooth": stepper(plain_live), "duration_lag_decode": stepper(path_live),
                     "posterior_64": lambda: whole_64.smooth(head)}, args.iters)
    us_batch = timed({"duration_lag_smooth": lambda: batch.reset().push(probs, flush=True),
                      "posterior": lambda: whole.smooth(probs)}, args.catch_up_iters)
    med = lambda d, k: d[k]["median"]
    rec = {"device": torch.cuda.get_device_name(0), "streams": B, "frames": T, "states": S, "max_duration": D, "lag": lag,
           "iters": args.iters, "catch_up_iters": args.catch_up_iters, "repeats": args.repeats,
           "carry_bytes_per_stream": live._carry[0].numel() // B,
           "live_us_per_push": us_live, "catch_up_us_per_push": us_batch,
           "live_over_plain_smooth": round(med(us_live, "duration_lag_smooth") / med(us_live, "plain_lag_smooth"), 2),
           "live_over_duration_decode": round(med(us_live, "duration_lag_smooth") / med(us_live, "duration_lag_decode"), 2),
           "live_over_posterior_64": round(med(us_live, "duration_lag_smooth") / med(us_live, "posterior_64"), 2),
           "catch_up_over_whole_video": round(med(us_batch, "duration_lag_smooth") / med(us_batch, "posterior"), 3),
           "catch_up_us_per_frame": round(med(us_batch, "duration_lag_smooth") / T, 4)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
