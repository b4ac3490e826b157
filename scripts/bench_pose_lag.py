#!/usr/bin/env python
"""What the fixed-lag pose-order posteriors and revised paths cost (developer aid, not a test; not part of bench.py).

The three shapes of scripts/bench_pose_posterior.py, S = C = 12 (a cycle over the twelve steps), lag 16, timed with device
events, the variants alternating inside every repeat, microseconds per call, through ctypes into preallocated buffers:

  live      16 streams x 1 frame, a step of a live loop: the stream is 64 frames old, so the call emits one frame per stream
  batch     64 streams x 256 frames in one call with flush (catching up)
  offline   one recording of 65,536 frames in one call with flush

  lag_smooth / lag_decode              qt_pose_lag_smooth (lagged, lagged_class, filtered, evidence) / qt_pose_lag_decode (lag_path,
                                       filtered) on the route the library picks
  lag_smooth_live / lag_smooth_batch   the same with QTCNN_POSE_LAG=1 / 2 (likewise lag_decode_*); the forced live route on the
                                       two long shapes runs a tenth of the iterations (one on the offline shape)
  posterior / decode                   qt_pose_posterior / qt_pose_order_decode on the same input in the same run, each behind the
                                       carry.zero_() that makes every call see the same video
  carry_zero                           that carry.zero_() alone, to subtract (the lag calls need none: carry_in is not written)

and `sweep`: 16 streams, n = 1 .. 16 new frames at lags 5, 16 and 63, both routes of both calls: where the batch route's second
launch starts to pay, which is what the threshold on n (lag + 1) in csrc/pose_posterior.hip rests on.  Before timing, both routes
must give the same bits, and on the two smaller shapes the result is held against the float64 loops of tests/_pose_lag_ref.py.

    python scripts/bench_pose_lag.py --out profiles/pose_lag.json

Prints one JSON line.  No threshold of a test rests on it."""
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
SHAPES = (("live", 16, 1, 64), ("batch", 64, 256, 0), ("offline", 1, 1 << 16, 0))      # name, streams, new frames, frames seen
S = C = 12
LAG = 16
SWITCH = "QTCNN_POSE_LAG"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="live,batch,offline,sweep")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_lag.py measures on the GPU; there is none")
    import _pose_lag_ref as G
    import _pose_order_ref as O
    M, Lm = importlib.import_module(PKG + ".pose_order"), importlib.import_module(PKG + "._lib")
    L = Lm.lib()
    dev = torch.device("cuda:0")
    os.environ.pop(SWITCH, None)

    def timed(variants):
        for fn, iters in variants.values():
            for _ in range(min(args.warmup, iters)):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(args.repeats):
            for name, (fn, iters) in variants.items():
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
    d_sc, d_tr = torch.from_numpy(sc).to(dev), torch.from_numpy(tr).to(dev)

    class Lagged:
        """one call of either function at a fixed place in a stream: the `seen` frames in front go through once, their carry is
        the carry_in of every timed call"""

        def __init__(self, which, probs_np, seen, lag, flush):
            self.which, self.lag, self.flush = which, lag, flush
            B, total, _ = probs_np.shape
            self.B, self.T, self.seen = B, total - seen, seen
            self.probs = torch.from_numpy(np.ascontiguousarray(probs_np[:, seen:])).to(dev)
            g0, g1 = G.span(seen, self.T, lag, flush)
            self.g0, self.count = g0, g1 - g0
            smooth = which == "smooth"
            self.fn = L.qt_pose_lag_smooth if smooth else L.qt_pose_lag_decode
            self.ws_query = L.qt_pose_lag_smooth_workspace_bytes if smooth else L.qt_pose_lag_decode_workspace_bytes
            carry_query = L.qt_pose_lag_smooth_carry_bytes if smooth else L.qt_pose_lag_decode_carry_bytes
            self.desc = M.PoseLagDesc(B, self.T, C, S, lag, int(flush), seen)
            nbytes = int(carry_query(ctypes.byref(self.desc)))
            self.carry_in = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
            self.carry_out = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
            if smooth:
                self.outs = [torch.empty(B, self.count, S, dtype=torch.float32, device=dev),
                             torch.empty(B, self.count, C, dtype=torch.float32, device=dev),
                             torch.empty(B, self.T, S, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float64, device=dev)]
            else:
                self.outs = [torch.empty(B, self.count, dtype=torch.int64, device=dev), torch.empty(B, self.T, dtype=torch.int64, device=dev)]
            self.ws = {}
            for forced in (None, "1", "2"):
                self._switch(forced)
                need = int(self.ws_query(ctypes.byref(self.desc)))
                self.ws[forced] = (torch.empty(max(need, 8), dtype=torch.uint8, device=dev), need)
            self._switch(None)
            if seen:
                head = torch.from_numpy(np.ascontiguousarray(probs_np[:, :seen])).to(dev)
                desc = M.PoseLagDesc(B, seen, C, S, lag, 0, 0)
                need = int(self.ws_query(ctypes.byref(desc)))
                ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
                sink = [torch.empty(B * seen * max(S, C), dtype=torch.float64, device=dev) for _ in self.outs]
                Lm.check(self.fn(ctypes.byref(desc), Lm.ptr(head), C, Lm.ptr(d_sc), Lm.ptr(d_tr), None, None, Lm.ptr(self.carry_in),
                                 *[Lm.ptr(t) for t in sink], Lm.ptr(ws) if need else None, need, Lm.stream_ptr()), "the frames in front")

        @staticmethod
        def _switch(forced):
            os.environ.pop(SWITCH, None)
            if forced is not None:
                os.environ[SWITCH] = forced

        def __call__(self, forced=None):
            self._switch(forced)
            ws, need = self.ws[forced]
            rc = self.fn(ctypes.byref(self.desc), Lm.ptr(self.probs), C, Lm.ptr(d_sc), Lm.ptr(d_tr), None,
                         Lm.ptr(self.carry_in) if self.seen else None, Lm.ptr(self.carry_out), *[Lm.ptr(t) for t in self.outs],
                         Lm.ptr(ws) if need else None, need, Lm.stream_ptr())
            self._switch(None)
            Lm.check(rc, "qt_pose_lag_" + self.which)

        def results(self, forced):
            for t in self.outs:
                t.fill_(float("nan") if t.is_floating_point() else -1)
            self.carry_out.fill_(0xFF)
            self(forced)
            return [t.cpu().numpy() for t in self.outs] + [self.carry_out.cpu().numpy()]

    rec = {"device": torch.cuda.get_device_name(0), "states": S, "classes": C, "lag": LAG, "iters": args.iters,
           "repeats": args.repeats, "shapes": {}}
    wanted = args.shapes.split(",")
    for name, B, T, seen in SHAPES:
        if name not in wanted:
            continue
        probs_np = O.make_probs(7, B, seen + T, C)
        flush = seen == 0
        smooth, decode = Lagged("smooth", probs_np, seen, LAG, flush), Lagged("decode", probs_np, seen, LAG, flush)
        errors = {}
        for call in (smooth, decode):                                  # both routes, the same bits; then against the loops
            live, batch = call.results("1"), call.results("2")
            assert all(O.bits(a) == O.bits(b) for a, b in zip(live, batch)), f"{name}/{call.which}: the routes differ"
            assert all(np.isfinite(g).all() for g in live[:-1] if g.dtype.kind == "f"), f"{name}/{call.which}: an output was not written"
        if B * (seen + T) <= 1 << 14:
            ref = G.split(G.smooth, probs_np, [seen] if seen else [], sc, tr, None, lag=LAG, flush_last=flush, F=np.float64)[3][-1][1]
            got = smooth.results(None)
            errors["probabilities"] = float(max(np.abs(g - w).max() for g, w in zip(got[:3], ref[:3])))
            assert errors["probabilities"] <= 1e-4, f"{name}: the device result is not the rule's"
            want = G.split(G.decode, probs_np, [seen] if seen else [], sc, tr, None, lag=LAG, flush_last=flush)[3][-1][1]
            assert (decode.results(None)[0] == want[0]).all(), f"{name}: the device path is not the rule's"

        probs = smooth.probs
        desc = M.PoseOrderDesc(B, T, C, S)
        carry = torch.zeros(B, S + 2, dtype=torch.float64, device=dev)
        post, filt = (torch.empty(B, T, S, dtype=torch.float32, device=dev) for _ in range(2))
        cls, ev = torch.empty(B, T, C, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float64, device=dev)
        need = L.qt_pose_posterior_workspace_bytes(ctypes.byref(desc))
        ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)

        def posterior():
            carry.zero_()
            Lm.check(L.qt_pose_posterior(ctypes.byref(desc), Lm.ptr(probs), C, Lm.ptr(d_sc), Lm.ptr(d_tr), None, Lm.ptr(carry),
                                         Lm.ptr(post), Lm.ptr(filt), Lm.ptr(cls), Lm.ptr(ev), Lm.ptr(ws) if need else None, need,
                                         Lm.stream_ptr()), "qt_pose_posterior")

        d_carry = torch.zeros(B, S + 2, dtype=torch.int64, device=dev)
        path, d_filt = (torch.empty(B, T, dtype=torch.int64, device=dev) for _ in range(2))
        emis = torch.empty(B, T, S, dtype=torch.int32, device=dev)
        d_need = L.qt_pose_order_workspace_bytes(ctypes.byref(desc))
        d_ws = torch.empty(max(d_need, 8), dtype=torch.uint8, device=dev)

        def order_decode():
            d_carry.zero_()
            Lm.check(L.qt_pose_order_decode(ctypes.byref(desc), Lm.ptr(probs), C, Lm.ptr(d_sc), Lm.ptr(d_tr), None,
                                            Lm.ptr(d_carry), Lm.ptr(path), Lm.ptr(d_filt), Lm.ptr(emis),
                                            Lm.ptr(d_ws) if d_need else None, d_need, Lm.stream_ptr()), "qt_pose_order_decode")

        slow = args.iters if T == 1 else (max(args.iters // 10, 2) if T < 1 << 12 else 1)
        variants = {"lag_smooth": (smooth, args.iters), "lag_decode": (decode, args.iters),
                    "lag_smooth_live": (lambda: smooth("1"), slow), "lag_smooth_batch": (lambda: smooth("2"), args.iters),
                    "lag_decode_live": (lambda: decode("1"), slow), "lag_decode_batch": (lambda: decode("2"), args.iters),
                    "posterior": (posterior, args.iters), "decode": (order_decode, args.iters),
                    "carry_zero": (lambda: carry.zero_(), args.iters)}
        rec["shapes"][name] = {"streams": B, "frames": T, "seen": seen, "emitted": smooth.count, "flush": flush,
                               "workspace_bytes": {"smooth": smooth.ws[None][1], "decode": decode.ws[None][1]},
                               "us_per_call": timed(variants), "max_abs_error": errors}
        del smooth, decode, probs, ws, d_ws
    if "sweep" in wanted:
        rec["sweep"] = {}
        for lag in (5, 16, 63):
            for n in (1, 2, 3, 4, 8, 16):
                probs_np = O.make_probs(9, 16, 64 + n, C)
                smooth, decode = Lagged("smooth", probs_np, 64, lag, False), Lagged("decode", probs_np, 64, lag, False)
                us = timed({"smooth_live": (lambda: smooth("1"), args.iters), "smooth_batch": (lambda: smooth("2"), args.iters),
                            "decode_live": (lambda: decode("1"), args.iters), "decode_batch": (lambda: decode("2"), args.iters)})
                rec["sweep"][f"lag{lag}_n{n}"] = {"steps": n * (lag + 1), **{k: v["median"] for k, v in us.items()}}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
