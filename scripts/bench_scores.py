#!/usr/bin/env python
"""What the score-based evaluation costs, and where its automatic route threshold comes from (developer aid, not a test; not
part of bench.py).

For rows x 12 logits at each size, with peaked scores (a trained-looking model: positives pile up in the top bin, negatives in
bin 0) and with flat scores (rows spread over the bins), per call:

  direct       qt_scores_update with route = direct: one 64-bit global atomic per (class, side, bin) cell of a row
  private      the same call with route = privatised: a workgroup per (row slice, class), u32 histogram in LDS
  copy         a device-to-device copy of the same rows * C * 4 bytes, for scale
  host         the host's work on one core, for scale: the same integers by numpy (quantise, np.add.at into the histograms)
               at every size; with --sklearn also roc_auc_score + average_precision_score per class

The device variants are timed with device events over `iters` back-to-back calls (the stream never drains), sized so that a
window is a fraction of a second; they alternate inside every repeat.  The two routes are checked to give the same state
before anything is timed.  The threshold QT_SCORES_AUTO_PRIVATE_ROWS goes where `private` first wins on the peaked case.

    python scripts/bench_scores.py --out profiles/scores.json

Prints one JSON line and, on stderr, the table of EXPERIMENTS.md "Score metrics"."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "multimodal-hierarchical-cnn-for-sun-salutation-pose-classification_amd"


def make_logits(torch, rows, C, peak, seed):
    gen = torch.Generator().manual_seed(seed)
    y = torch.randint(0, C, (rows,), generator=gen)
    z = torch.randn(rows, C, generator=gen)
    if peak:
        lift = torch.rand(rows, generator=gen) < 0.9
        z[torch.arange(rows)[lift], y[lift]] += peak
    return z, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[16, 64, 256, 1024, 4096, 16384, 65536, 1 << 22])
    ap.add_argument("--classes", type=int, default=12)
    ap.add_argument("--bits", type=int, default=12)
    ap.add_argument("--peak", type=float, default=12.0, help="what the label's logit is raised by in the peaked case")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-rows", type=int, default=1 << 24, help="rows per timed window (iters = window / rows, 4 .. 2000)")
    ap.add_argument("--sklearn", action="store_true", help="also time scikit-learn on the host (when it is installed)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_scores.py measures on the GPU; there is none")
    P = importlib.import_module(PKG)
    S = importlib.import_module(PKG + ".scores")
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    C, K = args.classes, 1 << args.bits
    rec = {"device": torch.cuda.get_device_name(0), "classes": C, "bits": args.bits, "repeats": args.repeats, "cases": []}
    for rows in args.rows:
        iters = max(4, min(2000, args.window_rows // rows))
        for case, peak in (("peaked", args.peak), ("flat", 0.0)):
            z_h, y_h = make_logits(torch, rows, C, peak, seed=rows + int(peak))
            z, y = z_h.to(dev), y_h.to(dev)
            meters = {}
            for name, route in (("direct", S.ROUTE_DIRECT), ("private", S.ROUTE_PRIVATE)):
                meters[name] = P.ScoreMeter(C, dev, bits=args.bits)
                meters[name].route = route
                meters[name].update(z, y)
            if not torch.equal(meters["direct"].state, meters["private"].state):
                raise SystemExit(f"the routes disagree at {rows} rows ({case})")
            dst = torch.empty_like(z)
            variants = {"direct": lambda: meters["direct"].update(z, y), "private": lambda: meters["private"].update(z, y),
                        "copy": lambda: dst.copy_(z)}
            for fn in variants.values():
                for _ in range(3):
                    fn()
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
            # the host's work on one core (scores already on the host: the copy is not charged)
            p_h = torch.softmax(z_h, 1).numpy()
            y_n = y_h.numpy()
            hist = np.zeros((C, 2, K), np.int64)
            t0 = time.perf_counter()
            q = np.minimum(K - 1, (p_h * np.float32(K)).astype(np.int64))
            side = (np.arange(C)[None, :] == y_n[:, None]).astype(np.int64)
            np.add.at(hist.reshape(-1), ((np.arange(C)[None, :] * 2 + side) * K + q).reshape(-1), 1)
            host_us = (time.perf_counter() - t0) * 1e6
            sk_us = None
            if args.sklearn:
                try:
                    from sklearn import metrics as M
                    t0 = time.perf_counter()
                    for k in range(C):
                        M.roc_auc_score(y_n == k, p_h[:, k])
                        M.average_precision_score(y_n == k, p_h[:, k])
                    sk_us = (time.perf_counter() - t0) * 1e6
                except ImportError:
                    pass
            med = {k: round(statistics.median(v), 2) for k, v in times.items()}
            row = {"rows": rows, "case": case, "iters": iters, "us": med,
                   "spread": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()},
                   "host_numpy_us": round(host_us, 1), "host_sklearn_us": None if sk_us is None else round(sk_us, 1)}
            rec["cases"].append(row)
            print(f"| {rows} | {case} | {med['direct']} | {med['private']} | {med['copy']} | {row['host_numpy_us']} | "
                  f"{row['host_sklearn_us'] if sk_us is not None else 'n/a'} |", file=sys.stderr, flush=True)
    # one result(): finalize launches + the one copy, host clock
    meter = P.ScoreMeter(C, dev, bits=args.bits)
    meter.update(z, y)
    meter.result()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    meter.result()
    rec["result_us"] = round((time.perf_counter() - t0) * 1e6, 1)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
