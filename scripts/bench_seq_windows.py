#!/usr/bin/env python
"""What forming window batches on the device costs (developer aid, not a test; not part of bench.py).

A CnnLstm batch of 16 windows x 16 frames formed from clips held on the device, timed with device events, the variants
alternating inside every repeat, for uint8 frames [N,224,224,3] (38.5 MB written) and f32 frames [N,3,224,224] (154 MB written):

  gather        SequenceWindows.gather into a preallocated output (qt_seq_gather_rows, csrc/seq_windows.hip)
  copy          a device-to-device copy of the same byte count: every byte read once and written once, the floor of any gather
  index_select  torch.index_select forming the same batch from the same starts (the index tensor made beforehand)

and beside them
  features      SequenceWindows.gather_features, F = 443, mode "standardize", 16 x 16 and 4096 x 16 windows
  plan          SequenceWindows.plan over 2^20 frames in clips of 300, seq_len 4, stride 2, both label rules (three launches,
                the upload of the clip offsets and the allocations included; `count` is not read)

    python scripts/bench_seq_windows.py --out profiles/seq_windows.json

Prints one JSON line.  No threshold rests on it."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "multimodal-hierarchical-cnn-for-sun-salutation-pose-classification_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=16)
    ap.add_argument("--seq-len", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_seq_windows.py measures on the GPU; there is none")
    P = importlib.import_module(PKG)
    dev = torch.device("cuda:0")
    B, T = args.windows, args.seq_len
    gen = torch.Generator(dev).manual_seed(1)

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

    def one_clip_plan(win, frames):
        plan = win.plan(torch.zeros(frames, dtype=torch.int64, device=dev), [frames])
        assert plan.count == frames - win.seq_len + 1
        return plan

    rec = {"device": torch.cuda.get_device_name(0), "windows": B, "seq_len": T, "iters": args.iters, "repeats": args.repeats}
    win = P.SequenceWindows(seq_len=T, stride=1, label="last", num_classes=2)
    for name, frames, make in (("u8", 512, lambda n: torch.randint(0, 256, (n, 224, 224, 3), dtype=torch.uint8, device=dev, generator=gen)),
                               ("f32", 256, lambda n: torch.randn((n, 3, 224, 224), device=dev, generator=gen))):
        src = make(frames)
        plan = one_clip_plan(win, frames)
        idx = torch.randperm(plan.count, device=dev, generator=gen)[:B]
        out = win.gather(src, plan, idx)
        index = (plan.starts[idx].long()[:, None] + torch.arange(T, device=dev)[None, :]).reshape(-1)
        flat = out.view(B * T, *src.shape[1:])
        assert torch.equal(torch.index_select(src, 0, index), flat)
        sink = torch.empty_like(flat)
        variants = {"gather": lambda: win.gather(src, plan, idx, out=out),
                    "copy": lambda: sink.copy_(src[:B * T]),
                    "index_select": lambda: torch.index_select(src, 0, index, out=sink)}
        nbytes = out.numel() * out.element_size()
        us = timed(variants, args.iters)
        rec[name] = {"bytes_written": nbytes, "source_frames": frames, "us_per_call": us,
                     "gather_gb_per_s_read_plus_written": round(2 * nbytes / us["gather"]["median"] * 1e-3, 1)}
        del src, out, sink, flat

    F, K = 443, 12
    rows = torch.randn((1 << 16, F), device=dev, generator=gen)
    rows[torch.rand(rows.shape, device=dev, generator=gen) < 0.2] = float("nan")
    labels = torch.randint(0, K, (rows.shape[0],), device=dev, generator=gen)
    means, stds = P.fit_class_stats(rows, labels, K)
    plan = win.plan(labels, [rows.shape[0]])
    rec["features_443_standardize"] = {}
    for windows in (B, 4096):
        idx = torch.randint(0, plan.count, (windows,), device=dev, generator=gen)
        out = win.gather_features(rows, plan, idx, mode="standardize", means=means, stds=stds)
        sink = torch.empty_like(out)
        us = timed({"features": lambda: win.gather_features(rows, plan, idx, mode="standardize", means=means, stds=stds, out=out),
                    "copy": lambda: sink.copy_(out)}, 4 * args.iters)
        rec["features_443_standardize"][f"{windows}x{T}"] = {"bytes_written": out.numel() * 4, "us_per_call": us}

    frames = 1 << 20
    labels = torch.repeat_interleave(torch.randint(0, K, (frames // 8,), device=dev, generator=gen), 8)
    lengths = [300] * (frames // 300) + [frames % 300]
    plans = {rule: P.SequenceWindows(seq_len=4, stride=2, label=rule, num_classes=K) for rule in ("uniform", "last")}
    variants = {rule: (lambda w=w: w.plan(labels, lengths)) for rule, w in plans.items()}
    # the three launches alone: qt_seq_windows_plan through ctypes into preallocated buffers
    import ctypes
    M, Lm = importlib.import_module(PKG + ".sequence_windows"), importlib.import_module(PKG + "._lib")
    L = Lm.lib()
    capacity = M.candidate_count(lengths, 4, 2)
    offsets = torch.tensor([0] + lengths, dtype=torch.int64).cumsum(0).to(torch.int32).to(dev)
    starts, window_labels = torch.empty(capacity, dtype=torch.int32, device=dev), torch.empty(capacity, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    for rule, code in (("uniform", M.QT_SEQ_LABEL_UNIFORM), ("last", M.QT_SEQ_LABEL_LAST)):
        desc = M.SeqWindowsDesc(frames, len(lengths), 4, 2, K, capacity, code)
        nbytes = L.qt_seq_windows_workspace_bytes(ctypes.byref(desc))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        variants[rule + "_launches_only"] = lambda desc=desc, ws=ws, nbytes=nbytes: Lm.check(L.qt_seq_windows_plan(
            ctypes.byref(desc), Lm.ptr(labels), Lm.ptr(offsets), Lm.ptr(starts), Lm.ptr(window_labels), Lm.ptr(count), Lm.ptr(ws),
            nbytes, Lm.stream_ptr()), "qt_seq_windows_plan")
    us = timed(variants, max(args.iters // 5, 2))
    rec["plan_2^20_frames"] = {"clips": len(lengths), "us_per_call": us,
                               "windows": {rule: w.plan(labels, lengths).count for rule, w in plans.items()}}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
