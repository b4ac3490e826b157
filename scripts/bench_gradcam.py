#!/usr/bin/env python
"""What Grad-CAM on the device costs (developer aid, not a test; not part of bench.py).

Three cases: base_cnn.layer4 hook tensors [B,512,7,7] at B = 1 and B = 256 with 224 x 224 frames, and the clip model's
conv3d_final_features tensors [32,1024,2,14,14] (clips of 8 frames), also with 224 x 224 frames.  Timed with device events, the
variants alternating inside every repeat so that drift of the box hits all alike:

  map_hip       qt_gradcam_map on the two hook tensors (csrc/gradcam.hip)
  map_copy      a device-to-device copy of the bytes the map reads (both tensors read once): the floor
  map_torch     the same rule in torch ops on the device (mean, broadcast multiply, sum, relu, amax, where)
  overlay_hip   qt_gradcam_overlay_u8 on uint8 frames
  overlay_copy  a device-to-device copy of the frames (read once, written once): the floor
  overlay_torch the same rule in torch ops on the device (gather the four taps, lerp, index the table, blend, cast)
  explain       GradCAM.explain on uint8 frames: preprocess, eval forward, one-hot backward, map, overlay   (--models)
  fwd_bwd       the model's eval forward and one-hot backward alone, on preprocessed images                  (--models)

    python scripts/bench_gradcam.py --models --out profiles/gradcam.json

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
os.environ.setdefault("QTCNN_RESNET18_WEIGHTS", "none")   # synthetic weights below


def torch_map(act, grad):
    import torch
    w = grad.mean(dim=2, keepdim=True)
    r = torch.relu((w * act).sum(dim=1))
    peak = r.amax(dim=1, keepdim=True)
    return torch.where(peak == 0, torch.zeros_like(r), r / peak)


def torch_overlay(cam, frames, lut, alpha):
    import torch
    B, H, W, _ = frames.shape
    h, w = cam.shape[1:]
    dev = frames.device

    def axis(dst, src):
        f = (torch.arange(dst, device=dev, dtype=torch.float32) + 0.5) * (src / dst) - 0.5
        fl = torch.floor(f)
        i = fl.long()
        return i.clamp(0, src - 1), (i + 1).clamp(0, src - 1), f - fl

    y0, y1, ty = axis(H, h)
    x0, x1, tx = axis(W, w)
    r0, r1 = cam[:, y0], cam[:, y1]
    top = r0[:, :, x0] + tx * (r0[:, :, x1] - r0[:, :, x0])
    bot = r1[:, :, x0] + tx * (r1[:, :, x1] - r1[:, :, x0])
    v = top + ty[None, :, None] * (bot - top)
    idx = torch.where(v > 0, (255.0 * v).clamp(max=255.0), torch.zeros_like(v)).long()
    colour = lut[idx].float()
    return (alpha * colour + (1.0 - alpha) * frames.float()).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--models", action="store_true", help="also time explain() against forward + backward on the models")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_gradcam.py measures on the GPU; there is none")
    P = importlib.import_module(PKG)
    G = importlib.import_module(PKG + ".gradcam")
    synth = importlib.import_module(PKG + ".synth")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1234)

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

    cases = {"layer4_b1": (1, 512, (7, 7), 1, (224, 224)), "layer4_b256": (256, 512, (7, 7), 256, (224, 224)),
             "clip_b32": (32, 1024, (2, 14, 14), 64, (224, 224))}
    rec = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats, "us_per_call": {}}
    drawer = P.GradCAM(P.StandardResNetCNN(12))   # overlay() does not run the model
    lut = drawer.lut.to(dev)
    for name, (B, C, pos, nframes, (H, W)) in cases.items():
        act = torch.relu(torch.randn((B, C) + pos, generator=gen)).to(dev)
        m = 0.5 + torch.randn((B, C) + (1,) * len(pos), generator=gen)
        grad = m.expand((B, C) + pos).contiguous().to(dev)
        a3, g3 = act.view(B, C, -1), grad.view(B, C, -1)
        both = torch.stack([a3, g3])
        sink = torch.empty_like(both)
        cam, _ = G.gradcam_map(act, grad)
        flat = cam.reshape(nframes, pos[-2], pos[-1])
        frames = torch.randint(0, 256, (nframes, H, W, 3), generator=gen, dtype=torch.uint8).to(dev)
        fsink = torch.empty_like(frames)
        variants = {"map_hip": lambda: G.gradcam_map(act, grad), "map_copy": lambda: sink.copy_(both),
                    "map_torch": lambda: torch_map(a3, g3), "overlay_hip": lambda: drawer.overlay(frames, flat),
                    "overlay_copy": lambda: fsink.copy_(frames), "overlay_torch": lambda: torch_overlay(flat, frames, lut, 0.4)}
        rec["us_per_call"][name] = timed(variants, args.iters)
        rec["us_per_call"][name]["map_bytes_read"] = both.numel() * 4
        rec["us_per_call"][name]["overlay_bytes_read_plus_written"] = 2 * frames.numel()
        diff = (torch_map(a3, g3) - cam.view(B, -1)).abs().max()
        rec["us_per_call"][name]["map_hip_vs_torch_max_abs"] = float(diff)

    if args.models:
        def model_case(model, frames, numerical, pre, B):
            model = model.to(dev).eval()
            explainer = P.GradCAM(model)
            images = pre(frames)

            def fwd_bwd():
                logits = model(images, numerical)
                one_hot = torch.zeros_like(logits).scatter_(1, logits.detach().argmax(1).view(-1, 1), 1.0)
                model.zero_grad(set_to_none=True)
                logits.backward(gradient=one_hot)

            return timed({"explain": lambda: explainer.explain(frames, numerical, preprocessor=pre), "fwd_bwd": fwd_bwd},
                         max(1, args.iters // 5))

        for B in (1, 256):
            model = P.QuadtreeCNN(12, mode="fusion", freeze_backbone=True)
            model.load_state_dict(synth.synth_state_dict(model))
            frames = torch.randint(0, 256, (B, 224, 224, 3), generator=gen, dtype=torch.uint8).to(dev)
            numerical = synth.synth_pose_features(B, salt=1).to(dev)
            rec["us_per_call"][f"layer4_b{B}"].update(model_case(model, frames, numerical, P.FramePreprocessor(channel_order="bgr"), B))
        B, T = 32, 8
        model = P.Quadtree3DCNN(12, sequence_length=T)
        model.load_state_dict(synth.synth_state_dict(model))
        frames = torch.randint(0, 256, (B, T, 224, 224, 3), generator=gen, dtype=torch.uint8).to(dev)
        numerical = synth.synth_pose_features(B * T, salt=1, realistic=True).view(B, T, 47).to(dev)
        rec["us_per_call"]["clip_b32"].update(model_case(model, frames, numerical, P.FramePreprocessor(channel_order="bgr"), B))
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
