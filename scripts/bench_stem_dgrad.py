"""Developer aid: conv1's data gradient down to the image (qt_stem_dgrad) alone at B = 256, and what d(loss)/d(image) adds
to a B = 256 bf16 QuadtreeCNN train step (forward + backward, no optimizer) with a trainable and with a frozen backbone.
    python scripts/bench_stem_dgrad.py [--iters N]"""
import argparse, json, os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("QTCNN_RESNET18_WEIGHTS", "none")
from _util import pkg
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()
L = pkg("_lib"); lib = L.lib(); synth = pkg("synth"); P = pkg()
dev = torch.device("cuda:0"); B = 256
HBM_PEAK = 8.0e12   # MI355X HBM3E, bytes/s


def timed(fn, iters, warm=3):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3   # us


out = {}
w = torch.randn(64, 3, 7, 7, device=dev) * 0.05
dx = torch.empty(B, 3, 224, 224, device=dev)
for dt in (torch.bfloat16, torch.float32):
    dy = torch.randn(B, 112, 112, 64, device=dev).to(dt)
    st = L.stream_ptr()
    fn = lambda: L.check(lib.qt_stem_dgrad(L.qt_dtype(dt), dy.data_ptr(), w.data_ptr(), dx.data_ptr(), B, st), "qt_stem_dgrad")
    us = timed(fn, args.iters)
    nbytes = dy.numel() * dy.element_size() + dx.numel() * 4
    name = "bf16" if dt == torch.bfloat16 else "f32"
    out[f"stem_dgrad_{name}_us"] = round(us, 1)
    out[f"stem_dgrad_{name}_GBps"] = round(nbytes / us / 1e3, 1)
    out[f"stem_dgrad_{name}_of_hbm_floor"] = round(nbytes / HBM_PEAK * 1e6 / us, 3)
    print(f"qt_stem_dgrad {name} B={B}: {us:.1f} us, {nbytes / us / 1e3:.0f} GB/s, "
          f"HBM floor {nbytes / HBM_PEAK * 1e6:.1f} us ({nbytes / HBM_PEAK * 1e6 / us:.0%} of it)", flush=True)
del dy

x = synth.synth_images(B, salt=5).to(dev)
f = synth.synth_pose_features(B, salt=5).to(dev)
y = synth.synth_labels(B, 12, salt=5).to(dev)
for frozen in (False, True):
    m = P.QuadtreeCNN(12, freeze_backbone=frozen, compute_dtype=torch.bfloat16, max_batch=B)
    m.load_state_dict(synth.synth_state_dict(m))
    m = m.to(dev).train()
    res = {}
    for want_dx in (False, True, False, True):   # interleaved: clock / thermal drift hits both alike
        xi = x.clone().requires_grad_(want_dx)

        def step():
            m.zero_grad(set_to_none=True)
            xi.grad = None
            torch.nn.functional.cross_entropy(m(xi, f), y).backward()
        res.setdefault(want_dx, []).append(timed(step, args.iters))
    base, with_dx = min(res[False]), min(res[True])
    tag = "frozen" if frozen else "trainable"
    out[f"step_{tag}_us"] = round(base, 1)
    out[f"step_{tag}_image_grad_us"] = round(with_dx, 1)
    print(f"QuadtreeCNN bf16 B={B} train step, {tag} backbone: {base / 1e3:.3f} ms, with image grad "
          f"{with_dx / 1e3:.3f} ms (+{(with_dx - base) / 1e3:.3f} ms)", flush=True)
    del m
    torch.cuda.empty_cache()
print(json.dumps(out))
