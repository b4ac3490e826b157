"""Developer aid: conv3d_block1's data gradient down to the clip (qt_conv3d_first_dgrad) alone at 32 clips x 8 frames of
224 x 224 (bf16 dy) beside a device-to-device copy of the same bytes (the HBM floor of this box), and what d(loss)/d(clip) adds
to a bf16 Quadtree3DCNN forward + backward at that size.
    python scripts/bench_clip_dgrad.py [--iters N] [--clips B]"""
import argparse, json, os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from _util import pkg
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--clips", type=int, default=32)
args = ap.parse_args()
L = pkg("_lib"); lib = L.lib(); synth = pkg("synth"); P = pkg()
dev = torch.device("cuda:0"); B, T, HW = args.clips, 8, 224


def timed(fn, iters, warm=3):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3   # us


out = {"clips": B, "frames": T, "hw": HW}
w = torch.randn(32, 3, 3, 3, 3, device=dev) * 0.15
dy = torch.randn(T, B, HW, HW, 32, device=dev).to(torch.bfloat16)
dx = torch.empty(B, T, 3, HW, HW, device=dev)
st = L.stream_ptr()
us = timed(lambda: L.check(lib.qt_conv3d_first_dgrad(L.QT_BF16, dy.data_ptr(), w.data_ptr(), dx.data_ptr(), B, T, HW, HW, st),
                           "qt_conv3d_first_dgrad"), args.iters)
nbytes = dy.numel() * 2 + dx.numel() * 4
# the floor: a copy that reads and writes as many bytes as the kernel (a copy of n bytes moves 2 n)
buf_a = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev); buf_b = torch.empty_like(buf_a)
copy_us = timed(lambda: buf_b.copy_(buf_a), args.iters)
copy_bw = 2 * buf_a.numel() / copy_us / 1e3    # GB/s
out.update(dgrad_us=round(us, 1), dgrad_GBps=round(nbytes / us / 1e3, 1), copy_GBps=round(copy_bw, 1),
           hbm_floor_us=round(copy_us, 1), dgrad_over_floor=round(us / copy_us, 2))
print(f"qt_conv3d_first_dgrad bf16 {B} x {T} x {HW}^2: {us:.1f} us for {nbytes / 1e9:.2f} GB ({nbytes / us / 1e3:.0f} GB/s); a copy of "
      f"the same bytes: {copy_us:.1f} us ({copy_bw:.0f} GB/s) -> {us / copy_us:.2f}x the floor", flush=True)
del dy, dx, buf_a, buf_b
torch.cuda.empty_cache()

x = synth.synth_images(B * T, salt=5, size=HW).view(B, T, 3, HW, HW).to(dev)
f = synth.synth_pose_features(B * T, salt=5, realistic=True).view(B, T, 47).to(dev)
y = synth.synth_labels(B, 12, salt=5).to(dev)
m = P.Quadtree3DCNN(12, sequence_length=T, compute_dtype=torch.bfloat16)
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
out.update(step_us=round(base, 1), step_clip_grad_us=round(with_dx, 1), step_delta_us=round(with_dx - base, 1))
print(f"Quadtree3DCNN bf16 forward + backward: {base / 1e3:.3f} ms, with the clip gradient {with_dx / 1e3:.3f} ms "
      f"(+{(with_dx - base) / 1e3:.3f} ms)", flush=True)
print(json.dumps(out))
