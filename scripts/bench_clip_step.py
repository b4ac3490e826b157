"""Developer aid: what global-norm gradient clipping costs a B = 256 bf16 QuadtreeCNN train step (zero_grad, forward,
cross-entropy, backward, optimizer step), and the norm kernel (qt_grad_norm_multi) alone.
  (a) torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0) in front of FusedAdam   -- what a user had to write before
  (b) FusedAdam(max_grad_norm=1.0)                                                     -- clipping inside the step
  (c) FusedAdam without clipping                                                       -- the default must not move
Three models on one GPU, random data, rounds interleaved a, b, c, a, b, c, ...: drift hits all three alike.  Per variant
the median over the rounds and their spread (max - min); (b) is "not slower" if it is within (a)'s spread.
    python scripts/bench_clip_step.py [--iters N] [--rounds R]"""
import argparse, json, os, statistics, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("QTCNN_RESNET18_WEIGHTS", "none")
from _util import pkg
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batch", type=int, default=256)
args = ap.parse_args()
L = pkg("_lib"); lib = L.lib(); eng = pkg("engine"); synth = pkg("synth"); P = pkg()
dev = torch.device("cuda:0"); B = args.batch
HBM_PEAK = 8.0e12   # MI355X HBM3E, bytes/s


def timed(fn, iters, warm=3):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3   # us


out = {"batch": B, "iters": args.iters, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
g = torch.Generator(device=dev).manual_seed(1234)
x = torch.randn(B, 3, 224, 224, device=dev, generator=g)
f = torch.randn(B, 47, device=dev, generator=g)
y = torch.randint(0, 12, (B,), device=dev, generator=g)


def variant(kind):
    m = P.QuadtreeCNN(12, compute_dtype=torch.bfloat16, max_batch=B)
    m.load_state_dict(synth.synth_state_dict(m))
    m = m.to(dev).train()
    opt = P.FusedAdam(m.parameters(), lr=1e-4, weight_decay=1e-4, model=m, max_grad_norm=1.0 if kind == "b" else None)

    def step():
        opt.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(m(x, f), y).backward()
        if kind == "a":
            torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
        opt.step()
    return m, opt, step


names = {"a": "torch_clip_then_fused_adam", "b": "fused_adam_max_grad_norm", "c": "fused_adam_unclipped"}
variants = {k: variant(k) for k in names}
times = {k: [] for k in names}
for _ in range(args.rounds):
    for k in names:
        times[k].append(timed(variants[k][2], args.iters))
for k, name in names.items():
    med, spread = statistics.median(times[k]), max(times[k]) - min(times[k])
    out[f"{name}_us"] = round(med, 1)
    out[f"{name}_spread_us"] = round(spread, 1)
    out[f"{name}_rounds_us"] = [round(t, 1) for t in times[k]]
    print(f"({k}) {name}: median {med / 1e3:.3f} ms, spread {spread / 1e3:.3f} ms over {args.rounds} rounds of "
          f"{args.iters} steps", flush=True)
out["overlapped"] = {k: bool(variants[k][0]._engine.last_adam_overlapped) for k in names}
out["last_grad_norm"] = float(variants["b"][1].last_grad_norm)
out["last_clip_coef"] = float(variants["b"][1].last_clip_coef)

# the norm kernel alone: over the model's own gradients (104 MB: they fit the 256 MB Infinity Cache, so this is what the
# step sees right after the backward wrote them, not an HBM rate), and over 1 GiB that cannot be cached
grads = [p.grad for p in variants["c"][0].parameters() if p.grad is not None]
big = [torch.randn(1 << 26, device=dev) for _ in range(4)]
for tag, ts in (("model_grads", grads), ("1GiB", big)):
    items = (eng.AdamItem * len(ts))(*[eng.AdamItem(None, t.data_ptr(), None, None, t.numel()) for t in ts])
    need = lib.qt_grad_norm_workspace_bytes(items, len(ts))
    ws = torch.empty(need // 4, device=dev)
    res = torch.empty(2, device=dev)
    st = L.stream_ptr()
    fn = lambda: L.check(lib.qt_grad_norm_multi(items, len(ts), 1.0, ws.data_ptr(), need, res.data_ptr(), st),
                         "qt_grad_norm_multi")
    us = timed(fn, 50, warm=5)
    nbytes = sum(t.numel() for t in ts) * 4
    ref = float(torch.sqrt(sum((t.double() ** 2).sum() for t in ts)))
    out[f"norm_{tag}_tensors"] = len(ts)
    out[f"norm_{tag}_MB"] = round(nbytes / 1e6, 1)
    out[f"norm_{tag}_us"] = round(us, 1)
    out[f"norm_{tag}_GBps"] = round(nbytes / us / 1e3, 1)
    out[f"norm_{tag}_rel_err_vs_f64"] = abs(float(res[0]) - ref) / ref
    print(f"qt_grad_norm_multi {tag}: {len(ts)} tensors, {nbytes / 1e6:.1f} MB, {us:.1f} us, {nbytes / us / 1e3:.0f} GB/s "
          f"({nbytes / us / 1e3 / (HBM_PEAK / 1e9):.0%} of the HBM peak), norm rel err vs float64 "
          f"{out[f'norm_{tag}_rel_err_vs_f64']:.1e}", flush=True)
print(json.dumps(out))
