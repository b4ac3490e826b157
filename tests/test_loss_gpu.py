"""The fused loss head on the GPU (csrc/loss.hip, <pkg>/loss.py): the C ABI against the float64 references and derived
bounds of tests/_loss_ref.py, the modules on the package's models, the epoch meter, and the absence of host reads."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import _loss_ref as R
from _util import pkg, rel_err

pytestmark = pytest.mark.gpu
POISON = 12345.0


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class Op:
    """qt_loss_forward / qt_loss_backward through ctypes, with padded rows (ld = C + 3 for the logits, C + 5 for dlogits): the
    logits' padding holds NaN, the gradient's POISON, and both are checked untouched."""

    def __init__(self, dev):
        self.M = pkg("loss")
        self.lib = pkg("_lib")
        self.L = self.lib.lib()
        self.dev = dev

    def run(self, kind, z, y, w, eps, gamma, reduction, gout, ignore_index=R.IGNORE, meter=None, want_pred=True):
        rows, C = z.shape
        dev, L = self.dev, self.L
        ld, ld_d = C + 3, C + 5
        zs = torch.full((rows, ld), float("nan"), device=dev)
        zs[:, :C] = z.to(dev)
        yd = y.to(dev)
        wd = None if w is None else w.to(dev)
        desc = self.M.LossDesc(0, kind, reduction, ignore_index, eps, gamma, self.lib.ptr(wd))
        loss = torch.full((rows + 2 if reduction == R.NONE else 3,), POISON, device=dev)
        state = torch.full((rows + 1, 2), POISON, device=dev)
        stats = torch.full((4,), POISON, dtype=torch.float64, device=dev)
        pred = torch.full((rows + 1,), -7, dtype=torch.int64, device=dev) if want_pred else None
        need = L.qt_loss_workspace_bytes(rows, C)
        ws = torch.empty(max(need // 8, 1), dtype=torch.float64, device=dev)
        self.lib.check(L.qt_loss_forward(ctypes.byref(desc), zs.data_ptr(), ld, yd.data_ptr(), rows, C, loss.data_ptr(),
                                         state.data_ptr(), stats.data_ptr(), self.lib.ptr(pred), self.lib.ptr(meter),
                                         ws.data_ptr() if need else None, need, self.lib.stream_ptr()), "qt_loss_forward")
        dz = torch.full((rows + 1, ld_d), POISON, device=dev)
        g = gout.to(dev)
        self.lib.check(L.qt_loss_backward(ctypes.byref(desc), zs.data_ptr(), ld, yd.data_ptr(), rows, C, state.data_ptr(),
                                          stats.data_ptr(), g.data_ptr(), dz.data_ptr(), ld_d, self.lib.stream_ptr()),
                       "qt_loss_backward")
        torch.cuda.synchronize()
        n = rows if reduction == R.NONE else 1
        assert bool((loss[n:] == POISON).all()) and bool((state[rows:] == POISON).all()) and float(stats[3]) == POISON
        assert bool((dz[:rows, C:] == POISON).all()) and bool((dz[rows:] == POISON).all()), "dlogits padding was written"
        assert bool(torch.isnan(zs[:, C:]).all())
        if pred is not None:
            assert int(pred[rows]) == -7
        return {"loss": loss[:n].cpu() if reduction == R.NONE else loss[0].cpu(), "dz": dz[:rows, :C].cpu(),
                "pred": None if pred is None else pred[:rows].cpu(), "stats": stats[:3].cpu(), "state": state[:rows].cpu()}


def _within(out, ref, what):
    rl = R.ratio(out["loss"].reshape(-1), ref["loss"].reshape(-1), ref["loss_bound"].reshape(-1))
    rg = R.ratio(out["dz"], ref["dz"], ref["dz_bound"])
    print(f"{what}: error / bound: loss {rl:.3f}, dlogits {rg:.3f}")
    assert rl <= 1.0, (what, "loss", rl)
    assert rg <= 1.0, (what, "dlogits", rg)


def _exact_bookkeeping(out, z, y):
    want = torch.max(z, 1).indices
    assert torch.equal(out["pred"], want)
    assert float(out["stats"][2]) == float((want == y).sum())


@pytest.mark.parametrize("rows,C", R.SHAPES)
def test_cross_entropy_op_within_derived_bounds(rows, C):
    op = Op(_dev())
    i = 0
    for with_w in (False, True):
        for eps in (0.0, 0.1):
            for ignored in ("no", "some", "all"):
                for red in (R.MEAN, R.SUM, R.NONE):
                    scale = R.SCALES[(i + rows + C) % 3]
                    i += 1
                    z = R.make_logits(rows, C, scale, seed=i)
                    y = R.make_labels(rows, C, ignored, seed=i)
                    w = R.make_weights(C, i) if with_w else None
                    g = R.make_grad_out(rows, red, i)       # != 1, read through the device pointer; a vector for NONE
                    out = op.run(R.CE, z, y, w, eps, 0.0, red, g)
                    _exact_bookkeeping(out, z, y)
                    what = f"ce {rows}x{C} w={with_w} eps={eps} ignored={ignored} {R.RED_NAME[red]} {scale}"
                    if bool((y == R.IGNORE).all()):
                        assert bool((out["dz"] == 0).all()), what
                        if red == R.MEAN:
                            assert math.isnan(float(out["loss"])), what      # as torch: the mean over nothing
                        else:
                            assert bool((out["loss"] == 0).all()), what
                        continue
                    _within(out, R.ce_ref(z, y, w, eps, red, g), what)


@pytest.mark.parametrize("rows,C", [(256, 12), (257, 12), (17, 17), (5, 65)])
def test_cross_entropy_op_every_logit_scale(rows, C):
    op = Op(_dev())
    for scale in R.SCALES:
        for red in (R.MEAN, R.NONE):
            z = R.make_logits(rows, C, scale, seed=77)
            y = R.make_labels(rows, C, "some", seed=77)
            w = R.make_weights(C, 77)
            g = R.make_grad_out(rows, red, 77)
            out = op.run(R.CE, z, y, w, 0.1, 0.0, red, g)
            _exact_bookkeeping(out, z, y)
            _within(out, R.ce_ref(z, y, w, 0.1, red, g), f"ce {rows}x{C} {scale} {R.RED_NAME[red]}")


@pytest.mark.parametrize("rows,C", R.SHAPES)
def test_focal_op_within_derived_bounds(rows, C):
    op = Op(_dev())
    i = 0
    for gamma in (0.0, 1.0, 2.0, 3.5):
        for red in (R.MEAN, R.SUM, R.NONE):
            scale = R.SCALES[(i + rows) % 3]
            i += 1
            z = R.make_logits(rows, C, scale, seed=100 + i)
            y = R.make_labels(rows, C, "no", seed=100 + i)
            alpha = R.make_weights(C, 100 + i)
            g = R.make_grad_out(rows, red, 100 + i)
            out = op.run(R.FOCAL, z, y, alpha, 0.0, gamma, red, g)
            _exact_bookkeeping(out, z, y)
            _within(out, R.focal_ref(z, y, alpha, gamma, red, g), f"focal {rows}x{C} gamma={gamma} {R.RED_NAME[red]} {scale}")


@pytest.mark.parametrize("C", [12, 17, 65])
def test_focal_rows_with_p_next_to_one_and_next_to_zero(C):
    op = Op(_dev())
    z = torch.zeros(4, C)
    z[0, 3] = 17.0 + math.log(C / 12)
    z[1, 3] = 19.0 + math.log(C / 12)     # 1 - p_3 < 1e-7
    z[2, 5] = 17.0 + math.log(C / 12)     # label 3: p_3 < 1e-7
    z[3, 5] = 30.0
    y = torch.tensor([3, 3, 3, 3])
    p = torch.softmax(z.double(), 1)[:, 3]
    assert float(1 - p[1]) < 1e-7 and float(p[2]) < 1e-7
    alpha = R.make_weights(C, 5)
    for gamma in (0.0, 1.0, 2.0, 3.5):
        g = R.make_grad_out(4, R.NONE, 5)
        out = op.run(R.FOCAL, z, y, alpha, 0.0, gamma, R.NONE, g)
        _within(out, R.focal_ref(z, y, alpha, gamma, R.NONE, g), f"focal confident rows C={C} gamma={gamma}")


@pytest.mark.parametrize("C", [12, 17, 65])
def test_argmax_tie_and_nan_rows_match_cpu_torch_max(C):
    op = Op(_dev())
    z = R.make_logits(6, C, "x1", seed=3)
    z[1, 2] = z[1, C - 1] = 9.0              # a tie: the first index wins (for C > 16 the two sit in different lanes)
    z[2, 7] = z[2, 4] = z[2, 11] = 8.0
    z[3, 5] = float("nan")                   # a NaN wins its row, whatever else is there
    z[3, 1] = 50.0
    y = torch.tensor([0, 2, 4, 5, 1, 3])
    want = torch.max(z, 1).indices
    assert want.tolist()[1:4] == [2, 4, 5]
    out = op.run(R.CE, z, y, None, 0.0, 0.0, R.NONE, torch.ones(6))
    assert torch.equal(out["pred"], want)
    assert float(out["stats"][2]) == float((want == y).sum())
    nan_rows = torch.isnan(out["loss"])
    assert nan_rows.tolist() == [False, False, False, True, False, False]
    assert bool(torch.isnan(out["dz"][3]).all()) and bool(torch.isfinite(out["dz"][[0, 1, 2, 4, 5]]).all())


@pytest.mark.parametrize("rows,C", [(256, 12), (257, 12), (17, 64), (5, 1000)])
def test_two_runs_are_bit_identical(rows, C):
    op = Op(_dev())
    z = R.make_logits(rows, C, "x1", seed=9)
    y = R.make_labels(rows, C, "some", seed=9)
    w = R.make_weights(C, 9)
    g = R.make_grad_out(rows, R.MEAN, 9)
    a = op.run(R.CE, z, y, w, 0.1, 0.0, R.MEAN, g)
    b = op.run(R.CE, z, y, w, 0.1, 0.0, R.MEAN, g)
    for k in ("loss", "dz", "stats", "state"):
        assert torch.equal(a[k].reshape(-1).view(torch.uint8), b[k].reshape(-1).view(torch.uint8)), k
    fa = op.run(R.FOCAL, z, y.clamp_min(0), w, 0.0, 3.5, R.SUM, g)
    fb = op.run(R.FOCAL, z, y.clamp_min(0), w, 0.0, 3.5, R.SUM, g)
    for k in ("loss", "dz", "stats"):
        assert torch.equal(fa[k].reshape(-1).view(torch.uint8), fb[k].reshape(-1).view(torch.uint8)), k


@pytest.mark.parametrize("rows,C", [(6, 12), (300, 12), (20, 17), (6, 65)])
def test_out_of_range_label_gives_nan_and_touches_nothing_else(rows, C):
    """the return path of a label the host cannot check: no indexing with it, NaN in its own outputs (Op.run checks every
    padding word)"""
    op = Op(_dev())
    z = R.make_logits(rows, C, "x1", seed=13)
    y = R.make_labels(rows, C, "no", seed=13)
    y[2] = C
    y[4] = -1
    good = [r for r in range(rows) if r not in (2, 4)]
    out = op.run(R.CE, z, y, R.make_weights(C, 13), 0.1, 0.0, R.NONE, torch.ones(rows))
    assert torch.isnan(out["loss"][[2, 4]]).all() and torch.isfinite(out["loss"][good]).all()
    assert torch.isnan(out["dz"][[2, 4]]).all() and torch.isfinite(out["dz"][good]).all()
    assert torch.equal(out["pred"], torch.max(z, 1).indices)
    for kind, red in ((R.CE, R.MEAN), (R.CE, R.SUM), (R.FOCAL, R.MEAN)):
        out = op.run(kind, z, y, R.make_weights(C, 13), 0.0, 2.0, red, torch.ones(1))
        assert math.isnan(float(out["loss"]))


# ----------------------------------------------------------------------------------------------------------------------
# module level
# ----------------------------------------------------------------------------------------------------------------------
def _model(kind):
    P, synth = pkg(), pkg("synth")
    if kind == "quadtree":
        m = P.QuadtreeCNN(12, dropout_rate=0.0, compute_dtype=torch.float32)
        x, f, y = synth.synth_images(4, salt=1), synth.synth_pose_features(4, salt=1), synth.synth_labels(4, 12, salt=1)
    else:   # the T = 5 / 64 x 64 golden shape of tests/test_clip3d_gpu.py
        m = P.Quadtree3DCNN(12, sequence_length=5, mode="quadtree_3d_fusion", dropout_rate=0.0, compute_dtype=torch.float32)
        x = synth.synth_images(2 * 5, salt=31, size=64).view(2, 5, 3, 64, 64)
        f = synth.synth_pose_features(2 * 5, salt=31, realistic=True).view(2, 5, 47)
        y = synth.synth_labels(2, 12, salt=31)
    m.load_state_dict(synth.synth_state_dict(m))
    return m, x, f, y


@pytest.mark.parametrize("kind", ["quadtree", "quadtree3d"])
@pytest.mark.parametrize("which", ["ce", "focal"])
def test_modules_on_the_models(kind, which):
    dev = _dev()
    P = pkg()
    m, x, f, y = _model(kind)
    m = m.to(dev).train()
    x, f, y = x.to(dev), f.to(dev), y.to(dev)
    alpha = [0.5 + 0.125 * c for c in range(12)]
    if which == "ce":
        fused = P.CrossEntropyLoss(weight=torch.tensor(alpha), label_smoothing=0.1).to(dev)
        ref_fn = lambda z: F.cross_entropy(z, y, weight=torch.tensor(alpha, device=z.device, dtype=z.dtype), label_smoothing=0.1)  # noqa: E731
    else:
        fused = P.FocalLoss(alpha=alpha, gamma=2.0, num_classes=12).to(dev)
        ref_fn = lambda z: R.focal_formula(z, y, torch.tensor(alpha, device=z.device, dtype=z.dtype), 2.0, R.MEAN)  # noqa: E731
    grads = {}
    for name, fn in (("fused", lambda z: fused(z, y)), ("torch", ref_fn)):
        m.zero_grad(set_to_none=True)
        logits = m(x, f)
        logits.retain_grad()
        loss = fn(logits)
        loss.backward()
        grads[name] = ({k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None},
                       logits.detach().cpu(), logits.grad.detach().cpu(), loss.detach().cpu())
    assert rel_err(grads["fused"][1], grads["torch"][1]) <= 1e-6     # the same logits both times
    assert set(grads["fused"][0]) == set(grads["torch"][0]) and len(grads["fused"][0]) > 10
    for k, gt in grads["torch"][0].items():
        assert rel_err(grads["fused"][0][k].cpu(), gt.cpu()) <= 1e-3, k     # the models' own f32 gradient tolerance
    # dlogits and the loss against the float64 reference, at the derived bound
    z, yc = grads["fused"][1], y.cpu()
    one = torch.ones(1)
    ref = R.ce_ref(z, yc, torch.tensor(alpha), 0.1, R.MEAN, one) if which == "ce" else \
        R.focal_ref(z, yc, torch.tensor(alpha), 2.0, R.MEAN, one)
    _within({"loss": grads["fused"][3], "dz": grads["fused"][2]}, ref, f"{which} on {kind}")
    # (loss * 0.5).backward(): the factor reaches the kernel through device memory
    logits = grads["fused"][1].to(dev).requires_grad_(True)
    (fused(logits, y) * 0.5).backward()
    assert torch.equal(logits.grad.cpu() * 2.0, grads["fused"][2])


def test_module_details():
    dev = _dev()
    P = pkg()
    z = R.make_logits(6, 12, "x1", seed=21).to(dev)
    y = R.make_labels(6, 12, "some", seed=21).to(dev)
    crit = P.CrossEntropyLoss(reduction="none")
    with torch.no_grad():
        out = crit(z.clone().requires_grad_(True), y)
    assert out.shape == (6,) and not out.requires_grad
    assert not crit(z, y).requires_grad                       # logits need no gradient: no row state, no graph
    # a column view of a wider matrix (the models hand out views) and a prediction buffer
    wide = torch.randn(6, 40, device=dev)
    view = wide[:, 5:17].detach().requires_grad_(True)
    pred = torch.empty(6, dtype=torch.int64, device=dev)
    loss = P.CrossEntropyLoss()(view, y, predictions=pred)
    loss.backward()
    ref = R.ce_ref(view.detach().cpu(), y.cpu(), None, 0.0, R.MEAN, torch.ones(1))
    _within({"loss": loss.detach().cpu(), "dz": view.grad.cpu()}, ref, "ce on a view")
    assert torch.equal(pred.cpu(), torch.max(view.detach().cpu(), 1).indices)
    # refusals: no torch fallback
    for bad in (lambda: crit(z.double(), y), lambda: crit(z.bfloat16(), y), lambda: crit(z, y.int()), lambda: crit(z.cpu(), y),
                lambda: crit(torch.zeros(2, 1025, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)),
                lambda: P.CrossEntropyLoss(weight=torch.ones(12))(z, y),           # weight still on the CPU
                lambda: crit(z, y, predictions=torch.empty(6, dtype=torch.int32, device=dev))):
        with pytest.raises(P.QtError):
            bad()
    zz = z.clone().requires_grad_(True)
    l2 = P.CrossEntropyLoss()(zz, y)
    with pytest.raises(P.QtError):
        torch.autograd.grad(l2, zz, create_graph=True)


def test_meter_follows_the_trainers_bookkeeping():
    dev = _dev()
    P = pkg()
    crit = P.CrossEntropyLoss()
    meter = P.LossMeter(dev)
    meter.state.fill_(3.0)
    meter.reset()
    st = [0.0, 0, 0, 0]
    bound = 0.0
    for step in range(5):
        rows = 256 if step != 3 else 300          # step 3 takes the partials + finalize path
        z = R.make_logits(rows, 12, "x1", seed=40 + step)
        y = R.make_labels(rows, 12, "no", seed=40 + step)
        if step == 2:
            z[17, 4] = float("nan")
        loss = crit(z.to(dev).requires_grad_(True), y.to(dev), meter=meter)
        loss.backward()
        # 3dcnn/train_3D_Quadtree_cnn_model.py:127-137 on the CPU copy of the same logits
        cpu_loss = F.cross_entropy(z.double(), y)
        predicted = torch.max(z, 1).indices
        R.meter_step(st, float(cpu_loss), rows, int((predicted == y).sum()))
        if math.isfinite(float(cpu_loss)):
            bound += float(R.ce_ref(z, y, None, 0.0, R.MEAN, torch.ones(1))["loss_bound"]) * rows
    res = meter.result()
    assert res["samples"] == st[1] == 256 * 3 + 300 and res["skipped_steps"] == st[3] == 1
    assert abs(res["accuracy"] * res["samples"] - st[2]) < 1e-6
    assert abs(res["loss"] - st[0] / st[1]) <= bound / st[1], (res["loss"], st[0] / st[1], bound / st[1])
    meter.reset()
    assert meter.result() == {"loss": 0.0, "accuracy": 0.0, "samples": 0, "skipped_steps": 0}
    # SUM adds the loss itself, NONE the sum of the row losses
    z, y = R.make_logits(9, 12, "x1", seed=50), R.make_labels(9, 12, "no", seed=50)
    P.CrossEntropyLoss(reduction="sum")(z.to(dev), y.to(dev), meter=meter)
    P.CrossEntropyLoss(reduction="none")(z.to(dev), y.to(dev), meter=meter)
    want = 2 * float(F.cross_entropy(z.double(), y, reduction="sum"))
    res = meter.result()
    assert res["samples"] == 18 and abs(res["loss"] * 18 - want) <= 1e-5 * want


def test_no_host_read_in_forward_backward_and_meter_update():
    dev = _dev()
    P = pkg()
    z = R.make_logits(256, 12, "x1", seed=60).to(dev).requires_grad_(True)
    y = R.make_labels(256, 12, "no", seed=60).to(dev)
    z2 = R.make_logits(300, 12, "x1", seed=61).to(dev).requires_grad_(True)
    y2 = R.make_labels(300, 12, "no", seed=61).to(dev)
    ce = P.CrossEntropyLoss(weight=torch.ones(12), label_smoothing=0.1).to(dev)
    fl = P.FocalLoss(alpha=[1.0] * 12, num_classes=12).to(dev)
    meter = P.LossMeter(dev)
    pred = torch.empty(256, dtype=torch.int64, device=dev)
    ce(z, y).backward()            # first launches outside the guarded region (code-object load)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        (ce(z, y, meter=meter, predictions=pred) * 0.5).backward()
        fl(z, y, meter=meter).backward()
        ce(z2, y2, meter=meter).backward()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert meter.result()["samples"] == 256 * 2 + 300
