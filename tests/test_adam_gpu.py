"""The Adam kernels and FusedAdam against the float64 rule of tests/_adam_ref.py, element by element, inside bounds derived
from adam_update's own roundings (see that module; tests/test_adam_ref_cpu.py shows that correct f32 arithmetic meets them
and that six wrong rules do not).

* kernel level, through the C ABI: qt_adam_multi(_scaled) at 1 / 4095 / 4096 / 4097 elements and
  qt_adam_pack_weights_batched(_scaled) on a 3x3 (32, 32) and a 1x1 (64, 64) item with stride-2 data-gradient layouts, f32
  and bf16 operands: every hyper-parameter set, step count and gradient scale of _adam_ref, the scalar and the float4 form
  bit for bit, the packed copies as the rounding of the new masters (qt_pack_weights_batched of them), and the edge class
  (a denominator of eps alone, 0 / 0, subnormal g * g) by adam_mixed's class;
* FusedAdam on plain device tensors (49 of them: two launches), every gradient prescribed: an lr schedule, two param groups
  with a late joiner and skipped gradients, clipping, resume through torch.save / torch.load, state from and to
  torch.optim.Adam;
* FusedAdam on the smallest plan-backed 2-D model whose parameters all train (AttentionHierarchicalCNN), prescribed
  gradients on every parameter, one and two param groups, f32 and bf16 operand copies.

Buffers handed to the kernels sit between tests/_guard.py's bands; gradients must come back byte for byte.  Every test
prints max(|err| / bound) before asserting it.  The float64 references of the plan model run on the device (torch float64
elementwise kernels); everything else is compared on the host.
"""
import ctypes
import io
import itertools

import numpy as np
import pytest
import torch

import _adam_ref as R
from _guard import Guard
from _util import pkg

pytestmark = pytest.mark.gpu

NORM_TOL = 1e-5      # tests/test_clip_adam_gpu.py's bound on the norm kernel


def _dev():
    return torch.device("cuda:0")


_PackItem = pkg("_abi").PackItem   # qt_pack_item


def _api():
    L = pkg("_lib")
    lib = L.lib()
    eng = pkg("engine")
    return L, lib, eng


def _desc(eng, hyper, scale, step):
    return eng.AdamDesc(hyper["lr"], hyper["betas"][0], hyper["betas"][1], hyper["eps"], hyper["weight_decay"], scale, step)


def _inout(guard, name, array):
    """a guarded buffer the kernel updates in place: bands checked, contents free"""
    t = guard.input(name, torch.from_numpy(np.ascontiguousarray(array)))
    guard.bufs[-1].kind = "inout"
    return t


def _items(eng, ps, gs, ms, vs):
    return (eng.AdamItem * len(ps))(*[eng.AdamItem(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel())
                                      for p, g, m, v in zip(ps, gs, ms, vs)])


def _shares(got, full):
    return {k: R.share(x.detach().reshape(-1).cpu(), full[k], full["b" + k]) for k, x in zip("pmv", got)}


def _run_multi(L, lib, eng, inputs, hyper, step, desc_scale, dev_coef):
    """one qt_adam_multi / qt_adam_multi_scaled call on guarded buffers; returns [(p, m, v)] on the host"""
    guard = Guard(_dev())
    ps = [_inout(guard, f"p{j}", x[0]) for j, x in enumerate(inputs)]
    gs = [guard.input(f"g{j}", torch.from_numpy(x[1])) for j, x in enumerate(inputs)]
    ms = [_inout(guard, f"m{j}", x[2]) for j, x in enumerate(inputs)]
    vs = [_inout(guard, f"v{j}", x[3]) for j, x in enumerate(inputs)]
    desc = _desc(eng, hyper, desc_scale, step)
    items = _items(eng, ps, gs, ms, vs)
    if dev_coef is None:
        L.check(lib.qt_adam_multi(items, len(ps), ctypes.byref(desc), L.stream_ptr()), "qt_adam_multi")
    else:
        coef = guard.input("coef", torch.tensor([dev_coef], dtype=torch.float32))
        L.check(lib.qt_adam_multi_scaled(items, len(ps), ctypes.byref(desc), coef.data_ptr(), L.stream_ptr()),
                "qt_adam_multi_scaled")
    guard.check()          # bands intact; gradients and the coefficient byte for byte
    return [(p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()) for p, m, v in zip(ps, ms, vs)]


# ---- kernel level ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hname", list(R.HYPERS))
def test_multi_kernel_inside_bounds(hname):
    """adam_multi_kernel: four tensors in one launch (one element; one element short of a block, a block, one more), every
    step count and gradient scale"""
    L, lib, eng = _api()
    hyper = R.HYPERS[hname]
    inputs = [R.main_inputs(n, 100 + n) for n in R.MULTI_SIZES]
    worst = dict(p=0.0, m=0.0, v=0.0)
    fails = []
    for step, scale in itertools.product(R.STEPS, R.SCALES):
        ds, dc = R.SCALES[scale]
        got = _run_multi(L, lib, eng, inputs, hyper, step, ds, dc)
        for x, out in zip(inputs, got):
            full = R.adam64_full(*x, hyper, step, R.effective_scale(ds, dc))
            for k, s in _shares([torch.from_numpy(o) for o in out], full).items():
                worst[k] = max(worst[k], s)
                if not s <= 1.0:
                    fails.append((step, scale, x[0].size, k, s))
    print(f"qt_adam_multi(_scaled), {hname}: max |err| / bound  p {worst['p']:.3f}  m {worst['m']:.3f}  v {worst['v']:.3f}")
    assert not fails, fails[:8]


BATCHED_ITEMS = [(32, 32, 3, 3), (64, 64, 1, 4)]      # (O, I, k, stride-2 data-gradient layout)


def _dgrad_slots(k, s2):
    return {2: 16, 3: 20, 4: 20}.get(s2, k * k)


def _run_batched(L, lib, eng, dt, inputs, hyper, step, desc_scale, dev_coef, shapes=BATCHED_ITEMS):
    """qt_adam_pack_weights_batched(_scaled) on guarded buffers, qt_adam_multi on plain copies of the same values (the
    scalar form: same bits), qt_pack_weights_batched on the new masters (same packed bits).  Returns [(w, m, v)]."""
    dev = _dev()
    guard = Guard(dev)
    n = len(shapes)
    items, state = (_PackItem * n)(), (eng.AdamItem * n)()
    keep, plain = [], []
    for j, ((O, I, k, s2), x) in enumerate(zip(shapes, inputs)):
        w, m, v = (_inout(guard, f"{nm}{j}", a) for nm, a in (("w", x[0]), ("m", x[2]), ("v", x[3])))
        g = guard.input(f"g{j}", torch.from_numpy(x[1]))
        fwd = guard.output(f"fwd{j}", (O * k * k * I,), dt, fill=0)
        dg = guard.output(f"dg{j}", (_dgrad_slots(k, s2) * O * I,), dt, fill=0)
        items[j] = _PackItem(w.data_ptr(), fwd.data_ptr(), dg.data_ptr(), O, I, k, s2)
        state[j] = eng.AdamItem(w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), w.numel())
        keep.append((w, g, m, v, fwd, dg))
        plain.append([torch.from_numpy(a.copy()).to(dev) for a in (x[0], x[1], x[2], x[3])])
    qdt, st = L.qt_dtype(dt), L.stream_ptr()
    desc = _desc(eng, hyper, desc_scale, step)
    pitems = _items(eng, [q[0] for q in plain], [q[1] for q in plain], [q[2] for q in plain], [q[3] for q in plain])
    if dev_coef is None:
        L.check(lib.qt_adam_pack_weights_batched(qdt, items, state, ctypes.byref(desc), n, st), "qt_adam_pack_weights_batched")
        L.check(lib.qt_adam_multi(pitems, n, ctypes.byref(desc), st), "qt_adam_multi")
    else:
        coef = guard.input("coef", torch.tensor([dev_coef], dtype=torch.float32))
        L.check(lib.qt_adam_pack_weights_batched_scaled(qdt, items, state, ctypes.byref(desc), coef.data_ptr(), n, st),
                "qt_adam_pack_weights_batched_scaled")
        L.check(lib.qt_adam_multi_scaled(pitems, n, ctypes.byref(desc), coef.data_ptr(), st), "qt_adam_multi_scaled")
    guard.check()
    again = (_PackItem * n)()
    fresh = []
    for j, (O, I, k, s2) in enumerate(shapes):
        fwd = torch.zeros_like(keep[j][4])
        dg = torch.zeros_like(keep[j][5])
        again[j] = _PackItem(keep[j][0].data_ptr(), fwd.data_ptr(), dg.data_ptr(), O, I, k, s2)
        fresh.append((fwd, dg))
    L.check(lib.qt_pack_weights_batched(qdt, again, n, st), "qt_pack_weights_batched")
    torch.cuda.synchronize()
    out = []
    for j in range(n):
        w, g, m, v, fwd, dg = keep[j]
        # NaN-proof comparisons: the bits
        for name, a, b in (("w", w, plain[j][0]), ("m", m, plain[j][2]), ("v", v, plain[j][3])):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (shapes[j], name, "float4 and scalar form differ")
        bits = torch.int32 if dt == torch.float32 else torch.int16
        assert torch.equal(fwd.view(bits), fresh[j][0].view(bits)), (shapes[j], "forward operand is not the new master's")
        assert torch.equal(dg.view(bits), fresh[j][1].view(bits)), (shapes[j], "data-gradient operand is not the new master's")
        out.append((w.cpu().numpy().reshape(-1), m.cpu().numpy().reshape(-1), v.cpu().numpy().reshape(-1)))
    return out, keep


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("hname", list(R.HYPERS))
def test_batched_kernel_inside_bounds(hname, dt):
    L, lib, eng = _api()
    hyper = R.HYPERS[hname]
    inputs = [R.main_inputs(O * I * k * k, 200 + O) for O, I, k, _ in BATCHED_ITEMS]
    worst = dict(p=0.0, m=0.0, v=0.0)
    fails = []
    for step, scale in itertools.product(R.STEPS, R.SCALES):
        ds, dc = R.SCALES[scale]
        got, keep = _run_batched(L, lib, eng, dt, inputs, hyper, step, ds, dc)
        for x, out, kept in zip(inputs, got, keep):
            assert float(kept[4].float().abs().sum()) > 0 and float(kept[5].float().abs().sum()) > 0
            full = R.adam64_full(*x, hyper, step, R.effective_scale(ds, dc))
            for k, s in _shares([torch.from_numpy(o) for o in out], full).items():
                worst[k] = max(worst[k], s)
                if not s <= 1.0:
                    fails.append((step, scale, x[0].size, k, s))
    print(f"qt_adam_pack_weights_batched(_scaled) {dt}, {hname}: max |err| / bound  p {worst['p']:.3f}  m {worst['m']:.3f}  "
          f"v {worst['v']:.3f}")
    assert not fails, fails[:8]


@pytest.mark.parametrize("hname", list(R.EDGE_HYPERS))
def test_edge_class(hname):
    """g = 0 with v = 0, eps = 0 with v = 0 (NaN / infinity exactly where f32 Adam gives them), subnormal g * g: the class of
    every element is adam_mixed's, the finite ones are inside their bound.  Both kernels."""
    L, lib, eng = _api()
    hyper = R.EDGE_HYPERS[hname]
    n = 32 * 32 * 9
    p, g, m, v, _ = R.edge_inputs(n, 23)
    for step in (1, 10):
        full = R.adam64_full(p, g, m, v, hyper, step)
        mixed = R.adam_mixed(p, g, m, v, hyper, step)
        multi = _run_multi(L, lib, eng, [(p, g, m, v)], hyper, step, 1.0, None)[0]
        batched, _ = _run_batched(L, lib, eng, torch.float32, [(p, g, m, v)], hyper, step, 1.0, None, shapes=[(32, 32, 3, 3)])
        for name, got in (("qt_adam_multi", multi), ("qt_adam_pack_weights_batched", batched[0])):
            special, worst = R.edge_check(got, mixed, full)
            print(f"{name}, {hname}, step {step}: {special} of {n} elements compared by class; finite ones: "
                  f"max |err| / bound {worst:.3f}")
            assert special >= 2 * (n // 5) and worst <= 1.0


# ---- FusedAdam on plain device tensors ------------------------------------------------------------------------------------
SIZES49 = [(7 * i) % 61 + 1 for i in range(46)] + [5000, 8192, 8193]        # crosses the 48-tensors-per-launch boundary
GROUP_A = R.HYPERS["reference"]
GROUP_B = R.HYPERS["existing"]
IN_B = set(range(25, 46)) | {48}
LATE, SKIPPING = 3, 30        # first gradient at step 4 (group A); no gradient at steps 2 and 5 (group B)


def _has_grad(i, step):
    if i == LATE:
        return step >= 4
    if i == SKIPPING:
        return step not in (2, 5)
    return True


def _always(i, step):
    return True


def _start_values():
    return [R.main_inputs(n, 300 + i)[0] for i, n in enumerate(SIZES49)]


def _grad_values(i, step):
    return R.main_inputs(SIZES49[i], 1000 * step + i)[1]


def _guarded_params(values):
    guard = Guard(_dev())
    return guard, [torch.nn.Parameter(_inout(guard, f"p{i}", x)) for i, x in enumerate(values)]


def _two_groups(params, **kw):
    a = [p for i, p in enumerate(params) if i not in IN_B]
    b = [p for i, p in enumerate(params) if i in IN_B]
    return pkg().FusedAdam([dict(params=a, **GROUP_A), dict(params=b, **GROUP_B)], **kw)


def _groups_now(opt, params):
    """[(hyper, indices)] from the optimizer's param groups as they stand before a step"""
    index = {id(p): i for i, p in enumerate(params)}
    return [(dict(lr=g["lr"], betas=tuple(g["betas"]), eps=g["eps"], weight_decay=g["weight_decay"]),
             [index[id(p)] for p in g["params"]]) for g in opt.param_groups]


def _compare(params, opt, sched):
    worst = 0.0
    for i, p in enumerate(params):
        st = opt.state.get(p, {})
        worst = max(worst, R.share(p.detach().cpu(), sched.p[i], sched.e[i][0]))
        if "exp_avg" in st:
            assert int(st["step"]) == sched.t[i], (i, st["step"], sched.t[i])
            worst = max(worst, R.share(st["exp_avg"].cpu(), sched.m[i], sched.e[i][1]),
                        R.share(st["exp_avg_sq"].cpu(), sched.v[i], sched.e[i][2]))
        else:
            assert sched.t[i] == 0
    return worst


def _drive(opt, params, sched, steps, has_grad=_always, clip=None, torch_rule=False, each_step=None, label=""):
    """Prescribed gradients for `steps`; after every step the optimizer's parameters and moments against the float64
    schedule.  Returns the largest share of a bound."""
    worst = 0.0
    for step in steps:
        grads = {i: _grad_values(i, step) for i in range(len(params)) if has_grad(i, step)}
        gguard = Guard(_dev())
        for i, p in enumerate(params):
            p.grad = gguard.input(f"g{i}", torch.from_numpy(grads[i])) if i in grads else None
        groups = _groups_now(opt, params)
        opt.step()
        gguard.check()                                  # gradients byte for byte, nothing written around them
        coef = None
        if clip is not None:
            norm64 = float(np.sqrt(sum(float((x.astype(np.float64) ** 2).sum()) for x in grads.values())))
            got_norm = opt.last_grad_norm.cpu()
            assert abs(float(got_norm) - norm64) <= NORM_TOL * norm64
            expect = torch.clamp(clip / (got_norm + 1e-6), max=1.0)
            assert expect.dtype == torch.float32
            assert torch.equal(opt.last_clip_coef.cpu().view(torch.int32), expect.view(torch.int32))
            coef = float(opt.last_clip_coef)
            assert 0.0 < coef < 1.0, "the step must clip"
        sched.step(groups, grads, coef=coef, torch_rule=torch_rule)
        if not torch_rule:
            w = _compare(params, opt, sched)
            print(f"{label} step {step}: max |err| / bound {w:.3f}")
            assert w <= 1.0, (label, step)
            worst = max(worst, w)
        if each_step is not None:
            each_step(step)
    return worst


def test_fused_adam_follows_reduce_lr_on_plateau():
    """twelve steps, torch.optim.lr_scheduler.ReduceLROnPlateau attached to the FusedAdam instance and fed a loss list
    that lowers lr twice"""
    values = _start_values()
    guard, params = _guarded_params(values)
    opt = pkg().FusedAdam(params, **GROUP_A)
    plateau = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=0.5, patience=1)
    losses = [1.0, 0.9, 0.9, 0.9, 0.8, 0.8, 0.8, 0.75, 0.7, 0.65, 0.6, 0.55]
    lrs = []

    def each_step(step):
        lrs.append(opt.param_groups[0]["lr"])
        plateau.step(losses[step - 1])
    sched = R.Schedule(values)
    worst = _drive(opt, params, sched, range(1, 13), each_step=each_step, label="plateau")
    guard.check()
    assert lrs[0] == GROUP_A["lr"] and lrs[-1] == GROUP_A["lr"] * 0.25 and len(set(lrs)) == 3, lrs
    print(f"ReduceLROnPlateau, 12 steps: max |err| / accumulated bound {worst:.3f}")


@pytest.mark.parametrize("max_norm", [None, 50.0], ids=["unclipped", "clipped"])
def test_fused_adam_two_groups_late_joiner_and_skipped_gradients(max_norm):
    values = _start_values()
    guard, params = _guarded_params(values)
    opt = _two_groups(params, max_grad_norm=max_norm)
    sched = R.Schedule(values)
    worst = _drive(opt, params, sched, range(1, 7), has_grad=_has_grad, clip=max_norm, label=f"groups clip={max_norm}")
    guard.check()
    assert sched.t[LATE] == 3 and sched.t[SKIPPING] == 4 and sched.t[0] == 6
    assert opt.state[params[LATE]]["step"] == 3 and opt.state[params[SKIPPING]]["step"] == 4
    print(f"two groups, max_grad_norm={max_norm}: max |err| / accumulated bound {worst:.3f}")


def test_fused_adam_resume_is_bit_exact():
    """five steps, state_dict() through torch.save / torch.load in memory into a new FusedAdam over cloned parameters, five
    more: the bits of the uninterrupted ten steps, inside the bounds"""
    values = _start_values()
    guard_a, pa = _guarded_params(values)
    oa = _two_groups(pa)
    sa = R.Schedule(values)
    worst = _drive(oa, pa, sa, range(1, 11), has_grad=_has_grad, label="uninterrupted")
    guard_b, pb = _guarded_params(values)
    ob = _two_groups(pb)
    sb = R.Schedule(values)
    _drive(ob, pb, sb, range(1, 6), has_grad=_has_grad, label="first half")
    buf = io.BytesIO()
    torch.save(ob.state_dict(), buf)
    buf.seek(0)
    saved = torch.load(buf)
    guard_c, pc = _guarded_params([p.detach().cpu().numpy() for p in pb])
    oc = _two_groups(pc)
    oc.load_state_dict(saved)
    assert all(type(st["step"]) is int for st in oc.state.values())
    worst = max(worst, _drive(oc, pc, sb, range(6, 11), has_grad=_has_grad, label="resumed"))
    for g in (guard_a, guard_b, guard_c):
        g.check()
    for i, (x, y) in enumerate(zip(pa, pc)):
        assert torch.equal(x.detach().view(torch.int32), y.detach().view(torch.int32)), i
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[x][key].view(torch.int32), oc.state[y][key].view(torch.int32)), (i, key)
        assert oa.state[x]["step"] == oc.state[y]["step"]
    print(f"resume: max |err| / accumulated bound {worst:.3f}")


def test_fused_adam_resumes_a_torch_adam_checkpoint():
    """torch.optim.Adam's state after three steps on the same device tensors (its `step` is a tensor) loads into
    FusedAdam; the next three steps are inside the bounds of the six-step float64 run, widened by torch_deviation for the
    three steps torch took"""
    values = _start_values()
    guard, params = _guarded_params(values)
    topt = torch.optim.Adam(params, foreach=False, **GROUP_A)
    sched = R.Schedule(values)
    _drive(topt, params, sched, range(1, 4), torch_rule=True)
    assert isinstance(topt.state[params[0]]["step"], torch.Tensor)
    sched.widen()
    print(f"torch.optim.Adam's own three steps: max |err| / widened bound {_compare(params, topt, sched):.3f} (not asserted)")
    opt = pkg().FusedAdam(params, **GROUP_A)
    opt.load_state_dict(topt.state_dict())
    worst = _drive(opt, params, sched, range(4, 7), label="after torch's checkpoint")
    guard.check()
    assert all(type(st["step"]) is int and st["step"] == 6 for st in opt.state.values())
    print(f"torch checkpoint -> FusedAdam: max |err| / widened bound {worst:.3f}")


def test_torch_adam_resumes_a_fused_adam_checkpoint():
    values = _start_values()
    guard, params = _guarded_params(values)
    opt = pkg().FusedAdam(params, **GROUP_A)
    sched = R.Schedule(values)
    as_torch = R.Schedule(values, mode="torch", bounds=False)     # torch's rule in float64, beside the library's
    measured = {}

    def each_step(step):
        grads = {i: _grad_values(i, step) for i in range(len(params))}
        # elements whose decay term does not cancel the gradient (|wd p + g| at least half of |wd p| + |g|): elsewhere
        # the f32 rounding of the weight decay itself is magnified in g' and says nothing about the betas
        wd = GROUP_A["weight_decay"]
        keep = [(wd * as_torch.p[i] + torch.from_numpy(grads[i]).double()).abs() >=
                0.5 * ((wd * as_torch.p[i]).abs() + torch.from_numpy(grads[i]).double().abs()) for i in range(len(params))]
        as_torch.step([(GROUP_A, list(range(len(params))))], grads)
        measured[step] = max(float(((opt.state[p]["exp_avg_sq"].cpu().double() - as_torch.v[i]).abs() / as_torch.v[i])[keep[i]]
                                   .max()) for i, p in enumerate(params) if bool(keep[i].any()))
    _drive(opt, params, sched, range(1, 4), each_step=each_step, label="before the hand-over")
    analytic = R.torch_deviation(GROUP_A, 1)["v"]
    print(f"exp_avg_sq of the kernels against torch's rule in float64, reference hyper-parameters: step 1 {measured[1]:.4e} "
          f"(analytic {analytic:.4e}), step 3 {measured[3]:.4e}")
    # the f32-beta rule's gap and nothing else.  From zero moments v' = fl(fl(omb2 * gd) * gd): two roundings; gd carries its
    # own rounding and the f32 rounding of the weight decay, each at most doubled by the cancellation the mask admits and
    # doubled again by the square: 2 + 2 * 2 * 2 = 10 unit roundoffs
    assert abs(measured[1] - analytic) <= 10 * R.U
    topt = torch.optim.Adam(params, foreach=False, **GROUP_A)
    topt.load_state_dict(opt.state_dict())
    before = [p.detach().clone() for p in params]
    _drive(topt, params, sched, range(4, 7), torch_rule=True)
    sched.widen()
    guard.check()
    assert all(int(topt.state[p]["step"]) == 6 for p in params)
    assert all(bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), b) for p, b in zip(params, before))
    print(f"FusedAdam checkpoint -> torch.optim.Adam, three steps: max |err| / widened bound "
          f"{_compare(params, topt, sched):.3f} (torch's arithmetic, not asserted)")


# ---- FusedAdam on a plan model --------------------------------------------------------------------------------------------
def _attention_model(dt):
    P = pkg()
    m = P.AttentionHierarchicalCNN(12, dropout_rate=0.0, compute_dtype=dt, max_batch=2)
    m.load_state_dict(pkg("synth").synth_state_dict(m))
    return m


def _eval_logits(m, data):
    m.eval()
    with torch.no_grad():
        return m(*data).float().clone()


def _prescribed(p, gen):
    """magnitudes 1e-6 .. 1e-1, log-uniform, random signs, made on the device"""
    mag = 10.0 ** (torch.rand(p.shape, generator=gen, device=p.device) * 5.0 - 6.0)
    sign = torch.where(torch.rand(p.shape, generator=gen, device=p.device) < 0.5, -1.0, 1.0)
    return (mag * sign).float().contiguous()


@pytest.mark.parametrize("n_groups", [1, 2], ids=["one_group", "two_groups"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_fused_adam_on_a_plan_model(dt, n_groups):
    """Two steps with prescribed gradients on every parameter and lr changed in between.  The gradients are not the
    plan's own, so the step is the serial qt_plan_adam_step (one group: the batched Adam + pack kernel over the model's
    real item list, which the plan hands over in chunks of at most 32, plus the multi-tensor kernel for the rest) or, with
    two groups, the multi-tensor kernel plus invalidate_weights.  Masters and moments per element inside the bounds; eval logits afterwards are those of a
    fresh model loaded from the stepped state_dict, bit for bit."""
    dev = _dev()
    P, synth = pkg(), pkg("synth")
    data = (synth.synth_images(2, salt=9).to(dev), synth.synth_pose_features(2, salt=9).to(dev))
    model = _attention_model(dt).to(dev)
    _eval_logits(model, data)                       # builds the plan and binds the parameters
    params = list(model.parameters())
    assert model._engine is not None and sum(i >= 0 for i in model._param_plan_index) > 32
    if n_groups == 1:
        opt = P.FusedAdam(params, model=model, **GROUP_A)
    else:
        half = len(params) // 2
        opt = P.FusedAdam([dict(params=params[:half], **GROUP_A), dict(params=params[half:], **GROUP_B)], model=model)
    sched = R.Schedule([p.detach() for p in params])
    gen = torch.Generator(device=dev).manual_seed(77)
    worst = 0.0
    for step in (1, 2):
        grads = {i: _prescribed(p, gen) for i, p in enumerate(params)}
        for i, p in enumerate(params):
            p.grad = grads[i].clone()
        groups = _groups_now(opt, params)
        opt.step()
        assert model._engine.last_adam_overlapped is False
        for i, p in enumerate(params):
            assert torch.equal(p.grad.view(torch.int32), grads[i].view(torch.int32)), f"step() changed gradient {i}"
        sched.step(groups, grads)
        w = 0.0
        for i, p in enumerate(params):
            st = opt.state[p]
            w = max(w, R.share(p.detach(), sched.p[i], sched.e[i][0]), R.share(st["exp_avg"], sched.m[i], sched.e[i][1]),
                    R.share(st["exp_avg_sq"], sched.v[i], sched.e[i][2]))
        print(f"plan model {dt}, {n_groups} group(s), step {step}: max |err| / bound {w:.3f}")
        assert w <= 1.0
        worst = max(worst, w)
        for g in opt.param_groups:
            g["lr"] = g["lr"] * 0.5
    got = _eval_logits(model, data)
    fresh = _attention_model(dt)
    fresh.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    want = _eval_logits(fresh.to(dev), data)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    print(f"plan model {dt}, {n_groups} group(s): max |err| / accumulated bound {worst:.3f}")
