"""tests/_adam_ref.py on its own, no GPU: the float64 reference and the schedule semantics against float64 torch.optim.Adam,
the f32 restatement of adam_update inside every derived bound on every input class tests/test_adam_gpu.py uses, six damaged
restatements outside them, the analytic gap between the library's rule (f32 betas) and torch's against the measured one, and
the conditions on the inputs (no f32 underflow / overflow in the main classes; the edge class lists which elements have one).
"""
import itertools

import numpy as np
import pytest
import torch

import _adam_ref as R

N_MAIN = 4097


# ---- anchor: adam64 in torch mode and the schedule against torch.optim.Adam on float64 CPU parameters ----------------------
GROUP_A = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
GROUP_B = dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.02)
ANCHOR_SIZES = [1, 7, 33, 5, 12]
LATE, SKIPPING = 2, 3          # parameter 2 gets its first gradient at step 4, parameter 3 has none at steps 2 and 5


def _has_grad(i, step):
    if i == LATE:
        return step >= 4
    if i == SKIPPING:
        return step not in (2, 5)
    return True


@pytest.mark.parametrize("max_norm", [None, 0.5])
def test_adam64_torch_mode_equals_float64_torch_adam(max_norm):
    """20 steps, two param groups, a late joiner, a skipped gradient, with and without clipping by the global norm: every
    element of p, exp_avg and exp_avg_sq within 1e-12 relative of torch.optim.Adam(foreach=False) in float64."""
    g = torch.Generator().manual_seed(5)
    start = [torch.randn(n, generator=g, dtype=torch.float64) for n in ANCHOR_SIZES]
    params = [torch.nn.Parameter(x.clone()) for x in start]
    groups = [(GROUP_A, [0, 1, 2]), (GROUP_B, [3, 4])]
    opt = torch.optim.Adam([dict(params=[params[i] for i in idx], **h) for h, idx in groups], foreach=False)
    sched = R.Schedule(start, mode="torch", bounds=False)
    for step in range(1, 21):
        grads = {i: torch.randn(n, generator=g, dtype=torch.float64) * 10.0 ** ((i + step) % 5 - 2)
                 for i, n in enumerate(ANCHOR_SIZES) if _has_grad(i, step)}
        for i, p in enumerate(params):
            p.grad = grads[i].clone() if i in grads else None
        if max_norm is not None:
            norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        sched.step(groups, grads, max_norm=max_norm)
        if max_norm is not None:
            assert abs(sched.last_norm - float(norm)) <= 1e-12 * float(norm)
    assert sched.t == [20, 20, 17, 18, 20]
    for i, p in enumerate(params):
        st = opt.state[p]
        assert int(st["step"]) == sched.t[i]
        for name, got, want in (("p", sched.p[i], p.detach()), ("m", sched.m[i], st["exp_avg"]),
                                ("v", sched.v[i], st["exp_avg_sq"])):
            rel = float(((got - want).abs() / want.abs().clamp_min(1e-300)).max())
            assert rel <= 1e-12, (i, name, rel)


# ---- the restatement inside the bounds ------------------------------------------------------------------------------------
def _case(hyper, step, scale, inputs, damage=None):
    p, g, m, v = inputs
    desc, dev = R.SCALES[scale]
    s = R.effective_scale(desc, dev)
    full = R.adam64_full(p, g, m, v, hyper, step, s)
    got = R.adam_mixed(p, g, m, v, hyper, step, s, damage)
    return full, {k: R.share(x, full[k], full["b" + k]) for k, x in zip("pmv", got)}


@pytest.mark.parametrize("hname", list(R.HYPERS))
def test_adam_mixed_stays_inside_every_bound(hname):
    """every step count and gradient scale of the GPU file at this hyper-parameter set; records the largest share"""
    inputs = R.main_inputs(N_MAIN, 11)
    worst = dict(p=0.0, m=0.0, v=0.0)
    for step, scale in itertools.product(R.STEPS, R.SCALES):
        full, shares = _case(R.HYPERS[hname], step, scale, inputs)
        assert int(R.chain_flags(full).sum()) == 0, (step, scale)
        for k, s in shares.items():
            assert s <= 1.0, (hname, step, scale, k, s)
            worst[k] = max(worst[k], s)
    print(f"adam_mixed, {hname}: largest share of the bound p {worst['p']:.3f} m {worst['m']:.3f} v {worst['v']:.3f}")
    assert max(worst.values()) > 0.05, "a bound nothing comes near tests nothing"


@pytest.mark.parametrize("damage", list(R.DAMAGES))
def test_damaged_restatement_misses_a_bound(damage):
    hname, step, scale = R.DAMAGES[damage]
    inputs = R.main_inputs(N_MAIN, 11)
    _, good = _case(R.HYPERS[hname], step, scale, inputs)
    _, bad = _case(R.HYPERS[hname], step, scale, inputs, damage)
    print(f"{damage} at ({hname}, step {step}, scale {scale}): shares {bad}; undamaged {good}")
    assert max(good.values()) <= 1.0
    assert max(bad.values()) > 1.0


def test_bounds_accumulate_over_a_schedule():
    """12 steps of adam_mixed fed its own f32 state stay inside the bounds a Schedule accumulates"""
    p, g, m, v = R.main_inputs(N_MAIN, 17)
    hyper = R.HYPERS["reference"]
    sched = R.Schedule([p])
    mp, mm, mv = p, np.zeros_like(p), np.zeros_like(p)
    r = np.random.RandomState(3)
    worst = 0.0
    for step in range(1, 13):
        grad = (g * r.choice([-1.0, 1.0], g.size)).astype(np.float32)
        mp, mm, mv = R.adam_mixed(mp, grad, mm, mv, hyper, step)
        sched.step([(hyper, [0])], {0: grad})
        for got, ref, b in ((mp, sched.p[0], sched.e[0][0]), (mm, sched.m[0], sched.e[0][1]), (mv, sched.v[0], sched.e[0][2])):
            s = R.share(got, ref, b)
            worst = max(worst, s)
            assert s <= 1.0, step
    print(f"12 steps: largest share of the accumulated bound {worst:.3f}")


# ---- the edge class -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hname", list(R.EDGE_HYPERS))
def test_edge_class_lists_its_elements(hname):
    p, g, m, v, kind = R.edge_inputs(1000, 23)
    hyper = R.EDGE_HYPERS[hname]
    for step in (1, 10):
        full = R.adam64_full(p, g, m, v, hyper, step)
        flagged = R.chain_flags(full).numpy()
        assert flagged[(kind == 2) | (kind == 3)].all(), "g * g is subnormal in f32 there"
        assert not flagged[kind == 4].any()
        if hname == "edge_eps":
            assert not flagged[(kind == 0) | (kind == 1)].any()       # exact zeros, a denominator of eps
        else:
            assert flagged[(kind == 0) | (kind == 1)].all()           # x / 0
        mixed = R.adam_mixed(p, g, m, v, hyper, step)
        cls = R.classify(mixed[0])
        if hname == "edge_eps":
            assert (cls <= 1).all()
        else:
            assert (cls[kind == 1] == 2).all() and (cls[kind == 0] == 3).all()      # 0 / 0, m / 0
            ref = torch.nn.Parameter(torch.zeros(1))                  # torch's f32 Adam gives NaN there too
            opt = torch.optim.Adam([ref], foreach=False, **hyper)
            ref.grad = torch.zeros(1)
            opt.step()
            assert bool(torch.isnan(ref.detach()).all())
        n, worst = R.edge_check(mixed, mixed, full)
        print(f"{hname} step {step}: {n} of {kind.size} elements took the class route; finite ones: share {worst:.3f}")
        assert n >= int(((kind == 2) | (kind == 3)).sum()) and worst <= 1.0


# ---- state from and to torch.optim.Adam (the part that needs no GPU) ---------------------------------------------------------
def test_fused_adam_load_state_dict_turns_torch_steps_into_ints():
    from _util import pkg
    P = pkg()
    ps = [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(3))]
    topt = torch.optim.Adam(ps, lr=1e-4, weight_decay=1e-4, foreach=False)
    for _ in range(3):
        for p in ps:
            p.grad = torch.randn_like(p)
        topt.step()
    assert isinstance(topt.state[ps[0]]["step"], torch.Tensor)
    opt = P.FusedAdam(ps, lr=1e-4, weight_decay=1e-4)
    opt.load_state_dict(topt.state_dict())
    for p in ps:
        st = opt.state[p]
        assert type(st["step"]) is int and st["step"] == 3
        assert torch.equal(st["exp_avg"], topt.state[p]["exp_avg"]) and torch.equal(st["exp_avg_sq"], topt.state[p]["exp_avg_sq"])
    assert opt._max_grad_norm() is None
    back = torch.optim.Adam(ps, lr=1e-4, weight_decay=1e-4, foreach=False)
    back.load_state_dict(opt.state_dict())
    for p in ps:
        p.grad = torch.randn_like(p)
    back.step()
    assert all(int(back.state[p]["step"]) == 4 for p in ps)
    sd = topt.state_dict()
    sd["state"][0]["step"] = torch.tensor(2.5)
    with pytest.raises(ValueError, match="step"):
        P.FusedAdam(ps, lr=1e-4).load_state_dict(sd)
    ams = torch.optim.Adam(ps, lr=1e-4, amsgrad=True, foreach=False)
    with pytest.raises(ValueError, match="amsgrad"):
        P.FusedAdam(ps, lr=1e-4).load_state_dict(ams.state_dict())


# ---- the gap to torch -----------------------------------------------------------------------------------------------------
def test_torch_deviation_against_the_measured_difference():
    """weight decay 0, so that both modes see the same gradient; step 1 from zero moments, then three steps"""
    p, g, _, _ = R.main_inputs(N_MAIN, 29)
    zero = np.zeros_like(p)
    hyper = dict(R.HYPERS["reference"], weight_decay=0.0)
    dev = R.torch_deviation(hyper, 1)
    a = R.adam64_full(p, g, zero, zero, hyper, 1, mode="abi")
    t = R.adam64_full(p, g, zero, zero, hyper, 1, mode="torch")
    meas = {k: float(((a[k] - t[k]).abs() / t[k].abs()).max()) for k in ("m", "v", "upd")}
    print(f"step 1: exp_avg_sq differs by {meas['v']:.4e} (analytic {dev['v']:.4e}), exp_avg by {meas['m']:.3e} "
          f"({dev['m']:.3e}), the update by {meas['upd']:.3e} (bound {dev['update']:.3e})")
    assert abs(dev["v"] - 1.29e-5) < 0.005e-5
    assert abs(meas["v"] - dev["v"]) <= 1e-6 * dev["v"]
    assert abs(meas["m"] - dev["m"]) <= 1e-6 * dev["m"] + 1e-15
    assert meas["upd"] <= dev["update"] * (1 + 1e-6)
    assert meas["upd"] < 1e-6, "the rule is self-consistent: v / bc2 = g^2 at step 1 in both modes"
    sa, st = R.Schedule([p], "abi", bounds=False), R.Schedule([p], "torch", bounds=False)
    r = np.random.RandomState(1)
    for step in range(1, 4):
        grad = g * r.uniform(0.5, 2.0, g.size).astype(np.float32)
        for s in (sa, st):
            s.step([(hyper, [0])], {0: grad})
        d = R.torch_deviation(hyper, step)
        assert float(((sa.v[0] - st.v[0]).abs() / st.v[0]).max()) <= d["v"] * (1 + 1e-6)
    # at (0.8, 0.95), the betas the older tests use, the same effect is below their 2e-6
    assert R.torch_deviation(R.HYPERS["existing"], 1)["v"] < 1e-6
