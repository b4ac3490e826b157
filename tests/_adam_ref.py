"""Float64 reference, f32 restatement and DERIVED per-element bounds for the Adam kernels (csrc/pack.hip: adam_update as
used by adam_multi_kernel and pack_weights_batched_kernel; csrc/plan.hip: adam_step; optim.py: FusedAdam).  Shared by
tests/test_adam_ref_cpu.py (no GPU: the reference against float64 torch.optim.Adam, the restatement inside the bounds, damaged
restatements outside them) and tests/test_adam_gpu.py (the kernels).

The rule the library promises ("abi" mode) is torch.optim.Adam's (L2 decay added to the gradient, bias-corrected moments, no
amsgrad) with the hyper-parameters AS THE C ABI CARRIES THEM: lr, betas, eps and weight decay are f32 values, 1 - beta is
f32(1) - f32(beta), and the bias corrections are formed in double from the f32 beta, step_size = lr / (1 - b1^t) and
1 / sqrt(1 - b2^t) each rounded to f32 once (make_adam_scalars).  "torch" mode takes the Python doubles the way torch does.

adam_update, rounding by rounding (fl = one f32 round-to-nearest, fma = one rounding of an exact product-sum):
    gs = fl(g * s)            gd = fma(wd, p, gs)
    t  = fl((1 - b1) * gd)    m' = fma(b1, m, t)
    vo = fl(b2 * v)           t1 = fl((1 - b2) * gd)     vn = fl(t1 * gd)      v' = fl(vo + vn)
    sq = fl(sqrt(v'))         D  = fma(sq, isb, eps)     q  = fl(m' / D)       p' = fma(-ss, q, p)

Bound rule (tests/_bounds.py): the standard forward error of exactly that chain, evaluated per element in float64.  Every
rounding of a computed value x^ contributes U * |x^| + ETA, with |x^| <= |x| + (the error x^ already carries), U = 2^-24 and
ETA = 2^-149 (gradual underflow: an f32 result never misses by more than the smallest subnormal); the errors are pushed
through each operation with its exact Lipschitz form (products: both factors' errors and their product; square root:
|a - b| / (sqrt a + sqrt b); quotient: (E_m + |q| E_D) / (D - E_D)).  The constants are the roundings listed above and the
two unit constants, nothing is fitted to what a kernel returns.  The bound on p' is therefore relative to |p| plus the
magnitude of the update, those on m' and v' to the magnitudes of their two terms.  Errors of the INPUTS (e_in) go through the
same forms, which is how a schedule of several steps accumulates its bound.  Overflow is not modelled: chain_flags()
shows, on the reference alone, that no intermediate of the main input classes leaves the normal f32 range.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
ETA = 2.0 ** -149
F32_MIN_NORMAL = 2.0 ** -126
F32_MAX = float(np.finfo(np.float32).max)

# (lr, beta1, beta2, eps, weight decay)
HYPERS = {
    "reference": dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4),   # the reference trainers'
    "existing": dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.02),     # test_adam_multi_kernel_*
    "wd0": dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
    "lr0": dict(lr=0.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4),
    "beta1_0": dict(lr=1e-4, betas=(0.0, 0.999), eps=1e-8, weight_decay=1e-4),
}
STEPS = [1, 2, 10, 1000, 100000]
# (grad_scale in the descriptor, coefficient read from device memory or None)
SCALES = {"none": (1.0, None), "desc": (0.5, None), "device": (1.0, 0.25), "both": (0.5, 0.25)}
MULTI_SIZES = [1, 4095, 4096, 4097]        # adam_multi_kernel: 4096 elements per block
DAMAGES = {   # damaged restatement -> the input class (hyper, step, scale) at which it must miss a bound
    "no_bias_correction": ("reference", 2, "none"),
    "adamw_decay": ("reference", 10, "none"),
    "eps_inside_sqrt": ("reference", 10, "none"),
    "beta2_for_first_moment": ("reference", 10, "none"),
    "scale_after_decay": ("reference", 10, "desc"),
    "step_off_by_one": ("reference", 1, "none"),
}


def f32(x):
    return float(np.float32(x))


def effective_scale(desc_scale, dev_coef):
    """grad_scale as the kernel forms it: the descriptor's f32 (0 means 1) times the device float, one f32 rounding"""
    s = np.float32(1.0 if desc_scale == 0 else desc_scale)
    return float(s if dev_coef is None else s * np.float32(dev_coef))


def scalars(hyper, step, mode="abi"):
    """the scalars of one step as doubles: lr b1 b2 eps wd omb1 omb2 ss (step_size) isb (1 / sqrt(bias correction 2))"""
    lr, (b1, b2), eps, wd = hyper["lr"], hyper["betas"], hyper["eps"], hyper["weight_decay"]
    step = int(step)
    if mode == "abi":
        lr, b1, b2, eps, wd = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)
        omb1 = float(np.float32(1) - np.float32(b1))
        omb2 = float(np.float32(1) - np.float32(b2))
        ss = f32(lr / (1.0 - b1 ** step))
        isb = f32(1.0 / math.sqrt(1.0 - b2 ** step))
    elif mode == "torch":
        omb1, omb2 = 1.0 - b1, 1.0 - b2
        ss = lr / (1.0 - b1 ** step)
        isb = 1.0 / math.sqrt(1.0 - b2 ** step)
    else:
        raise ValueError(mode)
    return dict(lr=lr, b1=b1, b2=b2, eps=eps, wd=wd, omb1=omb1, omb2=omb2, ss=ss, isb=isb)


def _d(x):
    return torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x).double()


def _rnd(x, e):
    """the error of fl(x^) where |x^ - x| <= e: what x^ carries plus its own rounding"""
    return e + U * (x.abs() + e) + ETA


def adam64_full(p, g, m, v, hyper, step, grad_scale=1.0, mode="abi", e_in=None):
    """One step in float64 with the per-element bounds of the kernel's chain.  p g m v: tensors of any float dtype on one
    device.  e_in: None or (E_p, E_m, E_v), bounds the inputs already carry.  Returns a dict: p m v (new values), bp bm bv
    (bounds on what adam_update leaves for them), upd (|step_size * m' / D|) and chain, the intermediates whose f32 range
    chain_flags() looks at."""
    h = scalars(hyper, step, mode)
    p, g, m, v = _d(p), _d(g), _d(m), _d(v)
    s = float(grad_scale)
    zero = torch.zeros_like(p)
    ep, em, ev = (zero, zero, zero) if e_in is None else (_d(x) for x in e_in)
    gs = g * s
    gd = h["wd"] * p + gs
    t = h["omb1"] * gd
    bm_old = h["b1"] * m
    m2 = bm_old + t
    vo = h["b2"] * v
    t1 = h["omb2"] * gd
    vn = t1 * gd
    v2 = vo + vn
    sq = torch.sqrt(v2)
    D = sq * h["isb"] + h["eps"]
    q = m2 / D
    upd = h["ss"] * q
    p2 = p - upd
    # ---- the error of the kernel's chain, rounding by rounding ----
    e_gs = _rnd(gs, zero)                                            # fl(g * s): g itself is exact
    e_gd = _rnd(gd, h["wd"] * ep + e_gs)                             # fma(wd, p, gs)
    e_t = _rnd(t, h["omb1"] * e_gd)                                  # fl(omb1 * gd)
    e_m = _rnd(m2, h["b1"] * em + e_t)                               # fma(b1, m, t)
    e_vo = _rnd(vo, h["b2"] * ev)                                    # fl(b2 * v)
    e_t1 = _rnd(t1, h["omb2"] * e_gd)                                # fl(omb2 * gd)
    e_vn = _rnd(vn, e_t1 * gd.abs() + t1.abs() * e_gd + e_t1 * e_gd)  # fl(t1 * gd)
    e_v = _rnd(v2, e_vo + e_vn)                                      # fl(vo + vn)
    low = torch.sqrt((v2 - e_v).clamp_min(0.0))
    e_sq = _rnd(sq, torch.where(e_v > 0, e_v / (sq + low).clamp_min(1e-300), zero))   # fl(sqrt(v'))
    e_D = _rnd(D, h["isb"] * e_sq)                                   # fma(sq, isb, eps)
    room = D - e_D
    ok = room > 0
    e_q = _rnd(q, torch.where(ok, (e_m + q.abs() * e_D) / room.clamp_min(1e-300), torch.full_like(p, float("inf"))))
    e_p = _rnd(p2, ep + h["ss"] * e_q)                               # fma(-ss, q, p)
    chain = dict(gs=gs, gd=gd, t=t, bm_old=bm_old, m=m2, vo=vo, t1=t1, vn=vn, v=v2, sq=sq, D=D, q=q, upd=upd, p=p2)
    return dict(p=p2, m=m2, v=v2, bp=e_p, bm=e_m, bv=e_v, upd=upd.abs(), chain=chain)


def adam64(p, g, m, v, hyper, step, grad_scale=1.0, mode="abi"):
    """torch.optim.Adam's rule in float64: (new p, new m, new v)"""
    r = adam64_full(p, g, m, v, hyper, step, grad_scale, mode)
    return r["p"], r["m"], r["v"]


def chain_flags(full):
    """per element: does any intermediate of the reference chain leave the normal f32 range (a non-zero magnitude below
    2^-126, a magnitude above the largest f32, or a non-finite value)?"""
    bad = None
    for x in full["chain"].values():
        a = x.abs()
        b = ((a > 0) & (a < F32_MIN_NORMAL)) | (a > F32_MAX) | ~torch.isfinite(x)
        bad = b if bad is None else (bad | b)
    return bad


def share(got, ref, bound):
    """max |got - ref| / bound over the elements (inf for a non-finite result or a missed zero bound)"""
    ref = _d(ref)
    got, bound = _d(got).to(ref.device), _d(bound).to(ref.device)
    if got.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300),
                    torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(r.max())


# ---- the kernel's own arithmetic in numpy f32 -----------------------------------------------------------------------------
def _fma(a, b, c):
    """an exact double product (24 x 24 bits) and a double sum, rounded to f32 once"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def adam_mixed(p, g, m, v, hyper, step, grad_scale=1.0, damage=None):
    """adam_update with one numpy f32 operation per rounding it spells out.  p g m v: f32 arrays.  Returns f32 (p, m, v).
    damage: None, or one of DAMAGES -- a wrong rule in the same arithmetic, which the bounds must reject."""
    F = np.float32
    p, g, m, v = (np.asarray(x, dtype=F) for x in (p, g, m, v))
    bc_step = step + 1 if damage == "step_off_by_one" else step
    h = scalars(hyper, bc_step, "abi")
    if damage == "no_bias_correction" and step >= 2:
        h["ss"], h["isb"] = h["lr"], 1.0
    lr, b1, b2, eps, wd, ss, isb = (F(h[k]) for k in ("lr", "b1", "b2", "eps", "wd", "ss", "isb"))
    s = F(grad_scale)
    one = F(1)
    with np.errstate(all="ignore"):
        if damage == "adamw_decay":
            p = (p * (one - lr * wd)).astype(F)
            gd = (g * s).astype(F)
        elif damage == "scale_after_decay":
            gd = (_fma(wd, p, g) * s).astype(F)
        else:
            gd = _fma(wd, p, (g * s).astype(F))
        bm = b2 if damage == "beta2_for_first_moment" else b1
        m2 = _fma(bm, m, ((one - bm) * gd).astype(F))
        vo = (b2 * v).astype(F)
        vn = (((one - b2) * gd).astype(F) * gd).astype(F)
        v2 = (vo + vn).astype(F)
        if damage == "eps_inside_sqrt":
            den = np.sqrt(_fma(v2, (isb * isb).astype(F), eps)).astype(F)
        else:
            den = _fma(np.sqrt(v2).astype(F), isb, eps)
        q = (m2 / den).astype(F)
        p2 = _fma(-ss, q, p)
    return p2, m2, v2


def classify(x):
    """0 finite and non-zero, 1 zero, 2 NaN, 3 infinite"""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.isnan(x), 2, np.where(np.isinf(x), 3, np.where(x == 0, 1, 0)))


# ---- the two modes against each other -------------------------------------------------------------------------------------
def torch_deviation(hyper, step):
    """First-order relative difference between the abi rule and torch's for a state run `step` steps from zero moments
    and for that step's update.  v and m: the weight of the new term, |f32(1) - f32(beta) - (1 - beta)| / (1 - beta), plus
    (step - 1) times the relative rounding of beta itself on the terms carried over (v relative to v, whose terms are
    non-negative; m relative to the sum of its terms' magnitudes).  update: m's figure, half of v's, and the matching
    bias-correction terms |step_size_abi / step_size_torch - 1| and |isb_abi / isb_torch - 1| (lr's own f32 rounding is in
    the first).  Explains the gap to torch; never a tolerance for a kernel."""
    a, t = scalars(hyper, step, "abi"), scalars(hyper, step, "torch")
    dm = abs(a["omb1"] - t["omb1"]) / t["omb1"] + (step - 1) * (abs(a["b1"] - t["b1"]) / t["b1"] if t["b1"] else 0.0)
    dv = abs(a["omb2"] - t["omb2"]) / t["omb2"] + (step - 1) * (abs(a["b2"] - t["b2"]) / t["b2"] if t["b2"] else 0.0)
    dss = abs(a["ss"] / t["ss"] - 1.0) if t["ss"] else 0.0
    disb = abs(a["isb"] / t["isb"] - 1.0)
    return dict(m=dm, v=dv, update=dm + 0.5 * dv + dss + disb)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def main_inputs(n, seed):
    """f32 arrays p g m v of n elements: gradients 1e-6 .. 1e3 and parameters 1e-4 .. 10 in magnitude (log-uniform, random
    signs, the extremes present from n >= 4 on), moments that such gradients leave: |m| in 0.1 .. 1 times a gradient of the
    element's scale, v in 0.1 .. 3 times its square."""
    r = np.random.RandomState(seed)
    lg = r.uniform(-6.0, 3.0, n)
    lp = r.uniform(-4.0, 1.0, n)
    if n >= 4:
        lg[:2], lp[:2] = (-6.0, 3.0), (1.0, -4.0)
        lg[-2:], lp[-2:] = (3.0, -6.0), (1.0, -4.0)
    g = r.choice([-1.0, 1.0], n) * 10.0 ** lg
    p = r.choice([-1.0, 1.0], n) * 10.0 ** lp
    m = r.choice([-1.0, 1.0], n) * 10.0 ** lg * r.uniform(0.1, 1.0, n)
    v = 10.0 ** (2 * lg) * r.uniform(0.1, 3.0, n)
    return tuple(x.astype(np.float32) for x in (p, g, m, v))


EDGE_KINDS = ["g0_v0", "g0_v0_m0_p0", "tiny_g", "tiny_g_v0", "plain"]


def edge_inputs(n, seed):
    """The edge class: element i is of kind EDGE_KINDS[i % 5].
      g0_v0         g = 0, v = 0, m != 0: with weight decay 0 the denominator is eps alone
      g0_v0_m0_p0   everything zero: 0 / eps = 0, and 0 / 0 = NaN when eps = 0
      tiny_g        |g| around 1e-21 (g * g is subnormal in f32), ordinary m and v
      tiny_g_v0     the same with v = 0 and m = 0: the new v is a subnormal
      plain         an element of the main class
    Returns (p, g, m, v, kind index per element)."""
    p, g, m, v = (x.copy() for x in main_inputs(n, seed))
    r = np.random.RandomState(seed + 1)
    kind = np.arange(n) % len(EDGE_KINDS)
    tiny = (r.choice([-1.0, 1.0], n) * r.uniform(0.5e-21, 2e-21, n)).astype(np.float32)
    k = kind == 0
    g[k], v[k] = 0, 0
    k = kind == 1
    p[k], g[k], m[k], v[k] = 0, 0, 0, 0
    k = kind == 2
    g[k] = tiny[k]
    k = kind == 3
    g[k], m[k], v[k] = tiny[k], 0, 0
    return p, g, m, v, kind


EDGE_HYPERS = {   # weight decay 0, or the decay term would hide g = 0 and the tiny gradients
    "edge_eps": dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
    "edge_eps0": dict(lr=1e-4, betas=(0.9, 0.999), eps=0.0, weight_decay=0.0),
}


def edge_check(got, mixed, full):
    """The edge class's comparison.  got / mixed: (p, m, v) from the code under test / from adam_mixed; full: adam64_full of
    the same inputs.  Every element must fall in adam_mixed's class (finite, zero, NaN, infinite); elements that are finite
    there and have a finite bound must be inside it.  Returns (elements whose reference chain leaves the normal f32 range
    or that are not finite and non-zero in some output, worst share of a bound among the finite ones)."""
    special = chain_flags(full).cpu().numpy().copy()
    worst = 0.0
    for x, y, r, b in zip(got, mixed, ("p", "m", "v"), ("bp", "bm", "bv")):
        cx, cy = classify(x), classify(y)
        assert np.array_equal(cx, cy), (r, "classes differ at", np.nonzero(cx != cy)[0][:8])
        special |= cy != 0
        ref, bound = full[r].cpu().numpy(), full[b].cpu().numpy()
        fin = (cy <= 1) & np.isfinite(bound) & np.isfinite(ref)
        if fin.any():
            worst = max(worst, share(np.asarray(x, np.float64)[fin], ref[fin], bound[fin]))
    return int(special.sum()), worst


# ---- schedules ------------------------------------------------------------------------------------------------------------
class Schedule:
    """A list of float64 parameters driven through step records with FusedAdam.step's semantics: a parameter's step counts
    only the steps in which it had a gradient, its moments start at zero with its first gradient, the global norm covers
    every parameter with a gradient in the step, each group brings its own hyper-parameters.  With bounds=True the
    per-element bounds accumulate from step to step (adam64_full's e_in)."""

    def __init__(self, params, mode="abi", bounds=True):
        self.p = [_d(x).clone() for x in params]
        self.m = [torch.zeros_like(x) for x in self.p]
        self.v = [torch.zeros_like(x) for x in self.p]
        self.t = [0] * len(self.p)
        self.mode, self.bounds = mode, bounds
        self.e = [tuple(torch.zeros_like(x) for _ in range(3)) for x in self.p]
        self.am = [torch.zeros_like(x) for x in self.p]     # sum of the magnitudes of exp_avg's terms
        self.w = [tuple(torch.zeros_like(x) for _ in range(3)) for x in self.p]   # widening by torch_deviation
        self.last_norm = None
        self.last_coef = None

    def load(self, i, step, m, v, e=None):
        self.t[i], self.m[i], self.v[i] = int(step), _d(m).clone(), _d(v).clone()
        if e is not None:
            self.e[i] = tuple(_d(x).clone() for x in e)

    def step(self, groups, grads, max_norm=None, coef=None, torch_rule=False):
        """groups: [(hyper, [parameter indices])]; grads: {index: gradient}; max_norm: clip by the global norm with
        torch's coefficient min(1, max_norm / (norm + 1e-6)) in double, unless `coef` gives the coefficient to use.
        torch_rule: this step is taken by torch.optim.Adam, not by the library: self.w collects, per element, what
        torch_deviation allows the two rules to differ by -- on exp_avg its figure times the sum of the magnitudes of
        exp_avg's terms, on exp_avg_sq its figure times exp_avg_sq, on p (summed over such steps) step_size times
        exp_avg's allowance over the denominator plus the update's magnitude times the remaining terms.  (The feedback
        of p's allowance through the decay term, weight decay times 1e-5 * lr, is left out.)  widen() adds it to the
        bounds."""
        sq = sum(float((_d(x) ** 2).sum()) for x in grads.values())
        self.last_norm = math.sqrt(sq)
        scale = 1.0
        if coef is not None:
            scale = float(coef)
        elif max_norm is not None:
            scale = min(1.0, max_norm / (self.last_norm + 1e-6))
        self.last_coef = scale
        for hyper, idx in groups:
            for i in idx:
                if i not in grads or grads[i] is None:
                    continue
                self.t[i] += 1
                r = adam64_full(self.p[i], grads[i], self.m[i], self.v[i], hyper, self.t[i], scale, self.mode,
                                self.e[i] if self.bounds else None)
                self.p[i], self.m[i], self.v[i] = r["p"], r["m"], r["v"]
                if self.bounds:
                    self.e[i] = (r["bp"], r["bm"], r["bv"])
                h = scalars(hyper, self.t[i], self.mode)
                self.am[i] = h["b1"] * self.am[i] + h["omb1"] * r["chain"]["gd"].abs()
                if torch_rule:
                    d = torch_deviation(hyper, self.t[i])
                    wm, wv = d["m"] * self.am[i], d["v"] * r["v"]
                    rest = d["update"] - d["m"]
                    self.w[i] = (self.w[i][0] + h["ss"] * wm / r["chain"]["D"] + r["upd"] * rest, wm, wv)

    def widen(self):
        """fold the allowance of the torch_rule steps into the accumulated bounds (once, after the last such step)"""
        for i in range(len(self.p)):
            self.e[i] = tuple(e + w for e, w in zip(self.e[i], self.w[i]))
            self.w[i] = tuple(torch.zeros_like(x) for x in self.w[i])
