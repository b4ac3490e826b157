"""Float64 references and DERIVED error bounds for the fused loss head (csrc/loss.hip), shared by tests/test_loss_gpu.py (the
kernels on the GPU) and tests/test_loss_cpu.py (a torch-f32 restatement in the kernels' place: correct f32 arithmetic meets the
bounds, three deliberately wrong versions miss them).

References: torch.nn.functional.cross_entropy and the reference FocalLoss formula (3dcnn/models.py:21-45) in float64 on the
CPU, gradients by autograd.

Bounds follow tests/_bounds.py's rule, evaluated per element in float64, for the arithmetic the kernel documents:
    a = argmax, m = z[a], d_k = fl(z_k - m)                     |err d_k| <= U |d_k|
    s1 = sum_{k != a} expf(d_k)   (f32, any order)              (C + 8) U s1 + sum e_k (R_EXP + U |d_k|)
    l = log1pf(s1)                                              err(s1) / (1 + s1) + R_LOG1P l
    -log p_y = fl(l - d_y),  1 - p_y = -expm1f(d_y - l),  p_k = expf(fl(d_k - l)),  (1 - p_y)^(gamma-1) = powf(...)
  * a sum of n f32 terms costs (n + 8) 2^-24 sum |term| (sum_bound);
  * every other f32 operation costs one rounding U of its result; where a short chain of products is lumped together the
    comment gives the count;
  * the cross-row sums are added in double: the reduced loss costs its own f32 rounding (2 U |ref|, as _bounds.py charges a
    double-accumulated output) plus the per-row errors (plus 2^-53-level slack).
  * the float64 references round too: log_softmax in double forms z - logsumexp(z), an absolute error of a few 2^-53
    (1 + max |z|) per row, which is all that is left of a loss of 1e-24 on a saturated row (double gives exactly 0 there).
    REF_SLACK = 16 * 2^-53 * (1 + max_k |z_k|) times the largest class weight is added per row for that, and the same
    factor (without the |z| part) per gradient element.
ASSUMPTION (the ROCm device-math accuracy table is not shipped with the toolkit this suite runs against): expf / log1pf /
expm1f / powf of the device library meet the OpenCL 3.0 single-precision figures (section 7.4 of the OpenCL C specification:
exp <= 3 ulp, log1p <= 2 ulp, expm1 <= 3 ulp, pow <= 16 ulp), the precision the AMD device library is written to; one ulp is
at most 2^-23 relative.  Nothing here is fitted to what a kernel returns."""
import torch
import torch.nn.functional as F

from _bounds import U, UD, ratio, sum_bound  # noqa: F401  (ratio is re-exported to the tests)

ULP_EXP, ULP_LOG1P, ULP_EXPM1, ULP_POW = 3, 2, 3, 16
R_EXP, R_LOG1P, R_EXPM1, R_POW = (2 * U * n for n in (ULP_EXP, ULP_LOG1P, ULP_EXPM1, ULP_POW))

CE, FOCAL = 0, 1
MEAN, SUM, NONE = 0, 1, 2
RED_NAME = {MEAN: "mean", SUM: "sum", NONE: "none"}
IGNORE = -100

# (rows, C): every mapping boundary of the kernel (C = 16 | 17: thread -> 16-lane row; 64 | 65: -> wave) with row counts on
# both sides of one workgroup's reach (256 rows for C <= 16, 16 for C <= 64, 4 above), odd sizes, C = 1 and the largest rows
SHAPES = [(1, 1), (2, 2), (256, 12), (257, 12), (65, 13), (63, 16), (16, 17), (17, 17), (64, 17), (2, 64), (65, 64), (1, 65),
          (4, 65), (5, 65), (2, 1000), (63, 1000)]
SCALES = ["x1", "x30", "+1e4"]


def make_logits(rows, C, scale, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(rows, C, generator=g)
    if scale == "x30":
        z = z * 30.0          # saturated softmax
    elif scale == "+1e4":
        z = z + 1e4           # only the max-subtraction keeps this finite
    return z.float()


def make_labels(rows, C, ignored, seed):
    """ignored: 'no' | 'some' (every third row, at least one when rows >= 2) | 'all'"""
    g = torch.Generator().manual_seed(seed + 1)
    y = torch.randint(0, C, (rows,), generator=g)
    if ignored == "all":
        y[:] = IGNORE
    elif ignored == "some":
        y[1::3] = IGNORE
    return y


def make_weights(C, seed):
    g = torch.Generator().manual_seed(seed + 2)
    return (0.25 + 1.75 * torch.rand(C, generator=g)).float()


def make_grad_out(rows, reduction, seed):
    g = torch.Generator().manual_seed(seed + 3)
    return (torch.randn(rows, generator=g) * 0.7 + 0.2).float() if reduction == NONE else torch.tensor([-1.75])


# ----------------------------------------------------------------------------------------------------------------------
# shared row model (float64 values + the error of l)
# ----------------------------------------------------------------------------------------------------------------------
def _rows(z):
    zd = z.double()
    C = z.shape[1]
    am = torch.max(z, 1).indices
    m = zd.gather(1, am[:, None])
    d = zd - m
    e1 = torch.exp(d).scatter(1, am[:, None], 0.0)
    s1 = e1.sum(1)
    l = torch.log1p(s1)
    ds1 = sum_bound(C, s1) + (e1 * (R_EXP + U * d.abs())).sum(1)
    dl = ds1 / (1.0 + s1) + R_LOG1P * l
    return d, l, dl


def ref_slack(z, wmax):
    """what the float64 reference itself may be off by, per row: (loss slack [rows], gradient slack scalar)"""
    return 16 * UD * (1.0 + z.double().abs().amax(1)) * wmax, 16 * UD * wmax


def _probs(d, l, dl, y_safe):
    """log p, p, x_k = p_k - [k == y] and their errors as the backward forms them"""
    logp = d - l[:, None]
    dlogp = dl[:, None] + U * d.abs() + U * logp.abs()
    p = torch.exp(logp)
    dp = p * (dlogp + R_EXP)
    hot = F.one_hot(y_safe, d.shape[1]).bool()
    x = torch.where(hot, torch.expm1(logp), p)
    dx = torch.where(hot, p * dlogp + R_EXPM1 * x.abs(), dp)
    return logp, dlogp, p, dp, x, dx


def _reduce(li, bi, den, reduction):
    """double accumulation of the row losses: (value, bound) of the reduced loss"""
    num = li.sum()
    dnum = bi.sum() + (li.numel() + 8) * 2 * UD * li.abs().sum()
    if reduction == MEAN:
        val = num / den
        return val, dnum / den + 2 * U * val.abs()
    return num, dnum + 2 * U * num.abs()


# ----------------------------------------------------------------------------------------------------------------------
# cross-entropy
# ----------------------------------------------------------------------------------------------------------------------
def ce_ref(z, y, w, eps, reduction, gout):
    """{loss, loss_bound, dz, dz_bound}; loss is [rows] for NONE.  z f32 [rows][C] (CPU), y int64, w f32 [C] or None,
    gout f32 [1] or [rows]."""
    rows, C = z.shape
    zd = z.double().requires_grad_(True)
    ref = F.cross_entropy(zd, y, weight=None if w is None else w.double(), ignore_index=IGNORE, reduction=RED_NAME[reduction],
                          label_smoothing=eps)
    go = gout.double() if reduction == NONE else gout.double()[0]
    (ref * go).sum().backward()
    d, l, dl = _rows(z)
    valid = y != IGNORE
    ys = torch.where(valid, y, torch.zeros_like(y))
    wd = torch.ones(C, dtype=torch.float64) if w is None else w.double()
    wy = torch.where(valid, wd[ys], torch.zeros(rows, dtype=torch.float64))
    dy = d.gather(1, ys[:, None])[:, 0]
    nll = l - dy
    dnll = dl + U * dy.abs() + U * nll.abs()
    a, b = 1.0 - eps, eps / C
    if eps == 0.0:
        li = wy * nll
        bi = wy * dnll + 2 * U * li.abs()                       # the product (and a spare rounding)
    else:
        t = wd * (l[:, None] - d)
        dt = wd * (dl[:, None] + U * d.abs()) + 2 * U * t.abs()  # the difference, the product
        S = t.sum(1)
        dS = dt.sum(1) + sum_bound(C, t.abs().sum(1))
        li = a * wy * nll + b * S
        # 1 - eps, eps / C, two products and the final add (or fma) on each term's path: at most 4 roundings
        bi = a * wy * dnll + b * dS + 4 * U * ((a * wy * nll).abs() + (b * S).abs())
    vf = valid.double()
    sl_loss, sl_grad = ref_slack(z, float(wd.max()))
    li, bi = li * vf, (bi + sl_loss) * vf
    den = wy.sum() if reduction == MEAN else torch.tensor(1.0, dtype=torch.float64)
    if reduction == NONE:
        loss, lb = li, bi
    else:
        loss, lb = _reduce(li, bi, den, reduction)
    # gradient: sc [c1 x_k + c2 (p_k W - w_k)],  sc = fl(g / fl(den))
    logp, dlogp, p, dp, x, dx = _probs(d, l, dl, ys)
    sc = ((go if reduction == NONE else go.expand(rows)) / den).abs()[:, None]
    c1 = (a * wy)[:, None]
    W = wd.sum()
    t1, t2a, t2b = c1 * x, b * p * W, (b * wd).expand(rows, C)
    nW = (C + 8) if (w is not None and eps > 0.0) else 0         # W is an f32 sum of C weights only when there are weights
    # roundings on a term's path: den -> f32, g / den, 1 - eps, (1 - eps) w_y, eps / C, p W, the products with c1 / c2,
    # the difference, the sum of the two parts, the product with sc: at most 10
    gb = sc * (c1 * dx + b * W * dp) + nW * U * sc * t2a.abs() + 10 * U * sc * (t1.abs() + t2a.abs() + t2b.abs())
    gb = (gb + sc * sl_grad) * vf[:, None]
    assert bool((torch.nan_to_num(ref.detach(), nan=0.0) - torch.nan_to_num(loss, nan=0.0)).abs().max() <=
                1e-12 * (1 + loss.abs().nan_to_num(0.0).max())), "the restated formula disagrees with F.cross_entropy"
    return {"loss": ref.detach(), "loss_bound": lb, "dz": zd.grad, "dz_bound": gb}


# ----------------------------------------------------------------------------------------------------------------------
# focal loss
# ----------------------------------------------------------------------------------------------------------------------
def focal_formula(z, y, alpha, gamma, reduction):
    """3dcnn/models.py:21-45 for a per-class alpha (any float dtype)"""
    log_pt = F.log_softmax(z, dim=-1)
    pt = torch.exp(log_pt).gather(1, y.view(-1, 1)).squeeze(1)
    log_pt = log_pt.gather(1, y.view(-1, 1)).squeeze(1)
    loss = -alpha[y] * (1 - pt).pow(gamma) * log_pt
    return loss.mean() if reduction == MEAN else loss.sum() if reduction == SUM else loss


def _focal_parts(d, l, dl, y, gamma):
    """mod = (1 - p_y)^gamma, q = (1 - p_y)^(gamma - 1) and their errors, from om = -expm1f(log p_y)"""
    dy = d.gather(1, y[:, None])[:, 0]
    logp = dy - l
    dlogp = dl + U * dy.abs() + U * logp.abs()
    p = torch.exp(logp)
    om = -torch.expm1(logp)
    dom = p * dlogp + R_EXPM1 * om
    zero = torch.zeros_like(om)
    if gamma == 0.0:
        return logp, dlogp, p, zero + 1.0, zero, zero, zero
    if gamma == 1.0:
        return logp, dlogp, p, om, dom, zero + 1.0, zero
    if gamma == 2.0:
        q, dq = om, dom
    else:   # powf(om, fl(gamma - 1)): its own accuracy, the base's error, the exponent's rounding
        q = om.pow(gamma - 1.0)
        lo = torch.where(om > 0, om.clamp_min(1e-300).log().abs(), zero)
        dq = (gamma - 1.0) * om.pow(gamma - 2.0) * dom + (R_POW + U * abs(gamma - 1.0) * lo) * q
    mod = q * om
    return logp, dlogp, p, mod, q * dom + om * dq + U * mod, q, dq


def focal_ref(z, y, alpha, gamma, reduction, gout):
    rows, C = z.shape
    zd = z.double().requires_grad_(True)
    ad = alpha.double()
    ref = focal_formula(zd, y, ad, gamma, reduction)
    go = gout.double() if reduction == NONE else gout.double()[0]
    (ref * go).sum().backward()
    d, l, dl = _rows(z)
    logp, dlogp, p, mod, dmod, q, dq = _focal_parts(d, l, dl, y, gamma)
    ay = ad[y]
    li = -ay * mod * logp
    sl_loss, sl_grad = ref_slack(z, float(ad.max()))
    bi = ay * (logp.abs() * dmod + mod * dlogp) + 3 * U * li.abs() + sl_loss   # two products and the sign-free third
    den = torch.tensor(float(rows) if reduction == MEAN else 1.0, dtype=torch.float64)
    if reduction == NONE:
        loss, lb = li, bi
    else:
        loss, lb = _reduce(li, bi, den, reduction)
    # gradient: sc coef x_k, coef = alpha_y [mod - gamma p q log p]
    dpy = p * (dlogp + R_EXP)
    second = gamma * p * q * logp.abs()
    coef = ay * (mod + second)
    dcoef = ay * (dmod + gamma * (q * logp.abs() * dpy + p * logp.abs() * dq + p * q * dlogp)) + 6 * U * coef
    _, _, _, _, x, dx = _probs(d, l, dl, y)
    sc = ((go if reduction == NONE else go.expand(rows)) / den).abs()[:, None]
    g = sc * coef[:, None] * x.abs()
    # den -> f32, g / den, three products (and one spare); the modulator's derivative makes the reference's own slack
    # (1 + gamma) times larger
    gb = sc * (dcoef[:, None] * x.abs() + coef[:, None] * dx) + 6 * U * g + sc * sl_grad * (1.0 + gamma)
    return {"loss": ref.detach(), "loss_bound": lb, "dz": zd.grad, "dz_bound": gb}


# ----------------------------------------------------------------------------------------------------------------------
# torch-f32 restatement of the kernels (CPU): what correct f32 arithmetic gives; `wrong` switches in one of three mistakes
# ----------------------------------------------------------------------------------------------------------------------
WRONG = ["mean_counts_ignored_rows", "smoothing_without_class_weights", "focal_gradient_without_modulator_derivative"]


def restated(kind, z, y, w, eps, gamma, reduction, gout, wrong=None):
    """(loss f32, dz f32) the way csrc/loss.hip computes them, every intermediate rounded to f32"""
    rows, C = z.shape
    f32 = torch.float32
    am = torch.max(z, 1).indices
    m = z.gather(1, am[:, None])
    d = z - m
    s1 = torch.exp(d).scatter(1, am[:, None], 0.0).sum(1, dtype=f32)
    l = torch.log1p(s1)
    one = torch.ones(C, dtype=f32)
    wv = one if w is None else w
    if kind == CE:
        valid = y != IGNORE
    else:
        valid = torch.ones(rows, dtype=torch.bool)
    ys = torch.where(valid, y, torch.zeros_like(y))
    wy = wv[ys]
    dy = d.gather(1, ys[:, None])[:, 0]
    logp = (d - l[:, None])
    hot = F.one_hot(ys, C).bool()
    x = torch.where(hot, torch.expm1(logp), torch.exp(logp))
    if kind == CE:
        li = wy * (l - dy)
        c1, c2 = wy, 0.0
        if eps > 0.0:
            sw = one if wrong == "smoothing_without_class_weights" else wv
            sm = (sw * (l[:, None] - d)).sum(1, dtype=f32)
            a, b = torch.tensor(1.0, dtype=f32) - eps, torch.tensor(eps, dtype=f32) / C
            li = a * li + b * sm
            c1, c2 = a * wy, b
        li = torch.where(valid, li, torch.zeros_like(li))
        den_rows = torch.ones(rows, dtype=torch.float64) if wrong == "mean_counts_ignored_rows" else valid.double()
        den = (wy.double() * den_rows).sum() if reduction == MEAN else torch.tensor(1.0, dtype=torch.float64)
        W = wv.sum(dtype=f32) if w is not None else torch.tensor(float(C))
        grad = c1[:, None] * x
        if eps > 0.0:
            grad = grad + c2 * (torch.exp(logp) * W - sw)
        grad = torch.where(valid[:, None], grad, torch.zeros_like(grad))
    else:
        ly = logp.gather(1, ys[:, None])[:, 0]
        pm1 = torch.expm1(ly)
        om = (-pm1).clamp_min(0.0)
        if gamma == 0.0:
            mod, coef = torch.ones_like(om), wy
        else:
            q = torch.ones_like(om) if gamma == 1.0 else om if gamma == 2.0 else om.pow(torch.tensor(gamma, dtype=f32) - 1.0)
            mod = q * om
            coef = wy * mod if wrong == "focal_gradient_without_modulator_derivative" else \
                wy * (mod - gamma * torch.exp(ly) * q * ly)
        li = -wy * mod * ly
        den = torch.tensor(float(rows) if reduction == MEAN else 1.0, dtype=torch.float64)
        grad = coef[:, None] * x
    loss = li if reduction == NONE else (li.double().sum() / den).float()
    g = gout if reduction == NONE else gout.expand(rows)
    scale = g / den.float()
    return loss, grad * scale[:, None]


# ----------------------------------------------------------------------------------------------------------------------
# the trainers' bookkeeping (3dcnn/train_3D_Quadtree_cnn_model.py:127-137) and the meter rule, on the host
# ----------------------------------------------------------------------------------------------------------------------
def meter_step(state, loss_value, rows, correct, reduction=MEAN):
    """state: [loss_sum, samples, correct, skipped]; loss_value: the reduced loss (NONE: the sum of the row losses)"""
    import math
    if math.isfinite(loss_value):
        state[0] += loss_value * rows if reduction == MEAN else loss_value
        state[1] += rows
        state[2] += correct
    else:
        state[3] += 1
    return state
