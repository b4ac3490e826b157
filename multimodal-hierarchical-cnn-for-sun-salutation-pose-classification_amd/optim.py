"""Adam for the plan-backed models: optimizer step and operand re-packing in one pass.

Same update rule and constructor arguments as the reference's optimizer
(`torch.optim.Adam(model.parameters(), lr=1e-4, weight_decay=1e-4)`,
/root/reference/Quadtree_from scratch/Quadtree_train.py:45; resnet/train_cnn_model.py:65): L2 weight decay
added to the gradient, bias-corrected moments, no amsgrad / maximize.  The arithmetic runs in
csrc/pack.hip: the conv / linear weights (99.6 % of the parameters) are updated inside the
one-launch kernel that re-packs them into the MFMA operand layouts, so masters, moments and packed
copies are each read / written once per step; the remaining small tensors take one multi-tensor
launch.  SURVEY.md 8(f) rank 1.

Right after a full `backward()` the bulk of the step runs on the plan's side stream, beside the fused stem backward
(the last kernel of the backward, which produces only conv1's weight gradient and leaves most of the HBM bandwidth
idle); conv1's filter is updated on the caller's stream, which has waited for the whole step when `step()` returns.
This order is taken only when nothing but the plan can have touched what Adam reads (`overlap_allowed`,
`PlanEngine.adam_overlap_ok`); otherwise, and with `QTCNN_ADAM_OVERLAP=0`, the step runs serially on the caller's
stream.  Both orders compute the same bits.

    opt = FusedAdam(model.parameters(), lr=1e-4, weight_decay=1e-4, model=model)

Without `model=` (or for parameters the plan does not know) it is a plain fused multi-tensor Adam.

Gradient clipping by the global 2-norm (the reference's trainers call `torch.nn.utils.clip_grad_norm_(model.parameters(),
1.0)` between backward() and step(): 3dcnn/train_3D_Quadtree_cnn_model.py:111-125) is part of the step:

    opt = FusedAdam(model.parameters(), lr=1e-4, weight_decay=1e-4, model=model, max_grad_norm=1.0)

One deterministic kernel pair (csrc/grad_norm.hip) reads the gradients once and leaves the norm and torch's clip
coefficient `min(1, max_norm / (norm + 1e-6))` in device memory; the Adam kernels multiply each gradient by that
coefficient as they read it.  The norm covers every parameter of every group of this optimizer that has a gradient in
this step.  Nothing is copied to the host and nothing waits for the device.  `opt.last_grad_norm` (the norm before
clipping) and `opt.last_clip_coef` are 0-dim f32 device tensors afterwards.  One difference from torch: `p.grad` is left
UNSCALED, because the scaling happens inside the update.  A clipped step runs serially on the caller's stream (the norm
needs conv1's weight gradient, the last thing the backward produces).  `grad_norm(parameters)` gives the same norm alone,
for logging.

The rule, precisely: Adam with the F32-ROUNDED hyper-parameters.  The C ABI carries lr, the betas, eps and the weight decay
as f32 and the kernel forms `1 - beta` as f32(1) - f32(beta); the bias corrections are computed in double from the same f32
beta, so the rule is self-consistent (v / (1 - b2^t) = g^2 at step 1).  torch.optim.Adam uses the Python doubles.  At the
reference's betas (0.9, 0.999) f32(1) - f32(0.999) = 0.00099998713 against torch's 0.001: after one step `exp_avg_sq` is
1.29e-5 relative below torch's (`exp_avg`: 2.4e-7), a gap that decays as the first steps' terms do, over about
1 / (1 - beta2) = 1000 steps (both rules' weights sum to 1 in the long run); the parameters differ by under 2e-5 * lr after 2,000
steps (float64 simulation of both rules).  tests/_adam_ref.py states the rule in float64 and derives per-element bounds
for the kernels; tests/test_adam_gpu.py holds them to it.  State moves both ways between FusedAdam and torch.optim.Adam
through state_dict() / load_state_dict(): `step` is a Python int here and is converted when a torch checkpoint is loaded.
"""
import ctypes
import math
import os

import torch

from . import _lib
from .engine import AdamDesc, AdamItem


# Parameter updates made through raw pointers (qt_adam_multi) do not bump torch's version counters: consumers that cache
# packed copies of parameters (video3d._ConvBlock.pack) compare this counter as well.
_raw_updates = 0


def raw_update_count():
    return _raw_updates


def overlap_allowed(engine, by_index, created_state, n_groups, n_steps):
    """The optimizer's half of the eligibility test for the overlapped step: the switch is on, one param group and one
    step value (the conditions of the fused call), and no optimizer state was created in this step() -- the first
    step's zeros_like run on the caller's stream, which the side stream does not wait for.  The engine checks the
    gradients (PlanEngine.adam_overlap_ok)."""
    if os.environ.get("QTCNN_ADAM_OVERLAP", "1") == "0":
        return False
    if created_state or n_groups != 1 or n_steps != 1:
        return False
    return engine is not None and engine.adam_overlap_ok(by_index)


def _norm_items(grads):
    """AdamItem array for the norm kernel (it reads `grad` and `numel` only)."""
    items = (AdamItem * len(grads))()
    for j, g in enumerate(grads):
        if g.is_sparse or g.dtype != torch.float32 or g.device.type != "cuda" or not g.is_contiguous() or \
                g.device != grads[0].device:
            raise _lib.QtError("the gradient norm kernel handles dense contiguous f32 gradients on one GPU")
        items[j] = AdamItem(None, g.data_ptr(), None, None, g.numel())
    return items


def _norm_workspace(L, items, n, device, cached=None):
    need = L.qt_grad_norm_workspace_bytes(items, n)
    if need == 0:
        _lib.check(-1, "qt_grad_norm_workspace_bytes")
    if cached is not None and cached.device == device and cached.numel() * 4 >= need:
        return cached
    return torch.empty(need // 4, dtype=torch.float32, device=device)


def grad_norm(parameters):
    """Global 2-norm of the gradients of `parameters` (a tensor or an iterable; those without .grad are skipped) as a 0-dim
    f32 device tensor: what torch.nn.utils.clip_grad_norm_ returns, from the kernel FusedAdam(max_grad_norm=...) uses,
    without scaling anything and without a host sync."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        raise _lib.QtError("grad_norm: no parameter has a gradient")
    grads = [g.contiguous() for g in grads]
    L = _lib.lib()
    items = _norm_items(grads)
    dev = grads[0].device
    with torch.cuda.device(dev):
        ws = _norm_workspace(L, items, len(grads), dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        _lib.check(L.qt_grad_norm_multi(items, len(grads), 1.0, ws.data_ptr(), ws.numel() * 4, out.data_ptr(),
                                        _lib.stream_ptr()), "qt_grad_norm_multi")
    return out[0]


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, model=None, max_grad_norm=None):
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1):
            raise ValueError("FusedAdam: invalid hyper-parameters")
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not max_grad_norm > 0 or math.isnan(max_grad_norm):
                raise ValueError("FusedAdam: max_grad_norm must be a positive number or None")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm))
        self._model = model
        self.last_grad_norm = None    # after a clipped step(): 0-dim f32 device tensors
        self.last_clip_coef = None
        self._norm_ws = None

    def _max_grad_norm(self):
        """One value for the whole optimizer (per-group clipping is not offered); read from the param groups, which is
        where load_state_dict() puts it."""
        values = {g.get("max_grad_norm") for g in self.param_groups}
        if len(values) > 1:
            raise ValueError("FusedAdam: every param group must carry the same max_grad_norm")
        return values.pop() if values else None

    def load_state_dict(self, state_dict):
        """Also takes a torch.optim.Adam checkpoint.  torch saves each parameter's `step` as a tensor; here it is a Python
        int (it goes into the kernels' descriptor, and step() must not read the device), so it is converted once, now.
        amsgrad / maximize checkpoints are refused: the kernels do not implement them."""
        for group in state_dict["param_groups"]:
            if group.get("amsgrad") or group.get("maximize"):
                raise ValueError("FusedAdam: cannot resume an amsgrad / maximize checkpoint")
        super().load_state_dict(state_dict)
        for st in self.state.values():
            if "step" in st and type(st["step"]) is not int:
                step = st["step"]
                value = float(step.item() if isinstance(step, torch.Tensor) else step)
                if value != int(value) or value < 0:
                    raise ValueError(f"FusedAdam: step {value!r} in the loaded state is not a step count")
                st["step"] = int(value)

    def _begin_clip(self, L, max_norm):
        """Everything the clipped step needs before its first update: the gradients of all groups (the norm is global),
        the norm kernel's workspace and the two output floats.  No device work yet."""
        grads = [(id(p), p.grad.contiguous()) for group in self.param_groups for p in group["params"] if p.grad is not None]
        self.last_grad_norm = self.last_clip_coef = None
        if not grads:
            return None
        items = _norm_items([g for _, g in grads])
        dev = grads[0][1].device
        with torch.cuda.device(dev):
            self._norm_ws = _norm_workspace(L, items, len(grads), dev, self._norm_ws)
            out = torch.empty(2, dtype=torch.float32, device=dev)   # fresh per step: earlier steps' values stay readable
        self.last_grad_norm, self.last_clip_coef = out[0], out[1]
        return {"grads": grads, "items": items, "ws": self._norm_ws, "out": out, "done": False}

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        engine = getattr(self._model, "_engine", None) if self._model is not None else None
        plan_index = {}
        if engine is not None and self._model._param_list is not None:
            plan_index = {id(p): i for p, i in zip(self._model._param_list, self._model._param_plan_index) if i >= 0}
        L = _lib.lib()
        max_norm = self._max_grad_norm()
        clip = self._begin_clip(L, max_norm) if max_norm is not None else None
        fused_groups = 0
        for group in self.param_groups:
            todo = []
            created_state = False
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse or p.dtype != torch.float32 or p.device.type != "cuda" or not p.is_contiguous():
                    raise _lib.QtError("FusedAdam handles dense contiguous f32 parameters on the GPU")
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    created_state = True
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if type(st["step"]) is not int:   # (load_state_dict() converts torch's tensor; nothing here reads the device)
                    raise _lib.QtError("FusedAdam: state['step'] must be a Python int; load optimizer state with "
                                       "load_state_dict()")
                st["step"] += 1
                todo.append((p, st))
            if not todo:
                continue
            steps = {st["step"] for _, st in todo}
            for step in sorted(steps):   # parameters that joined later have their own bias correction
                part = [(p, st) for p, st in todo if st["step"] == step]
                desc = AdamDesc(group["lr"], group["betas"][0], group["betas"][1], group["eps"], group["weight_decay"],
                                1.0, step)
                in_plan = {plan_index[id(p)]: (p.grad.contiguous(), st["exp_avg"], st["exp_avg_sq"])
                           for p, st in part if id(p) in plan_index}
                rest = [(p, st) for p, st in part if id(p) not in plan_index]
                # one fused call per step() at most: the plan re-packs every operand copy inside it
                if in_plan and engine is not None and fused_groups == 0 and len(steps) == 1 and \
                        len(self.param_groups) == 1:
                    with torch.cuda.device(engine.device):
                        if clip is None:
                            engine.adam_step(in_plan, desc, overlap=overlap_allowed(
                                engine, in_plan, created_state, len(self.param_groups), len(steps)))
                        else:   # one norm over the plan's gradients and the rest, one coefficient for both calls
                            extra = [g for pid, g in clip["grads"] if pid not in plan_index]
                            engine.adam_step(in_plan, desc, clip=(max_norm, _norm_items(extra) if extra else None,
                                                                  len(extra), clip["ws"], clip["out"]))
                            clip["done"] = True
                    fused_groups += 1
                else:
                    rest = part
                    if engine is not None:
                        engine.invalidate_weights()
                if rest:
                    items = (AdamItem * len(rest))()
                    keep = []
                    for j, (p, st) in enumerate(rest):
                        g = p.grad.contiguous()
                        keep.append(g)
                        items[j] = AdamItem(p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(),
                                            st["exp_avg_sq"].data_ptr(), p.numel())
                    with torch.cuda.device(rest[0][0].device):
                        if clip is None:
                            _lib.check(L.qt_adam_multi(items, len(rest), ctypes.byref(desc), _lib.stream_ptr()),
                                       "qt_adam_multi")
                        else:
                            if not clip["done"]:
                                _lib.check(L.qt_grad_norm_multi(clip["items"], len(clip["grads"]), max_norm,
                                                                clip["ws"].data_ptr(), clip["ws"].numel() * 4,
                                                                clip["out"].data_ptr(), _lib.stream_ptr()),
                                           "qt_grad_norm_multi")
                                clip["done"] = True
                            _lib.check(L.qt_adam_multi_scaled(items, len(rest), ctypes.byref(desc),
                                                              clip["out"].data_ptr() + 4, _lib.stream_ptr()),
                                       "qt_adam_multi_scaled")
                    global _raw_updates
                    _raw_updates += 1
        return loss
