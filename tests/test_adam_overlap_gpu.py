"""The optimizer step beside the stem backward (QTCNN_ADAM_OVERLAP, qt_plan_adam_step_overlapped) and the light fused
Adam + re-pack kernel behind it.

Both orders of the step must compute the same bits: parameters, both Adam moments, and the eval logits (which read the
packed operand copies).  The overlapped order is only taken when nothing but the plan can have touched what Adam reads;
every fall-back case is checked for the predicate and for its results.
"""
import ctypes

import pytest
import torch

from _util import pkg

gpu = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _make(kind, B):
    P = pkg()
    if kind == "attention":
        m = P.AttentionHierarchicalCNN(12, dropout_rate=0.0, compute_dtype=torch.bfloat16, max_batch=B)
    else:
        m = P.QuadtreeCNN(12, dropout_rate=0.0, compute_dtype=torch.bfloat16, max_batch=B,
                          freeze_backbone=(kind == "frozen"))
    m.load_state_dict(pkg("synth").synth_state_dict(m))
    return m.to(_dev()).train()


def _batch(B):
    synth = pkg("synth")
    # one image set of 8, tiled: the step only has to be long enough, not varied
    n = min(B, 8)
    rep = B // n
    x = synth.synth_images(n, salt=5).repeat(rep, 1, 1, 1).to(_dev())
    f = synth.synth_pose_features(n, salt=5).repeat(rep, 1).to(_dev())
    y = synth.synth_labels(n, 12, salt=5).repeat(rep).to(_dev())
    return x, f, y


def _backward(model, opt, data):
    x, f, y = data
    opt.zero_grad(set_to_none=True)
    torch.nn.functional.cross_entropy(model(x, f), y).backward()


def _state(model, opt, data):
    """Everything the step wrote, on the host: parameters, moments, eval logits (from the packed copies)."""
    out = {}
    for n, p in model.named_parameters():
        out["p/" + n] = p.detach().cpu()
        st = opt.state.get(p)
        if st:
            out["m/" + n] = st["exp_avg"].cpu()
            out["v/" + n] = st["exp_avg_sq"].cpu()
    model.eval()
    with torch.no_grad():
        out["eval_logits"] = model(data[0], data[1]).float().cpu()
    model.train()
    return out


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


class _Reducer:
    """Stands where dp.GradBucketReducer stands on one rank (the rehearsal): every bucket is ordered behind both producer
    streams and touched by a kernel on a communication stream, which the compute stream joins at the end."""

    def __init__(self):
        self.stream = None

    def __call__(self, bucket, phase, side_fence=None):
        if bucket is None:
            if self.stream is not None:
                torch.cuda.current_stream().wait_stream(self.stream)
            return
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=bucket.device)
        self.stream.wait_stream(torch.cuda.current_stream())
        side_fence(self.stream)
        bucket.record_stream(self.stream)
        with torch.cuda.stream(self.stream):
            bucket.mul_(1.0)


def _train(kind, B, overlap, monkeypatch, steps=3, between=None, dp=False):
    """`steps` train steps; returns (state, [engine.last_adam_overlapped per step]).  between(model, step): called
    between backward and optimizer step."""
    monkeypatch.setenv("QTCNN_ADAM_OVERLAP", "1" if overlap else "0")
    torch.manual_seed(0)
    P = pkg()
    model = _make(kind, B)
    if dp:
        model._grad_sync = _Reducer()   # picked up by the engine: the four-phase backward with its fences
    opt = P.FusedAdam(model.parameters(), lr=1e-3, weight_decay=1e-4, model=model)
    data = _batch(B)
    took = []
    for s in range(steps):
        _backward(model, opt, data)
        if between is not None:
            between(model, s)
        opt.step()
        took.append(model._engine.last_adam_overlapped)
    torch.cuda.synchronize()
    return _state(model, opt, data), took


@gpu
@pytest.mark.parametrize("kind,B", [("quadtree", 4), ("quadtree", 256), ("attention", 4), ("attention", 256),
                                    ("frozen", 4), ("frozen", 256)])
def test_overlapped_step_equals_serial_step(kind, B, monkeypatch):
    """Three train steps with the switch on and off: identical parameters, moments and eval logits.  B = 256 is the size
    at which the stem backward is long enough for a mis-ordered gradient read to show."""
    on, took_on = _train(kind, B, True, monkeypatch)
    off, took_off = _train(kind, B, False, monkeypatch)
    _assert_same(on, off, f"{kind} B={B}")
    assert took_off == [False, False, False]
    # the first step creates the optimizer state (serial); a frozen backbone has no stem backward to run beside
    assert took_on == ([False, False, False] if kind == "frozen" else [False, True, True])


def _mul_grad(model, s):
    if s == 2:
        model.classifier[0].weight.grad.mul_(0.5)


def _clone_grad(model, s):
    if s == 2:
        p = model.classifier[0].weight
        p.grad = p.grad.clone()


@gpu
@pytest.mark.parametrize("case", ["mul_", "clone", "dp"])
def test_fallbacks_equal_the_serial_path(case, monkeypatch):
    """A gradient changed in place, a replaced .grad and a data-parallel rehearsal all take the serial order and give
    what QTCNN_ADAM_OVERLAP=0 gives.  (The first step, state creation, is part of every run here.)"""
    between = {"mul_": _mul_grad, "clone": _clone_grad, "dp": None}[case]
    on, took = _train("quadtree", 4, True, monkeypatch, between=between, dp=(case == "dp"))
    off, _ = _train("quadtree", 4, False, monkeypatch, between=between, dp=(case == "dp"))
    _assert_same(on, off, case)
    assert took == ([False, False, False] if case == "dp" else [False, True, False])


@gpu
def test_second_step_without_backward_is_serial(monkeypatch):
    def run(overlap):
        monkeypatch.setenv("QTCNN_ADAM_OVERLAP", "1" if overlap else "0")
        P = pkg()
        model = _make("quadtree", 4)
        opt = P.FusedAdam(model.parameters(), lr=1e-3, weight_decay=1e-4, model=model)
        data = _batch(4)
        took = []
        for _ in range(2):
            _backward(model, opt, data)
            opt.step()
            took.append(model._engine.last_adam_overlapped)
            opt.step()    # same gradients again, no backward in between
            took.append(model._engine.last_adam_overlapped)
        torch.cuda.synchronize()
        return _state(model, opt, data), took
    on, took = run(True)
    off, _ = run(False)
    _assert_same(on, off, "step twice")
    assert took == [False, False, True, False]


@gpu
def test_eligibility_predicate(monkeypatch):
    """PlanEngine.adam_overlap_ok / optim.overlap_allowed say no in every fall-back case, and yes right after a plain
    full backward."""
    monkeypatch.setenv("QTCNN_ADAM_OVERLAP", "1")
    P, optim = pkg(), pkg("optim")
    model = _make("quadtree", 4)
    opt = P.FusedAdam(model.parameters(), lr=1e-3, model=model)
    data = _batch(4)
    _backward(model, opt, data)          # the first forward builds the engine
    eng = model._engine
    index = {id(p): i for p, i in zip(model._param_list, model._param_plan_index) if i >= 0}

    def by_index():
        return {index[id(p)]: (p.grad, None, None) for p in model.parameters() if id(p) in index and p.grad is not None}

    _backward(model, opt, data)
    assert eng.adam_overlap_ok(by_index())
    assert optim.overlap_allowed(eng, by_index(), False, 1, 1)
    assert not optim.overlap_allowed(eng, by_index(), True, 1, 1)     # state created in this step
    assert not optim.overlap_allowed(eng, by_index(), False, 2, 1)    # two param groups
    assert not optim.overlap_allowed(eng, by_index(), False, 1, 2)    # two step values
    monkeypatch.setenv("QTCNN_ADAM_OVERLAP", "0")
    assert not optim.overlap_allowed(eng, by_index(), False, 1, 1)
    monkeypatch.setenv("QTCNN_ADAM_OVERLAP", "1")

    model.classifier[3].bias.grad.mul_(0.5)                            # in-place op on a gradient
    assert not eng.adam_overlap_ok(by_index())

    _backward(model, opt, data)
    assert eng.adam_overlap_ok(by_index())
    model.classifier[3].bias.grad = model.classifier[3].bias.grad.clone()   # replaced .grad
    assert not eng.adam_overlap_ok(by_index())

    _backward(model, opt, data)
    opt.step()                                                         # consumed: a second step is serial
    assert not eng.adam_overlap_ok(by_index())

    _backward(model, opt, data)
    eng.grad_sync = lambda *a: None                                    # a data-parallel reducer is attached
    assert not eng.adam_overlap_ok(by_index())
    eng.grad_sync = None
    assert eng.adam_overlap_ok(by_index())
    torch.cuda.synchronize()


_PackItem = pkg("_abi").PackItem   # qt_pack_item


@gpu
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_fused_adam_pack_equals_plain_adam_then_pack(dt):
    """qt_adam_pack_weights_batched (float4 streams, tile staged in the compute dtype) against qt_adam_multi followed
    by qt_pack_weights_batched on the same inputs: masters, moments and both operand copies bit for bit, for a 3x3, a
    1x1 and every stride-2 data-gradient layout (1..4).  Two steps, so that non-zero moments go in as well."""
    L = pkg("_lib")
    lib = L.lib()
    eng = pkg("engine")
    dev = _dev()
    g = torch.Generator().manual_seed(7)
    shapes = [(64, 64, 3, 0), (128, 192, 1, 0), (128, 64, 3, 1), (128, 64, 1, 1), (128, 64, 3, 2), (256, 128, 3, 3),
              (256, 128, 1, 4)]
    qdt, st = L.qt_dtype(dt), L.stream_ptr()

    def side(fused):
        n = len(shapes)
        items, state, keep = (_PackItem * n)(), (eng.AdamItem * n)(), []
        gg = torch.Generator().manual_seed(11)
        for j, (O, I, k, s2) in enumerate(shapes):
            w = (torch.randn(O, I, k, k, generator=gg) * 0.05).to(dev)
            gr = (torch.randn(O, I, k, k, generator=gg) * 0.01).to(dev)
            m, v = torch.zeros_like(w), torch.zeros_like(w)
            fwd = torch.zeros(O * k * k * I, dtype=dt, device=dev)
            slots = {2: 16, 3: 20, 4: 20}.get(s2, k * k)
            dg = torch.zeros(slots * O * I, dtype=dt, device=dev)
            items[j] = _PackItem(w.data_ptr(), fwd.data_ptr(), dg.data_ptr(), O, I, k, s2)
            state[j] = eng.AdamItem(w.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), w.numel())
            keep.append((w, gr, m, v, fwd, dg))
        for step in (1, 2):
            desc = eng.AdamDesc(1e-3, 0.9, 0.999, 1e-8, 1e-4, 1.0, step)
            if fused:
                L.check(lib.qt_adam_pack_weights_batched(qdt, items, state, ctypes.byref(desc), n, st), "adam_pack")
            else:
                L.check(lib.qt_adam_multi(state, n, ctypes.byref(desc), st), "qt_adam_multi")
                L.check(lib.qt_pack_weights_batched(qdt, items, n, st), "qt_pack_weights_batched")
        torch.cuda.synchronize()
        return keep
    del g
    a, b = side(True), side(False)
    for ta, tb, shp in zip(a, b, shapes):
        for name, x, y in zip(("w", "grad", "m", "v", "fwd", "dgrad"), ta, tb):
            assert torch.equal(x, y), (shp, name)
        assert float(ta[4].float().abs().sum()) > 0 and float(ta[5].float().abs().sum()) > 0
