"""The evaluation report on the GPU (csrc/metrics.hip, <pkg>/metrics.py): the C ABI against the numpy references and the
derived bound of tests/_metrics_ref.py, with every buffer between guard bands (tests/_guard.py); the recorded outputs of the
reference's own evaluate_model; EvalMeter / predict; repeatability and the absence of host reads."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _metrics_ref as R
from _guard import Guard
from _util import ROOT, pkg

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class Op:
    """qt_metrics_update / qt_metrics_finalize through ctypes on guarded buffers: logits with ld = C + 3 and NaN padding,
    probs with ld_probs = C + 5 and poisoned padding, state / report / confidence / pred between bands."""

    def __init__(self, dev):
        self.M = pkg("metrics")
        self.lib = pkg("_lib")
        self.L = self.lib.lib()
        self.dev = dev

    # vectors are guarded as [n][1]: a band is 256 payload rows, and the whole vector is not one row
    @staticmethod
    def vec_out(g, name, n, dt, **kw):
        return g.output(name, (n, 1), dt, **kw).view(-1)

    @staticmethod
    def vec_in(g, name, a):
        return g.input(name, torch.from_numpy(np.ascontiguousarray(a, np.int64)).view(-1, 1)).view(-1)

    def new_state(self, g, C):
        return self.vec_out(g, "state", C * C + 4, torch.int64, fill=0)     # the caller zeroes the state once

    def logits(self, g, z):
        rows, C = z.shape
        zs = torch.full((rows, C + 3), NAN)
        zs[:, :C] = torch.from_numpy(z)
        return g.input("logits", zs[:, :C])

    def update(self, C, z=None, y=None, pred_in=None, state=None, g=None, outputs=True, ignore=R.IGNORE, nan_rows=False):
        """one call; returns numpy copies of what it wrote, and the guarded logits on the device"""
        g = g or Guard(self.dev)
        rows = len(z) if z is not None else len(pred_in)
        zt = self.logits(g, z) if z is not None else None
        yt = self.vec_in(g, "labels", y) if y is not None else None
        pt = self.vec_in(g, "pred_in", pred_in) if pred_in is not None else None
        if y is not None and state is None:
            state = self.new_state(g, C)
        probs = conf = pred = None
        ldp = C + 5
        if outputs and z is not None:
            probs = g.output("probs", (rows, ldp), torch.float32, written=False)
            conf = self.vec_out(g, "confidence", rows, torch.float32, written=not nan_rows)
            pred = self.vec_out(g, "pred", rows, torch.int64)
        desc = self.M.MetricsDesc(0, ignore)
        ptr = self.lib.ptr
        self.lib.check(self.L.qt_metrics_update(ctypes.byref(desc), ptr(zt), zt.stride(0) if zt is not None else 0, ptr(pt),
                                                ptr(yt), rows, C, ptr(state), ptr(probs), ldp, ptr(conf), ptr(pred),
                                                self.lib.stream_ptr()), "qt_metrics_update")
        g.check()
        out = {"logits_t": zt}
        if state is not None:
            out["state"] = state.cpu().numpy()
        if probs is not None:
            raw = probs.reshape(-1).view(torch.uint8).view(rows, ldp * 4)
            assert bool((raw[:, C * 4:] == 0xFF).all()), "padding columns of probs were written"
            out["probs"] = probs[:, :C].cpu().numpy()
            out["conf"] = conf.cpu().numpy()
            out["pred"] = pred.cpu().numpy()
            assert bool((out["pred"] >= 0).all()) and bool((out["pred"] < C).all()), "pred was not written everywhere"
        return out

    def finalize(self, C, state_np):
        g = Guard(self.dev)
        st = self.vec_in(g, "state", state_np)
        rep = self.vec_out(g, "report", 4 * C + 12, torch.float64, written=False)
        self.lib.check(self.L.qt_metrics_finalize(self.lib.ptr(st), C, self.lib.ptr(rep), self.lib.stream_ptr()),
                       "qt_metrics_finalize")
        g.check()
        raw = rep.view(torch.int64).cpu().numpy()
        assert not (raw == -1).any(), "an element of the report was not written"     # (the poison; NaN results are 0x7ff8..)
        return rep.cpu().numpy()

    def loss_pred(self, zt, y):
        """qt_loss_forward's `pred` on the same device buffer"""
        LM = pkg("loss")
        L = self.lib.lib()
        rows, C = zt.shape
        dev = self.dev
        yd = torch.from_numpy(np.asarray(y, np.int64)).to(dev)
        desc = LM.LossDesc(0, 0, 2, R.IGNORE, 0.0, 0.0, None)
        loss = torch.empty(rows, device=dev)
        stats = torch.empty(3, dtype=torch.float64, device=dev)
        pred = torch.full((rows,), -7, dtype=torch.int64, device=dev)
        need = L.qt_loss_workspace_bytes(rows, C)
        ws = torch.empty(max(need // 8, 1), dtype=torch.float64, device=dev)
        self.lib.check(L.qt_loss_forward(ctypes.byref(desc), zt.data_ptr(), zt.stride(0), yd.data_ptr(), rows, C, loss.data_ptr(),
                                         None, stats.data_ptr(), pred.data_ptr(), None, ws.data_ptr() if need else None, need,
                                         self.lib.stream_ptr()), "qt_loss_forward")
        torch.cuda.synchronize()
        return pred.cpu().numpy()


# ----------------------------------------------------------------------------------------------------------------------
# counting
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", R.SHAPES)
def test_exact_counts_and_predictions(rows, C):
    op = Op(_dev())
    z = R.make_logits(rows, C, seed=3 * rows + C)
    y = R.make_labels(rows, C, seed=rows + C)
    out = op.update(C, z=z, y=y)
    want_pred = R.argmax_ref(z)
    assert np.array_equal(out["pred"], want_pred)
    assert np.array_equal(out["state"], R.count(y, want_pred, C))
    assert int(out["state"][:C * C].sum()) == rows


@pytest.mark.parametrize("C", [12, 17, 65])
def test_same_prediction_as_the_loss_head(C):
    op = Op(_dev())
    z = R.make_logits(70, C, seed=C)              # multiples of 0.5: many tie rows
    z[1, 2] = z[1, C - 1] = 9.0                    # (for C > 16 the two sit in different lanes)
    z[2, 7] = z[2, 4] = z[2, 11] = 8.0
    z[3, 5], z[3, 1] = np.nan, 50.0                # a NaN wins its row
    z[4, 6], z[4, 2] = np.nan, np.nan              # the first NaN
    z[5, 8] = np.inf
    z[6, 3] = z[6, 9] = np.inf
    z[7, :] = -np.inf
    z[8, 0], z[8, C - 1] = -np.inf, np.inf
    y = R.make_labels(70, C, seed=C)
    out = op.update(C, z=z, y=y, nan_rows=True)
    want = R.argmax_ref(z)
    assert want[1:9].tolist() == [2, 4, 5, 2, 8, 3, 0, C - 1]
    srt = np.sort(z[9:], 1)
    assert int((srt[:, -1] == srt[:, -2]).sum()) >= 5
    assert np.array_equal(out["pred"], want)
    assert np.array_equal(out["pred"], op.loss_pred(out["logits_t"], y))
    assert np.array_equal(out["state"], R.count(y, want, C))


@pytest.mark.parametrize("C", [12, 65])
def test_three_updates_equal_one_update_of_the_concatenation(C):
    op = Op(_dev())
    parts = [(R.make_logits(n, C, seed=n), R.make_labels(n, C, seed=n)) for n in (5, 64, 300)]
    g = Guard(op.dev)
    state = op.new_state(g, C)
    for z, y in parts:
        out = op.update(C, z=z, y=y, state=state, g=g, outputs=False)
    zc, yc = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    one = op.update(C, z=zc, y=yc, outputs=False)["state"]
    assert out["state"][C * C + 3] == 3 and one[C * C + 3] == 1
    assert np.array_equal(out["state"][:C * C + 3], one[:C * C + 3])
    assert np.array_equal(one, R.count(yc, R.argmax_ref(zc), C))


@pytest.mark.parametrize("C,ignore", [(12, -100), (17, 3), (65, -100)])
def test_ignored_and_invalid_labels(C, ignore):
    op = Op(_dev())
    rows = 301
    z = R.make_logits(rows, C, seed=40 + C)
    y = R.make_labels(rows, C, seed=40 + C)
    y[1::7] = ignore
    y[2], y[9], y[130], y[300] = -5, C, 2 ** 40, -1
    out = op.update(C, z=z, y=y, ignore=ignore)
    want = R.count(y, R.argmax_ref(z), C, ignore_index=ignore)
    n_ign = int((y == ignore).sum())
    assert want[C * C:].tolist() == [rows - n_ign - 4, n_ign, 4, 1]
    assert np.array_equal(out["state"], want)
    assert int(out["state"][:C * C].sum()) == int(out["state"][C * C])       # the matrix sum equals `samples`
    assert np.array_equal(out["pred"], R.argmax_ref(z))                          # predictions do not depend on the label


@pytest.mark.parametrize("C", [12, 65])
def test_contention_all_rows_in_one_cell(C):
    op = Op(_dev())
    rows = 4099
    z = np.zeros((rows, C), np.float32)
    z[:, 7] = 2.0
    y = np.full(rows, 3, np.int64)
    st = op.update(C, z=z, y=y, outputs=False)["state"]
    assert int(st[3 * C + 7]) == rows and int(st[:C * C].sum()) == rows and st[C * C:].tolist() == [rows, 0, 0, 1]


@pytest.mark.parametrize("rows,C", [(300, 12), (70, 17), (130, 65), (33, 1024)])
def test_prediction_input_gives_the_same_state(rows, C):
    op = Op(_dev())
    z = R.make_logits(rows, C, seed=rows)
    y = R.make_labels(rows, C, seed=rows)
    y[0] = R.IGNORE
    a = op.update(C, z=z, y=y)
    b = op.update(C, pred_in=a["pred"], y=y)
    assert np.array_equal(a["state"], b["state"])
    p = a["pred"].copy()
    p[1], p[2], p[rows - 1] = C, -1, 2 ** 40          # out of range: invalid, nothing is indexed with them
    p[0] = C + 7                                       # (an ignored row stays ignored)
    c = op.update(C, pred_in=p, y=y)["state"]
    want = R.count(y, p, C)
    assert want[C * C:].tolist() == [rows - 4, 1, 3, 1]
    assert np.array_equal(c, want)


# ----------------------------------------------------------------------------------------------------------------------
# probabilities
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", [(1, 1), (63, 12), (257, 16), (300, 17), (129, 64), (130, 65), (33, 1024)])
@pytest.mark.parametrize("scale", [1.0, 20.0, 90.0])
def test_probabilities_within_the_derived_bound(rows, C, scale):
    op = Op(_dev())
    z = R.make_logits(rows, C, seed=rows + C, scale=scale / 3.0, step=0.25)
    out = op.update(C, z=z, outputs=True)            # no labels, no state: the video loop's call
    assert "state" not in out
    p, bound = R.softmax_ref(z)
    r = R.ratio(out["probs"], p, bound)
    print(f"probs {rows}x{C} scale {scale}: error / bound {r:.3f}")
    assert r <= 1.0, r
    assert np.array_equal(out["pred"], R.argmax_ref(z))
    picked = out["probs"][np.arange(rows), out["pred"]]
    assert np.array_equal(out["conf"].view(np.uint32), picked.view(np.uint32))      # bit for bit


@pytest.mark.parametrize("C", [12, 17, 65])
def test_non_finite_rows_have_torchs_nan_pattern(C):
    op = Op(_dev())
    z = R.make_logits(9, C, seed=C + 1)
    z[1, 3] = np.nan
    z[2, 7] = np.inf
    z[3, 2] = -np.inf                  # a finite row: p = 0 there
    z[4, :] = -np.inf
    z[5, 0], z[5, C - 1] = np.inf, np.inf
    z[6, C - 1] = np.nan
    out = op.update(C, z=z, nan_rows=True)
    want = R.nan_pattern(z)
    assert want.all(1).tolist() == [False, True, True, False, True, True, True, False, False]
    assert np.array_equal(np.isnan(out["probs"]), want)
    assert np.array_equal(np.isnan(out["conf"]), want.all(1))
    assert out["probs"][3, 2] == 0.0
    fin = ~want.all(1)
    p, bound = R.softmax_ref(np.where(np.isfinite(z[fin]), z[fin], -1e4))
    assert R.ratio(out["probs"][fin], p, bound) <= 1.0
    assert np.array_equal(out["pred"], R.argmax_ref(z))


# ----------------------------------------------------------------------------------------------------------------------
# finalize
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,n", [(1, 9), (2, 65), (12, 4099), (17, 300), (64, 5000), (65, 5000), (257, 20000), (1024, 50000)])
def test_finalize_matches_the_float64_reference(C, n):
    """1e-12 * max(1, |value|): double arithmetic and at most C + a few operations per value -> (C + 8) 2^-53 = 1.2e-13 at
    C = 1024 for the kernel, as much again for the numpy reference"""
    op = Op(_dev())
    rng = np.random.default_rng(C)
    y = rng.integers(0, C, size=n)
    p = np.where(rng.random(n) < 0.6, y, rng.integers(0, C, size=n))
    if C > 4:
        y[y == 3], p[p == 3] = 2, 2                      # an absent class
    st = R.count(y, p, C)
    st[C * C + 1], st[C * C + 2] = 11, 5
    got = op.finalize(C, st)
    want = R.report(st, C)
    assert R.close(got, want), np.abs(got - want).max()
    assert got[4 * C + 8:].tolist() == want[4 * C + 8:].tolist()
    assert np.array_equal(got[3 * C:4 * C], want[3 * C:4 * C])


def test_finalize_edge_states():
    op = Op(_dev())
    C = 5
    empty = op.finalize(C, np.zeros(C * C + 4, np.int64))
    assert not empty[:4 * C].any() and np.isnan(empty[4 * C:4 * C + 8]).all() and empty[4 * C + 8:].tolist() == [0, 0, 0, 0]
    for y, p in (([2], [2]), ([2], [4]), ([1, 1, 1], [1, 1, 1]), ([1, 1, 1], [1, 2, 1]), ([0, 4], [4, 0])):
        st = R.count(y, p, C)
        got, want = op.finalize(C, st), R.report(st, C)
        assert R.close(got, want), (y, p, got, want)
    s = R.scalars(op.finalize(C, R.count([1, 1, 1], [1, 1, 1], C)), C)
    assert s["r2"] == 1.0 and s["classes_present"] == 1 and s["macro_f1"] == 1.0
    assert np.isnan(R.scalars(op.finalize(C, R.count([2], [2], C)), C)["r2"])
    one = op.finalize(1, R.count([0, 0], [0, 0], 1))
    assert one.tolist()[:4] == [1.0, 1.0, 1.0, 2.0] and one[4 + 7] == 1.0


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "eval_metrics.npz"))


@pytest.mark.parametrize("i", range(5))
def test_fixture_cases_reproduce_the_reference_script(golden, i):
    dev = _dev()
    P = pkg()
    C = int(golden["num_classes"][i])
    z, y = torch.from_numpy(golden[f"logits{i}"]).to(dev), torch.from_numpy(golden[f"labels{i}"]).to(dev)
    meter = P.EvalMeter(C, dev, class_names=[f"pose{c}" for c in range(C)])
    step = 1024 if len(y) > 1000 else 16
    for a in range(0, len(y), step):
        assert meter.update(z[a:a + step], y[a:a + step]) is None
    assert np.array_equal(meter.confusion_matrix(), golden[f"cm{i}"])
    res = meter.result()
    got = [res[k] for k in ("accuracy", "precision", "recall", "f1", "r2")]
    assert R.close(got, golden[f"scalars{i}"]), (got, golden[f"scalars{i}"].tolist())
    cm = res["confusion_matrix"]
    assert cm.shape == (C, C) and cm.dtype == np.int64 and np.array_equal(R.present_submatrix(cm), golden[f"cm{i}"])
    assert np.array_equal(meter.confusion_matrix(present_only=False), cm)
    assert res["samples"] == len(y) and res["ignored"] == 0 and res["invalid"] == 0
    assert res["classes_present"] == golden[f"cm{i}"].shape[0] and res["updates"] == -(-len(y) // step)
    want = R.report(R.count(golden[f"labels{i}"], R.argmax_ref(golden[f"logits{i}"]), C), C)
    s = R.scalars(want, C)
    assert R.close([res["macro"][k] for k in ("precision", "recall", "f1")], [s["macro_precision"], s["macro_recall"], s["macro_f1"]])
    for j, k in enumerate(("precision", "recall", "f1")):
        assert R.close(res["per_class"][k], want[j * C:(j + 1) * C])
    assert np.array_equal(res["per_class"]["support"], cm.sum(1)) and res["per_class"]["names"][0] == "pose0"


# ----------------------------------------------------------------------------------------------------------------------
# module level
# ----------------------------------------------------------------------------------------------------------------------
def test_meter_with_the_fused_loss_and_merge():
    dev = _dev()
    P = pkg()
    C = 12
    crit = P.CrossEntropyLoss()
    lm, em, em2 = P.LossMeter(dev), P.EvalMeter(C, dev), P.EvalMeter(C, dev)
    ys, ps = [], []
    for step, rows in enumerate((256, 300, 7)):
        z = torch.from_numpy(R.make_logits(rows, C, seed=70 + step)).to(dev)
        y = torch.from_numpy(R.make_labels(rows, C, seed=70 + step)).to(dev)
        pred = torch.empty(rows, dtype=torch.int64, device=dev)
        crit(z, y, meter=lm, predictions=pred)
        em.update(predictions=pred, labels=y)
        probs, conf, p2 = em2.update(z, y, probs=True)
        assert torch.equal(p2, pred) and probs.shape == (rows, C) and conf.shape == (rows,)
        assert torch.equal(conf, probs.gather(1, p2[:, None])[:, 0])
        ys.append(y.cpu().numpy())
        ps.append(pred.cpu().numpy())
    a, b = em.result(), em2.result()
    assert a["accuracy"] == lm.result()["accuracy"] and a["samples"] == lm.result()["samples"] == 563
    assert np.array_equal(a["confusion_matrix"], b["confusion_matrix"]) and a["f1"] == b["f1"]
    want = R.count(np.concatenate(ys), np.concatenate(ps), C, calls=3)
    assert np.array_equal(em.state.cpu().numpy(), want)
    em.merge(em2)
    assert np.array_equal(em.state.cpu().numpy(), 2 * want)
    assert em.result()["accuracy"] == a["accuracy"] and em.result()["samples"] == 2 * 563
    em.reset()
    assert em.result()["samples"] == 0 and np.isnan(em.result()["accuracy"]) and not em.result()["confusion_matrix"].any()
    # a column view of a wider matrix, and predict()
    wide = torch.randn(9, 40, device=dev)
    probs, conf, pred = P.predict(wide[:, 5:17])
    ref, bound = R.softmax_ref(wide[:, 5:17].cpu().numpy())
    assert R.ratio(probs.cpu().numpy(), ref, bound) <= 1.0
    assert torch.equal(pred.cpu(), torch.max(wide[:, 5:17].cpu(), 1).indices)
    # refusals: no torch fallback
    y9 = torch.zeros(9, dtype=torch.int64, device=dev)
    z9 = torch.zeros(9, C, device=dev)
    for bad in (lambda: em.update(z9.cpu(), y9), lambda: em.update(z9.double(), y9), lambda: em.update(z9, y9.int()),
                lambda: em.update(z9, y9.cpu()), lambda: em.update(z9, y9[:4]), lambda: em.update(z9[:, :5], y9),
                lambda: em.update(z9), lambda: em.update(z9, y9, predictions=y9), lambda: em.update(labels=y9),
                lambda: em.update(predictions=y9, labels=y9, probs=True), lambda: em.merge(P.EvalMeter(5, dev)),
                lambda: P.predict(z9.bfloat16()), lambda: P.predict(torch.zeros(2, 1025, device=dev))):
        with pytest.raises(P.QtError):
            bad()


@pytest.mark.parametrize("rows,C", [(300, 12), (70, 17), (130, 65)])
def test_two_runs_are_bit_identical(rows, C):
    op = Op(_dev())
    z = R.make_logits(rows, C, seed=9, scale=7.0, step=0.25)
    y = R.make_labels(rows, C, seed=9)
    a, b = op.update(C, z=z, y=y), op.update(C, z=z, y=y)
    for k in ("probs", "conf", "pred", "state"):
        assert np.array_equal(a[k].reshape(-1).view(np.uint8), b[k].reshape(-1).view(np.uint8)), k
    ra, rb = op.finalize(C, a["state"]), op.finalize(C, b["state"])
    assert np.array_equal(ra.view(np.uint8), rb.view(np.uint8))


def test_no_host_read_in_update_and_result_is_the_only_sync():
    dev = _dev()
    P = pkg()
    C = 12
    z = torch.from_numpy(R.make_logits(256, C, seed=60)).to(dev)
    y = torch.from_numpy(R.make_labels(256, C, seed=60)).to(dev)
    z2 = torch.from_numpy(R.make_logits(300, 65, seed=61)).to(dev)
    y2 = torch.from_numpy(R.make_labels(300, 65, seed=61)).to(dev)
    meter, meter2, other = P.EvalMeter(C, dev), P.EvalMeter(65, dev), P.EvalMeter(C, dev)
    pred = torch.max(z, 1).indices
    meter.update(z, y, probs=True)            # first launches outside the guarded region (code-object load)
    meter.update(predictions=pred, labels=y)
    meter2.update(z2, y2)
    P.predict(z)
    meter.result()
    meter.reset()
    meter2.reset()
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        meter.update(z, y)
        out = meter.update(z, y, probs=True)
        meter.update(predictions=pred, labels=y)
        meter2.update(z2, y2)
        other.update(z, y)
        meter.merge(other)
        P.predict(z)
        with pytest.raises(RuntimeError):
            meter.result()                    # the one place that reads the device
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert out[0].shape == (256, C)
    res = meter.result()
    assert res["samples"] == 4 * 256 and res["updates"] == 4 and meter2.result()["samples"] == 300
