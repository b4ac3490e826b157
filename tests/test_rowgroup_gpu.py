"""Across the kernels that walk a row through csrc/qt_rowgroup.h: what each file's own tests pin inside that file, pinned
between the files.  The loss head, the evaluation meter and the timeline must name the same class on ties, NaN rows and
infinities, and the timeline's confidence must be the very f32 the meter wrote.  Integers and bit patterns only.

Two sentences of the plan for this file could not be kept as written, both on the rows whose softmax is NaN (one NaN or +inf
logit, or a row of -inf, makes every probability of the row NaN: include/qtcnn.h), and both by documented rules that
tests/test_timeline_gpu.py already pins, not by a fault:
  "qt_timeline_smooth with W = 1, fed metrics' probs, returns metrics' pred_out": the meter's pred_out is the argmax of the
  LOGITS (the column of the NaN, the first +inf); the timeline sees only the probabilities and names the first NaN, column 0.
  Measured on an MI355X: equal on the 40 rows of numbers, 0 on the 30 NaN rows, at every C.
  "its conf carries the bits of metrics' confidence": the smooth kernel stores one NaN, 0x7fc00000, for every NaN mean; the
  meter's NaN confidence is what the division left, 0xffc00000.  Measured: equal bits on the 40 rows of numbers.
So the timeline's pred is held to the total order on the probabilities it was given on every row and to pred_out on every
row of numbers, its conf to the meter's bits on every row of numbers and to the one NaN on the others; no row is left out."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _rowgroup_rows as RR
from _util import pkg

pytestmark = pytest.mark.gpu
ROWS = 70
SMALL_C = (1, 12, 16, 17, 64)        # one thread per row up to 16, a 16-lane group up to 64: the timeline's reach
LARGE_C = (65, 1024)                 # a wave per row


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def run(C):
    """the 70 rows at C through qt_loss_forward, qt_metrics_update and (C <= 64) qt_timeline_smooth with W = 1; computed
    once per C, shared, never written"""
    dev = _dev()
    Lm = pkg("_lib")
    ML, MM, MT = pkg("loss"), pkg("metrics"), pkg("timeline")
    L = Lm.lib()
    z = RR.make_logits(ROWS, C, seed=C)
    labels = np.random.default_rng(C).integers(0, C, ROWS).astype(np.int64)
    d_z, d_y = torch.from_numpy(z).to(dev), torch.from_numpy(labels).to(dev)

    ws_bytes = L.qt_loss_workspace_bytes(ROWS, C)
    d_ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
    d_loss = torch.empty(1, dtype=torch.float32, device=dev)
    d_stats = torch.empty(3, dtype=torch.float64, device=dev)
    d_lpred = torch.full((ROWS,), -1, dtype=torch.int64, device=dev)
    ldesc = ML.LossDesc(0, 0, 0, -100, 0.0, 0.0, None)   # f32, cross-entropy, mean
    Lm.check(L.qt_loss_forward(ctypes.byref(ldesc), Lm.ptr(d_z), C, Lm.ptr(d_y), ROWS, C, Lm.ptr(d_loss), None, Lm.ptr(d_stats),
                               Lm.ptr(d_lpred), None, Lm.ptr(d_ws), ws_bytes, Lm.stream_ptr()), "qt_loss_forward")

    d_probs = torch.full((ROWS, C), -1.0, dtype=torch.float32, device=dev)
    d_conf = torch.full((ROWS,), -1.0, dtype=torch.float32, device=dev)
    d_mpred = torch.full((ROWS,), -1, dtype=torch.int64, device=dev)
    mdesc = MM.MetricsDesc(0, -100)
    Lm.check(L.qt_metrics_update(ctypes.byref(mdesc), Lm.ptr(d_z), C, None, None, ROWS, C, None, Lm.ptr(d_probs), C,
                                 Lm.ptr(d_conf), Lm.ptr(d_mpred), Lm.stream_ptr()), "qt_metrics_update")
    out = {"z": z, "loss_pred": d_lpred.cpu().numpy(), "pred_out": d_mpred.cpu().numpy(), "probs": d_probs.cpu().numpy(),
           "confidence": d_conf.cpu().numpy()}
    if C <= 64:
        d_tpred = torch.full((ROWS,), -1, dtype=torch.int64, device=dev)
        d_tconf = torch.full((ROWS,), -1.0, dtype=torch.float32, device=dev)
        tdesc = MT.TimelineDesc(1, ROWS, C, 1, 1, 0.0, 0, 0)   # one stream of 70 frames, W = 1
        Lm.check(L.qt_timeline_smooth(ctypes.byref(tdesc), Lm.ptr(d_probs), C, None, None, None, None, None, C, Lm.ptr(d_tpred),
                                      Lm.ptr(d_tconf), Lm.stream_ptr()), "qt_timeline_smooth")
        out["timeline_pred"], out["timeline_conf"] = d_tpred.cpu().numpy(), d_tconf.cpu().numpy()
    for a in out.values():
        a.setflags(write=False)
    return out


def test_the_rows_hold_every_kind():
    for C in (17, 1024):
        z = RR.make_logits(ROWS, C, seed=C)
        nan, top = np.isnan(z), z == z.max(axis=1, keepdims=True)
        assert (nan.sum(axis=1) == 1).sum() >= 10 and ((z == np.inf).sum(axis=1) == 2).sum() >= 10
        assert (z == -np.inf).all(axis=1).sum() >= 10 and (np.abs(np.where(np.isfinite(z), z, 0)).max(axis=1) > 90).sum() >= 10
        two = np.flatnonzero((top.sum(axis=1) == 2) & np.isfinite(z).all(axis=1))
        gaps = {int(np.diff(np.flatnonzero(top[i]))[0]) for i in two}
        assert {1, 16} <= gaps, gaps


@pytest.mark.parametrize("C", SMALL_C + LARGE_C)
def test_loss_and_metrics_name_the_same_class(C):
    r = run(C)
    assert r["loss_pred"].tolist() == r["pred_out"].tolist()
    if C in SMALL_C:
        assert r["pred_out"].tolist() == RR.argmax_total_order(r["z"]).tolist()


@pytest.mark.parametrize("C", SMALL_C)
def test_timeline_names_the_class_of_the_probabilities_it_is_given(C):
    r = run(C)
    numbers = ~np.isnan(r["probs"]).any(axis=1)
    assert numbers.sum() >= ROWS // 2 and (~numbers).sum() >= (20 if C > 1 else 10)
    assert r["timeline_pred"].tolist() == RR.argmax_total_order(r["probs"]).tolist()
    assert r["timeline_pred"][numbers].tolist() == r["pred_out"][numbers].tolist()
    assert (r["timeline_pred"][~numbers] == 0).all()        # the first NaN of a row of NaNs


@pytest.mark.parametrize("C", SMALL_C)
def test_timeline_confidence_has_the_bits_of_the_meter(C):
    r = run(C)
    mine, meter = r["timeline_conf"].view(np.uint32), r["confidence"].view(np.uint32)
    numbers = ~np.isnan(r["confidence"])
    assert numbers.sum() >= ROWS // 2 and (~numbers).sum() >= 10
    assert mine[numbers].tolist() == meter[numbers].tolist()
    assert (mine[~numbers] == 0x7FC00000).all()             # the smooth kernel's one NaN, whatever NaN it was given
    rows = np.arange(ROWS)
    assert r["confidence"].view(np.uint32).tolist() == r["probs"][rows, r["pred_out"]].view(np.uint32).tolist()
