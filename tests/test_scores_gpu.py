"""The score-based evaluation on the GPU (csrc/scores.hip, <pkg>/scores.py): the C ABI against the numpy restatement of
tests/_scores_ref.py, integer for integer, with every buffer between guard bands (tests/_guard.py), scores with ld = C + 3
and NaN padding; both routes forced; the recorded scikit-learn values through the kernel; ScoreMeter; repeatability and the
absence of host reads.  For logits the restatement takes p from predict(logits) on the same device, so expf's rounding does
not enter and every count must be equal."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _scores_ref as R
from _guard import Guard
from _util import ROOT, pkg

pytestmark = pytest.mark.gpu
NAN = float("nan")
QT_ERR_UNSUPPORTED = -3
DIRECT, PRIVATE = 1, 2


def _header_int(name):
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    return int(re.search(rf"#define\s+{name}\s+(\d+)\b", header).group(1))


SCORES = pkg("scores")            # every test here needs the module
SLICE = _header_int("QT_SCORES_SLICE_ROWS")
# (C, bits, M, rows): every C in {1, 2, 12, 13, 16, 17, 64} (one thread per row up to 16, a 16-lane row above), every bits in
# {4, 8, 12, 14} (K below, at and above the finalize's 256 threads; 14 is the 128 KB LDS histogram), M in {1, 15, 64}, rows on
# both sides of a wave, of a tile (256 or 16 rows) and of the privatised route's slice
CASES = [(1, 4, 1, 1), (2, 8, 15, 63), (12, 12, 15, 64), (13, 4, 64, 65), (16, 14, 15, 257), (17, 12, 1, 257), (64, 8, 64, 65),
         (12, 12, 15, 257), (17, 4, 15, 63), (64, 14, 15, 64), (16, 12, 15, 1), (12, 8, 15, SLICE - 1), (12, 12, 15, SLICE),
         (13, 12, 64, SLICE + 1), (17, 8, 15, SLICE + 1), (64, 4, 1, SLICE)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class Op:
    """qt_scores_update / qt_scores_finalize through ctypes on guarded buffers"""

    def __init__(self, dev):
        self.S = pkg("scores")
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

    def new_state(self, g, C, bits, M):
        return self.vec_out(g, "state", R.cells(C, bits, M), torch.int64, fill=0)     # the caller zeroes the state once

    def scores(self, g, s):
        rows, C = s.shape
        wide = torch.full((rows, C + 3), NAN)
        wide[:, :C] = torch.from_numpy(s)
        return g.input("scores", wide[:, :C])

    def probs_of(self, s, kind):
        """the probabilities the kernel forms: predict() on the same device for logits, the rows themselves for probs"""
        if kind == R.PROBS:
            return s
        g = Guard(self.dev)
        return pkg("metrics").predict(self.scores(g, s))[0].cpu().numpy()

    def update(self, s, y, C, bits, M, kind, route, state=None, g=None, ignore=R.IGNORE, status=0):
        g = g or Guard(self.dev)
        st_t = self.scores(g, s)
        yt = self.vec_in(g, "labels", y)
        if state is None:
            state = self.new_state(g, C, bits, M)
        desc = self.S.ScoresDesc(0, kind, bits, M, route, ignore)
        got = self.L.qt_scores_update(ctypes.byref(desc), self.lib.ptr(st_t), st_t.stride(0), self.lib.ptr(yt), len(y), C,
                                      self.lib.ptr(state), self.lib.stream_ptr())
        if status:
            assert got == status, got
            return None
        self.lib.check(got, "qt_scores_update")
        g.check()
        return state

    def finalize(self, state, C, bits, M, curves=True):
        """(report float64, curves int64 [C][2][K] or None) of a state (numpy or a device tensor)"""
        g = Guard(self.dev)
        st = self.vec_in(g, "state", state.cpu().numpy() if isinstance(state, torch.Tensor) else state)
        rep = self.vec_out(g, "report", R.report_len(C, M), torch.float64, written=False)
        cv = self.vec_out(g, "curves", 2 * C * (1 << bits), torch.int64, fill=0x5A) if curves else None
        self.lib.check(self.L.qt_scores_finalize(self.lib.ptr(st), C, bits, M, self.lib.ptr(rep), self.lib.ptr(cv),
                                                 self.lib.stream_ptr()), "qt_scores_finalize")
        g.check()
        raw = rep.view(torch.int64).cpu().numpy()
        assert not (raw == -1).any(), "an element of the report was not written"       # (the poison; NaN results are 0x7ff8..)
        return rep.cpu().numpy(), (cv.cpu().numpy().reshape(C, 2, 1 << bits) if curves else None)


def _batch(rows, C, kind, seed):
    z, y = R.make_logits(rows, C, seed)
    s = z if kind == R.LOGITS else R.softmax_f32(z)
    return R.mix_in(s, y, C, kind)


@pytest.mark.parametrize("kind", [R.LOGITS, R.PROBS], ids=["logits", "probs"])
@pytest.mark.parametrize("C,bits,M,rows", CASES)
def test_state_and_report_equal_the_restatement_on_both_routes(C, bits, M, rows, kind):
    op = Op(_dev())
    s, y = _batch(rows, C, kind, seed=rows + 7 * C + bits)
    p = op.probs_of(s, kind)
    want = R.update(None, s, p, y, C, bits, M, kind)
    if rows > 13:
        assert min(want[-5:-1]) >= 1, "every row class occurs"
    direct = op.update(s, y, C, bits, M, kind, DIRECT).cpu().numpy()
    private = op.update(s, y, C, bits, M, kind, PRIVATE).cpu().numpy()
    for name, got in (("direct", direct), ("private", private)):
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (name, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    rep, curves = op.finalize(direct, C, bits, M)
    want_rep, want_curves = R.report(want, C, bits, M)
    assert R.close(rep, want_rep), np.nanmax(np.abs(rep - want_rep))
    o = 4 * C + 3 * M
    assert rep[o + 6:].tolist() == want_rep[o + 6:].tolist()                       # the counters, classes scored
    assert np.array_equal(rep[2 * C:3 * C], want_rep[2 * C:3 * C]) and np.array_equal(rep[4 * C:4 * C + M], want_rep[4 * C:4 * C + M])
    assert np.array_equal(curves, want_curves)


@pytest.mark.parametrize("i", range(5))
def test_recorded_scikit_learn_values_through_the_kernel(i):
    op = Op(_dev())
    g = np.load(os.path.join(ROOT, "tests", "golden", "score_metrics.npz"))
    C, bits, M = int(g["num_classes"][i]), int(g["bits"][i]), 15
    p, y = g[f"probs{i}"], g[f"labels{i}"]
    for route in (DIRECT, PRIVATE):
        rep, _ = op.finalize(op.update(p, y, C, bits, M, R.PROBS, route), C, bits, M, curves=False)
        assert R.close(rep[:C], g[f"auc{i}"]) and R.close(rep[C:2 * C], g[f"ap{i}"]), route
        for j, want in enumerate(g[f"topk{i}"]):
            if not np.isnan(want):
                assert R.close(rep[3 * C + j], want), (route, j)
        assert R.close(rep[4 * C + 3 * M], np.nanmean(g[f"auc{i}"])) and R.close(rep[4 * C + 3 * M + 2], np.nanmean(g[f"ap{i}"]))


def test_more_classes_than_the_cap_are_refused():
    op = Op(_dev())
    s, y = R.make_logits(9, 65, seed=1)
    op.update(s, y, 65, 12, 15, R.LOGITS, 0, state=torch.zeros(8, dtype=torch.int64, device=op.dev), status=QT_ERR_UNSUPPORTED)
    assert b"qt_scores_update" in op.L.qt_last_error()
    assert op.L.qt_scores_state_bytes(65, 12, 15) == 0


@pytest.mark.parametrize("kind", [R.LOGITS, R.PROBS], ids=["logits", "probs"])
def test_calls_on_a_split_batch_give_the_state_of_one_call(kind):
    op = Op(_dev())
    C, bits, M, rows = 12, 12, 15, 300
    s, y = _batch(rows, C, kind, seed=5)
    one = op.update(s, y, C, bits, M, kind, DIRECT).cpu().numpy()
    for cuts, routes in (((0, 1, rows), (DIRECT, PRIVATE)), ((0, 64, 257, rows), (PRIVATE, DIRECT, PRIVATE)), ((0, 299, rows), (0, 0))):
        g = Guard(op.dev)
        state = op.new_state(g, C, bits, M)
        for lo, hi, route in zip(cuts[:-1], cuts[1:], routes):
            op.update(s[lo:hi], y[lo:hi], C, bits, M, kind, route, state=state, g=g)
        got = state.cpu().numpy()
        assert np.array_equal(got[:-1], one[:-1]) and got[-1] == len(routes) and one[-1] == 1, cuts


def test_automatic_route_on_both_sides_of_its_threshold():
    op = Op(_dev())
    T = _header_int("QT_SCORES_AUTO_PRIVATE_ROWS")
    C, bits, M = 12, 12, 15
    s, y = _batch(T, C, R.PROBS, seed=9)
    for rows in (T - 1, T):
        want = R.update(None, s[:rows], s[:rows], y[:rows], C, bits, M, R.PROBS)
        assert np.array_equal(op.update(s[:rows], y[:rows], C, bits, M, R.PROBS, 0).cpu().numpy(), want), rows


@pytest.mark.parametrize("route", [DIRECT, PRIVATE])
def test_contention_all_rows_in_the_same_cells(route):
    op = Op(_dev())
    C, bits, M, rows = 12, 12, 15, 2 * SLICE + 3
    p = np.zeros((rows, C), np.float32)
    p[:, 7] = 1.0
    y = np.full(rows, 7, np.int64)
    st = op.update(p, y, C, bits, M, R.PROBS, route).cpu().numpy()
    K, H = 1 << bits, 2 * C * (1 << bits)
    hist = st[:H].reshape(C, 2, K)
    assert hist[7, 1, K - 1] == rows and int(hist[:, 0, 0].sum()) == rows * (C - 1) and int(hist.sum()) == rows * C
    assert st[H] == rows and st[H + C + 3 * (M - 1):H + C + 3 * M].tolist() == [rows, rows, rows * 65536]
    assert st[-5:].tolist() == [rows, 0, 0, 0, 1]


def test_finalize_of_counts_beyond_32_bits():
    op = Op(_dev())
    C, bits, M = 3, 8, 5
    rng = np.random.default_rng(3)
    st = np.zeros(R.cells(C, bits, M), np.int64)
    H = 2 * C * (1 << bits)
    st[:H] = rng.integers(0, 1 << 22, size=H)
    st[:H][rng.random(H) < 0.3] = 0
    n = int(st[:H].reshape(C, 2, -1)[0].sum())
    st[H:H + C] = [n - 2 * (n // 3), n // 3, n // 3]
    st[H + C:H + C + 3 * M] = np.array([[n // 5, n // 7, (n // 5) * 30000]] * M).reshape(-1)
    st[-5:] = [n, 3, 2, 1, 77]
    rep, curves = op.finalize(st, C, bits, M)
    want, want_curves = R.report(st, C, bits, M)
    assert int(st[:H].reshape(C, 2, -1)[0, 1].sum()) > 1 << 28          # A2 leaves 32 bits (and 2^53) far behind
    assert R.close(rep, want), np.nanmax(np.abs(rep - want))
    assert np.array_equal(curves, want_curves)


@pytest.mark.parametrize("C,bits,rows", [(12, 12, 300), (17, 14, 70)])
def test_two_runs_are_bit_identical(C, bits, rows):
    op = Op(_dev())
    M = 15
    s, y = _batch(rows, C, R.LOGITS, seed=9)
    out = []
    for route in (DIRECT, DIRECT, PRIVATE):
        st = op.update(s, y, C, bits, M, R.LOGITS, route)
        rep, curves = op.finalize(st, C, bits, M)
        out.append((st.cpu().numpy(), rep, curves))
    for a in out[1:]:
        assert np.array_equal(a[0], out[0][0]) and np.array_equal(a[2], out[0][2])
        assert np.array_equal(a[1].view(np.uint64), out[0][1].view(np.uint64))


def test_score_meter_end_to_end_without_host_reads():
    dev = _dev()
    P = pkg()
    C, bits, M = 12, 12, 15
    parts = [R.make_logits(n, C, seed=80 + n) for n in (256, 300, 7)]
    parts[1][1][::9] = R.IGNORE
    parts[1][0][5, 3] = np.nan
    zs = [torch.from_numpy(z).to(dev) for z, _ in parts]
    ys = [torch.from_numpy(y).to(dev) for _, y in parts]
    meter, other, pm = P.ScoreMeter(C, dev, class_names=[f"pose{c}" for c in range(C)]), P.ScoreMeter(C, dev), P.ScoreMeter(C, dev)
    meter.update(zs[0], ys[0])                       # first launches outside the guarded region (code-object load)
    pm.update(probs=P.predict(zs[0])[0], labels=ys[0])
    meter.result()
    meter.reset()
    pm.reset()
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for z, y in zip(zs[:2], ys[:2]):
            assert meter.update(z, y) is None
        other.update(zs[2], ys[2])
        meter.merge(other)
        for z, y in zip(zs, ys):
            pm.update(probs=P.predict(z)[0], labels=y)
        with pytest.raises(RuntimeError):
            meter.result()                           # the one place that reads the device
    finally:
        torch.cuda.set_sync_debug_mode(before)
    want = None
    for (z, y), zt in zip(parts, zs):
        want = R.update(want, z, P.predict(zt)[0].cpu().numpy(), y, C, bits, M, R.LOGITS)
    assert np.array_equal(meter.state.cpu().numpy(), want)
    rep, curves = R.report(want, C, bits, M)
    s = R.scalars(rep, C, M)
    res = meter.result()
    assert R.close(res["auc"], rep[:C]) and R.close(res["average_precision"], rep[C:2 * C]) and R.close(res["top_k"], rep[3 * C:4 * C])
    assert np.array_equal(res["support"], rep[2 * C:3 * C].astype(np.int64)) and res["names"][0] == "pose0"
    assert R.close([res["macro"]["auc"], res["weighted"]["auc"], res["macro"]["average_precision"], res["weighted"]["average_precision"]],
                   [s["macro_auc"], s["weighted_auc"], s["macro_ap"], s["weighted_ap"]])
    cal = res["calibration"]
    assert R.close([cal["ece"], cal["mce"]], [s["ece"], s["mce"]]) and np.array_equal(cal["count"], rep[4 * C:4 * C + M].astype(np.int64))
    assert R.close(cal["accuracy"], rep[4 * C + M:4 * C + 2 * M]) and R.close(cal["confidence"], rep[4 * C + 2 * M:4 * C + 3 * M])
    n_ign = int(sum((y == R.IGNORE).sum() for _, y in parts))
    assert (res["samples"], res["ignored"], res["invalid"], res["nan_rows"], res["updates"]) == (563 - n_ign - 1, n_ign, 0, 1, 3)
    assert res["classes_scored"] == C and res["top_k"][0] == want[2 * C * (1 << bits)] / res["samples"]
    # probabilities as given: the same histograms and calibration as the logits they came from; ranks may differ only by ties
    H = 2 * C * (1 << bits)
    ps = pm.state.cpu().numpy()
    assert np.array_equal(ps[:H], want[:H]) and np.array_equal(ps[H + C:-1], want[H + C:-1])
    # curves: numpy arrays over the occupied bins
    k = 3
    fpr, tpr, thr = meter.roc_curve(k)
    tot = np.append(curves[k].sum(0), 0)
    occ = np.nonzero(tot[:-1] > tot[1:])[0][::-1]
    Pk, Nk = int(curves[k, 0, 0]), int(curves[k, 1, 0])
    assert fpr[0] == 0 and tpr[0] == 0 and np.isinf(thr[0]) and fpr[-1] == 1 and tpr[-1] == 1
    assert np.array_equal(tpr[1:], curves[k, 0][occ] / Pk) and np.array_equal(fpr[1:], curves[k, 1][occ] / Nk)
    assert np.array_equal(thr[1:], occ / float(1 << bits))
    area = float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2))     # the trapezoid area over the occupied bins is the AUC
    assert R.close(area, res["auc"][k])
    prec, rec, thr2 = meter.pr_curve(k)
    assert prec[-1] == 1 and rec[-1] == 0 and rec[0] == 1 and len(thr2) == len(prec) - 1 and np.array_equal(thr2, thr[1:][::-1])
    assert R.close(-np.sum(np.diff(rec) * prec[:-1]), res["average_precision"][k])
    meter.reset()
    assert meter.result()["samples"] == 0 and np.isnan(meter.result()["auc"]).all()
    # refusals: no torch fallback
    z9, y9 = torch.zeros(9, C, device=dev), torch.zeros(9, dtype=torch.int64, device=dev)
    for bad in (lambda: meter.update(z9.cpu(), y9), lambda: meter.update(z9.double(), y9), lambda: meter.update(z9, y9.int()),
                lambda: meter.update(z9, y9.cpu()), lambda: meter.update(z9, y9[:4]), lambda: meter.update(z9[:, :5], y9),
                lambda: meter.update(z9), lambda: meter.update(z9, y9, probs=z9), lambda: meter.update(labels=y9),
                lambda: meter.update(probs=z9.bfloat16(), labels=y9), lambda: meter.update([[0.0] * C], y9[:1]),
                lambda: meter.merge(P.ScoreMeter(5, dev)), lambda: meter.merge(P.ScoreMeter(C, dev, bits=8)),
                lambda: meter.merge(P.EvalMeter(C, dev))):
        with pytest.raises(P.QtError):
            bad()
