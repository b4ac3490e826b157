"""Pose timeline on the GPU (csrc/timeline.hip, <pkg>/timeline.py): qt_timeline_smooth and qt_timeline_decode against the plain
rule of tests/_timeline_ref.py, every output compared for equality of bits (sums in a stated order, one IEEE division and
integers: there is nothing for a tolerance to cover), at the sizes where the tiling, the trips, the history and the state
carried between calls can go wrong.  Every buffer sits between poisoned guard bands (tests/_guard.py); the padding columns of
ld > C are poison and must come back untouched."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _timeline_ref as R
from _guard import Guard
from _util import pkg

pytestmark = pytest.mark.gpu
TILE, TRIP = R.TILE, R.TRIP
F32 = np.float32
POISON64 = -1            # eight 0xFF bytes as an int64


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _api():
    M, Lm = pkg("timeline"), pkg("_lib")
    return M, Lm, Lm.lib()


@functools.lru_cache(maxsize=None)
def smooth_case(batch, frames, C, W, special=True):
    """seeded probabilities with, where the stream is long enough, a NaN row, an inf row and rows of exact ties, and their
    reference; computed once, shared, never written"""
    probs = R.make_probs(1000 * W + 10 * C + batch, batch, frames, C)
    if special and frames >= 4:
        probs[0, frames // 2] = np.nan
        probs[-1, frames // 3] = np.inf
        probs[0, 0] = F32(0.125)                               # every class ties: index 0
        if C >= 3:
            probs[-1, frames - 1, [C - 1, C // 2]] = F32(2.0)  # two classes tie above the rest: the lower index
    ref = R.smooth_vectorised(probs, W)
    for a in (probs,) + ref:
        a.setflags(write=False)
    return probs, ref


def run_smooth(dev, probs, W, ld=None, hist=None, carry=True, want_smoothed=True):
    """qt_timeline_smooth through ctypes.  probs f32 [B,T,C]; ld: row stride of probs and of smoothed (columns C .. ld - 1 are
    poison: NaN in the input, untouched in the output); hist: None or (rows [B,W-1,C], counts [B]).  Returns (smoothed or
    None, pred, confidence, (hist_out, hist_count_out) or None) as numpy arrays."""
    M, Lm, L = _api()
    B, T, C = probs.shape
    ld = C if ld is None else ld
    padded = np.full((B, T, ld), np.nan, F32)
    padded[..., :C] = probs
    G = Guard(dev)
    d_probs = G.input("probs", torch.from_numpy(padded))
    d_hin = d_cin = None
    if hist is not None:
        d_hin = G.input("hist_in", torch.from_numpy(np.ascontiguousarray(hist[0], F32)))
        d_cin = G.input("hist_count_in", torch.from_numpy(np.ascontiguousarray(hist[1], np.int32)))
    d_sm = G.output("smoothed", (B, T, ld), torch.float32, written=False) if want_smoothed else None    # (a NaN mean is a value)
    d_pred = G.output("pred", (B, T), torch.int64)
    d_conf = G.output("confidence", (B, T), torch.float32, written=False)      # a NaN confidence is a legitimate value
    d_hout = G.output("hist_out", (B, W - 1, C), torch.float32, written=False) if carry and W > 1 else None
    d_cout = G.output("hist_count_out", (B,), torch.int32) if carry and W > 1 else None
    desc = M.TimelineDesc(B, T, C, W, 1, 0.0, 0, 0)
    Lm.check(L.qt_timeline_smooth(ctypes.byref(desc), Lm.ptr(d_probs), ld, Lm.ptr(d_hin), Lm.ptr(d_cin), Lm.ptr(d_hout),
                                  Lm.ptr(d_cout), Lm.ptr(d_sm), ld, Lm.ptr(d_pred), Lm.ptr(d_conf), Lm.stream_ptr()),
             "qt_timeline_smooth")
    G.check()
    sm = None
    if want_smoothed:
        sm = d_sm.cpu().numpy()
        assert (sm[..., C:].view(np.uint32) == 0xFFFFFFFF).all(), "padding columns of smoothed were written"
        sm = np.ascontiguousarray(sm[..., :C])
    pred = d_pred.cpu().numpy()
    assert (pred != POISON64).all(), "pred not written everywhere"
    hout = (d_hout.cpu().numpy(), d_cout.cpu().numpy()) if d_hout is not None else None
    return sm, pred, d_conf.cpu().numpy(), hout


def same_smooth(got, ref, what):
    sm, pred, conf, hist = got
    if sm is not None:
        assert R.bits(sm) == R.bits(ref[0]), (what, "smoothed", int((sm.view(np.uint32) != ref[0].view(np.uint32)).sum()))
    assert R.bits(pred) == R.bits(ref[1]), (what, "pred")
    assert R.bits(conf) == R.bits(ref[2]), (what, "confidence")
    if hist is not None:
        assert R.bits(hist[0]) == R.bits(ref[3]) and R.bits(hist[1]) == R.bits(ref[4]), (what, "history")


@pytest.mark.parametrize("C", [1, 12, 13, 16, 17, 64])
@pytest.mark.parametrize("W", [1, 2, 5, 64])
def test_smooth_bits_equal_the_rule(W, C):
    """frames: one; around the window; one tile, one frame fewer, one more; 2 TILE + 1 (a last tile of one frame).  C: one
    class, the 12 of the model, 13 and 16 (the DPP row's last lanes), 17 (the first wave-wide size), 64.  ld == C takes the
    16-byte loads where C is a multiple of 4, ld = C + 3 never does."""
    dev = _dev()
    for batch in (1, 3):
        for frames in sorted({1, W - 1, W, W + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1} - {0}):
            probs, ref = smooth_case(batch, frames, C, W)
            for ld in (C, C + 3):
                same_smooth(run_smooth(dev, probs, W, ld=ld), ref, (batch, frames, ld))


def test_smooth_ties_nan_and_inf_rows():
    dev = _dev()
    for C, W in ((12, 5), (64, 5)):
        T = TILE + 9
        probs = np.array(smooth_case(1, T, C, W, special=False)[0])
        probs[0, 3] = F32(0.25)                                 # a row of ties at a stream's start: n = 4 rows of which ...
        probs[0, 0:3] = F32(0.5)                                # ... all are ties
        probs[0, 20] = np.nan
        probs[0, 40] = np.inf
        hi, lo = (C - 2, 3) if C == 12 else (50, 20)            # (C = 64: the two sit in different DPP rows)
        probs[0, 60:60 + W, [hi, lo]] = F32(4.0)
        clean, _ = smooth_case(1, T, C, W, special=False)
        ref, base = R.smooth_vectorised(probs, W), R.smooth_vectorised(clean, W)
        got = run_smooth(dev, probs, W)
        same_smooth(got, ref, (C, W))
        sm, pred, conf, _ = got
        assert pred[0, :4].tolist() == [0, 0, 0, 0] and pred[0, 60 + W - 1] == lo
        nan_rows, inf_rows = np.isnan(sm[0]).all(axis=1), np.isinf(sm[0]).all(axis=1)
        assert nan_rows.tolist() == [20 <= f < 20 + W for f in range(T)]        # exactly the W frames that read the row
        assert inf_rows.tolist() == [40 <= f < 40 + W for f in range(T)]
        assert (sm.view(np.uint32)[0, nan_rows] == 0x7FC00000).all() and np.isnan(conf[0, nan_rows]).all()
        untouched = np.ones(T, bool)
        for at in (0, 20, 40, 60):
            untouched[at:at + 2 * W] = False
        assert R.bits(sm[0, untouched]) == R.bits(base[0][0, untouched])         # and no other frame


def test_smooth_without_the_smoothed_rows():
    dev = _dev()
    for C, W in ((12, 15), (17, 3)):
        probs, ref = smooth_case(3, TILE + 1, C, W)
        same_smooth(run_smooth(dev, probs, W, want_smoothed=False), ref, (C, W))
        same_smooth(run_smooth(dev, probs, W, carry=False, ld=C + 3), ref, (C, W, "no history kept"))


def test_history_counts_and_slots():
    """a count above W - 1 is W - 1, a negative one 0; slots at and beyond the count are poison here and must not be read;
    slots beyond the new count come back as zeros"""
    dev = _dev()
    C, W, B, T = 12, 5, 3, 2
    probs = R.make_probs(77, B, T, C)
    rows = R.make_probs(78, B, W - 1, C)
    for counts, model in (([9, 4, -3], [4, 4, 0]), ([1, 0, 2], [1, 0, 2])):
        given = rows.copy()
        for b, c in enumerate(model):
            given[b, c:] = np.nan
        ref = R.smooth_vectorised(probs, W, np.nan_to_num(given), np.array(model, np.int32))
        got = run_smooth(dev, probs, W, hist=(given, np.array(counts, np.int32)))
        same_smooth(got, ref, counts)
        assert not np.isnan(got[0]).any()
    assert got[3][1].tolist() == [3, 2, 4] and not got[3][0][1, 2:].any()


def _cuts(seed, T, pieces):
    rng = np.random.default_rng(seed)
    cuts = sorted(rng.choice(np.arange(2, T - 1), pieces - 2, replace=False).tolist()) if pieces > 2 else []
    return cuts + [T - 1]                                        # the last call is one frame


# ---- decode -------------------------------------------------------------------------------------------------------------
def run_decode(dev, pred, conf, C, min_run, min_conf, state=None, segments=None, capacity=32, flush=False):
    """qt_timeline_decode through ctypes.  state int64 [B,8] / segments int64 [B,capacity,4] as they are before the call (None:
    zeros / poison).  Returns (stable, state, segments) after it."""
    M, Lm, L = _api()
    B, T = pred.shape
    G = Guard(dev)
    d_pred = G.input("pred", torch.from_numpy(np.ascontiguousarray(pred, np.int64))) if T else None
    d_conf = G.input("confidence", torch.from_numpy(np.ascontiguousarray(conf, F32))) if T else None
    d_state = G.output("state", (B, R.STATE), torch.int64, fill=0)
    if state is not None:
        d_state.copy_(torch.from_numpy(np.ascontiguousarray(state, np.int64)))
    capacity = capacity if segments is None else segments.shape[1]
    d_seg = G.output("segments", (B, capacity, 4), torch.int64) if capacity else None
    if segments is not None and capacity:
        d_seg.copy_(torch.from_numpy(np.ascontiguousarray(segments, np.int64)))
    d_stable = G.output("stable", (B, T), torch.int64, fill=0x5A) if T else None
    desc = M.TimelineDesc(B, T, C, 1, min_run, min_conf, capacity, int(flush))
    Lm.check(L.qt_timeline_decode(ctypes.byref(desc), Lm.ptr(d_pred), Lm.ptr(d_conf), Lm.ptr(d_state), Lm.ptr(d_stable),
                                  Lm.ptr(d_seg), Lm.stream_ptr()), "qt_timeline_decode")
    G.check()
    stable = d_stable.cpu().numpy() if T else np.zeros((B, 0), np.int64)
    seg = d_seg.cpu().numpy() if capacity else np.zeros((B, 0, 4), np.int64)
    return stable, d_state.cpu().numpy(), seg


def same_decode(got, ref, what):
    for name, g, r in zip(("stable", "state", "segments"), got, ref):
        assert g.dtype == r.dtype and R.bits(g) == R.bits(r), (what, name)


@pytest.mark.parametrize("min_run", [1, 3, TRIP + 2])
def test_decode_equals_the_rule(min_run):
    """frames: one; a trip, one fewer, one more; two trips and one.  min_run = TRIP + 2: a run that qualifies only across a
    trip boundary, so the stable label of a whole trip comes from the carry"""
    dev = _dev()
    C, min_conf = 12, 0.5
    for batch in (1, 3):
        for frames in (1, TRIP - 1, TRIP, TRIP + 1, 2 * TRIP + 1):
            pred, conf = R.make_labels(300 + frames + batch, batch, frames, C, run=9, min_conf=min_conf)
            if min_run > TRIP:                                   # make such runs exist: no flicker in stream 0
                pred[0], conf[0] = 5, F32(0.9)
                if frames > TRIP:
                    pred[0, :TRIP - 3] = 4                       # ... and a run that starts inside the first trip
            empty = (np.zeros((batch, R.STATE), np.int64), np.full((batch, 32, 4), POISON64, np.int64))
            for flush in (False, True):
                ref = R.decode(pred, conf, C, min_run, min_conf, *empty, flush=flush)
                same_decode(run_decode(dev, pred, conf, C, min_run, min_conf, flush=flush), ref, (batch, frames, flush))
            if min_run == 3 and frames > TRIP:
                assert ref[1][:, R.TOTAL].min() >= 3 and (ref[0] == -1).any()
            if min_run > TRIP and frames == 2 * TRIP + 1:
                assert ref[0][0].tolist() == [-1] * (TRIP - 3 + min_run - 1) + [5] * (frames - (TRIP - 3 + min_run - 1))


PERIOD = R.AHEAD * TRIP    # the decode kernel works on AHEAD trips while it loads the next AHEAD: its loop runs again above this


@pytest.mark.parametrize("min_run", [1, 3, TRIP + 2])
def test_decode_across_the_prefetch_period(min_run):
    """frames: a period of the kernel's loop, one fewer, one more (a second pass of one frame: the hand-over of the loaded
    trips, the carry across the pass, a last group cut short after its first trip); two periods and one (a third pass)"""
    dev = _dev()
    C, min_conf = 12, 0.5
    for batch in (1, 3):
        for frames in (PERIOD - 1, PERIOD, PERIOD + 1, 2 * PERIOD + 1):
            pred, conf = R.make_labels(500 + frames + batch, batch, frames, C, run=9, min_conf=min_conf)
            if min_run > TRIP:                                   # a run that qualifies only behind the period's edge
                pred[0], conf[0] = 5, F32(0.9)
                pred[0, :PERIOD - 3] = 4
            empty = (np.zeros((batch, R.STATE), np.int64), np.full((batch, 96, 4), POISON64, np.int64))
            for flush in (False, True):
                ref = R.decode(pred, conf, C, min_run, min_conf, *empty, flush=flush)
                same_decode(run_decode(dev, pred, conf, C, min_run, min_conf, capacity=96, flush=flush), ref, (batch, frames, flush))
            if min_run == 3:
                assert 20 <= ref[1][:, R.TOTAL].min() and ref[1][:, R.TOTAL].max() <= 96 and (ref[0] == -1).any()
                assert frames < 2 * PERIOD or (ref[2][:, :, 0] >= PERIOD).all(axis=0).any()   # records of the later passes
            if min_run > TRIP and frames == 2 * PERIOD + 1:
                first = PERIOD - 3 + min_run - 1                 # label 4 qualifies at TRIP + 1, label 5 here, in the second pass
                assert ref[0][0].tolist() == [-1] * (min_run - 1) + [4] * (first - min_run + 1) + [5] * (frames - first)
                assert [r[:3] for r in R.segment_list(ref[1], ref[2])] == [(min_run - 1, first - min_run + 1, 4), (first, frames - first, 5)]


def test_decode_segment_and_run_open_across_the_period():
    """label 1 up to two frames before the period's edge, then label 2 with min_run 5: the run of 2 starts in the first pass and
    qualifies in the second, so the segment of 1 is open across the edge and is closed by a lane of the second pass; the segment
    of 2 is open across the next edge; capacity 2 leaves the third record unwritten"""
    dev = _dev()
    C, T = 4, 2 * PERIOD + 9
    pred = np.full((1, T), 2, np.int64)
    pred[0, :PERIOD - 2] = 1
    pred[0, -4:] = 3
    conf = np.linspace(0.6, 1.0, T, dtype=F32)[None]
    for capacity in (8, 2):
        empty = (np.zeros((1, R.STATE), np.int64), np.full((1, capacity, 4), POISON64, np.int64))
        for min_run in (5, 3):
            ref = R.decode(pred, conf, C, min_run, 0.5, *empty, flush=True)
            got = run_decode(dev, pred, conf, C, min_run, 0.5, capacity=capacity, flush=True)
            same_decode(got, ref, (capacity, min_run))
    ref = R.decode(pred, conf, C, 5, 0.5, np.zeros((1, R.STATE), np.int64), np.full((1, 8, 4), POISON64, np.int64), flush=True)
    assert [r[:3] for r in R.segment_list(ref[1], ref[2])] == [(4, PERIOD - 2, 1), (PERIOD + 2, T - 4 - (PERIOD + 2) + 4, 2)]
    ref = R.decode(pred, conf, C, 3, 0.5, np.zeros((1, R.STATE), np.int64), np.full((1, 8, 4), POISON64, np.int64), flush=True)
    assert [r[:3] for r in R.segment_list(ref[1], ref[2])] == [(2, PERIOD - 2, 1), (PERIOD, T - 2 - PERIOD, 2), (T - 2, 2, 3)]


def test_decode_run_across_a_trip_boundary_and_flush():
    dev = _dev()
    C = 4
    # a segment that is open across two trip boundaries, closed by a change in the third trip
    pred = np.full((1, 2 * TRIP + 10), 2, np.int64)
    pred[0, :5] = 1
    pred[0, -4:] = 3
    conf = np.linspace(0.6, 1.0, pred.shape[1], dtype=F32)[None]
    empty = (np.zeros((1, R.STATE), np.int64), np.full((1, 8, 4), POISON64, np.int64))
    ref = R.decode(pred, conf, C, 2, 0.5, *empty, flush=True)
    got = run_decode(dev, pred, conf, C, 2, 0.5, capacity=8, flush=True)
    same_decode(got, ref, "long segment")
    assert [r[:3] for r in R.segment_list(got[1], got[2])] == [(1, 5, 1), (6, 2 * TRIP + 1, 2), (2 * TRIP + 7, 3, 3)]
    # flush without an open segment (the stream ends in a gap), then frames == 0 with flush, twice
    pred, conf = np.array([[1, 1, 1, 9, 9, 0, 2]], np.int64), np.full((1, 7), 0.9, F32)
    ref = R.decode(pred, conf, C, 2, 0.5, *empty, flush=True)
    got = run_decode(dev, pred, conf, C, 2, 0.5, capacity=8, flush=True)
    same_decode(got, ref, "no open segment")
    assert got[1][0, R.TOTAL] == 1 and got[1][0, R.STABLE] == 0
    none = (np.zeros((1, 0), np.int64), np.zeros((1, 0), F32))
    ref = R.decode(pred, conf, C, 2, 0.5, *empty, flush=False)
    got = run_decode(dev, pred, conf, C, 2, 0.5, capacity=8, flush=False)
    same_decode(got, ref, "left open")
    for _ in range(2):                                           # the second flush adds nothing
        ref = R.decode(*none, C, 2, 0.5, ref[1], ref[2], flush=True)
        got = run_decode(dev, *none, C, 2, 0.5, state=got[1], segments=got[2], flush=True)
        same_decode(got, ref, "frames == 0 with flush")
    # an open segment, flushed by a call of no frames; then the stream goes on with the same label
    pred, conf = np.array([[1, 1, 1]], np.int64), np.full((1, 3), 0.9, F32)
    ref = R.decode(pred, conf, C, 2, 0.5, *empty)
    got = run_decode(dev, pred, conf, C, 2, 0.5, capacity=8)
    ref = R.decode(*none, C, 2, 0.5, ref[1], ref[2], flush=True)
    got = run_decode(dev, *none, C, 2, 0.5, state=got[1], segments=got[2], flush=True)
    same_decode(got, ref, "flush alone")
    assert R.segment_list(got[1], got[2])[0][:3] == (1, 2, 1)
    more = (np.array([[1, 1, 3, 3]], np.int64), np.full((1, 4), 0.9, F32))
    same_decode(run_decode(dev, *more, C, 2, 0.5, state=got[1], segments=got[2], flush=True),
                R.decode(*more, C, 2, 0.5, ref[1], ref[2], flush=True), "after a flush")


def test_decode_capacity_below_the_total():
    dev = _dev()
    C, T = 12, 2 * TRIP + 1
    pred, conf = R.make_labels(41, 3, T, C, run=5, flicker=0.0, low=0.0)
    empty = (np.zeros((3, R.STATE), np.int64), np.full((3, 4, 4), POISON64, np.int64))
    ref = R.decode(pred, conf, C, 1, 0.5, *empty, flush=True)
    got = run_decode(dev, pred, conf, C, 1, 0.5, capacity=4, flush=True)
    same_decode(got, ref, "capacity 4")
    assert got[1][:, R.TOTAL].min() > 12
    full = R.decode(pred, conf, C, 1, 0.5, empty[0], np.full((3, 64, 4), POISON64, np.int64), flush=True)
    assert R.bits(got[2]) == R.bits(full[2][:, :4]) and got[1][:, R.TOTAL].tolist() == full[1][:, R.TOTAL].tolist()
    # some records, then poison: capacity above the total
    got = run_decode(dev, pred[:, :20], conf[:, :20], C, 1, 0.5, capacity=64, flush=True)
    n = int(got[1][0, R.TOTAL])
    assert 0 < n < 64 and (got[2][0, n:] == POISON64).all() and (got[2][0, :n, 1] > 0).all()
    # capacity 0: segments may be NULL, the total still counts
    got = run_decode(dev, pred, conf, C, 1, 0.5, capacity=0, flush=True)
    assert got[1][:, R.TOTAL].tolist() == full[1][:, R.TOTAL].tolist() and R.bits(got[0]) == R.bits(ref[0])


# ---- the chunk contract -------------------------------------------------------------------------------------------------
def _pipeline(dev, probs, cuts, W, C, min_run, min_conf, capacity=64):
    """smooth then decode over consecutive calls cut at `cuts`, the state, the history and the records carried on the way a
    caller carries them; the last call flushes"""
    B, T = probs.shape[:2]
    hist, state, seg, parts = None, None, None, []
    for a, b in zip([0] + cuts, cuts + [T]):
        sm, pred, conf, hist = run_smooth(dev, probs[:, a:b], W, hist=hist)
        stable, state, seg = run_decode(dev, pred, conf, C, min_run, min_conf, state=state, segments=seg, capacity=capacity,
                                        flush=(b == T))
        parts.append((sm, pred, conf, stable))
    return [np.concatenate([p[i] for p in parts], axis=1) for i in range(4)] + [hist[0], hist[1], state, seg]


NAMES = ("smoothed", "pred", "confidence", "stable", "hist_out", "hist_count_out", "state", "segments")


@pytest.mark.parametrize("C, W, min_conf", [(12, 15, 0.3), (17, 64, 0.1)])
def test_chunks_give_the_bits_of_one_call(C, W, min_conf):
    dev = _dev()
    T = 2 * TILE + 1
    probs, ref = smooth_case(3, T, C, W)
    whole = _pipeline(dev, probs, [], W, C, 3, min_conf)
    same_smooth((whole[0], whole[1], whole[2], (whole[4], whole[5])), ref, "one call")
    empty = (np.zeros((3, R.STATE), np.int64), np.full((3, 64, 4), POISON64, np.int64))
    want = R.decode(ref[1], ref[2], C, 3, min_conf, *empty, flush=True)
    same_decode((whole[3], whole[6], whole[7]), want, "one call")
    assert want[1][:, R.TOTAL].min() >= 3
    for pieces in (2, 3):
        cuts = _cuts(C + pieces, T, pieces)
        assert len(cuts) == pieces - 1 and cuts[-1] == T - 1
        got = _pipeline(dev, probs, cuts, W, C, 3, min_conf)
        for name, w, g in zip(NAMES, whole, got):
            assert R.bits(w) == R.bits(g), (cuts, name)
    got = _pipeline(dev, probs, [TILE, 2 * TILE], W, C, 3, min_conf)         # the cuts on the tile (and trip) edges
    for name, w, g in zip(NAMES, whole, got):
        assert R.bits(w) == R.bits(g), ("tile edges", name)
    for b in range(3):                                                  # a stream alone has the bits it has in the batch
        alone = _pipeline(dev, probs[b:b + 1], _cuts(b, T, 3), W, C, 3, min_conf)
        for name, w, g in zip(NAMES, whole, alone):
            assert R.bits(w[b:b + 1]) == R.bits(g), (b, name)


def test_chunks_longer_than_the_decode_period():
    """a stream of PERIOD + TRIP + 1 frames in one call (a second pass of two trips, the last of one frame), and cut so that
    one call is longer than the period and the next starts inside what would have been its second pass"""
    dev = _dev()
    C, W, T = 12, 15, PERIOD + TRIP + 1
    probs, ref = smooth_case(3, T, C, W)
    whole = _pipeline(dev, probs, [], W, C, 3, 0.3)
    same_smooth((whole[0], whole[1], whole[2], (whole[4], whole[5])), ref, "one call")
    empty = (np.zeros((3, R.STATE), np.int64), np.full((3, 64, 4), POISON64, np.int64))
    want = R.decode(ref[1], ref[2], C, 3, 0.3, *empty, flush=True)
    same_decode((whole[3], whole[6], whole[7]), want, "one call")
    assert 20 <= want[1][:, R.TOTAL].min() and want[1][:, R.TOTAL].max() <= 64
    for cuts in ([PERIOD + 3], [5, PERIOD + 5 + 2], [PERIOD, T - 1]):
        got = _pipeline(dev, probs, cuts, W, C, 3, 0.3)
        for name, w, g in zip(NAMES, whole, got):
            assert R.bits(w) == R.bits(g), (cuts, name)
    alone = _pipeline(dev, probs[1:2], [PERIOD + 1], W, C, 3, 0.3)
    for name, w, g in zip(NAMES, whole, alone):
        assert R.bits(w[1:2]) == R.bits(g), ("alone", name)


# ---- the Python class ---------------------------------------------------------------------------------------------------
def test_the_video_loop_end_to_end():
    """predict -> PoseTimeline.update -> FrameAnnotator.draw on 8 frames of 64 x 48 per step, no host synchronisation; then
    finish(), segments() against the rule and transitions() against a Python count"""
    dev = _dev()
    P = pkg()
    C, W, min_run, min_conf, steps, N = 12, 3, 2, 0.2, 5, 8
    rng = np.random.default_rng(5)
    lead = np.repeat(rng.integers(0, C, steps * N // 5 + 1), 5)[:steps * N]
    logits = rng.standard_normal((steps * N, C)).astype(F32)
    logits[np.arange(steps * N), lead] += F32(3.0)
    d_logits = torch.from_numpy(logits).to(dev)
    frames = torch.from_numpy(rng.integers(0, 256, (N, 48, 64, 3), dtype=np.uint8)).to(dev)
    atlas = torch.from_numpy(rng.integers(0, 256, (C + 14, 8, 12), dtype=np.uint8))
    annotator = P.FrameAnnotator(atlas=(atlas, torch.full((C + 14,), 12, dtype=torch.int32)), caption_origin=(2, 2))
    names = [f"pose{k}" for k in range(C)]
    timeline = P.PoseTimeline(C, dev, window=W, min_run=min_run, min_confidence=min_conf, capacity=16, class_names=names)
    annotator.draw(frames, pred=torch.zeros(N, dtype=torch.int64, device=dev))      # (the tables' upload is not the loop's)
    outs, shown = [], []
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for s in range(steps):
            probs, _, _ = P.predict(d_logits[s * N:(s + 1) * N])
            pred, conf, stable, rows = timeline.update(probs, smoothed=True)
            shown.append(annotator.draw(frames, pred=stable, confidence=conf))
            outs.append((probs, rows, pred, conf, stable))
        timeline.finish()
        counts, dwell = timeline.transitions()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    probs = torch.cat([o[0] for o in outs]).cpu().numpy()[None]
    ref = R.smooth(probs, W)
    got = [torch.cat([o[i] for o in outs]).cpu().numpy()[None] for i in (1, 2, 3, 4)]
    assert got[0].shape == (1, steps * N, C) and R.bits(got[0]) == R.bits(ref[0])
    assert R.bits(got[1]) == R.bits(ref[1]) and R.bits(got[2]) == R.bits(ref[2])
    want = R.decode(ref[1], ref[2], C, min_run, min_conf, np.zeros((1, R.STATE), np.int64), np.zeros((1, 16, 4), np.int64), flush=True)
    assert R.bits(got[3]) == R.bits(want[0]) and R.bits(timeline.state.cpu().numpy()) == R.bits(want[1])
    assert (want[0] == -1).any() and 3 <= want[1][0, R.TOTAL] <= 16
    listed = R.segment_list(want[1], want[2])
    assert timeline.segments() == [[(a, n, names[k], m) for a, n, k, m in listed]]
    tensors = timeline.segments(as_tensors=True)[0]
    assert tensors["label"].tolist() == [k for _, _, k, _ in listed] and tensors["mean_confidence"].tolist() == [m for *_, m in listed]
    want_counts, want_dwell = R.transitions(want[1], want[2], C)
    assert counts.dtype == torch.int64 and counts.cpu().numpy().tolist() == want_counts.tolist() and want_counts.sum() == len(listed) - 1
    assert dwell.cpu().numpy().tolist() == want_dwell.tolist()
    # the drawn frames: the caption of the stable label, none where there is none
    for s in range(steps):
        d_stable = torch.from_numpy(want[0][0, s * N:(s + 1) * N]).to(dev)
        again = annotator.draw(frames, pred=d_stable, confidence=torch.from_numpy(ref[2][0, s * N:(s + 1) * N]).to(dev))
        assert torch.equal(shown[s], again)
        blank = d_stable < 0
        assert torch.equal(shown[s][blank], frames[blank]) and not torch.equal(shown[s][~blank], frames[~blank])


def test_the_python_class():
    dev = _dev()
    P = pkg()
    C, W, S, T = 12, 15, 3, 2 * TILE + 1
    probs, ref = smooth_case(S, T, C, W)
    d_probs = torch.from_numpy(np.array(probs)).to(dev)
    timeline = P.PoseTimeline(C, dev, streams=S, window=W, min_run=3, min_confidence=0.3, capacity=4)
    want = R.decode(ref[1], ref[2], C, 3, 0.3, np.zeros((S, R.STATE), np.int64), np.zeros((S, 4, 4), np.int64), flush=True)
    chunks = [(0, 5), (5, TILE), (TILE, TILE + 1), (TILE + 1, T)]
    parts = [timeline.update(d_probs[:, a:b], smoothed=True) for a, b in chunks]       # (views with a stream stride of their own)
    timeline.finish()
    for i, r in enumerate((ref[1], ref[2], want[0], ref[0])):
        g = torch.cat([p[i] for p in parts], dim=1)
        assert g.device == d_probs.device and R.bits(g.cpu().numpy()) == R.bits(r), i
    assert R.bits(timeline.state.cpu().numpy()) == R.bits(want[1]) and R.bits(timeline.records.cpu().numpy()) == R.bits(want[2])
    assert want[1][:, R.TOTAL].min() > 4
    with pytest.raises(P.QtError, match=rf"closed {int(want[1][0, R.TOTAL])} segments.*capacity = 4"):
        timeline.segments()
    counts, dwell = timeline.transitions()                         # the records that exist
    want_counts, want_dwell = R.transitions(want[1], want[2], C)
    assert counts.cpu().numpy().tolist() == want_counts.tolist() and dwell.cpu().numpy().tolist() == want_dwell.tolist()
    # reset: the same video again gives the same state
    timeline.reset()
    assert not timeline.state.any()
    timeline.update(d_probs)
    timeline.finish()
    assert R.bits(timeline.state.cpu().numpy()) == R.bits(want[1])
    # one stream takes [frames, C]; a window of one keeps no history
    one = P.PoseTimeline(C, dev, window=1, min_run=1)
    pred, conf, stable = one.update(d_probs[1])
    assert tuple(pred.shape) == (T,) and torch.equal(pred, stable) and torch.equal(pred, d_probs[1].argmax(dim=1))
    padded = torch.zeros(T, C + 4, device=dev)
    padded[:, :C] = d_probs[1]
    assert torch.equal(one.reset().update(padded[:, :C])[1], conf)     # a row stride above C is taken as it is
    # refusals: no torch fallback
    with pytest.raises(P.QtError, match="no CPU or torch fallback"):
        timeline.update(d_probs.cpu())
    with pytest.raises(P.QtError, match="f32"):
        timeline.update(d_probs.double())
    with pytest.raises(P.QtError, match="probs must be"):
        timeline.update(d_probs[:2])
    with pytest.raises(P.QtError, match="probs must be"):
        timeline.update(d_probs[0])
    with pytest.raises(P.QtError, match="probs must be"):
        timeline.update(d_probs[:, :, :5])
    with pytest.raises(P.QtError, match="tensor"):
        timeline.update(np.array(probs))
