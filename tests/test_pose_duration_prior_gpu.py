"""The learner of the chain with hold durations on the GPU (csrc/pose_duration_prior.hip, csrc/pose_duration_sweep.h,
<pkg>/pose_order.py): qt_pose_duration_prior_expect against the float64 loops of tests/_pose_duration_prior_ref.py, beside the
same loops with the rule's own precision (double levels, f32 terms, double sums) on the same inputs: e_kernel <= 4 e_mixed +
2^-20, the form and constants of tests/test_pose_duration_posterior_gpu.py (the factor covers the device's exp2 and log2 and
the regrouped sums).  The counts are measured relative to max(1, count), the evidence relative to max(1, |Z|).  Every figure is
printed before it is asserted (pytest -s shows them).  Every buffer sits between poisoned guard bands (tests/_guard.py), the
workspace is exactly the queried size and NaN-filled, the padding columns of ld > C are NaN, and the inputs must come back byte
for byte.  The hard counts and the M-step are compared for equality with the integer loops and the numpy M-step.

Measured on an MI355X (EXPERIMENTS.md, "Pose-duration learner"): the largest share of the bound that any output uses is 0.32, at
(S, C, D, T) = (16, 12, 8, 70), and 0.31 at (64, 64, 128, 300); an E-step of a 9,000-frame video takes 34.2 ms at S = 12, D = 64,
what qt_pose_duration_posterior takes with dur_counts alone (34.3 ms), and 192 ms against 174 ms at S = 64, D = 128."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _pose_duration_prior_ref as A
import _pose_duration_ref as Q
import _pose_order_ref as R
from _guard import Guard
from _util import pkg

pytestmark = pytest.mark.gpu
F32 = np.float32
FACTOR, FLOOR = 4.0, 2.0 ** -20
OUT = ("trans_counts", "start_counts", "dur_counts", "totals")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _api():
    M, Lm = pkg("pose_order"), pkg("_lib")
    return M, Lm, Lm.lib()


def chain(S, C):
    return R.cyclic_prior([s % C for s in range(S)], -39, -300, skip=-800, other=-3000)


def init_for(S):
    return ((np.arange(S, dtype=np.int64) * 977) % 4001 - 4000).astype(np.int32)


def durations(S, D, seed=0):
    """(dur, dur_open) int32 [S, D]: seeded scores in [-500, 0] so that many lengths compete, some lengths forbidden;
    dur_open a table of its own, not the suffix maximum"""
    rng = np.random.default_rng(100 * S + D + seed)
    dur = -rng.integers(0, 501, (S, D))
    dur[rng.random((S, D)) < 0.15] = R.TRANS_FLOOR
    open_ = np.maximum(Q.suffix_max(dur), -rng.integers(0, 60, (S, D)))
    return dur.astype(np.int32), open_.astype(np.int32)


def _i32(a):
    return None if a is None else torch.from_numpy(np.array(a, np.int32))


def _accumulators(G, S, D, before, start_counts=True):
    out = [G.output("trans_counts", (S, S), torch.float64, fill=0),
           G.output("start_counts", (S,), torch.float64, fill=0) if start_counts else None,
           G.output("dur_counts", (S, D), torch.float64, fill=0), G.output("totals", (2,), torch.float64, fill=0)]
    if before is not None:
        for t, b in zip(out, before):
            if t is not None:
                t.copy_(torch.from_numpy(np.ascontiguousarray(b, np.float64)))
    return out


def _numpy(ts):
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def run(dev, probs, sc, tr, dur, init=None, dur_open=None, lengths=None, ld=None, before=None, start_counts=True):
    """qt_pose_duration_prior_expect through ctypes.  probs f32 [B,T,C]; ld: row stride (columns C .. ld - 1 are NaN); before:
    the four accumulators as they are before the call (zeros).  Returns (trans_counts, start_counts, dur_counts, totals)."""
    M, Lm, L = _api()
    B, T, C = probs.shape
    S, D = np.shape(dur)
    ld = C if ld is None else ld
    padded = np.full((B, T, ld), np.nan, F32)
    padded[..., :C] = probs
    G = Guard(dev)
    d_probs = G.input("probs", torch.from_numpy(padded))
    d_sc, d_tr, d_init = G.input("state_class", _i32(sc)), G.input("trans", _i32(tr)), G.input("init", _i32(init))
    d_dur, d_open, d_len = G.input("dur", _i32(dur)), G.input("dur_open", _i32(dur_open)), G.input("lengths", _i32(lengths))
    acc = _accumulators(G, S, D, before, start_counts)
    desc = M.PoseDurationDesc(B, T, C, S, D)
    need = L.qt_pose_duration_prior_workspace_bytes(ctypes.byref(desc))
    assert need == 8 * (2 * B * T * S + B * (S * S + S + S * D + 1))
    d_ws = G.workspace("workspace", need)
    Lm.check(L.qt_pose_duration_prior_expect(ctypes.byref(desc), Lm.ptr(d_probs), ld, Lm.ptr(d_sc), Lm.ptr(d_tr), Lm.ptr(d_init),
                                             Lm.ptr(d_dur), Lm.ptr(d_open), Lm.ptr(d_len), *[Lm.ptr(t) for t in acc], Lm.ptr(d_ws),
                                             need, Lm.stream_ptr()), "qt_pose_duration_prior_expect")
    G.check()
    return _numpy(acc)


def run_posterior(dev, probs, sc, tr, dur, init=None, dur_open=None, lengths=None):
    """(log2_evidence [B], dur_counts [S,D]) of qt_pose_duration_posterior on the same inputs, from zero"""
    M, Lm, L = _api()
    B, T, C = probs.shape
    S, D = np.shape(dur)
    up = lambda a: None if a is None else _i32(a).to(dev)
    d_probs = torch.from_numpy(np.array(probs, F32)).to(dev)
    tabs = [up(a) for a in (sc, tr, init, dur, dur_open, lengths)]
    ev = torch.empty(B, dtype=torch.float64, device=dev)
    counts = torch.zeros(S, D, dtype=torch.float64, device=dev)
    desc = M.PoseDurationDesc(B, T, C, S, D)
    need = L.qt_pose_duration_posterior_workspace_bytes(ctypes.byref(desc))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    Lm.check(L.qt_pose_duration_posterior(ctypes.byref(desc), Lm.ptr(d_probs), C, *[Lm.ptr(t) for t in tabs], None, None, None,
                                          Lm.ptr(ev), Lm.ptr(counts), Lm.ptr(ws), need, Lm.stream_ptr()),
             "qt_pose_duration_posterior")
    return ev.cpu().numpy(), counts.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(S, C, D, T, batch, lens=None, with_init=False):
    """seeded probabilities with, where the stream is long enough, a NaN row, a row of zeros, rows of equal probabilities and a
    saturated 1.0, the tables, and their references (float64, mixed); computed once, shared, never written"""
    probs = R.make_probs(1000 * S + 10 * C + batch + D, batch, T, C)
    if T >= 6:
        probs[0, T // 2] = np.nan
        probs[-1, T // 3] = 0.0
        probs[0, 1] = F32(1.0 / C)
        probs[-1, T - 2:] = F32(0.25)
        probs[0, 4] = 0.0
        probs[0, 4, C // 2] = 1.0
    sc, tr = chain(S, C)
    dur, open_ = durations(S, D)
    init = init_for(S) if with_init else None
    lengths = None if lens is None else np.array({"ragged": [T, 1, T // 2 + 1], "equal": [T - 1] * 3}[lens][:batch], np.int32)
    args = (probs, sc, tr, dur, init, open_, lengths)
    ref64, mixed = A.loops64(*args), A.loops_mixed(*args)
    for a in (probs, sc, tr, dur, open_) + ref64 + mixed:
        a.setflags(write=False)
    return args, ref64, mixed


def errors(got, ref64):
    """the three counts' errors relative to max(1, count), the evidence's relative to max(1, |Z|)"""
    es = [float((np.abs(g - w) / np.maximum(1.0, w)).max()) for g, w in zip(got[:3], ref64[:3])]
    return es + [float(abs(got[3][0] - ref64[3][0]) / max(1.0, abs(ref64[3][0])))]


def within_bound(got, ref64, mixed, what):
    for g in got:
        assert np.isfinite(g).all(), (what, "not finite")
    assert got[3][1] == ref64[3][1], (what, "frames")
    share = 0.0
    for name, e_k, e_m in zip(OUT, errors(got, ref64), errors(mixed, ref64)):
        bound = FACTOR * e_m + FLOOR
        share = max(share, e_k / bound)
        print(f"pose_duration_prior {what}: {name} kernel {e_k:.3e} mixed {e_m:.3e} share of the bound {e_k / bound:.3f}")
        assert e_k <= bound, (what, name, e_k, e_m)
    print(f"pose_duration_prior {what}: largest share of the bound {share:.3f}")


def same(got, want, what):
    for name, g, w in zip(OUT, got, want):
        if g is not None and w is not None:
            assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
            assert R.bits(g) == R.bits(w), (what, name, int((g != w).sum()), np.argwhere(g != w)[:4].tolist())


# (S, C, D, T, batch, lengths, init given, ld - C)
SHAPES = [(1, 1, 1, 1, 1, None, False, 0),                 # the smallest
          (2, 2, 2, 2, 1, None, True, 0),                  # one transition, no uncut segment
          (2, 2, 2, 3, 1, None, False, 1),                 # the first uncut segment
          (16, 12, 8, 70, 1, None, True, 3),               # 16 lanes per state, its last size
          (17, 12, 8, 70, 3, "equal", False, 0),           # 4 lanes per state, its first size
          (12, 12, 64, 3 * 64 + 5, 3, "ragged", True, 3),  # the ring wraps three times; lengths frames, 1 and in between
          (64, 64, 128, 300, 1, None, True, 1)]            # the LDS limit is raised, 16 xi slots per lane


@pytest.mark.parametrize("S,C,D,T,batch,lens,with_init,pad", SHAPES)
def test_accuracy_against_the_float64_loops(S, C, D, T, batch, lens, with_init, pad):
    dev = _dev()
    args, ref64, mixed = case(S, C, D, T, batch, lens, with_init)
    got = run(dev, *args, ld=C + pad)
    within_bound(got, ref64, mixed, (S, C, D, T))
    assert abs(got[1].sum() - batch) <= 1e-5 * batch              # (f32 terms: a term near 1 is off by about 1e-7 of itself)
    if T == 1:
        assert not got[0].any()
    if T <= 2:
        assert not got[2].any()
    # the posterior's kernel on the same inputs: the same sweeps, so the same bits
    ev, counts = run_posterior(dev, *args)
    total = np.float64(0)
    for z in ev:
        total = total + z
    assert R.bits(got[2]) == R.bits(counts) and R.bits(got[3][:1]) == R.bits(np.array([total]))


def test_repeats_a_stream_alone_and_accumulation():
    """the same call twice gives the same bits; a stream alone gives its partial of the batch: per-stream calls summed in
    stream order are the batch's bits; the accumulators are added to, not overwritten; start_counts may be NULL"""
    dev = _dev()
    for S, C, D, T in ((12, 12, 16, 150), (17, 12, 5, 70)):
        args, ref64, mixed = case(S, C, D, T, 3, "ragged", True)
        probs, sc, tr, dur, init, open_, lengths = args
        first = run(dev, *args)
        within_bound(first, ref64, mixed, (S, T))
        same(run(dev, *args), first, (S, T, "again"))
        total = [np.zeros_like(a) for a in first]
        for b, n in enumerate(lengths):
            alone = run(dev, probs[b:b + 1, :n], sc, tr, dur, init, open_)
            for acc, a in zip(total, alone):
                acc += a                                                             # ascending stream, from zero
        same(tuple(total), first, (S, T, "alone"))
        rng = np.random.default_rng(S)
        before = (rng.random((S, S)) * 8, rng.random(S), np.arange(S * D, dtype=np.float64).reshape(S, D) / 8, np.array([-3.5, 7.0]))
        added = run(dev, *args, before=before)
        same(added, tuple(b + f for b, f in zip(before, first)), (S, T, "added to"))
        without = run(dev, *args, start_counts=False)
        assert without[1] is None
        same(without, first, (S, T, "no start_counts"))


# ---- hard counts ------------------------------------------------------------------------------------------------------------------
def run_count(dev, path, S, D, start=None, lengths=None, ld=None, before=None):
    M, Lm, L = _api()
    B, T = path.shape
    ld = T if ld is None else ld

    def padded(a):
        if a is None:
            return None
        whole = np.full((B, ld), S // 2, np.int64)                         # a valid step behind every row: it must not count
        whole[:, :T] = a
        return torch.from_numpy(whole)[:, :T]

    G = Guard(dev)
    d_path, d_start, d_len = G.input("path", padded(path)), G.input("start", padded(start)), G.input("lengths", _i32(lengths))
    acc = _accumulators(G, S, D, before)
    desc = M.PoseDurationDesc(B, T, 1, S, D)
    need = L.qt_pose_duration_prior_workspace_bytes(ctypes.byref(desc))
    d_ws = G.workspace("workspace", need)
    Lm.check(L.qt_pose_duration_prior_count_paths(ctypes.byref(desc), Lm.ptr(d_path), Lm.ptr(d_start), ld, Lm.ptr(d_len),
                                                  *[Lm.ptr(t) for t in acc], Lm.ptr(d_ws), need, Lm.stream_ptr()),
             "qt_pose_duration_prior_count_paths")
    G.check()
    return _numpy(acc)


def test_hard_counts_are_the_integer_loops():
    dev = _dev()
    Pk = pkg()
    # runs of labelled steps, labels outside [0, S), ragged, more than one chunk of 1024 frames, a row stride
    S, D = 7, 6
    rng = np.random.default_rng(11)
    path = np.repeat(rng.integers(-1, S + 1, (3, 800)), 3, axis=1)[:, :2100].astype(np.int64)
    path[0, 1020:1030] = np.arange(10) % S
    lengths = np.array([2100, 1, 1025], np.int32)
    for lens in (None, lengths):
        got = run_count(dev, path, S, D, None, lens, ld=2104)
        same(got, A.count_paths(path, S, D, None, lens), ("runs", lens is None))
        device = Pk.PoseDurationDecoder(*R.cyclic_prior(range(S), -10, -100), np.zeros((S, D), np.int32), dev).count_durations(
            torch.from_numpy(path).to(dev), None if lens is None else torch.from_numpy(lens).to(dev))
        assert R.bits(got[2]) == R.bits(device.cpu().numpy().astype(np.float64))           # qt_pose_duration_count
    before = (np.full((S, S), 2.5), np.full(S, 0.25), np.full((S, D), 1.5), np.array([-9.0, 4.0]))
    added = run_count(dev, path, S, D, None, lengths, before=before)
    same(added, tuple(b + c for b, c in zip(before, A.count_paths(path, S, D, None, lengths))), "added to")
    assert added[3][0] == -9.0                                                             # the evidence is left alone
    # the decoder's segments: holds of 20 frames under D = 8 are joined segments, which count on the diagonal
    S = C = 4
    D = 8
    probs, _ = Q.make_tracks(2, 3, 90, C, run=20)
    sc, tr = R.cyclic_prior(range(S), -20, -300, other=-3000)
    dur = Q.hold_prior(S, D, 2, D, inside=-10, outside=-4000)
    lengths = np.array([90, 47, 1], np.int32)
    dec = Pk.PoseDurationDecoder(sc, tr, dur, dev, streams=3)
    d_path, _, d_start = dec.decode(torch.from_numpy(probs).to(dev), lengths=torch.from_numpy(lengths).to(dev), start=True)
    path, start = d_path.cpu().numpy(), d_start.cpu().numpy()
    got = run_count(dev, path, S, D, start, lengths)
    same(got, A.count_paths(path, S, D, start, lengths), "segments")
    assert np.diag(got[0]).sum() >= 5 and got[2].sum() >= 5
    path[0, 30:40] = -1                                                    # entries outside [0, S) count nowhere
    same(run_count(dev, path, S, D, start, lengths, ld=93), A.count_paths(path, S, D, start, lengths), "segments, labels missing")


# ---- the M-step -------------------------------------------------------------------------------------------------------------------
def run_update(dev, tc, st, dc, tr, init, dur, pseudo, dur_pseudo, in_place=False, with_open=True):
    """(trans, init or None, dur, dur_open or None) of qt_pose_duration_prior_update, and qt_pose_prior_update's (trans, init) on
    the same counts"""
    M, Lm, L = _api()
    S, D = dur.shape
    G = Guard(dev)
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))
    d_tc, d_st, d_dc = G.input("trans_counts", f64(tc)), G.input("start_counts", f64(st)), G.input("dur_counts", f64(dc))
    d_allowed = G.input("allowed", _i32(tr > R.TRANS_FLOOR))
    d_dur_allowed = G.input("dur_allowed", _i32(dur > R.TRANS_FLOOR))
    if in_place:
        d_tr = d_tr_out = G.output("trans", (S, S), torch.int32, fill=0)
        d_dur = d_dur_out = G.output("dur", (S, D), torch.int32, fill=0)
        d_init = d_init_out = None if init is None else G.output("init", (S,), torch.int32, fill=0)
        d_tr.copy_(_i32(tr)), d_dur.copy_(_i32(dur))
        if init is not None:
            d_init.copy_(_i32(init))
    else:
        d_tr, d_dur, d_init = G.input("trans_in", _i32(tr)), G.input("dur_in", _i32(dur)), G.input("init_in", _i32(init))
        d_tr_out, d_dur_out = G.output("trans_out", (S, S), torch.int32, fill=0), G.output("dur_out", (S, D), torch.int32, fill=0)
        d_init_out = None if init is None else G.output("init_out", (S,), torch.int32, fill=0)
    d_open = G.output("dur_open_out", (S, D), torch.int32, fill=0) if with_open else None
    Lm.check(L.qt_pose_duration_prior_update(S, D, Lm.ptr(d_tc), Lm.ptr(d_st), Lm.ptr(d_dc), Lm.ptr(d_allowed), Lm.ptr(d_dur_allowed),
                                             pseudo, dur_pseudo, Lm.ptr(d_tr), Lm.ptr(d_init), Lm.ptr(d_dur), Lm.ptr(d_tr_out),
                                             Lm.ptr(d_init_out), Lm.ptr(d_dur_out), Lm.ptr(d_open), Lm.stream_ptr()),
             "qt_pose_duration_prior_update")
    G.check()
    plain_tr = torch.zeros(S, S, dtype=torch.int32, device=dev)
    plain_init = None if init is None else torch.zeros(S, dtype=torch.int32, device=dev)
    old_tr, old_init = _i32(tr).to(dev), None if init is None else _i32(init).to(dev)
    Lm.check(L.qt_pose_prior_update(S, Lm.ptr(d_tc), Lm.ptr(d_st), Lm.ptr(d_allowed), pseudo, Lm.ptr(old_tr), Lm.ptr(old_init),
                                    Lm.ptr(plain_tr), Lm.ptr(plain_init), Lm.stream_ptr()), "qt_pose_prior_update")
    torch.cuda.synchronize(dev)
    return _numpy((d_tr_out, d_init_out, d_dur_out, d_open)), _numpy((plain_tr, plain_init))


@pytest.mark.parametrize("S,D", [(1, 1), (5, 24), (64, 128)])
def test_m_step(S, D):
    dev = _dev()
    rng = np.random.default_rng(S + D)
    tc, st, dc = rng.random((S, S)) * 40, rng.random(S), rng.random((S, D)) * 3
    sc, tr = R.cyclic_prior(range(S), -39, -300, skip=-800 if S > 2 else None, other=R.TRANS_FLOOR)
    dur = (-rng.integers(0, 2000, (S, D))).astype(np.int32)
    if D > 2:
        dur[rng.random((S, D)) < 0.2] = R.TRANS_FLOOR
        dur[:, 1] = -5                                                   # (no row without an allowed length)
        dc[S // 2] = 0                                                   # an empty row
        dc[0, 2:] = 0
    init = init_for(S)
    for pseudo, dur_pseudo in ((0.25, 0.01), (0.0, 0.0), (1.0, 1.0)):
        (new_tr, new_init, new_dur, new_open), (plain_tr, plain_init) = run_update(dev, tc, st, dc, tr, init, dur, pseudo, dur_pseudo)
        assert R.bits(new_tr) == R.bits(plain_tr) and R.bits(new_init) == R.bits(plain_init)         # qt_pose_prior_update's bits
        want = A.dur_rows(dc, dur, None, dur_pseudo).astype(np.int32)
        assert R.bits(new_dur) == R.bits(want), (pseudo, np.argwhere(new_dur != want)[:4].tolist())
        assert R.bits(new_open) == R.bits(A.suffix_max(want))
        assert (new_dur[dur == R.TRANS_FLOOR] == R.TRANS_FLOOR).all()
        if dur_pseudo == 0 and D > 2:
            assert R.bits(new_dur[S // 2]) == R.bits(dur[S // 2])                                  # the empty row keeps dur_in
        again, _ = run_update(dev, tc, st, dc, tr, init, dur, pseudo, dur_pseudo, in_place=True)
        for g, w in zip(again, (new_tr, new_init, new_dur, new_open)):
            assert R.bits(g) == R.bits(w)
        bare, _ = run_update(dev, tc, st, dc, tr, None, dur, pseudo, dur_pseudo, with_open=False)
        assert bare[1] is None and bare[3] is None and R.bits(bare[0]) == R.bits(new_tr) and R.bits(bare[2]) == R.bits(new_dur)
    if D > 2:                                                            # every entry allowed: expected_duration_prior itself
        free = np.full((S, D), -700, np.int32)
        (_, _, new_dur, _), _ = run_update(dev, tc, st, dc + 0.125, tr, init, free, 0.0, 0.5)
        assert R.bits(new_dur) == R.bits(pkg().expected_duration_prior(dc + 0.125, 0.5))


# ---- the class --------------------------------------------------------------------------------------------------------------------
def test_the_learner_fits_and_hands_its_tables_over_without_a_host_sync():
    """seed 0 of the learning test (tests/test_pose_duration_prior_cpu.py) on the device: `fit` under torch's sync debug mode and
    on a stream that is not the default one; the evidence per frame after four iterations exceeds the start's by at least half
    the rise the float64 reference shows (a table entry moves by 1/256 bit under f32 rounding, which cannot eat half); the modal
    lengths are the reference's; load_tables into the three users, which then give the bits of freshly made ones"""
    dev = _dev()
    Pk = pkg()
    probs, _ = Q.make_tracks(0, 6, 160, 6, run=9)
    sc, tr = R.cyclic_prior(range(6), stay=R.TRANS_FLOOR, advance=-64, skip=-1024, other=R.TRANS_FLOOR)
    dur = np.full((6, 24), -1174, np.int32)
    ref = A.fit([(probs, None)], sc, tr, dur, iterations=4, pseudo_count=0.0, dur_pseudo_count=0.01)
    ref_rise = ref[4][4][0] / ref[4][4][1] - ref[4][0][0] / ref[4][0][1]
    d_probs = torch.from_numpy(probs).to(dev)
    learner = Pk.PoseDurationLearner(sc, tr, dur, dev, pseudo_count=0.0, dur_pseudo_count=0.01)
    bits, frames = learner.zero().accumulate(d_probs).totals()
    assert frames == 6 * 160
    first = bits / frames
    users = (Pk.PoseDurationDecoder(sc, tr, dur, dev, streams=6), Pk.PoseDurationPosterior(sc, tr, dur, dev, streams=6),
             Pk.PoseDurationLagDecoder(sc, tr, dur, dev, lag=8, streams=6))
    users[2].push(d_probs[:, :5])                                       # a stream under way: load_tables starts it anew
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(side):
            learner.fit([d_probs], 2)
            learner.fit([(d_probs, None)], 2)
            learner.zero().accumulate(d_probs)
            for user in users:
                assert user.load_tables(learner.trans, learner.init, learner.dur, learner.dur_open) is user
    finally:
        torch.cuda.set_sync_debug_mode("default")
    side.synchronize()
    assert users[2].seen == 0
    bits, frames = learner.totals()
    rise = bits / frames - first
    print(f"pose_duration_prior learner: evidence per frame {first:.4f} -> {bits / frames:.4f}, rise {rise:.4f}, float64 reference "
          f"{ref_rise:.4f}")
    assert rise >= 0.5 * ref_rise and ref_rise >= 0.4
    _, new_tr, new_init, new_dur, new_open = learner.tables()
    assert new_init is None and new_tr.dtype == np.int32 and new_dur.shape == (6, 24)
    assert (new_dur.argmax(axis=1) == ref[2].argmax(axis=1)).all() and (new_dur.argmax(axis=1) + 1 == 9).all()
    assert R.bits(new_open) == R.bits(A.suffix_max(new_dur)) and (new_tr[tr == R.TRANS_FLOOR] == R.TRANS_FLOOR).all()
    fresh = (Pk.PoseDurationDecoder(sc, new_tr, new_dur, dev, streams=6, dur_open=new_open),
             Pk.PoseDurationPosterior(sc, new_tr, new_dur, dev, streams=6, dur_open=new_open),
             Pk.PoseDurationLagDecoder(sc, new_tr, new_dur, dev, lag=8, streams=6, dur_open=new_open))
    for loaded, made in zip(users, fresh):
        if isinstance(loaded, Pk.PoseDurationDecoder):
            got, want = loaded.decode(d_probs, start=True, score=True), made.decode(d_probs, start=True, score=True)
        elif isinstance(loaded, Pk.PoseDurationPosterior):
            got, want = loaded.smooth(d_probs, begin=True, evidence=True), made.smooth(d_probs, begin=True, evidence=True)
        else:
            got, want = loaded.push(d_probs, flush=True, start=True)[1:], made.push(d_probs, flush=True, start=True)[1:]
        for g, w in zip(got, want):
            assert torch.equal(g, w), type(loaded).__name__
    # ragged batches, hard counts and the refusals of the class
    lengths = np.array([160, 1, 81, 160, 7, 33], np.int32)
    d_len = torch.from_numpy(lengths).to(dev)
    ragged = Pk.PoseDurationLearner(sc, tr, dur, dev, init=init_for(6), dur_open=None, learn_init=True)
    ragged.accumulate(d_probs, d_len)
    want = run(dev, probs, sc, tr, dur, init_for(6), None, lengths)
    same((ragged.counts.cpu().numpy(), ragged.start_counts.cpu().numpy(), ragged.dur_counts.cpu().numpy(),
          ragged._totals.cpu().numpy()), want, "the class, ragged")
    ragged.update()
    assert ragged.dur_open is None and ragged.tables()[2].shape == (6,)
    path, _, start = users[0].decode(d_probs, lengths=d_len, start=True)
    hard = Pk.PoseDurationLearner(sc, tr, dur, dev)
    hard.accumulate_paths(path, start, d_len).accumulate_paths(path[0], None)
    both = [a + b for a, b in zip(A.count_paths(path.cpu().numpy(), 6, 24, start.cpu().numpy(), lengths),
                                  A.count_paths(path[:1].cpu().numpy(), 6, 24))]
    same((hard.counts.cpu().numpy(), hard.start_counts.cpu().numpy(), hard.dur_counts.cpu().numpy(), hard._totals.cpu().numpy()),
         tuple(both), "the class, hard counts")
    for bad in (lambda: learner.accumulate(d_probs.cpu()), lambda: learner.accumulate(d_probs.double()),
                lambda: learner.accumulate(d_probs[:, :0]), lambda: learner.accumulate(d_probs, d_len[:2]),
                lambda: learner.accumulate(d_probs, d_len.long()), lambda: learner.accumulate_paths(path.int()),
                lambda: learner.accumulate_paths(path, start[:, :5]), lambda: learner.accumulate_paths(path.cpu()),
                lambda: users[0].load_tables(learner.trans.long()), lambda: users[0].load_tables(learner.trans, None, learner.dur[:, :5]),
                lambda: users[0].load_tables(learner.trans, None, None, learner.dur_open),
                lambda: users[1].load_tables(learner.trans.cpu())):
        with pytest.raises(Pk.QtError):
            bad()
    with pytest.raises(ValueError):
        learner.fit([d_probs], -1)
    kept = users[1].dur.clone()
    users[1].load_tables(learner.trans)                                 # dur None: the current table stays
    assert torch.equal(users[1].dur, kept) and users[1].init is None
