"""Pose-order decoding with hold durations on the GPU (csrc/pose_duration.hip, <pkg>/pose_order.py): qt_pose_duration_decode and
qt_pose_duration_count against the plain loops of tests/_pose_duration_ref.py, through ctypes and through PoseDurationDecoder.
Every number is an integer from the emission score on, so every output is compared for equality of bytes, at the sizes where
the lane groups (S around 16), the ring (frames around D and several times D), the emission chunks of 64 frames and ragged
lengths can go wrong.  Every buffer sits between poisoned guard bands (tests/_guard.py), the workspace is exactly the queried
size and poisoned, the padding columns of ld > C are NaN, and the inputs must come back byte for byte."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _pose_duration_ref as Q
import _pose_order_ref as R
from _guard import Guard
from _util import pkg

pytestmark = pytest.mark.gpu
F32 = np.float32


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _api():
    M, Lm = pkg("pose_order"), pkg("_lib")
    return M, Lm, Lm.lib()


def chain(S, C):
    """a loose left-to-right cycle over S states, state s emitting class s mod C (for S = 2 of C = 64 two far-apart classes)"""
    classes = [5, 40] if (C, S) == (64, 2) else [s % C for s in range(S)]
    return R.cyclic_prior(classes, -39, -300, skip=-800, other=-3000)


def init_for(S):
    return ((np.arange(S, dtype=np.int64) * 977) % 4001 - 4000).astype(np.int32)


def durations(S, D, seed=0):
    """(dur, dur_open) int32 [S, D]: seeded scores in [-500, 0] so that many lengths compete, some lengths forbidden, equal
    neighbours (ties between lengths); dur_open a table of its own, not the suffix maximum"""
    rng = np.random.default_rng(100 * S + D + seed)
    dur = -rng.integers(0, 501, (S, D))
    dur[rng.random((S, D)) < 0.15] = R.TRANS_FLOOR
    dur[:, 1::4] = dur[:, 0::4][:, :dur[:, 1::4].shape[1]]
    open_ = np.maximum(Q.suffix_max(dur), -rng.integers(0, 60, (S, D)))
    return dur.astype(np.int32), open_.astype(np.int32)


def run(dev, probs, sc, tr, dur, init=None, dur_open=None, lengths=None, ld=None, want_start=True, want_score=True):
    """qt_pose_duration_decode through ctypes.  probs f32 [B,T,C]; ld: row stride (columns C .. ld - 1 are NaN).  Returns
    (path, start or None, score or None) as numpy."""
    M, Lm, L = _api()
    B, T, C = probs.shape
    S, D = np.shape(dur)
    ld = C if ld is None else ld
    padded = np.full((B, T, ld), np.nan, F32)
    padded[..., :C] = probs
    G = Guard(dev)
    i32 = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int32))
    d_probs = G.input("probs", torch.from_numpy(padded))
    d_sc, d_tr, d_init = G.input("state_class", i32(sc)), G.input("trans", i32(tr)), G.input("init", i32(init))
    d_dur, d_open, d_len = G.input("dur", i32(dur)), G.input("dur_open", i32(dur_open)), G.input("lengths", i32(lengths))
    d_path = G.output("path", (B, T), torch.int64)
    d_start = G.output("start", (B, T), torch.int64) if want_start else None
    d_score = G.output("score", (B,), torch.int64) if want_score else None
    desc = M.PoseDurationDesc(B, T, C, S, D)
    need = L.qt_pose_duration_workspace_bytes(ctypes.byref(desc))
    assert need == (B * T * S * 2 + 7) // 8 * 8
    d_ws = G.workspace("workspace", need)
    Lm.check(L.qt_pose_duration_decode(ctypes.byref(desc), Lm.ptr(d_probs), ld, Lm.ptr(d_sc), Lm.ptr(d_tr), Lm.ptr(d_init),
                                       Lm.ptr(d_dur), Lm.ptr(d_open), Lm.ptr(d_len), Lm.ptr(d_path), Lm.ptr(d_start),
                                       Lm.ptr(d_score), Lm.ptr(d_ws), need, Lm.stream_ptr()), "qt_pose_duration_decode")
    G.check()
    return (d_path.cpu().numpy(), d_start.cpu().numpy() if want_start else None, d_score.cpu().numpy() if want_score else None)


def same(got, ref, what):
    for name, g, w in zip(("path", "start", "score"), got, ref):
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
            assert R.bits(g) == R.bits(w), (what, name, int((g != w).sum()), np.argwhere(g != w)[:4].tolist())


@functools.lru_cache(maxsize=None)
def tracks(batch, frames, C):
    """seeded probabilities with, where the stream is long enough, a NaN row, a row of zeros and rows of equal probabilities;
    computed once, shared, never written"""
    probs = R.make_probs(10 * C + batch + 1000 * frames, batch, frames, C)
    if frames >= 6:
        probs[0, frames // 2] = np.nan
        probs[-1, frames // 3] = 0.0
        probs[0, 1] = F32(1.0 / C)
        probs[-1, frames - 2:] = F32(0.25)
    probs.setflags(write=False)
    return probs


# (S, D, C, batch, init given, dur_open given, lengths: None / "equal" / "ragged", ld - C): a pairwise selection
SHAPES = [(1, 1, 1, 1, False, False, None, 0), (2, 2, 12, 3, True, True, "ragged", 3), (12, 63, 12, 3, False, True, "equal", 1),
          (16, 64, 64, 1, True, False, None, 0), (17, 65, 12, 3, True, True, "ragged", 5), (64, 128, 64, 1, False, True, None, 0),
          (12, 128, 1, 3, True, False, "ragged", 2), (64, 1, 12, 3, True, False, "equal", 0), (17, 2, 64, 1, False, True, None, 1),
          (1, 64, 12, 3, True, True, "equal", 4), (2, 128, 1, 1, False, False, None, 0), (16, 65, 1, 3, False, True, "ragged", 1),
          (64, 63, 1, 1, True, False, None, 3), (12, 2, 64, 3, False, False, "ragged", 0), (2, 64, 64, 3, False, True, "ragged", 0),
          (16, 1, 12, 1, True, True, None, 2), (64, 65, 12, 3, False, False, "equal", 0), (1, 128, 64, 3, True, False, "ragged", 1)]


@pytest.mark.parametrize("S,D,C,batch,with_init,with_open,lens,pad", SHAPES)
def test_bits_equal_the_rule(S, D, C, batch, with_init, with_open, lens, pad):
    """frames: one; D - 1, D and D + 1 (the ring before its first wrap and at it), 2 D + 3 and 300 (after several, and across
    the emission chunks of 64).  S: 12 as in the model, 16 and 17 around the lane groups' switch, 1, 2, 64."""
    dev = _dev()
    sc, tr = chain(S, C)
    dur, open_ = durations(S, D)
    for T in sorted({1, D - 1, D, D + 1, 2 * D + 3, 300} - {0}):
        probs = tracks(batch, T, C)
        lengths = None if lens is None or batch == 1 else np.array([max(1, T - 1)] * 3 if lens == "equal" else [T, 1, T // 2 + 1], np.int32)
        args = (sc, tr, dur, init_for(S) if with_init else None, open_ if with_open else None, lengths)
        same(run(dev, probs, *args, ld=C + pad), Q.decode(probs, *args), (S, D, T))


@pytest.mark.parametrize("mixed", [False, True])
def test_saturated_tables(mixed):
    """every emission at -8192 and every table at -65536 for 4 D + 5 frames of 64 states and D = 128 (the ring wraps four
    times while every score falls at the fastest rate there is); and the same with one state whose rows of trans and dur
    are all zeros"""
    dev = _dev()
    S, D, C = 64, 128, 64
    T = 4 * D + 5
    probs = np.zeros((1, T, C), F32)
    sc = np.arange(S, dtype=np.int32)
    tr, init, dur = np.full((S, S), -65536, np.int32), np.full(S, -65536, np.int32), np.full((S, D), -65536, np.int32)
    if mixed:
        tr[37], dur[37] = 0, 0
    ref = Q.decode(probs, sc, tr, dur, init)
    if mixed:
        assert set(ref[0][0].tolist()) == {37} and ref[2][0] == -8192 * T - 65536         # nothing but init is paid for
    else:                                          # beta[0] is two floors, then five segments (4 x 128 + 5) and four joins
        assert ref[2][0] == -8192 * T - 65536 * (2 + 5 + 4)
    same(run(dev, probs, sc, tr, dur, init), ref, ("saturated", mixed))
    same(run(dev, probs, sc, tr, dur, init, dur_open=np.zeros_like(dur)), Q.decode(probs, sc, tr, dur, init, np.zeros_like(dur)),
         ("saturated, open", mixed))


def test_special_probabilities_and_a_class_out_of_range():
    dev = _dev()
    S = C = 12
    D, T = 9, 70
    one = F32(1.0)
    probs = np.array(tracks(2, T, C))
    values = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-42, 2.0 ** -32, np.nextafter(F32(2.0 ** -32), F32(0)), 1.0, 1.5, -0.5, 3e38]
    probs[0, 3:3 + len(values), 4] = values
    probs[1, 20:20 + len(values), :] = np.array(values, F32)[:, None]
    probs[1, 40:44] = np.nan
    probs[0, 50:60] = F32(0.125)
    sc, tr = chain(S, C)
    dur, open_ = durations(S, D, seed=1)
    same(run(dev, probs, sc, tr, dur, None, open_), Q.decode(probs, sc, tr, dur, None, open_), "special")
    bad = np.array(sc)
    bad[3], bad[9], bad[11] = C, -1, 2 ** 31 - 1
    ref = Q.decode(probs, bad, tr, dur, None, open_)
    same(run(dev, probs, bad, tr, dur, None, open_), ref, "state_class")
    assert R.bits(ref[0]) != R.bits(Q.decode(probs, sc, tr, dur, None, open_)[0])


def test_tables_out_of_range_are_clamped():
    """trans, init, dur and dur_open outside [-65536, 0] (ctypes only: the module refuses them); lengths outside 1 .. frames"""
    dev = _dev()
    S = C = 12
    D, T = 20, 90
    probs = tracks(3, T, C)
    sc, tr = chain(S, C)
    dur, open_ = durations(S, D, seed=2)
    tr, dur, open_, init = np.array(tr), np.array(dur), np.array(open_), init_for(S)
    tr[0, 1], tr[3, 4], tr[5, 5], tr[7, 2] = 5, 2 ** 31 - 1, -2 ** 31, -65537
    dur[0, 3], dur[2, 7], dur[4, 0], dur[11, 19] = 9, 2 ** 31 - 1, -2 ** 31, -65537
    open_[1, 2], open_[3, 3], open_[5, 19] = 1, -2 ** 31, 2 ** 31 - 1
    init[2], init[4] = 77, -10 ** 9
    lengths = np.array([T + 1, -5, 2 ** 31 - 1], np.int32)
    ref = Q.decode(probs, sc, tr, dur, init, open_, lengths)
    same(run(dev, probs, sc, tr, dur, init, open_, lengths), ref, "clamped")
    clip = lambda a: np.clip(a, -65536, 0)
    same(ref, Q.decode(probs, sc, clip(tr), clip(dur), clip(init), clip(open_), np.array([T, 1, T], np.int32)), "the rule clamps")
    same(run(dev, probs, sc, tr, dur, init, open_, np.array([0, T, 5], np.int32)),
         Q.decode(probs, sc, tr, dur, init, open_, np.array([1, T, 5], np.int32)), "lengths")


def test_optional_outputs_repeats_and_a_stream_alone():
    """start and score NULL; the same call twice gives the same bits; a stream alone equals itself in a batch, and a stream
    with lengths[b] = L equals the call on its first L frames"""
    dev = _dev()
    for S, D, T in ((12, 16, 150), (17, 5, 70)):
        C = S
        probs = tracks(3, T, C)
        sc, tr = chain(S, C)
        dur, open_ = durations(S, D, seed=3)
        init = init_for(S)
        lengths = np.array([T // 3, T, 66], np.int32)
        ref = Q.decode(probs, sc, tr, dur, init, open_, lengths)
        first = run(dev, probs, sc, tr, dur, init, open_, lengths)
        same(first, ref, (S, T))
        same(run(dev, probs, sc, tr, dur, init, open_, lengths), first, (S, T, "again"))
        same(run(dev, probs, sc, tr, dur, init, open_, lengths, want_start=False, want_score=False), ref, (S, T, "path only"))
        for b, n in enumerate(lengths):
            alone = run(dev, probs[b:b + 1, :n], sc, tr, dur, init, open_)
            same(alone, tuple(r[b:b + 1, :n] if r.ndim == 2 else r[b:b + 1] for r in ref), (S, T, "alone", b))


@pytest.mark.parametrize("D", [1, 2, 7, 128])
def test_geometric_durations_score_what_qt_pose_order_decode_scores(D):
    """on the device, against the plain decoder's own kernels (short route and tiled route): the best score for every D, and
    at D = 1 with a table of zeros the path, byte for byte"""
    dev = _dev()
    P, M = pkg(), pkg("pose_order")
    stay = M.prob_score(0.9)
    for S, C, B, T in ((12, 12, 2, 50), (17, 12, 1, 150), (6, 5, 3, 300)):
        probs = tracks(B, T, C)
        sc, tr = R.cyclic_prior([s % C for s in range(S)], stay, -850, skip=-3000, other=-20000)
        init = init_for(S)
        d_probs = torch.from_numpy(np.array(probs)).to(dev)
        plain = P.PoseOrderDecoder(sc, tr, dev, streams=B, init=init)
        plain_path, _ = plain.decode(d_probs)
        geo = P.PoseDurationDecoder(sc, tr, M.geometric_durations(stay, S, D), dev, streams=B, init=init, dur_open=None)
        path, _, score = geo.decode(d_probs, score=True)
        assert score.dtype == torch.int64 and torch.equal(score, plain.carry[:, 1]), (D, S, T)
        if D == 1:
            assert torch.equal(path, plain_path)
        flat = P.PoseDurationDecoder(sc, tr, np.zeros((S, 1), np.int32), dev, streams=B, init=init)
        assert torch.equal(flat.decode(d_probs)[0], plain_path)


def run_count(dev, path, S, D, lengths=None, ld=None, counts=None):
    M, Lm, L = _api()
    B, T = path.shape
    ld = T if ld is None else ld
    padded = np.full((B, ld), 1, np.int64)                       # (a run that would go on behind a row's end)
    padded[:, :T] = path
    G = Guard(dev)
    d_path = G.input("path", torch.from_numpy(padded))
    d_len = G.input("lengths", None if lengths is None else torch.from_numpy(np.ascontiguousarray(lengths, np.int32)))
    d_counts = G.output("counts", (S, D), torch.int64, fill=0)
    if counts is not None:
        d_counts.copy_(torch.from_numpy(counts))
    desc = M.PoseDurationDesc(B, T, 1, S, D)
    Lm.check(L.qt_pose_duration_count(ctypes.byref(desc), Lm.ptr(d_path), ld, Lm.ptr(d_len), Lm.ptr(d_counts), Lm.stream_ptr()),
             "qt_pose_duration_count")
    G.check()
    return d_counts.cpu().numpy()


def test_count_durations():
    """against the walk: seeded paths with entries outside [0, S), runs of D and D + 1, a -1 tail, lengths (ragged, 1, out of
    range), ld_path > frames, more than one workgroup; two calls add up"""
    dev = _dev()
    for seed, (B, T, S, D) in enumerate([(1, 1, 3, 4), (3, 40, 3, 4), (2, 700, 12, 16), (3, 300, 64, 128), (1, 300, 1, 1)]):
        rng = np.random.default_rng(seed)
        path = np.empty((B, T), np.int64)
        for b in range(B):
            f = 0
            while f < T:
                n = int(rng.integers(1, 2 * D + 2))
                path[b, f:f + n] = rng.integers(0, S) if rng.random() > 0.1 else rng.choice([-1, S, 1 << 40])
                f += n
        if T >= 40:
            path[0, 5:5 + D], path[0, 5 + D:6 + 2 * D] = 0, S - 1                  # a run of D and one of D + 1
            path[-1, T - 7:] = -1
        for lengths in (None, np.array([T, 1, T // 2][:B], np.int32), np.array([T + 3, 0, -1][:B], np.int32)):
            for ld in (T, T + 3):
                want = Q.count_durations(path, S, D, lengths)
                got = run_count(dev, path, S, D, lengths, ld)
                assert got.dtype == np.int64 and R.bits(got) == R.bits(want), (B, T, S, D, ld)
        want = Q.count_durations(path, S, D)
        assert R.bits(run_count(dev, path, S, D, counts=want)) == R.bits(2 * want) and (T < 40 or want.sum() > 0)
    hand = np.array([[0, 0, 1, 1, 1, 2, 2, 2, 2, 0, 0, 0, 0, 0, 1, 2, 2]], np.int64)
    assert run_count(dev, hand, 3, 4).tolist() == [[0, 0, 0, 1], [1, 0, 1, 0], [0, 0, 0, 1]]


def test_decoder_class():
    """PoseDurationDecoder: dur_open "suffix_max", a table and None; lengths, start, score, path_class, cycles, [frames, C]
    for one stream, count_durations on its own path; the refusals of CPU tensors and other dtypes"""
    dev = _dev()
    P, M = pkg(), pkg("pose_order")
    C = S = 4
    B, T, D = 2, 200, 12
    rng = np.random.default_rng(11)
    lead = ((np.arange(T)[None, :] + np.array([[0], [7]])) // 8) % C               # a new step every 8 frames
    probs = np.full((B, T, C), F32(0.05), F32)
    np.put_along_axis(probs, lead[..., None], F32(0.85), axis=2)
    probs += rng.uniform(0, 0.01, probs.shape).astype(F32)
    sc, tr = M.cyclic_prior(range(C), stay=M.prob_score(0.9), advance=M.prob_score(0.1))
    dur = M.hold_prior(S, D, 4, 10)
    d_probs = torch.from_numpy(probs).to(dev)
    lengths = np.array([T, 131], np.int32)
    d_len = torch.from_numpy(lengths).to(dev)
    for dur_open, ref_open in (("suffix_max", Q.suffix_max(dur)), (np.zeros_like(dur), np.zeros_like(dur)), (None, None)):
        dec = P.PoseDurationDecoder(sc, tr, dur, dev, streams=B, dur_open=dur_open, class_names=["a", "b", "c", "d"])
        path, path_class, start, score = dec.decode(d_probs, lengths=d_len, start=True, score=True)
        want = Q.decode(probs, sc, tr, dur, None, ref_open, lengths)
        same((path.cpu().numpy(), start.cpu().numpy(), score.cpu().numpy()), want, dur_open if isinstance(dur_open, str) else "table")
        want_class = np.where(want[0] >= 0, sc.astype(np.int64)[np.maximum(want[0], 0)], -1)
        assert path_class.dtype == torch.int64 and R.bits(path_class.cpu().numpy()) == R.bits(want_class)
        rounds = dec.cycles(path)
        assert rounds.dtype == torch.int64 and rounds.cpu().numpy().tolist() == R.cycles(want[0], C - 1, 0)[0].tolist()
        counts = dec.count_durations(path, d_len)
        assert counts.dtype == torch.int64 and R.bits(counts.cpu().numpy()) == R.bits(Q.count_durations(want[0], S, D, lengths))
    assert rounds.cpu().numpy().tolist()[0] >= 5 and int(counts.sum()) > 10
    assert len(dec.decode(d_probs)) == 2 and dec.decode(d_probs, score=True)[2].shape == (B,)
    # labelled steps of any batch size, and the table fitted to them
    labels = torch.from_numpy(lead.astype(np.int64)).to(dev)
    counts = dec.count_durations(torch.cat([labels, labels[:1]]))
    assert R.bits(counts.cpu().numpy()) == R.bits(Q.count_durations(np.concatenate([lead, lead[:1]]), S, D))
    fitted = M.duration_prior(counts.cpu().numpy())
    assert fitted.shape == (S, D) and (fitted.argmax(axis=1) == 7).all()             # every interior hold is 8 frames long
    # one stream, [frames, C]
    single = P.PoseDurationDecoder(sc, tr, dur, dev)
    path, path_class, start = single.decode(d_probs[0, :40], start=True)
    want = Q.decode(probs[:1, :40], sc, tr, dur, None, Q.suffix_max(dur))
    assert path.shape == (40,) and R.bits(path.cpu().numpy()[None]) == R.bits(want[0]) and R.bits(start.cpu().numpy()[None]) == R.bits(want[1])
    assert single.cycles(path, wrap_from=1, wrap_to=2).cpu().numpy().tolist() == R.cycles(want[0], 1, 2)[0].tolist()
    for bad in (lambda: single.decode(d_probs[0, :4].cpu()), lambda: single.decode(d_probs[0, :4].double()),
                lambda: single.decode(d_probs[:, :4]), lambda: single.decode(d_probs[0, :4], lengths=d_len[:1].long()),
                lambda: single.decode(d_probs[0, :4], lengths=d_len[:1].cpu()), lambda: single.decode(d_probs[0, :4], lengths=d_len),
                lambda: single.cycles(path.cpu()), lambda: single.cycles(path.int()), lambda: single.count_durations(path.cpu()),
                lambda: single.count_durations(path.int()), lambda: single.count_durations(path, lengths=d_len)):
        with pytest.raises(P.QtError):
            bad()


def test_a_side_stream_without_a_host_sync():
    """decode, cycles and count_durations under a stream that is not the default one and under torch's sync debug mode (the
    plain decoder's video-loop test checks that one the same way); the results are the loops'"""
    dev = _dev()
    P, M = pkg(), pkg("pose_order")
    S = C = 12
    B, T, D = 2, 140, 24
    probs = np.array(tracks(B, T, C))
    sc, tr = chain(S, C)
    dur, _ = durations(S, D, seed=4)
    lengths = np.array([T, 77], np.int32)
    dec = P.PoseDurationDecoder(sc, tr, dur, dev, streams=B)
    d_probs, d_len = torch.from_numpy(probs).to(dev), torch.from_numpy(lengths).to(dev)
    dec.decode(d_probs)                                                             # (the workspace's first allocation is not the loop's)
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(side):
            path, path_class, start, score = dec.decode(d_probs, lengths=d_len, start=True, score=True)
            rounds = dec.cycles(path)
            counts = dec.count_durations(path, d_len)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    side.synchronize()
    want = Q.decode(probs, sc, tr, dur, None, Q.suffix_max(dur), lengths)
    same((path.cpu().numpy(), start.cpu().numpy(), score.cpu().numpy()), want, "side stream")
    assert rounds.cpu().numpy().tolist() == R.cycles(want[0], S - 1, 0)[0].tolist()
    assert R.bits(counts.cpu().numpy()) == R.bits(Q.count_durations(want[0], S, D, lengths))
