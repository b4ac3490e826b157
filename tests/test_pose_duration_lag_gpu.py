"""Fixed-lag pose-order decoding with hold durations on the GPU (csrc/pose_duration_lag.hip, <pkg>/pose_order.py):
qt_pose_duration_lag_decode against qt_pose_duration_decode on every prefix (both kernels run), against the integer loops of
tests/_pose_duration_lag_ref.py (outputs and the unpacked carry), under splits of the stream into calls, against
qt_pose_lag_decode where the two rules coincide, and through PoseDurationLagDecoder with host synchronisation forbidden.
Everything is an integer, so everything is compared for equality.  Every call through ctypes has its outputs between poisoned
guard bands (tests/_guard.py), a workspace of exactly the queried size and poisoned, a poisoned carry_out, NaN in the padding
columns of ld > C, and inputs (carry_in included) that must come back byte for byte.

Measured on an MI355X (python scripts/bench_pose_duration_lag.py; EXPERIMENTS.md, "Fixed-lag pose durations"), 16 streams, S = 12,
D = 64, lag = 16, medians: a push of 16 x 1 frame 19.8 us (PoseLagDecoder.push on the same frames 16.5 us); a catch-up push of
16 x 4096 frames with flush 10.01 ms (PoseDurationDecoder.decode of the same videos 5.87 ms, PoseLagDecoder.push 1.18 ms).
Context, not thresholds: nothing here asserts a time."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _pose_duration_lag_ref as DL
import _pose_duration_ref as Q
import _pose_lag_ref as G
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
    """a loose left-to-right cycle over S states, state s emitting class s mod C"""
    return R.cyclic_prior([s % C for s in range(S)], -39, -300, skip=-800, other=-3000)


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


def tables(C, S, D, with_init=True, with_open=True):
    """(state_class, trans, dur, init or None, dur_open or None): the arguments of the loops after probs"""
    sc, tr = chain(S, C)
    dur, open_ = durations(S, D)
    return sc, tr, dur, init_for(S) if with_init else None, open_ if with_open else None


@functools.lru_cache(maxsize=None)
def tracks(batch, frames, C):
    """seeded probabilities with a NaN row, a row of zeros and rows of equal probabilities; computed once, shared, never
    written"""
    probs = R.make_probs(10 * C + batch + 1000 * frames, batch, frames, C, run=5)
    if frames >= 6:
        probs[0, frames // 2] = np.nan
        probs[-1, frames // 3] = 0.0
        probs[0, 1] = F32(1.0 / C)
        probs[-1, frames - 2:] = F32(0.25)
    probs.setflags(write=False)
    return probs


def i32(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int32))


def run(dev, probs, tab, lag, seen=0, flush=True, carry=None, pad=0, want=(True, True, True)):
    """one qt_pose_duration_lag_decode through ctypes.  probs f32 [B, n, C] (the call's new frames); carry: the carry_out
    bytes of the call before (uint8 [B, stride]) or None at seen == 0; pad: ld - C; want: lag_start, filtered, score.
    Returns ((lag_path, lag_start, filtered, score) as numpy or None, carry_out bytes)."""
    M, Lm, L = _api()
    sc, tr, dur, init, open_ = tab
    B, n, C = probs.shape
    S, D = dur.shape
    ld = C + pad
    g0, g1 = G.span(seen, n, lag, flush)
    count = g1 - g0
    padded = np.full((B, n, ld), np.nan, F32)
    padded[..., :C] = probs
    gd = Guard(dev)
    d_probs = gd.input("probs", torch.from_numpy(padded)) if n else None
    d_sc, d_tr, d_init = gd.input("state_class", i32(sc)), gd.input("trans", i32(tr)), gd.input("init", i32(init))
    d_dur, d_open = gd.input("dur", i32(dur)), gd.input("dur_open", i32(open_))
    desc = M.PoseDurationLagDesc(B, n, C, S, D, lag, int(flush), seen)
    stride = DL.carry_stride(S, D, lag)
    assert L.qt_pose_duration_lag_carry_bytes(ctypes.byref(desc)) == B * stride
    d_cin = None
    if seen:
        assert carry.shape == (B, stride)
        d_cin = gd.input("carry_in", torch.from_numpy(np.ascontiguousarray(carry)))
    d_cout = gd.output("carry_out", (B, stride), torch.uint8)
    outs = [gd.output("lag_path", (B, count), torch.int64)]
    outs += [gd.output(name, (B, m), torch.int64) if w else None
             for name, m, w in (("lag_start", count, want[0]), ("filtered", n, want[1]), ("score", n, want[2]))]
    need = L.qt_pose_duration_lag_workspace_bytes(ctypes.byref(desc))
    assert need == DL.workspace_bytes(B, n, S)
    d_ws = gd.workspace("workspace", need) if need else None
    at = lambda t, m: Lm.ptr(t) if t is not None and m else None
    Lm.check(L.qt_pose_duration_lag_decode(ctypes.byref(desc), Lm.ptr(d_probs), ld, Lm.ptr(d_sc), Lm.ptr(d_tr), Lm.ptr(d_init),
                                           Lm.ptr(d_dur), Lm.ptr(d_open), Lm.ptr(d_cin), Lm.ptr(d_cout), at(outs[0], count),
                                           at(outs[1], count), at(outs[2], n), at(outs[3], n), Lm.ptr(d_ws), need,
                                           Lm.stream_ptr()), "qt_pose_duration_lag_decode")
    gd.check()
    return tuple(None if t is None else t.cpu().numpy() for t in outs), d_cout.cpu().numpy()


def stream(dev, probs, cuts, tab, lag, flush_last=True, **kw):
    """consecutive calls cut at `cuts`: (the outputs joined along the frame axis, the last carry)"""
    edges = [0] + list(cuts) + [probs.shape[1]]
    carry, calls = None, []
    for k, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        outs, carry = run(dev, probs[:, a:b], tab, lag, seen=a, flush=flush_last and k == len(edges) - 2, carry=carry, **kw)
        calls.append(outs)
    return tuple(None if calls[0][i] is None else np.concatenate([o[i] for o in calls], axis=1) for i in range(4)), carry


def same(got, want, what):
    for name, g, w in zip(("lag_path", "lag_start", "filtered", "score"), got, want):
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
            assert R.bits(g) == R.bits(w), (what, name, int((g != w).sum()), np.argwhere(g != w)[:4].tolist())


def same_carry(carry, state, tab, lag, what):
    B, (S, D) = carry.shape[0], tab[2].shape
    try:
        DL.same_state(DL.unpack_carry(carry.tobytes(), B, S, D, lag, state["seen"]), state)
    except AssertionError as e:
        raise AssertionError((what, "carry", str(e)))


def loops(probs, tab, lag, flush=True):
    _, outs, state = DL.decode(probs, *tab, lag=lag, flush=flush)
    return outs, state


def whole_video(dev, probs, tab, lengths):
    """qt_pose_duration_decode through ctypes on probs [B, T, C]: (path, start, score)"""
    M, Lm, L = _api()
    sc, tr, dur, init, open_ = tab
    B, T, C = probs.shape
    S, D = dur.shape
    up = lambda a: None if a is None else i32(a).to(dev)
    d = [torch.from_numpy(np.array(probs)).to(dev)] + [up(a) for a in (sc, tr, init, dur, open_, lengths)]
    path, start = (torch.empty((B, T), dtype=torch.int64, device=dev) for _ in range(2))
    score = torch.empty(B, dtype=torch.int64, device=dev)
    desc = M.PoseDurationDesc(B, T, C, S, D)
    need = L.qt_pose_duration_workspace_bytes(ctypes.byref(desc))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    Lm.check(L.qt_pose_duration_decode(ctypes.byref(desc), Lm.ptr(d[0]), C, *[Lm.ptr(t) for t in d[1:]], Lm.ptr(path),
                                       Lm.ptr(start), Lm.ptr(score), Lm.ptr(ws), need, Lm.stream_ptr()), "qt_pose_duration_decode")
    return path.cpu().numpy(), start.cpu().numpy(), score.cpu().numpy()


# ---- against the existing kernel -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,with_open", [(12, True), (12, False), (17, True)])
def test_every_emitted_frame_is_the_whole_video_kernel_on_a_prefix(S, with_open):
    """each stream replicated 2 T times into one qt_pose_duration_decode call: replica g cut at min(g + lag, T - 1) + 1 frames
    (lag_path and lag_start of frame g), replica T + g at g + 1 frames (score and filtered of frame g)"""
    dev = _dev()
    C, D, T, lag, B = 12, 8, 40, 5, 2
    tab = tables(C, S, D, with_open=with_open)
    probs = tracks(B, T, C)
    got, _ = run(dev, probs, tab, lag)
    lengths = np.array([min(g + lag, T - 1) + 1 for g in range(T)] + [g + 1 for g in range(T)], np.int32)
    for b in range(B):
        path, start, score = whole_video(dev, np.repeat(probs[b:b + 1], 2 * T, axis=0), tab, lengths)
        g = np.arange(T)
        want = (path[g, g], start[g, g], path[T + g, g], score[T:])
        same(tuple(o[b] for o in got), want, (S, with_open, b))


@pytest.mark.parametrize("n", [1, 16, 17])
def test_a_one_call_flush_within_the_lag_is_the_whole_video_kernel(n):
    dev = _dev()
    C, S, D, lag, B = 12, 12, 8, 16, 2
    tab = tables(C, S, D)
    probs = tracks(B, 40, C)[:, :n]
    got, _ = run(dev, probs, tab, lag)
    path, start, score = whole_video(dev, probs, tab, None)
    assert R.bits(got[0]) == R.bits(path) and R.bits(got[1]) == R.bits(start) and R.bits(got[3][:, -1]) == R.bits(score)


# ---- against the integer loops ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,S", [(1, 1), (2, 2), (12, 12), (12, 16), (12, 17), (64, 64)])
def test_bits_equal_the_loops(C, S):
    """outputs and the unpacked carry, init given and NULL, dur_open given and NULL, ld > C"""
    dev = _dev()
    T, B = 40, 2
    probs = tracks(B, T, C)
    for D in (1, 3, 8):
        for k, lag in enumerate((0, 1, 5, 16, 63)):
            for with_init in (True, False):
                tab = tables(C, S, D, with_init, with_open=bool((k + with_init) % 2))
                got, carry = run(dev, probs, tab, lag, pad=3)
                want, state = loops(probs, tab, lag)
                same(got, want, (C, S, D, lag, with_init))
                same_carry(carry, state, tab, lag, (C, S, D, lag, with_init))


@pytest.mark.parametrize("C,S", [(12, 12), (64, 64)])
def test_a_long_table_wraps_the_ring(C, S):
    """D = 128 over 150 frames: the ring wraps, S = 64 raises the LDS limit, a chunk of 64 emissions is crossed; in one call
    and cut at 100 frames"""
    dev = _dev()
    T, D, lag, B = 150, 128, 16, 2
    tab = tables(C, S, D)
    probs = tracks(B, T, C)
    want, state = loops(probs, tab, lag)
    for cuts in ([], [100]):
        got, carry = stream(dev, probs, cuts, tab, lag, pad=1)
        same(got, want, (C, S, cuts))
        same_carry(carry, state, tab, lag, (C, S, cuts))


# ---- splits ------------------------------------------------------------------------------------------------------------------------
def test_splits_keep_the_bits():
    dev = _dev()
    C, S, D, T, lag, B = 12, 12, 8, 40, 5, 2
    tab = tables(C, S, D)
    probs = tracks(B, T, C)
    want, state = loops(probs, tab, lag)
    for cuts in [[c] for c in range(1, T)] + [[3, 7], [8, 16, 24], [1, 2, 3], [5, 6, 39], [13, 26, 27]]:
        got, carry = stream(dev, probs, cuts, tab, lag)
        same(got, want, cuts)
        same_carry(carry, state, tab, lag, cuts)
    # one frame per call to the end, then a flush alone
    (path, start, filt, score), carry = stream(dev, probs, list(range(1, T)), tab, lag, flush_last=False)
    assert path.shape == (B, T - lag) and filt.shape == (B, T)
    rest, last = run(dev, probs[:, :0], tab, lag, seen=T, flush=True, carry=carry)
    assert rest[0].shape == (B, lag) and rest[2].shape == (B, 0)
    same((np.concatenate([path, rest[0]], axis=1), np.concatenate([start, rest[1]], axis=1), filt, score), want, "flush alone")
    same_carry(last, state, tab, lag, "flush alone")
    # no flush leaves the last lag frames pending, and they are what a call without flush would not have changed
    pending, pstate = loops(probs, tab, lag, flush=False)
    assert pending[0].shape == (B, T - lag)
    same((path, start, filt, score), pending, "pending")
    same_carry(carry, pstate, tab, lag, "pending")


def test_call_boundaries_around_the_lag_the_table_and_the_chunk():
    dev = _dev()
    C, S, D, lag, B = 12, 13, 24, 16, 1
    tab = tables(C, S, D)
    sizes = (1, 2, lag, lag + 1, D, D + 1, 64, 65, 130)
    probs = tracks(B, D + 1 + max(sizes), C)
    for seen in (0, 1, lag - 1, lag, lag + 1, D - 1, D, D + 1):
        head = carry = None
        if seen:
            head, carry = run(dev, probs[:, :seen], tab, lag, flush=False)
        for n in sizes:
            got, last = run(dev, probs[:, seen:seen + n], tab, lag, seen=seen, carry=carry)
            if seen:
                got = tuple(np.concatenate([h, g], axis=1) for h, g in zip(head, got))
            want, state = loops(probs[:, :seen + n], tab, lag)
            same(got, want, (seen, n))
            same_carry(last, state, tab, lag, (seen, n))


# ---- where the rules coincide ------------------------------------------------------------------------------------------------------
def plain_lag(dev, probs, sc, tr, init, lag):
    """qt_pose_lag_decode through ctypes, one call with flush: (lag_path, filtered)"""
    M, Lm, L = _api()
    B, T, C = probs.shape
    S = len(sc)
    desc = M.PoseLagDesc(B, T, C, S, lag, 1, 0)
    up = lambda a: None if a is None else i32(a).to(dev)
    d_probs, d_sc, d_tr, d_init = torch.from_numpy(np.array(probs)).to(dev), up(sc), up(tr), up(init)
    cout = torch.empty(L.qt_pose_lag_decode_carry_bytes(ctypes.byref(desc)), dtype=torch.uint8, device=dev)
    need = L.qt_pose_lag_decode_workspace_bytes(ctypes.byref(desc))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    path, filt = (torch.empty((B, T), dtype=torch.int64, device=dev) for _ in range(2))
    Lm.check(L.qt_pose_lag_decode(ctypes.byref(desc), Lm.ptr(d_probs), C, Lm.ptr(d_sc), Lm.ptr(d_tr), Lm.ptr(d_init), None,
                                  Lm.ptr(cout), Lm.ptr(path), Lm.ptr(filt), Lm.ptr(ws) if need else None, need, Lm.stream_ptr()),
             "qt_pose_lag_decode")
    return path.cpu().numpy(), filt.cpu().numpy()


@pytest.mark.parametrize("C,S", [(12, 12), (12, 17)])
def test_a_table_of_one_frame_is_the_plain_lag_kernel(C, S):
    dev = _dev()
    T, B = 40, 2
    probs = tracks(B, T, C)
    sc, tr = chain(S, C)
    dur = np.zeros((S, 1), np.int32)
    for trans, init, lag in ((tr, init_for(S), 5), (tr, None, 16), (np.zeros_like(tr), None, 5)):
        got, _ = run(dev, probs, (sc, trans, dur, init, None), lag)
        path, filt = plain_lag(dev, probs, sc, trans, init, lag)
        assert R.bits(got[0]) == R.bits(path) and R.bits(got[2]) == R.bits(filt), (S, lag)
        assert (got[1] == np.arange(T)[None, :]).all()


def test_ties_go_to_the_lowest_state_and_the_shortest_segment():
    dev = _dev()
    C, S, D, T, lag = 12, 12, 8, 40, 5
    probs = np.full((2, T, C), F32(1.0 / C), F32)
    tab = (np.arange(S, dtype=np.int32), np.zeros((S, S), np.int32), np.zeros((S, D), np.int32), None, None)
    for cuts in ([], [7], [1, 30]):
        (path, start, filt, score), _ = stream(dev, probs, cuts, tab, lag)
        assert not path.any() and not filt.any() and (start == np.arange(T)[None, :]).all(), cuts
        assert (score == int(R.q(F32(1.0 / C))) * np.arange(1, T + 1)[None, :]).all()


def test_streams_do_not_meet():
    dev = _dev()
    C, S, D, T, lag, B = 12, 12, 8, 40, 5, 3
    tab = tables(C, S, D)
    probs = tracks(B, T, C)
    got, carry = stream(dev, probs, [17], tab, lag)
    other = np.array(probs)
    other[1] = tracks(B, T, C)[0][::-1]
    changed, ccarry = stream(dev, other, [17], tab, lag)
    assert R.bits(got[0][1]) != R.bits(changed[0][1])
    for b in (0, 2):
        assert all(R.bits(g[b]) == R.bits(c[b]) for g, c in zip(got, changed)) and R.bits(carry[b]) == R.bits(ccarry[b])
    for b in range(B):                                           # a stream alone gives its batch bits
        alone, acarry = stream(dev, probs[b:b + 1], [17], tab, lag)
        assert all(R.bits(a[0]) == R.bits(g[b]) for a, g in zip(alone, got)) and R.bits(acarry[0]) == R.bits(carry[b])
    bare, bcarry = stream(dev, probs, [17], tab, lag, want=(False, False, False))    # dropping the optional outputs
    assert bare[1] is None and bare[2] is None and bare[3] is None
    assert R.bits(bare[0]) == R.bits(got[0]) and R.bits(bcarry) == R.bits(carry)


# ---- the module --------------------------------------------------------------------------------------------------------------------
def test_the_live_loop_reads_nothing_back():
    """16 streams x 1 frame for 40 steps and a push that only flushes, with host synchronisation an error; the joined outputs
    are one push of the whole video, and the loops"""
    dev = _dev()
    P = pkg()
    C, S, D, T, lag, B = 12, 12, 8, 40, 5, 16
    sc, tr, dur, init, open_ = tab = tables(C, S, D)
    probs = tracks(B, T, C)
    d_probs = torch.from_numpy(np.array(probs)).to(dev)
    dec = P.PoseDurationLagDecoder(sc, tr, dur, dev, lag, streams=B, init=init, dur_open=open_)
    dec.push(d_probs[:, :1], flush=True, start=True, filtered=True, score=True)       # (the workspace, before the mode is set)
    dec.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        parts = []
        for f in range(T):
            out = dec.push(d_probs[:, f:f + 1], start=True, filtered=True, score=True)
            assert out[0] == max(0, f - lag) and out[1].shape == (B, int(f >= lag)) and out[3].shape == (B, 1)
            parts.append(out[1:])
        out = dec.push(d_probs[:, :0], flush=True, start=True, filtered=True, score=True)
        assert out[0] == T - lag and out[1].shape == (B, lag) and out[3].shape == (B, 0) and dec.seen == T
        parts.append(out[1:])
        joined = [torch.cat([p[i] for p in parts], dim=1) for i in range(4)]
        dec.reset()
        first, *whole = dec.push(d_probs, flush=True, start=True, filtered=True, score=True)
        short = dec.reset().push(d_probs, flush=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert first == 0 and len(short) == 2 and torch.equal(short[1], whole[0])
    want, _ = loops(probs, tab, lag)
    same(tuple(t.cpu().numpy() for t in joined), want, "joined")
    same(tuple(t.cpu().numpy() for t in whole), want, "whole")
    one = P.PoseDurationLagDecoder(sc, tr, dur, dev, lag, init=init, dur_open=open_)     # [n, C] with one stream
    first, path, start = one.push(d_probs[3], flush=True, start=True)
    assert path.shape == (T,) and R.bits(path.cpu().numpy()) == R.bits(want[0][3]) and R.bits(start.cpu().numpy()) == R.bits(want[1][3])
    for bad in (lambda: dec.push(d_probs.cpu()), lambda: dec.push(d_probs.double()), lambda: dec.push(d_probs[:3]),
                lambda: dec.push(d_probs[:, :0]), lambda: dec.push(d_probs[0])):
        with pytest.raises(P.QtError):
            bad()
