"""Fixed-lag pose-order posteriors with hold durations on the GPU (csrc/pose_duration_lag_posterior.hip, <pkg>/pose_order.py):
qt_pose_duration_lag_smooth against qt_pose_duration_posterior on every prefix, bit for bit (both kernels run: the second takes
the stream in 40 copies with lengths 1 .. 40); against the loops of tests/_pose_duration_lag_posterior_ref.py in float64 beside
the same loops in the rule's mixed precision, e_kernel <= 4 e_mixed + 2^-20, the project's bound; under splits of the stream
into calls (outputs and carry byte for byte, the carry also against the loops' packed state); and through
PoseDurationLagSmoother with host synchronisation forbidden.  Every call through ctypes has its outputs between poisoned guard
bands (tests/_guard.py), a workspace of exactly the queried size and poisoned, a poisoned carry_out, NaN in the padding columns
of ld > C, and inputs (carry_in included) that must come back byte for byte.  The probabilities and tables are
tests/test_pose_duration_lag_gpu.py's: a NaN row, a row of zeros, ties and forbidden lengths are present.

Measured on an MI355X: the largest share of the accuracy bound that any case here uses is 0.27 (S = C = 64, D = 128, lag = 63,
the rows conditioned on the first 64 frames).  python scripts/bench_pose_duration_lag_posterior.py (EXPERIMENTS.md, "Fixed-lag
pose-duration posteriors"), 16 streams, S = 12, D = 64, lag = 16, medians: a push of 16 x 1 frame 35.9 us (PoseLagSmoother.push
on the same frames 17.8 us, PoseDurationLagDecoder.push 18.0 us); a catch-up push of 16 x 4096 frames with flush 14.56 ms
(PoseDurationPosterior.smooth of the same videos 15.10 ms).  Context, not thresholds: nothing here asserts a time."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _pose_duration_lag_posterior_ref as LS
import _pose_duration_lag_ref as DL
import _pose_duration_posterior_ref as PR
import _pose_order_ref as R
from _guard import Guard
from _util import pkg

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
FACTOR, FLOOR = 4.0, 2.0 ** -20
OUT = ("lagged", "lagged_class", "lagged_begin", "filtered", "log2_evidence")
ALL = (True, True, True, True)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _api():
    M, Lm = pkg("pose_order"), pkg("_lib")
    return M, Lm, Lm.lib()


def i32(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int32))


def run(dev, probs, tab, lag, seen=0, flush=True, carry=None, pad=0, want=ALL):
    """one qt_pose_duration_lag_smooth through ctypes.  probs f32 [B, n, C] (the call's new frames); carry: the carry_out bytes
    of the call before (uint8 [B, stride]) or None at seen == 0; pad: ld - C; want: lagged_class, lagged_begin, filtered,
    log2_evidence.  Returns ((lagged, lagged_class, lagged_begin, filtered, log2_evidence) as numpy or None, carry_out bytes)."""
    M, Lm, L = _api()
    sc, tr, dur, init, open_ = tab
    B, n, C = probs.shape
    S, D = dur.shape
    ld = C + pad
    g0, g1 = LS.span(seen, n, lag, flush)
    count = g1 - g0
    padded = np.full((B, n, ld), np.nan, F32)
    padded[..., :C] = probs
    gd = Guard(dev)
    d_probs = gd.input("probs", torch.from_numpy(padded)) if n else None
    d_sc, d_tr, d_init = gd.input("state_class", i32(sc)), gd.input("trans", i32(tr)), gd.input("init", i32(init))
    d_dur, d_open = gd.input("dur", i32(dur)), gd.input("dur_open", i32(open_))
    desc = M.PoseDurationLagDesc(B, n, C, S, D, lag, int(flush), seen)
    stride = LS.carry_stride(S, D, lag)
    assert L.qt_pose_duration_lag_smooth_carry_bytes(ctypes.byref(desc)) == B * stride
    d_cin = None
    if seen:
        assert carry.shape == (B, stride)
        d_cin = gd.input("carry_in", torch.from_numpy(np.ascontiguousarray(carry)))
    d_cout = gd.output("carry_out", (B, stride), torch.uint8)
    outs = [gd.output("lagged", (B, count, S), torch.float32)]
    outs += [gd.output(name, shape, dt) if w else None
             for name, shape, dt, w in (("lagged_class", (B, count, C), torch.float32, want[0]),
                                        ("lagged_begin", (B, count, S), torch.float32, want[1]),
                                        ("filtered", (B, n, S), torch.float32, want[2]),
                                        ("log2_evidence", (B, n), torch.float64, want[3]))]
    need = L.qt_pose_duration_lag_smooth_workspace_bytes(ctypes.byref(desc))
    assert need == LS.workspace_bytes(B, n, S)
    d_ws = gd.workspace("workspace", need) if need else None
    at = lambda t, m: Lm.ptr(t) if t is not None and m else None
    Lm.check(L.qt_pose_duration_lag_smooth(ctypes.byref(desc), Lm.ptr(d_probs), ld, Lm.ptr(d_sc), Lm.ptr(d_tr), Lm.ptr(d_init),
                                           Lm.ptr(d_dur), Lm.ptr(d_open), Lm.ptr(d_cin), Lm.ptr(d_cout), at(outs[0], count),
                                           at(outs[1], count), at(outs[2], count), at(outs[3], n), at(outs[4], n), Lm.ptr(d_ws),
                                           need, Lm.stream_ptr()), "qt_pose_duration_lag_smooth")
    gd.check()
    return tuple(None if t is None else t.cpu().numpy() for t in outs), d_cout.cpu().numpy()


def stream(dev, probs, cuts, tab, lag, flush_last=True, **kw):
    """consecutive calls cut at `cuts`: (the outputs joined along the frame axis, the last carry)"""
    edges = [0] + list(cuts) + [probs.shape[1]]
    carry, calls = None, []
    for k, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        outs, carry = run(dev, probs[:, a:b], tab, lag, seen=a, flush=flush_last and k == len(edges) - 2, carry=carry, **kw)
        calls.append(outs)
    return tuple(None if calls[0][i] is None else np.concatenate([o[i] for o in calls], axis=1) for i in range(5)), carry


def same(got, want, what):
    for name, g, w in zip(OUT, got, want):
        if g is not None and w is not None:
            assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
            assert R.bits(g) == R.bits(w), (what, name, int((g != w).sum()), np.argwhere(g != w)[:4].tolist())


def whole_video(dev, probs, tab, lengths):
    """qt_pose_duration_posterior through ctypes on probs [B, T, C]: (posterior, class_posterior, begin, log2_evidence)"""
    M, Lm, L = _api()
    sc, tr, dur, init, open_ = tab
    B, T, C = probs.shape
    S, D = dur.shape
    up = lambda a: None if a is None else i32(a).to(dev)
    d = [torch.from_numpy(np.array(probs)).to(dev)] + [up(a) for a in (sc, tr, init, dur, open_, lengths)]
    post, begin = (torch.empty((B, T, S), dtype=torch.float32, device=dev) for _ in range(2))
    cls = torch.empty((B, T, C), dtype=torch.float32, device=dev)
    ev = torch.empty(B, dtype=torch.float64, device=dev)
    desc = M.PoseDurationDesc(B, T, C, S, D)
    need = L.qt_pose_duration_posterior_workspace_bytes(ctypes.byref(desc))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    Lm.check(L.qt_pose_duration_posterior(ctypes.byref(desc), Lm.ptr(d[0]), C, *[Lm.ptr(t) for t in d[1:]], Lm.ptr(post),
                                          Lm.ptr(cls), Lm.ptr(begin), Lm.ptr(ev), None, Lm.ptr(ws), need, Lm.stream_ptr()),
             "qt_pose_duration_posterior")
    return tuple(t.cpu().numpy() for t in (post, cls, begin, ev))


def errors(got, ref64):
    """(e of the four probability outputs, the evidence's error relative to max(1, |evidence|))"""
    e = max(float(np.abs(g.astype(F64) - w).max(initial=0.0)) for g, w in zip(got[:4], ref64[:4]))
    return e, float((np.abs(got[4] - ref64[4]) / np.maximum(1.0, np.abs(ref64[4]))).max(initial=0.0))


def share_of_bound(got, ref64, mixed, what):
    """asserts e_kernel <= 4 e_mixed + 2^-20 for the probabilities and for the evidence; returns the largest share used"""
    shares = []
    for name, e_k, e_m in zip(("e", "evidence"), errors(got, ref64), errors(mixed, ref64)):
        print(f"pose_duration_lag_smooth {what}: {name} kernel {e_k:.3e} mixed {e_m:.3e} share {e_k / (FACTOR * e_m + FLOOR):.3f}")
        assert e_k <= FACTOR * e_m + FLOOR, (what, name, e_k, e_m)
        shares.append(e_k / (FACTOR * e_m + FLOOR))
    return max(shares)


# ---- contract 1: the whole-video kernel on every prefix, and the loops ----------------------------------------------------------
LAGS = (0, 1, 5, 16, 63)


@pytest.mark.parametrize("with_tables", [True, False])
@pytest.mark.parametrize("C,S,D", [(4, 5, 7), (12, 12, 64), (6, 20, 9)])       # (6, 20, 9): 4 lanes per state
def test_every_emitted_row_is_the_whole_video_kernel_on_a_prefix(C, S, D, with_tables):
    """one stream of 40 frames; qt_pose_duration_posterior takes it in 40 copies with lengths 1 .. 40, every prefix in one
    launch.  Beside the bits, the project's accuracy bound against the float64 loops"""
    dev = _dev()
    T = 40
    tab = LS.tables(C, S, D, with_init=with_tables, with_open=with_tables)
    probs = LS.tracks(1, T, C)
    post, cls, begin, ev = whole_video(dev, np.repeat(probs, T, axis=0), tab, np.arange(1, T + 1, dtype=np.int32))
    g = np.arange(T)
    largest = 0.0
    for lag in LAGS:
        got, _ = run(dev, probs, tab, lag, pad=3 * (lag % 2))
        at = np.minimum(g + lag, T - 1)                                        # the copy with F = at + 1 frames
        want = (post[at, g][None], cls[at, g][None], begin[at, g][None], post[g, g][None], ev[None])
        same(got, want, (C, S, D, lag, with_tables))
        if lag == 0:
            assert R.bits(got[0]) == R.bits(got[3])                            # lag = 0 is filtered
        _, ref64, _ = LS.smooth(probs, *tab[:3], tab[3], tab[4], lag=lag, flush=True, F=F64)
        _, mixed, _ = LS.smooth(probs, *tab[:3], tab[3], tab[4], lag=lag, flush=True, F=F32)
        largest = max(largest, share_of_bound(got, ref64, mixed, (C, S, D, lag, with_tables)))
        assert np.abs(got[0].sum(axis=-1, dtype=F64) - 1.0).max() <= S * 2.0 ** -22
    print(f"pose_duration_lag_smooth {(C, S, D, with_tables)}: largest share of the bound {largest:.3f}")


@pytest.mark.parametrize("n", [1, 16, 17])
def test_a_one_call_flush_within_the_lag_is_the_whole_video_kernel(n):
    dev = _dev()
    C, S, D, lag, B = 12, 12, 8, 16, 2
    tab = LS.tables(C, S, D)
    probs = LS.tracks(B, 40, C)[:, :n]
    got, _ = run(dev, probs, tab, lag)
    post, cls, begin, ev = whole_video(dev, probs, tab, None)
    same(got[:3], (post, cls, begin), n)
    assert R.bits(got[4][:, -1]) == R.bits(ev)


# ---- contract 2: splits ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _long():
    """200 frames of two streams at D = 64, lag = 16 and the mixed loops' state after them; computed once, never written"""
    C, S, D, T, lag, B = 12, 12, 64, 200, 16, 2
    tab = LS.tables(C, S, D)
    probs = LS.tracks(B, T, C)
    _, _, state = LS.smooth(probs, *tab, lag=lag, flush=True, F=F32)
    return tab, probs, state


def carry_is_the_loops(carry, state, S, D, lag):
    B = carry.shape[0]
    LS.same_carry(LS.unpack_carry(carry.tobytes(), B, S, D, lag, state["seen"]), LS.carry_fields(state, S, D, lag),
                  LS.level_bound(S, D, state["seen"]))


def test_splits_keep_the_bits():
    dev = _dev()
    (sc, tr, dur, init, open_), probs, state = _long()
    tab, (S, D), lag, T = (sc, tr, dur, init, open_), dur.shape, 16, probs.shape[1]
    want, carry = run(dev, probs, tab, lag)
    carry_is_the_loops(carry, state, S, D, lag)
    marks = [1, 15, 16, 17, 63, 64, 65, 128, 199]
    for cuts in [[c] for c in marks] + [marks]:
        got, last = stream(dev, probs, cuts, tab, lag, pad=len(cuts) % 2)
        same(got, want, cuts)
        assert R.bits(last) == R.bits(carry), cuts
    # without a flush the last lag frames stay pending; a call of no frames brings them
    head, pending = run(dev, probs, tab, lag, flush=False)
    rest, last = run(dev, probs[:, :0], tab, lag, seen=T, flush=True, carry=pending)
    assert head[0].shape[1] == T - lag and rest[0].shape[1] == lag and rest[3].shape[1] == 0
    same(tuple(np.concatenate([h, r], axis=1) for h, r in zip(head, rest)), want, "flush alone")
    assert R.bits(last) == R.bits(carry) == R.bits(pending)
    # 48 frames, one per call
    want48, carry48 = run(dev, probs[:, :48], tab, lag)
    got, last = stream(dev, probs[:, :48], list(range(1, 48)), tab, lag)
    same(got, want48, "one frame per call")
    assert R.bits(last) == R.bits(carry48)


def test_the_limits():
    """S = C = 64, D = 128, lag = 63 over 300 frames: the LDS limit is raised, the ring wraps, every window has its full length.
    Eight prefixes F: the rows conditioned on them equal the whole-video kernel's bits and hold the bound against the loops"""
    dev = _dev()
    C = S = 64
    D, lag, T = 128, 63, 300
    tab = LS.tables(C, S, D)
    probs = LS.tracks(1, T, C)
    got, carry = run(dev, probs, tab, lag, pad=1)
    split, last = stream(dev, probs, [129], tab, lag)
    same(split, got, "cut at 129")
    assert R.bits(last) == R.bits(carry)
    prefixes = np.array([1, 2, 64, 65, 128, 129, 257, 300], np.int32)
    outs = whole_video(dev, np.repeat(probs, len(prefixes), axis=0), tab, prefixes)
    args = (np.repeat(probs, len(prefixes), axis=0), *tab[:3], tab[3], tab[4], prefixes)
    ref64, mixed = PR.loops64(*args), PR.loops_mixed(*args)

    def rows(source, k, F):
        """of prefix F (copy k): what the fixed-lag call conditions on it, as (lagged, class, begin, filtered, evidence)"""
        gs = np.arange(236, 300) if F == T else np.array([F - 1 - lag]) if F > lag else np.array([], np.int64)
        return (source[0][k, gs], source[1][k, gs], source[2][k, gs], source[0][k, F - 1:F], source[3][k:k + 1]), gs

    largest = 0.0
    for k, F in enumerate(int(p) for p in prefixes):
        want, gs = rows(outs, k, F)
        mine = (got[0][0, gs], got[1][0, gs], got[2][0, gs], got[3][0, F - 1:F], got[4][0, F - 1:F])
        same(mine, want, F)
        largest = max(largest, share_of_bound(mine, rows(ref64, k, F)[0], rows(mixed, k, F)[0], ("limits", F)))
    print(f"pose_duration_lag_smooth limits: largest share of the bound {largest:.3f}")


def test_streams_do_not_meet():
    dev = _dev()
    C, S, D, T, lag, B = 12, 12, 8, 40, 5, 16
    tab = LS.tables(C, S, D)
    probs = LS.tracks(B, T, C)
    got, carry = stream(dev, probs, [17], tab, lag)
    for b in range(B):                                           # a stream alone gives its batch bits
        alone, acarry = stream(dev, probs[b:b + 1], [17], tab, lag)
        assert all(R.bits(a[0]) == R.bits(g[b]) for a, g in zip(alone, got)) and R.bits(acarry[0]) == R.bits(carry[b]), b
    again, acarry = stream(dev, probs, [17], tab, lag)           # every run the same bits
    same(again, got, "again")
    assert R.bits(acarry) == R.bits(carry)


def test_nothing_outside_the_buffers_is_written():
    """the guard bands of `run` around every output, the workspace and carry_out, the inputs and carry_in unchanged, at sizes
    that leave odd tails (S = 13: the int16 rows end off an 8-byte boundary), with every optional output and with none"""
    dev = _dev()
    C, S, D, T, lag, B = 12, 13, 24, 70, 5, 3
    tab = LS.tables(C, S, D)
    probs = LS.tracks(B, T, C)
    full, carry = stream(dev, probs, [1, 30, 65], tab, lag, pad=3)
    bare, bcarry = stream(dev, probs, [1, 30, 65], tab, lag, want=(False, False, False, False))
    assert all(b is None for b in bare[1:]) and R.bits(bare[0]) == R.bits(full[0]) and R.bits(bcarry) == R.bits(carry)
    _, _, state = LS.smooth(probs, *tab, lag=lag, flush=True, F=F32)
    carry_is_the_loops(carry, state, S, D, lag)
    assert (LS.pack_carry(state, S, D, lag)[:, -6:] == 0).all() and (carry[:, -6:] == 0).all()      # 2 lag S = 130 -> 6 of padding


# ---- the module --------------------------------------------------------------------------------------------------------------------
def test_the_live_loop_reads_nothing_back():
    """predict -> PoseDurationLagDecoder.push and PoseDurationLagSmoother.push -> confidence -> FrameAnnotator.draw, 16 streams x
    1 frame for 40 steps and a push that only flushes, with host synchronisation an error; the joined rows are one push of the
    whole video"""
    dev = _dev()
    P, M = pkg(), pkg("pose_order")
    C, S, D, T, lag, B = 12, 12, 8, 40, 5, 16
    sc, tr, dur, init, open_ = tab = LS.tables(C, S, D)
    rng = np.random.default_rng(5)
    lead = (np.arange(T)[None, :] // 4 + np.arange(B)[:, None]) % C
    logits = rng.standard_normal((B, T, C)).astype(F32)
    np.put_along_axis(logits, lead[..., None], np.take_along_axis(logits, lead[..., None], 2) + F32(4.0), 2)
    d_logits = torch.from_numpy(logits).to(dev)
    frames = torch.from_numpy(rng.integers(0, 256, (B, 48, 64, 3), dtype=np.uint8)).to(dev)
    atlas = torch.from_numpy(rng.integers(0, 256, (C + 14, 8, 12), dtype=np.uint8))
    annotator = P.FrameAnnotator(atlas=(atlas, torch.full((C + 14,), 12, dtype=torch.int32)), caption_origin=(2, 2))
    dec = P.PoseDurationLagDecoder(sc, tr, dur, dev, lag, streams=B, init=init, dur_open=open_)
    post = P.PoseDurationLagSmoother(sc, tr, dur, dev, lag, streams=B, init=init, dur_open=open_)
    annotator.draw(frames, pred=torch.zeros(B, dtype=torch.int64, device=dev))      # (the tables' upload is not the loop's)
    warm = torch.full((B, 1, C), 0.5, device=dev)
    for _ in range(lag + 1):                                                         # (nor is the first allocation of anything)
        dec.push(warm), post.push(warm, by_class=True, begin=True, filtered=True, evidence=True)
    dec.reset(), post.reset()
    outs, shown, rows_all = [], [], []
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for f in range(T + 1):
            last = f == T
            rows = P.predict(d_logits[:, f])[0][:, None, :] if not last else rows[:, :0]
            if not last:
                rows_all.append(rows)
            first_d, lag_path = dec.push(rows, flush=last)
            first, lagged, cls, begin, filt, ev = post.push(rows, flush=last, by_class=True, begin=True, filtered=True, evidence=True)
            conf = post.confidence(lagged, lag_path)
            assert first == first_d == max(0, f - lag) and lagged.shape == (B, lag if last else int(f >= lag), S)
            assert filt.shape == (B, 0 if last else 1, S) and ev.shape == (B, 0 if last else 1) and ev.dtype == torch.float64
            if lagged.shape[1] == 1:
                shown.append(annotator.draw(frames, pred=dec.state_class[lag_path[:, 0]].long(), confidence=conf[:, 0]))
            outs.append((lagged, cls, begin, filt, ev, conf, lag_path))
        video = torch.cat(rows_all, dim=1)
        whole = post.reset().push(video, flush=True, by_class=True, begin=True, filtered=True, evidence=True)
        short = post.reset().push(video, flush=True)
        holds = post.holds(whole[3])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert post.seen == dec.seen == T and whole[0] == 0 and len(short) == 2 and len(shown) == T - lag
    joined = [torch.cat([o[i] for o in outs], dim=1) for i in range(7)]
    for got, want in zip(joined[:5], whole[1:]):
        assert got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want)
    assert torch.equal(short[1], whole[1])
    x = video.cpu().numpy()
    _, ref64, _ = LS.smooth(x, *tab, lag=lag, flush=True, F=F64)
    _, mixed, _ = LS.smooth(x, *tab, lag=lag, flush=True, F=F32)
    share_of_bound(tuple(t.cpu().numpy() for t in joined[:5]), ref64, mixed, "live loop")
    _, (path, _, _, _), _ = DL.decode(x, *tab, lag=lag, flush=True)
    assert (joined[6].cpu().numpy() == path).all()
    want_conf = np.take_along_axis(joined[0].cpu().numpy(), path[..., None], axis=2)[..., 0]
    assert joined[5].dtype == torch.float32 and R.bits(joined[5].cpu().numpy()) == R.bits(want_conf)
    assert holds.dtype == torch.float64 and holds.shape == (B, S)
    assert np.abs(holds.cpu().numpy() - whole[3].cpu().numpy().astype(F64).sum(axis=1)).max() <= 1e-9
    assert not torch.equal(shown[0], frames)
    one = P.PoseDurationLagSmoother(sc, tr, dur, dev, lag, init=init, dur_open=open_)     # [n, C] with one stream
    first, lagged, ev = one.push(video[3], flush=True, evidence=True)
    assert lagged.shape == (T, S) and ev.shape == (T,) and torch.equal(lagged, whole[1][3]) and torch.equal(ev, whole[5][3])
    for bad in (lambda: post.push(video.cpu()), lambda: post.push(video.double()), lambda: post.push(video[:3]),
                lambda: post.push(video[:, :0]), lambda: post.push(video[0]), lambda: post.holds(whole[1][:3]),
                lambda: post.confidence(whole[1], joined[6][:, :3])):
        with pytest.raises(P.QtError):
            bad()
    # the stream limit is enforced on the host, and load_tables starts the streams anew
    post.seen = M.MAX_SMOOTH_STREAM_FRAMES - 1
    with pytest.raises(P.QtError, match="at most"):
        post.push(video[:, :2])
    post.load_tables(torch.from_numpy(np.ascontiguousarray(tr, np.int32)).to(dev))
    assert post.seen == 0
