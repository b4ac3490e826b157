"""Pose-order posteriors on the GPU (csrc/pose_posterior.hip, <pkg>/pose_order.py): qt_pose_posterior against the float64 loops
of tests/_pose_posterior_ref.py, beside the same loops in numpy f32 on the same inputs: e_kernel <= 4 e_f32 + 2^-20, the form and
constants of tests/test_lstm_stream_gpu.py (the factor covers the device's exp2 and log2 and the regrouping of the tiled route).
e is the largest absolute error of posterior, filtered and class_posterior; the evidence is measured in bits, relative to
max(1, |evidence|).  Every figure is printed before it is asserted (pytest -s shows them).  Every buffer sits between poisoned
guard bands (tests/_guard.py), the workspace is exactly the queried size and NaN-filled, the padding columns of ld > C are NaN,
and the inputs must come back byte for byte.  Where only the short route runs, a split of a stream into calls must change no bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _pose_order_ref as O
import _pose_posterior_ref as R
from _guard import Guard
from _util import pkg

pytestmark = pytest.mark.gpu
TILE = R.TILE
F32 = np.float32
FACTOR, FLOOR = 4.0, 2.0 ** -20
NAMES = ("posterior", "filtered", "class_posterior", "evidence", "carry")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _api():
    M, Lm = pkg("pose_order"), pkg("_lib")
    return M, Lm, Lm.lib()


def classes_for(S, C):
    return [5, 40, 63] if (C, S) == (64, 3) else [s % C for s in range(S)]


def prior(S, C, kind="mixing"):
    """mixing: the left-to-right cycle of the decoder's tests; stay: 0 on the diagonal and -65536 elsewhere; zero: all zero"""
    sc, tr = O.cyclic_prior(classes_for(S, C), -30, -600, skip=-3000, other=-20000)
    if kind == "stay":
        tr = np.full_like(tr, -65536)
        np.fill_diagonal(tr, 0)
    elif kind == "zero":
        tr = np.zeros_like(tr)
    return sc, tr


def init_for(S):
    return ((np.arange(S, dtype=np.int64) * 977) % 4001 - 4000).astype(np.int32)      # in [-4000, 0], no two alike for S <= 64


def trip_frames(S):
    """the first count at which the scan stages its products more than once: trip + 2 tiles, the last of one frame"""
    return (pkg("pose_order").posterior_scan_trip_tiles(S) + 1) * TILE + 1


@functools.lru_cache(maxsize=None)
def case(batch, frames, C, S, with_init, kind="mixing"):
    """seeded probabilities with, where the stream is long enough, a NaN row, a row of zeros, rows of equal probabilities and a
    saturated 1.0, and their references (float64, f32) from a zeroed carry; computed once, shared, never written"""
    probs = O.make_probs(1000 * S + 10 * C + batch, batch, frames, C)
    if frames >= 6:
        probs[0, frames // 2] = np.nan
        probs[-1, frames // 3] = 0.0
        probs[0, 1] = F32(1.0 / C)
        probs[-1, frames - 2:] = F32(0.25)
        probs[0, 4] = 0.0
        probs[0, 4, C // 2] = 1.0
    sc, tr = prior(S, C, kind)
    init = init_for(S) if with_init else None
    ref64, ref32 = R.loops64(probs, sc, tr, init), R.loops32(probs, sc, tr, init)
    for a in (probs, sc, tr) + ref64 + ref32:
        a.setflags(write=False)
    return probs, sc, tr, init, ref64, ref32


def run(dev, probs, sc, tr, init=None, carry=None, ld=None, optional=True):
    """qt_pose_posterior through ctypes.  probs f32 [B,T,C]; ld: row stride (columns C .. ld - 1 are NaN); carry float64
    [B,S+2] as before the call or None for zeros.  Returns (posterior, filtered, class_posterior, evidence, carry) as numpy, the
    middle three None without `optional`."""
    M, Lm, L = _api()
    B, T, C = probs.shape
    S = len(sc)
    ld = C if ld is None else ld
    padded = np.full((B, T, ld), np.nan, F32)
    padded[..., :C] = probs
    G = Guard(dev)
    d_probs = G.input("probs", torch.from_numpy(padded))
    d_sc = G.input("state_class", torch.from_numpy(np.array(sc, np.int32)))
    d_tr = G.input("trans", torch.from_numpy(np.array(tr, np.int32)))
    d_init = G.input("init", None if init is None else torch.from_numpy(np.ascontiguousarray(init, np.int32)))
    d_carry = G.output("carry", (B, S + 2), torch.float64, fill=0)
    if carry is not None:
        d_carry.copy_(torch.from_numpy(np.ascontiguousarray(carry, np.float64)))
    d_post = G.output("posterior", (B, T, S), torch.float32)
    d_filt = G.output("filtered", (B, T, S), torch.float32) if optional else None
    d_cls = G.output("class_posterior", (B, T, C), torch.float32) if optional else None
    d_ev = G.output("log2_evidence", (B,), torch.float64) if optional else None
    desc = M.PoseOrderDesc(B, T, C, S)
    need = L.qt_pose_posterior_workspace_bytes(ctypes.byref(desc))
    assert (need == 0) == (T <= TILE), (T, need)
    d_ws = G.workspace("workspace", need) if need else None
    Lm.check(L.qt_pose_posterior(ctypes.byref(desc), Lm.ptr(d_probs), ld, Lm.ptr(d_sc), Lm.ptr(d_tr), Lm.ptr(d_init),
                                 Lm.ptr(d_carry), Lm.ptr(d_post), Lm.ptr(d_filt), Lm.ptr(d_cls), Lm.ptr(d_ev), Lm.ptr(d_ws), need,
                                 Lm.stream_ptr()), "qt_pose_posterior")
    G.check()
    get = lambda t: None if t is None else t.cpu().numpy()
    return get(d_post), get(d_filt), get(d_cls), get(d_ev), get(d_carry)


def errors(got, ref64):
    """(e of the three probability outputs, the evidence's error in bits relative to max(1, |evidence|))"""
    e = max(float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(got[:3], ref64[:3]) if g is not None)
    ev = 0.0 if got[3] is None else float((np.abs(got[3] - ref64[3]) / np.maximum(1.0, np.abs(ref64[3]))).max())
    return e, ev


def within_bound(got, ref64, ref32, what):
    S = got[0].shape[-1]
    for g in got:
        assert g is None or np.isfinite(g).all(), (what, "not finite")
    for name, g in zip(NAMES[:3], got[:3]):
        if g is not None:
            off = float(np.abs(g.sum(axis=-1, dtype=np.float64) - 1.0).max())
            assert off <= S * 2.0 ** -22, (what, name, "row sum", off)
    (e_k, ev_k), (e_f, ev_f) = errors(got, ref64), errors(ref32, ref64)
    print(f"pose_posterior {what}: e_kernel {e_k:.3e} e_f32 {e_f:.3e} ratio {e_k / max(e_f, 1e-30):.2f}; "
          f"evidence {ev_k:.3e} f32 {ev_f:.3e}")
    assert e_k <= FACTOR * e_f + FLOOR, (what, e_k, e_f)
    assert ev_k <= FACTOR * ev_f + FLOOR, (what, "evidence", ev_k, ev_f)
    return FACTOR * e_f + FLOOR


def same(got, want, what, names=NAMES):
    for name, g, w in zip(NAMES, got, want):
        if g is not None and name in names:
            assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
            assert O.bits(g) == O.bits(w), (what, name, int((g != w).sum()), np.argwhere(g != w)[:4].tolist())


@pytest.mark.parametrize("C,S", [(1, 1), (2, 2), (12, 12), (16, 16), (17, 17), (64, 64), (8, 12), (64, 3)])
def test_accuracy_against_the_float64_loops(C, S):
    """frames: one, two; a tile less one, a tile (the short route's last size), a tile and one (the tiled route's first), two
    tiles and three, the first count at which the scan stages twice.  S: 12 as in the model, 16 and 17 around the register
    path's limit, 64; repeated classes; few states among many classes.  Batch 1 with ld == C and init NULL, batch 3 with
    ld = C + 3 and init given.  Three tables: the mixing cycle of the decoder's tests, stay-only, all zero."""
    dev = _dev()
    for kind in ("mixing", "stay", "zero"):
        for batch in (1, 3):
            for frames in (1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, trip_frames(S)):
                probs, sc, tr, init, ref64, ref32 = case(batch, frames, C, S, batch == 3, kind)
                got = run(dev, probs, sc, tr, init, ld=C if batch == 1 else C + 3)
                within_bound(got, ref64, ref32, (C, S, kind, batch, frames))
                assert got[4][:, 0].tolist() == [frames] * batch and O.bits(got[4][:, 1]) == O.bits(got[3])
                assert np.abs(np.exp2(got[4][:, 2:]) - got[1][:, -1]).max() <= 2.0 ** -22      # a_last is the last filtered row's
                if frames == 1:
                    assert O.bits(got[0]) == O.bits(got[1])


def test_an_all_floor_table():
    """every transition -65536: 256 bits down per frame and more at the NaN row, on both routes"""
    dev = _dev()
    for frames in (TILE, 3 * TILE + 2):
        probs, sc, tr, init, _, _ = case(3, frames, 12, 12, True)
        floor = np.full_like(tr, -65536)
        got = run(dev, probs, sc, floor, init)
        within_bound(got, R.loops64(probs, sc, floor, init), R.loops32(probs, sc, floor, init), ("floor", frames))


def test_one_state_pins_q_and_the_double_sums():
    """S = 1, trans = 0: every c_f is the frame's emission score, so 256 log2_evidence is the sum of q exactly, on both routes"""
    dev = _dev()
    one = F32(1.0)
    values = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-42, 2.0 ** -32, np.nextafter(F32(2.0 ** -32), F32(0)),
              np.nextafter(F32(2.0 ** -32), one), 1.0, np.nextafter(one, F32(0)), 0.5, -0.5, 3.0, 0.3, 1e-5]
    rng = np.random.default_rng(3)
    values += (2.0 ** rng.uniform(-33, 0.2, 3 * TILE)).astype(F32).tolist()
    column = np.array(values, F32)
    for frames in (TILE - 3, len(values)):
        probs = np.full((2, frames, 3), F32(0.5), F32)
        probs[0, :, 1], probs[1, :, 1] = column[:frames], column[::-1][:frames]
        sc, tr = np.array([1], np.int32), np.zeros((1, 1), np.int32)
        post, filt, cls, ev, carry = run(dev, probs, sc, tr)
        want = O.q_array(probs[:, :, 1]).sum(axis=1)
        assert (256.0 * ev).tolist() == want.tolist() and (256.0 * carry[:, 1]).tolist() == want.tolist()
        assert (post == 1).all() and (filt == 1).all() and (carry[:, 2] == 0).all()
        assert (cls[..., 1] == 1).all() and (cls[..., 0] == 0).all() and (cls[..., 2] == 0).all()
        again = run(dev, probs, sc, tr, carry=carry)
        assert (256.0 * again[4][:, 1]).tolist() == (2 * want).tolist() and (256.0 * again[3]).tolist() == want.tolist()


def test_a_zero_table_forgets_the_other_frames():
    """all-zero trans and distinct classes: posterior[f] is frame f's own scores normalised, whatever order the others come in"""
    dev = _dev()
    S = C = 12
    for frames in (TILE - 7, 2 * TILE + 3):
        probs, sc, _, _, _, _ = case(1, frames, C, S, False)
        tr = np.zeros((S, S), np.int32)
        weight = np.exp2(R.scores(probs[0], sc, np.float64))
        own = weight / weight.sum(axis=1, keepdims=True)
        order = np.random.default_rng(9).permutation(frames)
        for rows in (np.arange(frames), order):
            shuffled = np.ascontiguousarray(probs[:, rows])
            got = run(dev, shuffled, sc, tr)
            ref64 = R.loops64(shuffled, sc, tr)
            bound = within_bound(got, ref64, R.loops32(shuffled, sc, tr), ("zero table", frames))
            assert np.abs(ref64[0][0] - own[rows]).max() <= 1e-12
            assert np.abs(got[0][0] - own[rows]).max() <= bound + 1e-12 and np.abs(got[1][0] - own[rows]).max() <= bound + 1e-12


def test_a_stay_only_table_gives_one_row_for_every_frame():
    """stay 0 and -65536 elsewhere: no mass changes state (2^-256 is nothing), so the posterior is the same row at every frame"""
    dev = _dev()
    for frames in (TILE, 2 * TILE + 3):
        probs, sc, tr, init, ref64, ref32 = case(3, frames, 12, 12, True, "stay")
        got = run(dev, probs, sc, tr, init)
        bound = within_bound(got, ref64, ref32, ("stay only", frames))
        assert np.abs(ref64[0] - ref64[0][:, :1]).max() <= 1e-12
        assert np.abs(got[0] - got[0][:, :1]).max() <= 2 * bound


def test_streams_do_not_meet():
    """one frame of one stream made one-hot: every other stream keeps its bits; a stream alone gives the bits it has in a batch"""
    dev = _dev()
    for C, S, frames in ((12, 12, 40), (12, 12, 2 * TILE + 3), (17, 17, TILE + 2)):
        probs, sc, tr, init, _, _ = case(3, frames, C, S, True)
        first = run(dev, probs, sc, tr, init, ld=C + 1)
        same(run(dev, probs, sc, tr, init, ld=C + 1), first, (S, frames, "again"))
        changed = np.array(probs)
        changed[1, frames // 2] = 0.0
        changed[1, frames // 2, 3] = 1.0
        second = run(dev, changed, sc, tr, init, ld=C + 1)
        assert O.bits(second[0][1]) != O.bits(first[0][1])
        for b in (0, 2):
            same(tuple(x[b] for x in second), tuple(x[b] for x in first), (S, frames, "beside a changed stream", b))
        for b in range(3):
            alone = run(dev, probs[b:b + 1], sc, tr, init)
            same(alone, tuple(x[b:b + 1] for x in first), (S, frames, "alone", b))
        only = run(dev, probs, sc, tr, init, ld=C + 1, optional=False)
        same(only, first, (S, frames, "posterior only"), names=("posterior", "carry"))


def test_every_split_on_the_short_route_keeps_the_bits():
    """a 40-frame stream in two calls at every cut and in three at a handful: filtered, the evidence total and the carry are
    the bits of one call, and the last call's posterior is the bits of the one-call posterior on its frames"""
    dev = _dev()
    T, S = 40, 12
    probs, sc, tr, init, ref64, ref32 = case(2, T, S, S, True)
    whole = run(dev, probs, sc, tr, init)
    within_bound(whole, ref64, ref32, "one call of 40")
    for cuts in [[c] for c in range(1, T)] + [[1, 2], [7, 8], [13, 30], [20, 39], [38, 39]]:
        carry, parts = None, []
        for a, b in zip([0] + cuts, cuts + [T]):
            parts.append(run(dev, probs[:, a:b], sc, tr, init, carry=carry, ld=S + 1))
            carry = parts[-1][4]
        assert O.bits(np.concatenate([p[1] for p in parts], axis=1)) == O.bits(whole[1]), cuts
        assert O.bits(carry) == O.bits(whole[4]), cuts
        assert O.bits(parts[-1][0]) == O.bits(whole[0][:, cuts[-1]:]), cuts
        assert np.abs(sum(p[3] for p in parts) - whole[3]).max() <= 1e-9 * np.abs(whole[3]).max(), cuts


def test_splits_across_the_two_routes():
    """150 frames cut at 64, 65 and 100: each call against the float64 loops from the carry it was given"""
    dev = _dev()
    T, S = 150, 12
    probs, sc, tr, init, whole64, _ = case(2, T, S, S, True)
    for cut in (64, 65, 100):
        carry = carry64 = carry32 = None
        for a, b in ((0, cut), (cut, T)):
            ref64 = R.loops64(probs[:, a:b], sc, tr, init, carry64)
            ref32 = R.loops32(probs[:, a:b], sc, tr, init, carry32)
            got = run(dev, probs[:, a:b], sc, tr, init, carry=carry)
            within_bound(got, ref64, ref32, ("split", cut, a, b))
            carry, carry64, carry32 = got[4], ref64[4], ref32[4]
        assert carry[:, 0].tolist() == [T, T]
        rel = lambda total: float((np.abs(total - whole64[3]) / np.maximum(1.0, np.abs(whole64[3]))).max())
        assert rel(carry[:, 1]) <= FACTOR * rel(carry32[:, 1]) + FLOOR, (cut, rel(carry[:, 1]), rel(carry32[:, 1]))


def test_the_video_loop_without_a_host_sync():
    """predict -> PoseTimeline.update -> PoseOrderDecoder.decode -> PosePosterior.smooth -> confidence -> FrameAnnotator.draw
    under torch's sync debug mode: chunks of 8 frames (short route), then a longer one (tiled route); [frames, C] and
    [streams, frames, C]; a row-strided and a transposed probs; the QtErrors"""
    dev = _dev()
    P, M = pkg(), pkg("pose_order")
    C, steps, N = 12, 4, 8
    rng = np.random.default_rng(5)
    T = steps * N + TILE + 8
    lead = (np.arange(T) // 3) % C
    logits = rng.standard_normal((T, C)).astype(F32)
    logits[np.arange(T), lead] += F32(3.0)
    d_logits = torch.from_numpy(logits).to(dev)
    frames = torch.from_numpy(rng.integers(0, 256, (N, 48, 64, 3), dtype=np.uint8)).to(dev)
    atlas = torch.from_numpy(rng.integers(0, 256, (C + 14, 8, 12), dtype=np.uint8))
    annotator = P.FrameAnnotator(atlas=(atlas, torch.full((C + 14,), 12, dtype=torch.int32)), caption_origin=(2, 2))
    timeline = P.PoseTimeline(C, dev, window=3, min_run=2)
    sc, tr = M.cyclic_prior(range(C), stay=-40, advance=-500, skip=-2500)
    decoder = P.PoseOrderDecoder(sc, tr, dev)
    posterior = P.PosePosterior(sc, tr, dev)
    annotator.draw(frames, pred=torch.zeros(N, dtype=torch.int64, device=dev))      # (the tables' upload is not the loop's)
    warm = torch.full((TILE + 8, C), 0.5, device=dev)
    decoder.decode(warm), posterior.smooth(warm)                                    # (nor is the workspaces' first allocation)
    decoder.reset(), posterior.reset()
    wide = torch.full((2, 2 * TILE, C + 4), float("nan"), device=dev)
    pair = P.PosePosterior(sc, tr, dev, streams=2)
    pair.smooth(wide[:, :, :C])
    pair.reset()
    outs, shown = [], []
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        bounds = [(s * N, (s + 1) * N) for s in range(steps)] + [(steps * N, T)]
        for a, b in bounds:
            probs, _, _ = P.predict(d_logits[a:b])
            pred, _, stable, rows = timeline.update(probs, smoothed=True)
            path, path_class = decoder.decode(rows)
            post, filt, cls, ev = posterior.smooth(rows, filtered=True, by_class=True, evidence=True)
            conf = posterior.confidence(post, path)
            if b - a == N:
                shown.append(annotator.draw(frames, pred=path_class, confidence=conf))
            outs.append((rows, path, post, filt, cls, ev, conf))
        both = torch.stack([o[0] for o in outs[:steps]]).reshape(2, 2 * N, C)       # two streams of 16 frames
        wide[:, :2 * N, :C] = both
        strided = pair.smooth(wide[:, :2 * N, :C])                                  # a slice of a wider tensor
        pair.reset()
        turned = pair.smooth(both.transpose(1, 2).contiguous().transpose(1, 2))     # the class axis not the fastest: copied
        pair.reset()
        wide[:, :, :C] = 0.25
        long_pair = pair.smooth(wide[:, :, :C], filtered=True)                      # rows C + 4 apart, passed as they are
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(strided, turned) and strided.shape == (2, 2 * N, C)
    assert long_pair[0].shape == (2, 2 * TILE, C) and bool(torch.isfinite(long_pair[0]).all())
    carry64 = carry32 = None
    for (a, b), (rows, path, post, filt, cls, ev, conf) in zip(bounds, outs):
        x = rows.cpu().numpy()[None]
        ref64, ref32 = R.loops64(x, sc, tr, None, carry64), R.loops32(x, sc, tr, None, carry32)
        carry64, carry32 = ref64[4], ref32[4]
        got = tuple(t.cpu().numpy()[None] for t in (post, filt, cls)) + (ev.cpu().numpy(),)
        assert post.shape == (b - a, C) and cls.shape == (b - a, C) and ev.shape == (1,) and ev.dtype == torch.float64
        within_bound(got, ref64, ref32, ("loop", a, b))
        want_conf = np.take_along_axis(got[0][0], path.cpu().numpy()[:, None], axis=1)[:, 0]
        assert conf.dtype == torch.float32 and conf.shape == path.shape and O.bits(conf.cpu().numpy()) == O.bits(want_conf)
    assert O.bits(posterior.carry.cpu().numpy()[:, 0]) == O.bits(np.array([float(T)]))
    for s in range(steps):                                                          # the drawn confidence is the drawn label's
        again = annotator.draw(frames, pred=decoder._state_class64[outs[s][1]], confidence=outs[s][6].clone())
        assert torch.equal(shown[s], again) and not torch.equal(shown[s], frames)
    posterior.reset()
    fresh = posterior.smooth(outs[0][0])
    assert torch.equal(fresh, outs[0][2]) and isinstance(fresh, torch.Tensor)
    good = outs[0][0]
    for bad in (good.cpu(), good.double(), good[None].expand(2, -1, -1), good[:0], good[:, None, None, :], [[0.5] * C]):
        with pytest.raises(P.QtError):
            posterior.smooth(bad)
    with pytest.raises(P.QtError):
        posterior.confidence(fresh, outs[0][1].to(torch.int32))
    with pytest.raises(P.QtError):
        posterior.confidence(fresh[:, :5], outs[0][1])
    with pytest.raises(P.QtError):
        posterior.confidence(fresh.cpu(), outs[0][1])
    if torch.cuda.device_count() > 1:
        with pytest.raises(P.QtError):
            posterior.smooth(good.to("cuda:1"))
