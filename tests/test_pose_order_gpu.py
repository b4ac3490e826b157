"""Pose-order decoding on the GPU (csrc/pose_order.hip, <pkg>/pose_order.py): qt_pose_order_decode against the plain loops of
tests/_pose_order_ref.py.  Every number is an integer from the emission score on, so every output is compared for equality, at
the sizes where the two routes, the tiles, the scan's trips and the carry between calls can go wrong.  Every buffer sits
between poisoned guard bands (tests/_guard.py), the workspace is exactly the queried size and NaN-filled, the padding columns of
ld > C are NaN, and the inputs must come back byte for byte."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _pose_order_ref as R
from _guard import Guard
from _util import pkg

pytestmark = pytest.mark.gpu
TILE, GROUP = R.TILE, R.GROUP
F32 = np.float32


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _api():
    M, Lm = pkg("pose_order"), pkg("_lib")
    return M, Lm, Lm.lib()


def prior(S, C=None):
    """a left-to-right cycle over S states; state s emits class s, or s mod C, or for C = 64, S = 3 three far-apart classes"""
    C = S if C is None else C
    classes = [5, 40, 63] if (C, S) == (64, 3) else [s % C for s in range(S)]
    return R.cyclic_prior(classes, -30, -600, skip=-3000, other=-20000)


def init_for(S):
    return ((np.arange(S, dtype=np.int64) * 977) % 4001 - 4000).astype(np.int32)      # in [-4000, 0], no two alike for S <= 64


def long_frames(S):
    """a call that makes the scan stage its tile products more than once"""
    return (R.scan_trip_tiles(S) + 1) * TILE + 5


@functools.lru_cache(maxsize=None)
def case(batch, frames, C, S, with_init, special=True):
    """seeded probabilities with, where the stream is long enough, a NaN row, a row of zeros and rows of equal probabilities,
    and their reference from a zeroed carry; computed once, shared, never written"""
    probs = R.make_probs(1000 * S + 10 * C + batch, batch, frames, C)
    if special and frames >= 6:
        probs[0, frames // 2] = np.nan
        probs[-1, frames // 3] = 0.0
        probs[0, 1] = F32(1.0 / C)
        probs[-1, frames - 2:] = F32(0.25)
    sc, tr = prior(S, C)
    init = init_for(S) if with_init else None
    ref = R.decode(probs, sc, tr, init)
    for a in (probs, sc, tr) + ref:
        a.setflags(write=False)
    return probs, sc, tr, init, ref


def run(dev, probs, sc, tr, init=None, carry=None, ld=None, want_filtered=True, want_emissions=True):
    """qt_pose_order_decode through ctypes.  probs f32 [B,T,C]; ld: row stride (columns C .. ld - 1 are NaN); carry int64
    [B,S+2] as before the call or None for zeros.  Returns (path, filtered or None, emissions or None, carry) as numpy."""
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
    d_carry = G.output("carry", (B, S + 2), torch.int64, fill=0)
    if carry is not None:
        d_carry.copy_(torch.from_numpy(np.ascontiguousarray(carry, np.int64)))
    d_path = G.output("path", (B, T), torch.int64)
    d_filt = G.output("filtered", (B, T), torch.int64) if want_filtered else None
    d_em = G.output("emissions", (B, T, S), torch.int32) if want_emissions else None
    desc = M.PoseOrderDesc(B, T, C, S)
    need = L.qt_pose_order_workspace_bytes(ctypes.byref(desc))
    assert (need == 0) == (T <= TILE), (T, need)
    d_ws = G.workspace("workspace", need) if need else None
    Lm.check(L.qt_pose_order_decode(ctypes.byref(desc), Lm.ptr(d_probs), ld, Lm.ptr(d_sc), Lm.ptr(d_tr), Lm.ptr(d_init),
                                    Lm.ptr(d_carry), Lm.ptr(d_path), Lm.ptr(d_filt), Lm.ptr(d_em), Lm.ptr(d_ws), need,
                                    Lm.stream_ptr()), "qt_pose_order_decode")
    G.check()
    path = d_path.cpu().numpy()
    assert ((path >= 0) & (path < S)).all(), "path not written everywhere"
    filt = d_filt.cpu().numpy() if want_filtered else None
    em = d_em.cpu().numpy() if want_emissions else None
    assert filt is None or ((filt >= 0) & (filt < S)).all(), "filtered not written everywhere"
    return path, filt, em, d_carry.cpu().numpy()


def same(got, ref, what):
    for name, g, w in zip(("path", "filtered", "emissions", "carry"), got, ref):
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
            assert R.bits(g) == R.bits(w), (what, name, int((g != w).sum()), np.argwhere(g != w)[:4].tolist())


@pytest.mark.parametrize("C,S", [(1, 1), (2, 2), (12, 12), (13, 13), (16, 16), (17, 17), (64, 64), (8, 12), (64, 3)])
def test_bits_equal_the_rule(C, S):
    """frames: one, two; a tile less one, a tile (the short route's last size), a tile and one (the tiled route's first), two
    tiles and three, the first count at which the scan stages twice, a group of tiles and one more (the scan's second level)
    and, at 64 states where a trip is one product, two groups and one more (the second level stages twice).  S: 12 as in the model, 13 and 16 and 17 around the
    register path's limit, 64; repeated classes; few states among many classes.  Batch 1 with ld == C and init NULL, batch 3
    with ld = C + 3 and init given."""
    dev = _dev()
    two_levels_twice = ((2 * GROUP + 1) * TILE + 3,) if S == 64 else ()
    for batch in (1, 3):
        for frames in (1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, long_frames(S), (GROUP + 1) * TILE + 3) + two_levels_twice:
            probs, sc, tr, init, ref = case(batch, frames, C, S, batch == 3)
            same(run(dev, probs, sc, tr, init, ld=C if batch == 1 else C + 3), ref, (batch, frames))


def test_many_groups():
    """545 tiles of 12 states: 18 groups, so the scan's second level stages its 17 group products in two trips"""
    dev = _dev()
    probs, sc, tr, init, ref = case(1, 17 * GROUP * TILE + 7, 12, 12, True)
    assert 17 > R.scan_trip_tiles(12)
    same(run(dev, probs, sc, tr, init), ref, "18 groups")


def test_emission_scores_on_the_device():
    """q at its edges, through the kernel: one class per frame"""
    dev = _dev()
    one = F32(1.0)
    values = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-42, 2.0 ** -32, np.nextafter(F32(2.0 ** -32), F32(0)),
              np.nextafter(F32(2.0 ** -32), one), 1.0, np.nextafter(one, F32(0)), 0.5, -0.5, 3.0, 0.3, 1e-5]
    rng = np.random.default_rng(3)
    values += (2.0 ** rng.uniform(-33, 0.2, 3 * TILE)).astype(F32).tolist()
    probs = np.array(values, F32).reshape(1, -1, 1)
    sc, tr = prior(1)
    got = run(dev, probs, sc, tr)
    assert got[2][0, :, 0].tolist() == [R.q(v) for v in probs[0, :, 0]]
    same(got, R.decode(probs, sc, tr), "q")


def test_rows_of_nan_zeros_and_ties():
    """whole rows of NaN, of zeros and of equal probabilities score every state alike: the lowest index must win each time"""
    dev = _dev()
    for S, T in ((12, TILE - 4), (12, 3 * TILE + 7), (17, 2 * TILE + 1)):
        probs = np.array(case(1, T, S, S, False, special=False)[0])
        probs[0, 0:3] = np.nan
        probs[0, 10:14] = 0.0
        probs[0, 20:30] = F32(0.125)
        probs[0, T - 3:] = F32(0.5)
        sc, tr = prior(S)
        ref = R.decode(probs, sc, tr)
        same(run(dev, probs, sc, tr), ref, (S, T))
        assert (ref[2][0, 0:3] == R.SCORE_FLOOR).all() and ref[1][0, 0] == 0
    # all frames alike and trans all zero: every path ties, the all-lowest-index path comes out
    for T in (TILE, 2 * TILE + 3):
        probs = np.full((2, T, 12), F32(0.25), F32)
        sc, tr = prior(12)
        got = run(dev, probs, sc, np.zeros_like(tr))
        same(got, R.decode(probs, sc, np.zeros_like(tr)), T)
        assert not got[0].any() and not got[1].any()


def test_trans_and_init_are_clamped_and_a_class_out_of_range_scores_the_floor():
    dev = _dev()
    S = C = 12
    for T in (TILE - 1, 2 * TILE + 3):
        probs, sc, tr, _, _ = case(3, T, C, S, False)
        wild = np.array(tr)
        wild[0, 1], wild[3, 4], wild[5, 5], wild[7, 2] = 5, 2 ** 31 - 1, -2 ** 31, -65537
        init = init_for(S)
        init[2], init[4] = 77, -10 ** 9
        ref = R.decode(probs, sc, wild, init)
        same(run(dev, probs, sc, wild, init), ref, ("clamped", T))
        same(ref, R.decode(probs, sc, np.clip(wild, -65536, 0), np.clip(init, -65536, 0)), "the rule clamps")
        bad = np.array(sc)
        bad[3], bad[9], bad[11] = C, -1, 2 ** 31 - 1
        ref = R.decode(probs, bad, tr)
        got = run(dev, probs, bad, tr)
        same(got, ref, ("state_class", T))
        assert (got[2][:, :, [3, 9, 11]] == R.SCORE_FLOOR).all()


def test_optional_outputs_and_repeats():
    """filtered and emissions NULL; the same call twice gives the same bits; a stream alone equals itself in a batch"""
    dev = _dev()
    for C, S, T in ((12, 12, 5), (12, 12, 3 * TILE + 9), (17, 17, TILE + 2)):
        probs, sc, tr, init, ref = case(3, T, C, S, True)
        first = run(dev, probs, sc, tr, init)
        same(first, ref, (S, T))
        same(run(dev, probs, sc, tr, init), first, (S, T, "again"))
        same(run(dev, probs, sc, tr, init, want_filtered=False, want_emissions=False), ref, (S, T, "path only"))
        for b in range(3):
            alone = run(dev, probs[b:b + 1], sc, tr, init)
            same(alone, tuple(r[b:b + 1] for r in ref), (S, T, "alone", b))


@pytest.mark.parametrize("S", [12, 17])
def test_splits_across_the_two_routes(S):
    """short + tiled, tiled + short, three calls, a call of one frame: filtered, emissions and the last carry are the bits of
    one call, every call's path is the rule's path of that call from the carry it was given, and the last call's path is the
    one-call path on its frames"""
    dev = _dev()
    T = 3 * TILE + 20
    probs, sc, tr, init, whole = case(3, T, S, S, True)
    for cuts in ([40], [T - 34], [30, 30 + TILE + 16], [TILE, 2 * TILE], [T - 1], [1, T - TILE]):
        want = R.decode_split(probs, sc, tr, init, cuts)
        assert R.bits(want[1]) == R.bits(whole[1]) and R.bits(want[2]) == R.bits(whole[2]) and R.bits(want[3]) == R.bits(whole[3])
        assert R.bits(want[4]) == R.bits(whole[0][:, cuts[-1]:])
        carry, parts = None, []
        for a, b in zip([0] + cuts, cuts + [T]):
            got = run(dev, probs[:, a:b], sc, tr, init, carry=carry, ld=S + 1)
            carry = got[3]
            parts.append(got)
        joined = [np.concatenate([p[i] for p in parts], axis=1) for i in range(3)]
        same((joined[0], joined[1], joined[2], carry), want[:4], cuts)
        assert R.bits(parts[-1][0]) == R.bits(whole[0][:, cuts[-1]:]), cuts


def test_decoder_class_cycles_and_reset():
    """PoseOrderDecoder over chunks of both routes; cycles across call boundaries against a Python count; reset"""
    dev = _dev()
    P, M = pkg(), pkg("pose_order")
    C, B, T = 4, 2, 5 * TILE
    rng = np.random.default_rng(11)
    lead = ((np.arange(T)[None, :] + np.array([[0], [7]])) // 8) % C               # a new step every 8 frames: 10 rounds
    probs = np.full((B, T, C), F32(0.05), F32)
    np.put_along_axis(probs, lead[..., None], F32(0.85), axis=2)
    probs += rng.uniform(0, 0.01, probs.shape).astype(F32)
    sc, tr = M.cyclic_prior(range(C), stay=M.prob_score(0.9), advance=M.prob_score(0.1))
    decoder = P.PoseOrderDecoder(sc, tr, dev, streams=B, class_names=["a", "b", "c", "d"])
    d_probs = torch.from_numpy(probs).to(dev)
    cuts = [0, 32, 3 * TILE, 3 * TILE + 1, T]                                      # short, tiled, one frame, tiled
    assert all(lead[0, c - 1] == C - 1 and lead[0, c] == 0 for c in cuts[1:3])      # two cuts fall on a wrap of stream 0
    carry, last, total, on_a_cut = None, None, np.zeros(B, np.int64), 0
    got_total = torch.zeros(B, dtype=torch.int64, device=dev)
    for a, b in zip(cuts[:-1], cuts[1:]):
        path, path_class, filt, em = decoder.decode(d_probs[:, a:b], filtered=True, emissions=True)
        want = R.decode(probs[:, a:b], sc, tr, None, carry)
        carry = want[3]
        same((path.cpu().numpy(), filt.cpu().numpy(), em.cpu().numpy(), decoder.carry.cpu().numpy()), want, (a, b))
        assert path_class.dtype == torch.int64 and R.bits(path_class.cpu().numpy()) == R.bits(sc.astype(np.int64)[want[0]])
        on_a_cut += int(last is not None and last[0] == C - 1 and want[0][0, 0] == 0)
        counts, last = R.cycles(want[0], C - 1, 0, last)
        total += counts
        got = decoder.cycles(path)
        assert got.dtype == torch.int64 and got.cpu().numpy().tolist() == counts.tolist(), (a, b)
        got_total += got
    assert total.tolist() == got_total.cpu().numpy().tolist() and total[0] >= 9 and on_a_cut >= 1
    # one stream, [frames, C]; reset starts anew
    single = P.PoseOrderDecoder(sc, tr, dev)
    path, path_class = single.decode(d_probs[0, :40])
    want = R.decode(probs[:1, :40], sc, tr)
    assert path.shape == (40,) and R.bits(path.cpu().numpy()[None]) == R.bits(want[0])
    assert single.cycles(path, wrap_from=1, wrap_to=2).cpu().numpy().tolist() == R.cycles(want[0], 1, 2)[0].tolist()
    single.decode(d_probs[0, 40:50])
    single.reset()
    path, _ = single.decode(d_probs[0, :40])
    assert R.bits(path.cpu().numpy()[None]) == R.bits(want[0]) and R.bits(single.carry.cpu().numpy()) == R.bits(want[3])
    with pytest.raises(P.QtError):
        single.decode(d_probs[0, :4].cpu())
    with pytest.raises(P.QtError):
        single.decode(d_probs[0, :4].double())
    with pytest.raises(P.QtError):
        single.decode(d_probs[:, :4])


def test_the_video_loop_without_a_host_sync():
    """predict -> PoseTimeline.update -> PoseOrderDecoder.decode -> cycles -> FrameAnnotator.draw, 8 frames of 64 x 48 per step,
    under torch's sync debug mode; then one longer chunk through the tiled route the same way"""
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
    annotator.draw(frames, pred=torch.zeros(N, dtype=torch.int64, device=dev))      # (the tables' upload is not the loop's)
    decoder.decode(torch.full((TILE + 8, C), 0.5, device=dev))                      # (nor is the workspace's first allocation)
    decoder.reset()
    rounds = torch.zeros(1, dtype=torch.int64, device=dev)
    outs, shown = [], []
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        bounds = [(s * N, (s + 1) * N) for s in range(steps)] + [(steps * N, T)]
        for a, b in bounds:
            probs, _, _ = P.predict(d_logits[a:b])
            pred, conf, stable, rows = timeline.update(probs, smoothed=True)
            path, path_class = decoder.decode(rows)
            rounds += decoder.cycles(path)
            if b - a == N:
                shown.append(annotator.draw(frames, pred=path_class, confidence=conf))
            outs.append((rows, path, path_class, conf))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    carry, last, total = None, None, 0
    for (a, b), (rows, path, path_class, _) in zip(bounds, outs):
        want = R.decode(rows.cpu().numpy()[None], sc, tr, None, carry)
        carry = want[3]
        assert R.bits(path.cpu().numpy()[None]) == R.bits(want[0]), (a, b)
        assert R.bits(path_class.cpu().numpy()) == R.bits(sc.astype(np.int64)[want[0][0]])
        counts, last = R.cycles(want[0], C - 1, 0, last)
        total += int(counts[0])
    assert int(rounds[0]) == total and total >= 2
    for s in range(steps):                                                          # the drawn frames carry the path's class
        again = annotator.draw(frames, pred=outs[s][2].clone(), confidence=outs[s][3])
        assert torch.equal(shown[s], again) and not torch.equal(shown[s], frames)
