"""The pose-order learner on the GPU (csrc/pose_posterior.hip, csrc/pose_prior.hip, <pkg>/pose_order.py): qt_pose_prior_expect
against the float64 loops of tests/_pose_prior_ref.py, beside the same loops in numpy f32 on the same inputs:
e_kernel <= 4 e_f32 + 2^-20, the form and constants of tests/test_pose_posterior_gpu.py.  e is the largest
|counts - counts64| / max(1, counts64) over counts and start_counts; the evidence total is measured in bits, relative to
max(1, |evidence|).  Every figure is printed before it is asserted (pytest -s shows them).  Every buffer sits between poisoned
guard bands (tests/_guard.py), the workspace is exactly the queried size and NaN-filled, the padding columns of ld > C are NaN,
and the inputs must come back byte for byte.  Then: the counts' row and column sums against qt_pose_posterior's own rows,
accumulation and repeatability, qt_pose_prior_count_paths (exact), qt_pose_prior_update against the float64 M-step, and
PoseOrderLearner.fit with no host synchronisation."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _pose_order_ref as O
import _pose_prior_ref as R
import test_pose_posterior_gpu as TP
from _guard import Guard
from _util import pkg

pytestmark = pytest.mark.gpu
TILE = R.TILE
F32 = np.float32
FACTOR, FLOOR = TP.FACTOR, TP.FLOOR
_dev, _api = TP._dev, TP._api


@functools.lru_cache(maxsize=None)
def case(batch, frames, C, S, with_init, kind="mixing"):
    """the probabilities of the posterior's `case` (a NaN row, a row of zeros, rows of equal probabilities, a saturated 1.0) and
    the learner's references (float64, f32); computed once, shared, never written"""
    probs = O.make_probs(1000 * S + 10 * C + batch, batch, frames, C)
    if frames >= 6:
        probs[0, frames // 2] = np.nan
        probs[-1, frames // 3] = 0.0
        probs[0, 1] = F32(1.0 / C)
        probs[-1, frames - 2:] = F32(0.25)
        probs[0, 4] = 0.0
        probs[0, 4, C // 2] = 1.0
    sc, tr = TP.prior(S, C, kind)
    init = TP.init_for(S) if with_init else None
    ref64, ref32 = R.loops64(probs, sc, tr, init), R.loops32(probs, sc, tr, init)
    for a in (probs, sc, tr) + ref64 + ref32:
        a.setflags(write=False)
    return probs, sc, tr, init, ref64, ref32


def run(dev, probs, sc, tr, init=None, ld=None, into=None):
    """qt_pose_prior_expect through ctypes.  into: (counts, start_counts, totals) as before the call, or None for zeros.
    Returns the three accumulators as numpy."""
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
    acc = [G.output(name, shape, torch.float64, fill=0) for name, shape in (("counts", (S, S)), ("start_counts", (S,)),
                                                                            ("totals", (2,)))]
    if into is not None:
        for d, h in zip(acc, into):
            d.copy_(torch.from_numpy(np.ascontiguousarray(h, np.float64)))
    desc = M.PoseOrderDesc(B, T, C, S)
    need = L.qt_pose_prior_workspace_bytes(ctypes.byref(desc))
    assert need > 0
    d_ws = G.workspace("workspace", need)
    Lm.check(L.qt_pose_prior_expect(ctypes.byref(desc), Lm.ptr(d_probs), ld, Lm.ptr(d_sc), Lm.ptr(d_tr), Lm.ptr(d_init),
                                    Lm.ptr(acc[0]), Lm.ptr(acc[1]), Lm.ptr(acc[2]), Lm.ptr(d_ws), need, Lm.stream_ptr()),
             "qt_pose_prior_expect")
    G.check()
    return tuple(t.cpu().numpy() for t in acc)


def errors(got, ref64):
    """(e over counts and start_counts, the evidence total's error in bits relative to max(1, |evidence|))"""
    e = max(float((np.abs(g - w) / np.maximum(1.0, w)).max()) for g, w in zip(got[:2], ref64[:2]))
    return e, float(abs(got[2][0] - ref64[2][0]) / max(1.0, abs(ref64[2][0])))


def within_bound(got, ref64, ref32, what):
    for g in got:
        assert g.dtype == np.float64 and np.isfinite(g).all(), (what, "not finite")
    assert got[2][1] == ref64[2][1], (what, "frames", got[2][1])
    (e_k, ev_k), (e_f, ev_f) = errors(got, ref64), errors(ref32, ref64)
    print(f"pose_prior {what}: e_kernel {e_k:.3e} e_f32 {e_f:.3e} ratio {e_k / max(e_f, 1e-30):.2f}; "
          f"evidence {ev_k:.3e} f32 {ev_f:.3e}")
    assert e_k <= FACTOR * e_f + FLOOR, (what, e_k, e_f)
    assert ev_k <= FACTOR * ev_f + FLOOR, (what, "evidence", ev_k, ev_f)
    return FACTOR * e_f + FLOOR


@pytest.mark.parametrize("C,S", [(1, 1), (2, 2), (12, 12), (16, 16), (17, 17), (64, 64), (8, 12), (64, 3)])
def test_accuracy_against_the_float64_loops(C, S):
    """frames: one, two; a tile less one, a tile (the short route's last size), a tile and one (the tiled route's first), two
    tiles and three, the first count at which the scan stages twice.  S: 12 as in the model, 16 and 17 around the register
    path's limit, 64 (the partial in LDS beside the table); repeated classes; few states among many classes.  Batch 1 with
    ld == C and init NULL, batch 3 with ld = C + 3 and init given.  Three tables: the mixing cycle, stay-only, all zero."""
    dev = _dev()
    for kind in ("mixing", "stay", "zero"):
        for batch in (1, 3):
            for frames in (1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, TP.trip_frames(S)):
                probs, sc, tr, init, ref64, ref32 = case(batch, frames, C, S, batch == 3, kind)
                got = run(dev, probs, sc, tr, init, ld=C if batch == 1 else C + 3)
                within_bound(got, ref64, ref32, (C, S, kind, batch, frames))
                total = float(got[0].sum())
                assert abs(total - batch * (frames - 1)) <= 1e-4 * max(1, batch * frames) and abs(got[1].sum() - batch) <= 1e-4
                if frames == 1:
                    assert O.bits(got[0]) == O.bits(np.zeros((S, S)))


def test_an_all_floor_table():
    """every transition -65536: 256 bits down per frame and more at the NaN row, on both routes"""
    dev = _dev()
    for frames in (TILE, 3 * TILE + 2):
        probs, sc, tr, init, _, _ = case(3, frames, 12, 12, True)
        floor = np.full_like(tr, -65536)
        got = run(dev, probs, sc, floor, init)
        within_bound(got, R.loops64(probs, sc, floor, init), R.loops32(probs, sc, floor, init), ("floor", frames))


def test_row_and_column_sums_are_the_posterior_kernels_rows():
    """on the same inputs and a zeroed carry: the row sums of counts are the sum over frames 0 .. n - 2 of qt_pose_posterior's
    rows, the column sums that over frames 1 .. n - 1, within the accuracy bound times n"""
    dev = _dev()
    for C, S, batch, frames in ((12, 12, 3, 40), (12, 12, 1, 2 * TILE + 3), (17, 17, 3, TILE + 1), (64, 64, 1, TILE),
                                (64, 64, 3, 2 * TILE + 3), (8, 12, 3, TP.trip_frames(12))):
        probs, sc, tr, init, ref64, ref32 = case(batch, frames, C, S, batch == 3)
        got = run(dev, probs, sc, tr, init)
        bound = within_bound(got, ref64, ref32, ("beside qt_pose_posterior", S, batch, frames)) * frames
        post = TP.run(dev, probs, sc, tr, init, optional=False)[0].astype(np.float64)
        rows = float(np.abs(got[0].sum(axis=1) - post[:, :-1].sum(axis=(0, 1))).max())
        cols = float(np.abs(got[0].sum(axis=0) - post[:, 1:].sum(axis=(0, 1))).max())
        print(f"pose_prior beside qt_pose_posterior {(S, batch, frames)}: rows {rows:.3e} columns {cols:.3e} bound {bound:.3e}")
        assert rows <= bound and cols <= bound


def test_accumulation_and_repeatability():
    """two calls into one accumulator are the float64 sum of the two references; the same call twice into zeroed accumulators
    gives identical bits; streams do not meet: a permuted batch permutes nothing but the order of addition"""
    dev = _dev()
    for C, S, (b1, f1), (b2, f2) in ((12, 12, (3, 2 * TILE + 3), (1, 40)), (17, 17, (1, TILE + 1), (3, TILE)),
                                     (64, 64, (3, TILE - 1), (3, TILE + 1))):
        one, two = case(b1, f1, C, S, True), case(b2, f2, C, S, True)
        first = run(dev, *one[:4], ld=C + 1)
        assert all(O.bits(a) == O.bits(b) for a, b in zip(run(dev, *one[:4], ld=C + 1), first)), (S, "again")
        both = run(dev, *two[:4], into=first)
        sum64 = tuple(a + b for a, b in zip(one[4], two[4]))
        sum32 = tuple(a + b for a, b in zip(one[5], two[5]))
        within_bound(both, sum64, sum32, ("two calls", S))
        if b1 > 1:
            probs = one[0]
            turned = run(dev, np.ascontiguousarray(probs[::-1]), *one[1:4])
            within_bound(turned, one[4], one[5], ("permuted batch", S))
            alone = [run(dev, probs[b:b + 1], *one[1:4]) for b in range(b1)]
            summed = tuple(sum(a[k] for a in alone) for k in range(3))
            assert max(float(np.abs(summed[k] - first[k]).max()) for k in range(2)) <= 1e-9 * f1      # (double additions only)
            assert abs(summed[2][0] - first[2][0]) <= 1e-9 * abs(first[2][0]) and summed[2][1] == first[2][1]


def count(dev, path, S, into=None):
    """qt_pose_prior_count_paths through ctypes; num_classes of the descriptor is not used"""
    M, Lm, L = _api()
    B, T = path.shape
    G = Guard(dev)
    d_path = G.input("path", torch.from_numpy(np.ascontiguousarray(path, np.int64)))
    acc = [G.output(name, shape, torch.float64, fill=0) for name, shape in (("counts", (S, S)), ("start_counts", (S,)),
                                                                            ("totals", (2,)))]
    if into is not None:
        for d, h in zip(acc, into):
            d.copy_(torch.from_numpy(np.ascontiguousarray(h, np.float64)))
    desc = M.PoseOrderDesc(B, T, 1, S)
    need = L.qt_pose_prior_workspace_bytes(ctypes.byref(desc))
    d_ws = G.workspace("workspace", need)
    Lm.check(L.qt_pose_prior_count_paths(ctypes.byref(desc), Lm.ptr(d_path), Lm.ptr(acc[0]), Lm.ptr(acc[1]), Lm.ptr(acc[2]),
                                         Lm.ptr(d_ws), need, Lm.stream_ptr()), "qt_pose_prior_count_paths")
    G.check()
    return tuple(t.cpu().numpy() for t in acc)


def test_count_paths_is_exact():
    """frames 1, 2, a tile, a tile and one, more than one chunk of 1,024 and a chunk boundary; states outside [0, S) (negative,
    S itself, far beyond int32) take their transitions and starts out; onto accumulators that hold integers already"""
    dev = _dev()
    rng = np.random.default_rng(17)
    for S in (1, 12, 64):
        for B, T in ((1, 1), (3, 1), (3, 2), (2, TILE), (3, TILE + 1), (2, 1024), (3, 1025), (2, 2500)):
            path = rng.integers(0, S, (B, T))
            path[rng.random((B, T)) < 0.7] //= 2                # some entries well above 1
            bad = rng.random((B, T)) < 0.05
            path[bad] = rng.choice([-1, S, S + 3, 1 << 40, -(1 << 33)], size=int(bad.sum()))
            if T >= 2:
                path[0, 0], path[-1, -1] = S, -1
            want = R.count_paths(path, S)
            got = count(dev, path, S)
            for name, g, w in zip(("counts", "start_counts", "totals"), got, want):
                assert O.bits(g) == O.bits(w), (S, B, T, name)
            again = count(dev, path, S, into=got)
            assert all(O.bits(g) == O.bits(2 * w) for g, w in zip(again, want)), (S, B, T, "accumulated")
    clean = np.tile(np.arange(2500) // 3 % 12, (2, 1))
    got = count(dev, clean, 12, into=(np.zeros((12, 12)), np.zeros(12), np.array([-7.5, 3.0])))
    assert got[0].sum() == 2 * 2499 and got[1].tolist() == [2.0] + [0.0] * 11 and got[2].tolist() == [-7.5, 5003.0]


def update(dev, counts, start, tr, init, pseudo, learn_init, in_place):
    """qt_pose_prior_update through ctypes; allowed = the table is above -65536.  Returns (trans_out, init_out or None)."""
    M, Lm, L = _api()
    S = tr.shape[0]
    G = Guard(dev)
    d_counts = G.input("counts", torch.from_numpy(np.ascontiguousarray(counts, np.float64)))
    d_start = G.input("start_counts", torch.from_numpy(np.ascontiguousarray(start, np.float64)))
    d_allowed = G.input("allowed", torch.from_numpy((np.asarray(tr) > -65536).astype(np.int32)))
    as_i32 = lambda a: torch.from_numpy(np.array(a, np.int32))
    if in_place:
        d_tin = d_tout = G.output("trans", (S, S), torch.int32, fill=0)
        d_tin.copy_(as_i32(tr))
        d_iin = d_iout = None
        if learn_init:
            d_iin = d_iout = G.output("init", (S,), torch.int32, fill=0)
            d_iin.copy_(as_i32(np.zeros(S) if init is None else init))
    else:
        d_tin = G.input("trans_in", as_i32(tr))
        d_iin = G.input("init_in", None if init is None else as_i32(init))
        d_tout = G.output("trans_out", (S, S), torch.int32)
        d_iout = G.output("init_out", (S,), torch.int32) if learn_init else None
    Lm.check(L.qt_pose_prior_update(S, Lm.ptr(d_counts), Lm.ptr(d_start), Lm.ptr(d_allowed), float(pseudo), Lm.ptr(d_tin),
                                    Lm.ptr(d_iin), Lm.ptr(d_tout), Lm.ptr(d_iout), Lm.stream_ptr()), "qt_pose_prior_update")
    G.check()
    return d_tout.cpu().numpy(), None if d_iout is None else d_iout.cpu().numpy()


def test_update_is_the_float64_m_step():
    """fed the kernel's own counts as read back: trans_out and init_out are m_step's; an entry whose 256 log2(r / R) lies within
    1e-6 of a half-integer may differ by 1, and such entries are fewer than 1 % of the table"""
    dev = _dev()
    for C, S, batch, frames, kind in ((12, 12, 3, 2 * TILE + 3, "mixing"), (12, 12, 3, TILE, "stay"), (64, 64, 3, TILE + 1, "mixing"),
                                      (17, 17, 1, 1, "mixing"), (64, 3, 3, 40, "zero"), (1, 1, 1, 2, "mixing")):
        probs, sc, tr, init, _, _ = case(batch, frames, C, S, batch == 3, kind)
        counts, start, _ = run(dev, probs, sc, tr, init)
        counts = np.array(counts)
        if S >= 12:
            counts[5] = 0.0                                     # a row nothing went through keeps its old values at pseudo_count 0
        for pseudo in (0.0, 0.5):
            for learn_init in (False, True):
                want_tr, want_init, near, near_init = R.m_step(counts, start, tr, init, None, pseudo, learn_init)
                for in_place in (False, True):
                    got_tr, got_init = update(dev, counts, start, tr, init, pseudo, learn_init, in_place)
                    what = (S, frames, kind, pseudo, learn_init, in_place)
                    assert got_tr.dtype == np.int32 and (got_tr[np.asarray(tr) == -65536] == -65536).all(), what
                    off = got_tr.astype(np.int64) != want_tr
                    assert not (off & ~near).any() and np.abs(got_tr - want_tr).max() <= 1, (what, np.argwhere(off)[:4].tolist())
                    assert near.sum() < 0.01 * near.size, (what, int(near.sum()))
                    if pseudo == 0.0 and S >= 12:
                        assert got_tr[5].tolist() == np.asarray(tr)[5].tolist(), what
                    if learn_init:
                        off = got_init.astype(np.int64) != want_init
                        assert not (off & ~near_init).any() and np.abs(got_init - want_init).max() <= 1, what
                        assert near_init.sum() < max(1, 0.01 * near_init.size), what
                    else:
                        assert got_init is None


def test_fit_without_a_host_sync():
    """fit(videos, 3) is three hand-made rounds of zero / accumulate / update, bit for bit, under torch's sync debug mode; a
    decoder and a posterior after load_tables give the bits of fresh objects built from learner.tables(); accumulate_paths
    takes the decoder's path; the QtErrors"""
    dev = _dev()
    P, M = pkg(), pkg("pose_order")
    C = S = 12
    sc, tr = M.cyclic_prior(range(C), stay=-256, advance=-512, skip=-768, other=-3000)
    tr[3, 9] = tr[7, 0] = -65536                                # forbidden, and they stay so
    rng = np.random.default_rng(23)
    videos = []
    for shape in ((3, 2 * TILE + 6, C), (40, C), (1, TILE, C)):
        n = shape[-2]
        logits = rng.standard_normal(shape).astype(F32)
        lead = (np.arange(n) // 4) % C
        logits[..., np.arange(n), lead] += F32(3.0)
        videos.append(torch.softmax(torch.from_numpy(logits).to(dev), dim=-1))
    init = TP.init_for(S)
    make = lambda: P.PoseOrderLearner(sc, tr, dev, init=init, pseudo_count=0.25, learn_init=True, class_names=None)
    by_hand, fitted, hard = make(), make(), make()               # (the tables' upload is not the loop's)
    decoder, posterior = P.PoseOrderDecoder(sc, tr, dev), P.PosePosterior(sc, tr, dev)
    for v in videos:                                            # (the workspaces' first allocations are not the loop's)
        fitted.accumulate(v)
    decoder.decode(videos[1]), posterior.smooth(videos[1])
    fitted.zero()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        assert fitted.fit(videos, 3) is fitted
        for _ in range(3):
            by_hand.zero()
            for v in videos:
                by_hand.accumulate(v)
            by_hand.update()
        decoder.load_tables(fitted.trans, fitted.init), posterior.load_tables(fitted.trans, fitted.init)
        path, _ = decoder.decode(videos[1])
        post = posterior.smooth(videos[1])
        hard.accumulate_paths(path).accumulate_paths(path[None].expand(2, -1))
        hard.update()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for name in ("trans", "init", "counts", "start_counts", "_totals"):
        a, b = getattr(fitted, name).cpu().numpy(), getattr(by_hand, name).cpu().numpy()
        assert a.dtype == b.dtype and O.bits(a) == O.bits(b), name
    bits, frames = fitted.totals()
    assert frames == 3 * (2 * TILE + 6) + 40 + TILE and isinstance(frames, int) and np.isfinite(bits) and bits < 0
    t_sc, t_tr, t_init = fitted.tables()
    assert t_sc.tolist() == sc.tolist() and t_tr.dtype == np.int32 and t_tr.shape == (S, S) and t_init.shape == (S,)
    assert t_tr[3, 9] == -65536 and t_tr[7, 0] == -65536 and (t_tr != tr).any() and (t_init != init).any()
    assert (t_tr <= 0).all() and (t_tr >= -65536).all() and np.abs(np.exp2(t_tr / 256.0).sum(axis=1) - 1).max() <= S / 512
    fresh_d, fresh_p = P.PoseOrderDecoder(t_sc, t_tr, dev, init=t_init), P.PosePosterior(t_sc, t_tr, dev, init=t_init)
    assert torch.equal(fresh_d.decode(videos[1])[0], path) and torch.equal(fresh_p.smooth(videos[1]), post)
    want = R.count_paths(np.tile(path.cpu().numpy()[None], (3, 1, 1)).reshape(3, -1), S)
    assert hard.counts.cpu().numpy().tolist() == want[0].tolist() and hard.totals() == (0.0, 120)
    plain = P.PoseOrderLearner(sc, tr, dev)                     # no init, none learned
    plain.fit(videos[:1], 1)
    assert plain.init is None and plain.tables()[2] is None
    decoder.load_tables(plain.trans, plain.init)
    assert decoder.init is None and int(decoder.carry.abs().sum()) == 0
    good = videos[1]
    for bad in (good.cpu(), good.double(), good[:0], good[:, None, None, :], good[None, :, :0], [[0.5] * C]):
        with pytest.raises(P.QtError):
            fitted.accumulate(bad)
    for bad in (path.cpu(), path.to(torch.int32), path[:0], path[None, None], [0, 1]):
        with pytest.raises(P.QtError):
            fitted.accumulate_paths(bad)
    for bad in ((fitted.trans.cpu(), None), (fitted.trans.to(torch.int64), None), (fitted.trans[:5], None),
                (fitted.trans, fitted.init[:3]), (fitted.trans, fitted.init.cpu()), (t_tr, None)):
        with pytest.raises(P.QtError):
            posterior.load_tables(*bad)
    with pytest.raises(ValueError):
        fitted.fit(videos, -1)
