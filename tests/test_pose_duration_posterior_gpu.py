"""Pose-order posteriors with hold durations on the GPU (csrc/pose_duration_posterior.hip, <pkg>/pose_order.py):
qt_pose_duration_posterior against the float64 loops of tests/_pose_duration_posterior_ref.py, beside the same loops with the
rule's own precision (double levels, f32 inside an L and in every 2^) on the same inputs: e_kernel <= 4 e_mixed + 2^-20, the
form and constants of tests/test_pose_posterior_gpu.py (the factor covers the device's exp2 and log2 and the regrouped sums).
e is the largest absolute error of posterior, class_posterior and begin; the evidence is measured relative to
max(1, |evidence|), dur_counts relative to max(1, counts).  Every figure is printed before it is asserted (pytest -s shows
them).  Every buffer sits between poisoned guard bands (tests/_guard.py), the workspace is exactly the queried size and
NaN-filled, the padding columns of ld > C are NaN, and the inputs must come back byte for byte."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _pose_duration_posterior_ref as P
import _pose_duration_ref as Q
import _pose_order_ref as R
from _guard import Guard
from _util import pkg

pytestmark = pytest.mark.gpu
F32 = np.float32
FACTOR, FLOOR = 4.0, 2.0 ** -20
OUT = ("posterior", "class_posterior", "begin", "evidence", "dur_counts")


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


def run(dev, probs, sc, tr, dur, init=None, dur_open=None, lengths=None, ld=None, want=OUT, counts=None):
    """qt_pose_duration_posterior through ctypes.  probs f32 [B,T,C]; ld: row stride (columns C .. ld - 1 are NaN); want: the
    outputs that are not NULL; counts: dur_counts as before the call (zeros).  Returns (posterior, class_posterior, begin,
    evidence, dur_counts) as numpy, None for those not asked for."""
    M, Lm, L = _api()
    B, T, C = probs.shape
    S, D = np.shape(dur)
    ld = C if ld is None else ld
    padded = np.full((B, T, ld), np.nan, F32)
    padded[..., :C] = probs
    G = Guard(dev)
    i32 = lambda a: None if a is None else torch.from_numpy(np.array(a, np.int32))
    d_probs = G.input("probs", torch.from_numpy(padded))
    d_sc, d_tr, d_init = G.input("state_class", i32(sc)), G.input("trans", i32(tr)), G.input("init", i32(init))
    d_dur, d_open, d_len = G.input("dur", i32(dur)), G.input("dur_open", i32(dur_open)), G.input("lengths", i32(lengths))
    d_post = G.output("posterior", (B, T, S), torch.float32) if "posterior" in want else None
    d_cls = G.output("class_posterior", (B, T, C), torch.float32) if "class_posterior" in want else None
    d_begin = G.output("begin", (B, T, S), torch.float32) if "begin" in want else None
    d_ev = G.output("log2_evidence", (B,), torch.float64) if "evidence" in want else None
    d_counts = G.output("dur_counts", (S, D), torch.float64, fill=0) if "dur_counts" in want else None
    if counts is not None:
        d_counts.copy_(torch.from_numpy(np.ascontiguousarray(counts, np.float64)))
    desc = M.PoseDurationDesc(B, T, C, S, D)
    need = L.qt_pose_duration_posterior_workspace_bytes(ctypes.byref(desc))
    assert need == 8 * (2 * B * T * S + B * S * D)
    d_ws = G.workspace("workspace", need)
    Lm.check(L.qt_pose_duration_posterior(ctypes.byref(desc), Lm.ptr(d_probs), ld, Lm.ptr(d_sc), Lm.ptr(d_tr), Lm.ptr(d_init),
                                          Lm.ptr(d_dur), Lm.ptr(d_open), Lm.ptr(d_len), Lm.ptr(d_post), Lm.ptr(d_cls),
                                          Lm.ptr(d_begin), Lm.ptr(d_ev), Lm.ptr(d_counts), Lm.ptr(d_ws), need, Lm.stream_ptr()),
             "qt_pose_duration_posterior")
    G.check()
    return tuple(None if t is None else t.cpu().numpy() for t in (d_post, d_cls, d_begin, d_ev, d_counts))


@functools.lru_cache(maxsize=None)
def case(S, C, D, T, batch, lens=None, with_init=False, floor=False):
    """seeded probabilities with, where the stream is long enough, a NaN row, a row of zeros, rows of equal probabilities and a
    saturated 1.0, the tables, and their references (float64, mixed); computed once, shared, never written.  floor: every
    table at -65536.  From 1000 frames on every probability is an eighth of itself, so that the levels reach about -7,000 bits."""
    probs = R.make_probs(1000 * S + 10 * C + batch + D, batch, T, C)
    if T >= 6:
        probs[0, T // 2] = np.nan
        probs[-1, T // 3] = 0.0
        probs[0, 1] = F32(1.0 / C)
        probs[-1, T - 2:] = F32(0.25)
        probs[0, 4] = 0.0
        probs[0, 4, C // 2] = 1.0
    if T >= 1000:
        probs *= F32(0.125)                                 # three bits more per frame: the posteriors stay, the levels fall
    sc, tr = chain(S, C)
    dur, open_ = durations(S, D)
    init = init_for(S) if with_init else None
    if floor:
        tr, dur, open_, init = (np.full_like(a, R.TRANS_FLOOR) for a in (tr, dur, open_, init_for(S)))
    lengths = None if lens is None else np.array({"ragged": [T, 1, T // 2 + 1], "equal": [T - 1] * 3}[lens][:batch], np.int32)
    args = (probs, sc, tr, dur, init, open_, lengths)
    ref64, mixed = P.loops64(*args)[:5], P.loops_mixed(*args)[:5]
    for a in (probs, sc, tr, dur, open_) + ref64 + mixed:
        a.setflags(write=False)
    return args, ref64, mixed


def errors(got, ref64):
    """(e of the three probability outputs, the evidence's error relative to max(1, |evidence|), dur_counts' relative to
    max(1, counts)); None for what is not there"""
    es = [float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(got[:3], ref64[:3]) if g is not None]
    ev = None if got[3] is None else float((np.abs(got[3] - ref64[3]) / np.maximum(1.0, np.abs(ref64[3]))).max())
    ct = None if got[4] is None else float((np.abs(got[4] - ref64[4]) / np.maximum(1.0, ref64[4])).max())
    return (max(es) if es else None), ev, ct


def within_bound(got, ref64, mixed, lengths, what, class_rows=True):
    """class_rows: every state's class is in range, so the rows of class_posterior sum to 1 too"""
    B, T = ref64[0].shape[:2]
    S = ref64[0].shape[-1]
    for g in got:
        assert g is None or np.isfinite(g).all(), (what, "not finite")
    for b in range(B):
        n = Q.stream_length(lengths, b, T)
        for name, g in zip(OUT[:3], got[:3]):
            if g is None:
                continue
            assert not g[b, n:].any(), (what, name, "rows beyond the stream's length")
            if name == "posterior" or (name == "class_posterior" and class_rows):
                off = float(np.abs(g[b, :n].sum(axis=-1, dtype=np.float64) - 1.0).max())
                assert off <= S * 2.0 ** -22, (what, name, "row sum", off)
    for name, e_k, e_m in zip(("e", "evidence", "dur_counts"), errors(got, ref64), errors(mixed, ref64)):
        if e_k is None:
            continue
        print(f"pose_duration_posterior {what}: {name} kernel {e_k:.3e} mixed {e_m:.3e} ratio {e_k / max(e_m, 1e-30):.2f}")
        assert e_k <= FACTOR * e_m + FLOOR, (what, name, e_k, e_m)


def same(got, want, what):
    for name, g, w in zip(OUT, got, want):
        if g is not None and w is not None:
            assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
            assert R.bits(g) == R.bits(w), (what, name, int((g != w).sum()), np.argwhere(g != w)[:4].tolist())


# (S, C, D, T, batch, lengths, init given, ld - C)
SHAPES = [(1, 1, 1, 1, 1, None, False, 0),                 # the smallest
          (16, 12, 8, 70, 1, None, True, 3),               # 16 lanes per state, its last size
          (17, 12, 8, 70, 3, "equal", False, 0),           # 4 lanes per state, its first size
          (12, 12, 64, 3 * 64 + 5, 3, "ragged", True, 3),  # the ring wraps three times; lengths frames, 1 and in between
          (64, 64, 128, 300, 1, None, True, 1),            # the LDS limit is raised
          (12, 12, 64, 1536, 1, None, False, 0)]           # levels near -7,000 bits: an f32 level misses by orders of magnitude


@pytest.mark.parametrize("S,C,D,T,batch,lens,with_init,pad", SHAPES)
def test_accuracy_against_the_float64_loops(S, C, D, T, batch, lens, with_init, pad):
    dev = _dev()
    args, ref64, mixed = case(S, C, D, T, batch, lens, with_init)
    got = run(dev, *args, ld=C + pad)
    within_bound(got, ref64, mixed, args[6], (S, C, D, T))
    if T == 1536:
        assert ref64[3][0] < -6000                          # an f32 level there has an ulp of 2^-11 bits: 3e-4 of a probability


def test_all_floor_tables():
    """every table at -65536 and a NaN row: 256 bits and more down per segment, nothing underflows to -inf"""
    dev = _dev()
    args, ref64, mixed = case(12, 12, 8, 70, 3, "ragged", True, floor=True)
    got = run(dev, *args, ld=15)
    within_bound(got, ref64, mixed, args[6], "floor")
    assert ref64[3][0] < -2000


def test_optional_outputs_repeats_and_a_stream_alone():
    """dur_counts alone and the posterior alone give the bits of the call with everything; the same call twice gives the same
    bits; a stream alone equals itself in a batch, a stream with lengths[b] = L the call on its first L frames; dur_counts is
    added to"""
    dev = _dev()
    for S, C, D, T in ((12, 12, 16, 150), (17, 12, 5, 70)):
        args, ref64, mixed = case(S, C, D, T, 3, "ragged", True)
        probs, sc, tr, dur, init, open_, lengths = args
        first = run(dev, *args)
        within_bound(first, ref64, mixed, lengths, (S, T))
        same(run(dev, *args), first, (S, T, "again"))
        only = run(dev, *args, want=("dur_counts",))
        assert only[:4] == (None,) * 4
        same(only, first, (S, T, "dur_counts alone"))
        same(run(dev, *args, want=("posterior",)), first, (S, T, "posterior alone"))
        same(run(dev, *args, want=("class_posterior", "evidence", "dur_counts")), first, (S, T, "no posterior"))
        before = np.arange(S * D, dtype=np.float64).reshape(S, D) / 8
        added = run(dev, *args, want=("dur_counts",), counts=before)[4]
        assert R.bits(added) == R.bits(before + first[4])
        total = np.zeros((S, D))
        for b, n in enumerate(lengths):
            alone = run(dev, probs[b:b + 1, :n], sc, tr, dur, init, open_)
            same(alone[:4], tuple(r[b:b + 1, :n] if r.ndim == 3 else r[b:b + 1] for r in first[:4]), (S, T, "alone", b))
            total += alone[4]                                                # ascending stream, from zero
        assert R.bits(total) == R.bits(first[4])


def test_special_probabilities_and_a_class_out_of_range():
    dev = _dev()
    S = C = 12
    D, T = 9, 70
    probs = np.array(case(S, C, D, T, 2)[0][0])
    values = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-42, 2.0 ** -32, np.nextafter(F32(2.0 ** -32), F32(0)), 1.0, 1.5, -0.5, 3e38]
    probs[0, 3:3 + len(values), 4] = values
    probs[1, 20:20 + len(values), :] = np.array(values, F32)[:, None]
    probs[1, 40:44] = np.nan
    sc, tr = chain(S, C)
    dur, open_ = durations(S, D, seed=1)
    bad = np.array(sc)
    bad[3], bad[9], bad[11] = C, -1, 2 ** 31 - 1
    for classes in (sc, bad):
        args = (probs, classes, tr, dur, None, open_, None)
        within_bound(run(dev, *args), P.loops64(*args)[:5], P.loops_mixed(*args)[:5], None,
                     "special" if classes is sc else "state_class", class_rows=classes is sc)


def _near_certain(seed, S, D, T):
    """(probs [1,T,S], lead [T]): one class at 1.0 per frame along the cycle 0, 1, .., holds of 3 .. D - 1 frames"""
    rng = np.random.default_rng(seed)
    lead, s = [], int(rng.integers(0, S))
    while len(lead) < T:
        lead += [s] * int(rng.integers(3, D))
        s = (s + 1) % S
    lead = np.array(lead[:T])
    probs = np.zeros((1, T, S), F32)
    probs[0, np.arange(T), lead] = 1.0
    return probs, lead


def test_agreement_with_the_decoder():
    """a near-certain video: the argmax of the posterior is PoseDurationDecoder's path, and the expected duration counts are
    the hard counts of that path, on the frames where the float64 loops' two best states are more than 0.1 apart (seed 3: the
    loops leave out no frame at all)"""
    dev = _dev()
    Pk = pkg()
    S = C = 6
    D, T = 12, 160
    probs, lead = _near_certain(3, S, D, T)
    sc, tr = R.cyclic_prior(range(S), -39, -300, skip=-800, other=-3000)
    np.fill_diagonal(tr, R.TRANS_FLOOR)
    dur = Q.hold_prior(S, D, 3, D - 1, inside=-10, outside=-4000)
    ref = P.loops64(probs, sc, tr, dur, None, Q.suffix_max(dur))
    top = np.sort(ref[0][0], axis=1)
    clear = top[:, -1] - top[:, -2] > 0.1
    assert clear.mean() >= 0.95
    d_probs = torch.from_numpy(probs).to(dev)
    path, _ = Pk.PoseDurationDecoder(sc, tr, dur, dev).decode(d_probs)
    post = Pk.PoseDurationPosterior(sc, tr, dur, dev)
    posterior = post.smooth(d_probs)
    counts = post.expected_durations(d_probs)
    path = path.cpu().numpy()[0]
    assert (path == lead).all()
    assert (posterior.cpu().numpy()[0].argmax(axis=1)[clear] == path[clear]).all()
    hard = Q.count_durations(path[None], S, D)
    assert hard.sum() >= 10 and np.abs(counts.cpu().numpy() - hard).max() <= 1e-3


def test_the_class_and_a_side_stream_without_a_host_sync():
    """PoseDurationPosterior: smooth with every output, confidence, holds, expected_durations and zero under a stream that is
    not the default one and under torch's sync debug mode; the outputs are the bits of the ctypes call on the same inputs;
    expected_durations over two batches is the sum of the two; [frames, C] for one stream; the refusals"""
    dev = _dev()
    Pk, M = pkg(), pkg("pose_order")
    S = C = 12
    B, T, D = 2, 140, 24
    args, _, _ = case(S, C, D, T, B)
    probs, sc, tr, dur = (np.array(a) for a in args[:4])                            # (writable copies: the class uploads them)
    lengths = np.array([T, 77], np.int32)
    open_ = Q.suffix_max(dur)
    post = Pk.PoseDurationPosterior(sc, tr, dur, dev, streams=B, class_names=[str(c) for c in range(C)])
    dec = Pk.PoseDurationDecoder(sc, tr, dur, dev, streams=B)
    d_probs, d_len = torch.from_numpy(np.array(probs)).to(dev), torch.from_numpy(lengths).to(dev)
    other = torch.from_numpy(np.array(probs[:, ::-1])).to(dev)
    post.smooth(d_probs)                                                            # (the workspace's first allocation is not the loop's)
    post.expected_durations(d_probs)
    post.zero()
    path, _ = dec.decode(d_probs, lengths=d_len)
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(side):
            posterior, by_class, begin, evidence = post.smooth(d_probs, lengths=d_len, by_class=True, begin=True, evidence=True)
            confidence = post.confidence(posterior, path)
            holds = post.holds(begin)
            first = post.expected_durations(d_probs, d_len).clone()
            post.zero()
            second = post.expected_durations(other).clone()
            post.zero()
            post.expected_durations(d_probs, d_len)
            both = post.expected_durations(other).clone()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    side.synchronize()
    want = run(dev, probs, sc, tr, dur, None, open_, lengths)
    same((posterior.cpu().numpy(), by_class.cpu().numpy(), begin.cpu().numpy(), evidence.cpu().numpy(), first.cpu().numpy()), want,
         "the class")
    assert holds.dtype == torch.float64 and holds.shape == (B, S)
    assert np.abs(holds.cpu().numpy() - want[2].sum(axis=1, dtype=np.float64)).max() <= 1e-9       # (float64 sums of 140 f32 in two orders)
    p, c = want[0], confidence.cpu().numpy()
    path = path.cpu().numpy()
    assert c.dtype == F32 and (c[1, 77:] == 0).all() and (path[1, 77:] == -1).all()
    assert R.bits(c[0]) == R.bits(p[0][np.arange(T), path[0]]) and R.bits(c[1, :77]) == R.bits(p[1][np.arange(77), path[1, :77]])
    assert float(first.sum()) > 1 and float(second.sum()) > 1 and torch.equal(both, first + second)
    assert len(post.smooth(d_probs, evidence=True)) == 2 and isinstance(post.smooth(d_probs), torch.Tensor)
    single = Pk.PoseDurationPosterior(sc, tr, dur, dev)
    flat, flat_begin = single.smooth(d_probs[0, :40], begin=True)
    alone = run(dev, probs[:1, :40], sc, tr, dur, None, open_)
    assert flat.shape == (40, S) and R.bits(flat.cpu().numpy()[None]) == R.bits(alone[0])
    assert single.holds(flat_begin).shape == (1, S) and single.confidence(flat, torch.from_numpy(path[0, :40]).to(dev)).shape == (40,)
    for bad in (lambda: single.smooth(d_probs[0, :4].cpu()), lambda: single.smooth(d_probs[0, :4].double()),
                lambda: single.smooth(d_probs[:, :4]), lambda: single.smooth(d_probs[0, :4], lengths=d_len[:1].long()),
                lambda: single.smooth(d_probs[0, :4], lengths=d_len), lambda: single.expected_durations(d_probs[0, :4].cpu()),
                lambda: single.expected_durations(d_probs[0, :4], lengths=d_len), lambda: single.confidence(flat.cpu(), flat),
                lambda: single.confidence(flat, torch.zeros(39, dtype=torch.int64, device=dev)),
                lambda: single.holds(flat_begin.double()), lambda: single.holds(flat_begin[:, :3])):
        with pytest.raises(Pk.QtError):
            bad()
