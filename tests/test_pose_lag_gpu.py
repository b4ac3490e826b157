"""Fixed-lag pose-order posteriors and revised paths on the GPU (qt_pose_lag_smooth in csrc/pose_posterior.hip, qt_pose_lag_decode
in csrc/pose_order.hip, PoseLagSmoother / PoseLagDecoder in <pkg>/pose_order.py).

Smooth: every lagged row against row 0 of the EXISTING kernel (qt_pose_posterior on the window's frames, from the carry of the
frames in front of it) for equality of bits, and against the float64 loops of tests/_pose_lag_ref.py beside the same loops in
numpy f32: e_kernel <= 4 e_f32 + 2^-20, the bound of tests/test_pose_posterior_gpu.py.  Decode: every output equal to the integer
loops, and one case against qt_pose_order_decode on every prefix.  Both routes (QTCNN_POSE_LAG=1 live, 2 batch) and every split of
a stream into calls must give the same bits, outputs and carry.  Every output sits between poisoned guard bands (tests/_guard.py),
the workspace is exactly the queried size and NaN-filled, carry_out is handed over poisoned, and the inputs (carry_in among them)
must come back byte for byte.  Every figure is printed before it is asserted (pytest -s shows them).

Measured on an MI355X: the largest share of the accuracy bound that any case uses is 0.41 (stay-only table, S = 12, lag 1:
e_kernel 1.29e-6 against e_f32 5.6e-7); the mixing table uses 0.19, the all-zero table 0.07, S = 64 at most 0.23.  The two routes
give the same figures, as they must.  The whole file takes 6 s."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import _pose_lag_ref as G
import _pose_order_ref as O
from _guard import Guard
from _util import pkg

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
FACTOR, FLOOR = 4.0, 2.0 ** -20
SHAPES = [(1, 1), (2, 2), (12, 12), (12, 13), (16, 16), (12, 17), (64, 64)]
LAGS = (0, 1, 5, 16, 63)
LIVE, BATCH = "1", "2"


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _api():
    M, Lm = pkg("pose_order"), pkg("_lib")
    return M, Lm, Lm.lib()


class route:
    """QTCNN_POSE_LAG for the calls inside: "1" the live route, "2" the batch route, None the library's own choice"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.pop("QTCNN_POSE_LAG", None)
        if self.value is not None:
            os.environ["QTCNN_POSE_LAG"] = self.value

    def __exit__(self, *exc):
        os.environ.pop("QTCNN_POSE_LAG", None)
        if self.old is not None:
            os.environ["QTCNN_POSE_LAG"] = self.old


def prior(S, C, kind="mixing"):
    """mixing: the left-to-right cycle of the decoder's tests; stay: 0 on the diagonal and -65536 elsewhere; zero: all zero"""
    sc, tr = O.cyclic_prior([s % C for s in range(S)], -30, -600, skip=-3000, other=-20000)
    if kind == "stay":
        tr = np.full_like(tr, -65536)
        np.fill_diagonal(tr, 0)
    elif kind == "zero":
        tr = np.zeros_like(tr)
    return sc, tr


def init_for(S):
    return ((np.arange(S, dtype=np.int64) * 977) % 4001 - 4000).astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(batch, frames, C, S, kind="mixing"):
    """seeded probabilities with a NaN row, rows of zeros, rows of equal probabilities (ties) and a saturated 1.0; shared,
    never written"""
    probs = O.make_probs(1000 * S + 10 * C + batch, batch, frames, C)
    if frames >= 6:
        probs[0, frames // 2] = np.nan
        probs[-1, frames // 3] = 0.0
        probs[0, 1] = F32(1.0 / C)
        probs[-1, frames - 2:] = F32(0.25)
        probs[0, 4] = 0.0
        probs[0, 4, C // 2] = 1.0
    sc, tr = prior(S, C, kind)
    init = init_for(S)
    for a in (probs, sc, tr, init):
        a.setflags(write=False)
    return probs, sc, tr, init


@functools.lru_cache(maxsize=None)
def smooth_refs(batch, frames, C, S, kind, lag):
    probs, sc, tr, init = case(batch, frames, C, S, kind)
    return (G.smooth(probs, sc, tr, init, lag=lag, flush=True, F=F64), G.smooth(probs, sc, tr, init, lag=lag, flush=True, F=F32))


def _call(dev, which, probs, sc, tr, init, lag, flush, seen, carry, ld, optional):
    """one call through ctypes.  probs f32 [B,n,C]; carry: the bytes of the call before (None with seen == 0).  Returns
    (g0, outputs as numpy, carry_out bytes)."""
    M, Lm, L = _api()
    B, n, C = probs.shape
    S = len(sc)
    ld = C if ld is None else ld
    padded = np.full((B, n, ld), np.nan, F32)
    padded[..., :C] = probs
    g0, g1 = G.span(seen, n, lag, flush)
    count = g1 - g0
    desc = M.PoseLagDesc(B, n, C, S, lag, int(flush), seen)
    smooth = which == "smooth"
    carry_bytes = int((L.qt_pose_lag_smooth_carry_bytes if smooth else L.qt_pose_lag_decode_carry_bytes)(ctypes.byref(desc)))
    assert carry_bytes == B * (G.smooth_carry_stride if smooth else G.decode_carry_stride)(S, lag)
    need = int((L.qt_pose_lag_smooth_workspace_bytes if smooth else L.qt_pose_lag_decode_workspace_bytes)(ctypes.byref(desc)))
    forced = os.environ.get("QTCNN_POSE_LAG")
    assert need % 8 == 0 and (need == 0) == (forced == LIVE or (forced is None and G.live(which, n, lag)) or n == 0), (need, forced)
    Gd = Guard(dev)
    d_probs = Gd.input("probs", torch.from_numpy(padded)) if n else None
    d_sc = Gd.input("state_class", torch.from_numpy(np.array(sc, np.int32)))
    d_tr = Gd.input("trans", torch.from_numpy(np.array(tr, np.int32)))
    d_init = Gd.input("init", None if init is None else torch.from_numpy(np.array(init, np.int32)))
    d_in = None
    if seen:
        assert carry is not None and len(carry) == carry_bytes
        d_in = Gd.input("carry_in", torch.from_numpy(np.frombuffer(bytes(carry), np.uint8).copy()))
    d_out = Gd.output("carry_out", (carry_bytes,), torch.uint8)
    d_ws = Gd.workspace("workspace", need) if need else None
    if smooth:
        d_lag = Gd.output("lagged", (B, count, S), torch.float32) if count else None
        d_cls = Gd.output("lagged_class", (B, count, C), torch.float32) if optional and count else None
        d_filt = Gd.output("filtered", (B, n, S), torch.float32) if optional and n else None
        d_ev = Gd.output("log2_evidence", (B,), torch.float64) if optional else None
        Lm.check(L.qt_pose_lag_smooth(ctypes.byref(desc), Lm.ptr(d_probs), ld, Lm.ptr(d_sc), Lm.ptr(d_tr), Lm.ptr(d_init),
                                      Lm.ptr(d_in), Lm.ptr(d_out), Lm.ptr(d_lag), Lm.ptr(d_cls), Lm.ptr(d_filt), Lm.ptr(d_ev),
                                      Lm.ptr(d_ws), need, Lm.stream_ptr()), "qt_pose_lag_smooth")
        outs = (d_lag, d_cls, d_filt, d_ev)
        empty = (np.zeros((B, 0, S), F32), np.zeros((B, 0, C), F32) if optional else None,
                 np.zeros((B, 0, S), F32) if optional else None, None)
    else:
        d_path = Gd.output("lag_path", (B, count), torch.int64) if count else None
        d_filt = Gd.output("filtered", (B, n), torch.int64) if optional and n else None
        Lm.check(L.qt_pose_lag_decode(ctypes.byref(desc), Lm.ptr(d_probs), ld, Lm.ptr(d_sc), Lm.ptr(d_tr), Lm.ptr(d_init),
                                      Lm.ptr(d_in), Lm.ptr(d_out), Lm.ptr(d_path), Lm.ptr(d_filt), Lm.ptr(d_ws), need,
                                      Lm.stream_ptr()), "qt_pose_lag_decode")
        outs = (d_path, d_filt)
        empty = (np.zeros((B, 0), np.int64), np.zeros((B, 0), np.int64) if optional else None)
    Gd.check()
    return g0, tuple(e if t is None else t.cpu().numpy() for t, e in zip(outs, empty)), d_out.cpu().numpy().tobytes()


def run(dev, which, probs, sc, tr, init, lag, cuts=(), flush_last=True, ld=None, optional=True, routes=None):
    """a stream in consecutive calls cut at `cuts` (routes: QTCNN_POSE_LAG per call, None for the library's choice): (the
    outputs joined along the frame axis, the evidence summed; the last carry as the loops' state; the calls' own returns)"""
    B, n, _ = probs.shape
    S = len(sc)
    edges = [0] + list(cuts) + [n]
    carry, calls = None, []
    for k, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        with route(None if routes is None else routes[k % len(routes)]):
            g0, outs, carry = _call(dev, which, probs[:, a:b], sc, tr, init, lag, flush_last and k == len(edges) - 2, a, carry, ld, optional)
        calls.append((g0, outs))
    joined = []
    for i in range(len(calls[0][1])):
        parts = [o[i] for _, o in calls]
        if parts[0] is None:
            joined.append(None)
        elif parts[0].ndim == 1:
            joined.append(sum(parts))
        else:
            joined.append(np.concatenate(parts, axis=1))
    unpack = G.unpack_smooth_carry if which == "smooth" else G.unpack_decode_carry
    return tuple(joined), unpack(carry, B, S, lag, n), calls


def same(got, want, what, evidence_bits=True):
    """outputs and states bit for bit; a split's evidence is a sum of the calls' and agrees to rounding"""
    (g_out, g_state, _), (w_out, w_state, _) = got, want
    for i, (g, w) in enumerate(zip(g_out, w_out)):
        if g is None or w is None:
            continue
        if g.ndim == 1 and g.dtype == F64 and not evidence_bits:
            assert np.abs(g - w).max() <= 1e-9 * max(1.0, float(np.abs(w).max())), (what, "evidence")
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, i, g.dtype, g.shape, w.shape)
        assert O.bits(g) == O.bits(w), (what, i, int((g != w).sum()), np.argwhere(g != w)[:4].tolist())
    G.same_state(g_state, w_state)


def posterior_rows(dev, probs, sc, tr, init, lag):
    """what the EXISTING kernel says: for every g, row 0 of qt_pose_posterior on frames [g, min(g + lag, last)] from the carry
    of frames [0, g) (carried frame by frame: calls of at most 64 frames); and that split's filtered rows and carry.  Windows
    of one length go as one batched call, a window per (frame, stream)."""
    M, Lm, L = _api()
    B, n, C = probs.shape
    S = len(sc)
    t = lambda a, dt: torch.from_numpy(np.array(a, dt)).to(dev)
    d_sc, d_tr, d_init = t(sc, np.int32), t(tr, np.int32), t(init, np.int32)
    d_probs = t(probs, F32)

    def call(d_p, carry):
        b, frames = d_p.shape[0], d_p.shape[1]
        post = torch.empty(b, frames, S, dtype=torch.float32, device=dev)
        desc = M.PoseOrderDesc(b, frames, C, S)
        assert frames <= 64 and L.qt_pose_posterior_workspace_bytes(ctypes.byref(desc)) == 0
        Lm.check(L.qt_pose_posterior(ctypes.byref(desc), Lm.ptr(d_p), C, Lm.ptr(d_sc), Lm.ptr(d_tr), Lm.ptr(d_init), Lm.ptr(carry),
                                     Lm.ptr(post), None, None, None, None, 0, Lm.stream_ptr()), "qt_pose_posterior")
        return post

    carry = torch.zeros(B, S + 2, dtype=torch.float64, device=dev)
    before, filt = [], []
    for g in range(n):
        before.append(carry.clone())
        filt.append(call(d_probs[:, g:g + 1].contiguous(), carry))      # at frames == 1 the posterior is the filtered row
    rows = {}
    for length in sorted({min(g + lag, n - 1) - g + 1 for g in range(n)}):
        gs = [g for g in range(n) if min(g + lag, n - 1) - g + 1 == length]
        windows = torch.cat([d_probs[:, g:g + length] for g in gs]).contiguous()
        post = call(windows, torch.cat([before[g] for g in gs]).contiguous())
        for k, g in enumerate(gs):
            rows[g] = post[k * B:(k + 1) * B, 0]
    return (torch.stack([rows[g] for g in range(n)], dim=1).cpu().numpy(), torch.cat(filt, dim=1).cpu().numpy(), carry.cpu().numpy())


@pytest.mark.parametrize("C,S", SHAPES)
def test_smooth_is_the_existing_kernel_bit_for_bit(C, S):
    """70 frames, 2 streams, every lag: the smallest shapes that cross the S <= 16 register form, the tile of 64 and the lag
    cap.  lagged[g] == row 0 of qt_pose_posterior on the window; filtered, evidence_total and a_last are that kernel's on the
    frame-by-frame split; on the library's route (batch here) and on the forced live route"""
    dev = _dev()
    probs, sc, tr, init = case(2, 70, C, S)
    for lag in LAGS:
        rows, filt, carry = posterior_rows(dev, probs, sc, tr, init, lag)
        for forced in (None, LIVE):
            (lagged, _, filtered, _), state, _ = run(dev, "smooth", probs, sc, tr, init, lag, routes=[forced], ld=C + 3)
            assert O.bits(lagged) == O.bits(rows), (C, S, lag, forced, np.argwhere(lagged != rows)[:4].tolist())
            assert O.bits(filtered) == O.bits(filt), (C, S, lag, forced)
            assert O.bits(state["total"]) == O.bits(carry[:, 1]) and O.bits(state["a_last"]) == O.bits(carry[:, 2:].astype(F32))
            if lag == 0:
                assert O.bits(lagged) == O.bits(filtered)


def _errors(got, ref64):
    e = max(float(np.abs(g.astype(F64) - w).max()) for g, w in zip(got[:3], ref64[:3]))
    ev = float((np.abs(got[3] - ref64[3]) / np.maximum(1.0, np.abs(ref64[3]))).max())
    return e, ev


@pytest.mark.parametrize("C,S", [(12, 12), (12, 17), (64, 64)])
def test_accuracy_against_the_float64_loops(C, S):
    """e_kernel <= 4 e_f32 + 2^-20 for lagged, lagged_class and filtered (the evidence likewise, relative to max(1, |evidence|)),
    on the mixing, stay-only and all-zero tables, with rows of NaN, zeros, ties and a saturated 1.0 among the inputs; a row
    sums to one within S 2^-22.  The largest share of the bound used is printed."""
    dev = _dev()
    share = 0.0
    for kind in ("mixing", "stay", "zero"):
        for lag in (1, 16, 63) if S <= 17 else (16,):                                # (the loops at S = 64 take a second per lag)
            probs, sc, tr, init = case(2, 70, C, S, kind)
            (_, ref64, _), (_, ref32, _) = smooth_refs(2, 70, C, S, kind, lag)
            for forced in (LIVE, BATCH):
                got, _, _ = run(dev, "smooth", probs, sc, tr, init, lag, routes=[forced])
                assert all(np.isfinite(g).all() for g in got)
                for g in got[:3]:
                    assert float(np.abs(g.sum(axis=-1, dtype=F64) - 1.0).max()) <= S * 2.0 ** -22
                (e_k, ev_k), (e_f, ev_f) = _errors(got, ref64), _errors(ref32, ref64)
                share = max(share, e_k / (FACTOR * e_f + FLOOR))
                print(f"pose_lag {(C, S, kind, lag, forced)}: e_kernel {e_k:.3e} e_f32 {e_f:.3e} share {e_k / (FACTOR * e_f + FLOOR):.3f}; "
                      f"evidence {ev_k:.3e} f32 {ev_f:.3e}")
                assert e_k <= FACTOR * e_f + FLOOR, (C, S, kind, lag, forced, e_k, e_f)
                assert ev_k <= FACTOR * ev_f + FLOOR, (C, S, kind, lag, forced, "evidence", ev_k, ev_f)
    print(f"pose_lag {(C, S)}: largest share of the bound used {share:.3f}")


@pytest.mark.parametrize("which", ["smooth", "decode"])
def test_both_routes_and_every_two_call_split_keep_the_bits(which):
    """40 frames at lag 5 (S = 12) and at lag 16 (S = 17): one call on the live route, one on the batch route, and every split
    into two calls on the library's own choice (smooth: n (lag + 1) <= 16 goes live, so cuts near either end mix the routes)"""
    dev = _dev()
    for (C, S), lag in (((12, 12), 5), ((12, 17), 16)):
        probs, sc, tr, init = case(2, 40, C, S)
        whole = run(dev, which, probs, sc, tr, init, lag, routes=[LIVE])
        same(run(dev, which, probs, sc, tr, init, lag, routes=[BATCH], ld=C + 1), whole, (which, S, "batch route"))
        for cut in range(1, 40) if lag == 5 else (1, 3, 4, 16, 17, 36, 37, 39):
            same(run(dev, which, probs, sc, tr, init, lag, cuts=[cut]), whole, (which, S, "split", cut), evidence_bits=False)
        for cuts, routes in (([1, 2], None), ([7, 8, 30], [BATCH, LIVE]), ([13, 14, 15, 16], [LIVE, BATCH]), ([20, 39], None)):
            same(run(dev, which, probs, sc, tr, init, lag, cuts=cuts, routes=routes), whole, (which, S, cuts), evidence_bits=False)
        # without flush the last lag frames stay pending; a flush without frames emits them
        head = run(dev, which, probs, sc, tr, init, lag, flush_last=False, routes=[BATCH])
        assert head[0][0].shape[1] == 40 - lag and O.bits(head[0][0]) == O.bits(whole[0][0][:, :40 - lag])
        G.same_state(head[1], whole[1])
        for forced in (LIVE, BATCH):
            with route(forced):
                g0, outs, carry = _call(dev, which, probs[:, :0], sc, tr, init, lag, True, 40,
                                        (G.pack_smooth_carry if which == "smooth" else G.pack_decode_carry)(head[1], S, lag).tobytes(),
                                        None, True)
            assert g0 == 40 - lag and O.bits(outs[0]) == O.bits(whole[0][0][:, 40 - lag:]), (which, forced)
            unpack = G.unpack_smooth_carry if which == "smooth" else G.unpack_decode_carry
            G.same_state(unpack(carry, 2, S, lag, 40), whole[1])


@pytest.mark.parametrize("which", ["smooth", "decode"])
def test_call_sizes_around_the_lag_and_the_tile(which):
    """lag 16, S = 13: `seen` frames in one call, then n more with flush, for seen in {0, 1, lag - 1, lag, lag + 1} and n in
    {1, 2, lag, lag + 1, 64, 65, 130}, the second call on either route: the bits of one call over seen + n frames"""
    dev = _dev()
    lag, C, S = 16, 12, 13
    probs, sc, tr, init = case(2, 17 + 130, C, S)
    for n in (1, 2, lag, lag + 1, 64, 65, 130):
        for seen in (0, 1, lag - 1, lag, lag + 1):
            x = probs[:, :seen + n]
            whole = run(dev, which, x, sc, tr, init, lag)
            for forced in (LIVE, BATCH):
                got = run(dev, which, x, sc, tr, init, lag, cuts=[seen] if seen else [], routes=[None, forced] if seen else [forced])
                same(got, whole, (which, n, seen, forced), evidence_bits=False)
                assert got[2][-1][0] == max(0, seen - lag) and got[2][-1][1][0].shape[1] == seen + n - max(0, seen - lag)


def test_streams_do_not_meet():
    """frames of one stream made one-hot: every other stream keeps its bits; a stream alone gives the bits it has in a batch;
    the optional outputs change nothing"""
    dev = _dev()
    lag, C, S = 5, 12, 12
    probs, sc, tr, init = case(3, 40, C, S)
    for which in ("smooth", "decode"):
        for forced in (LIVE, BATCH):
            first = run(dev, which, probs, sc, tr, init, lag, cuts=[9], routes=[forced])
            changed = np.array(probs)
            changed[1, 18:24] = 0.0
            changed[1, 18:24, 3] = 1.0                                              # (six frames: one alone need not move a path)
            second = run(dev, which, changed, sc, tr, init, lag, cuts=[9], routes=[forced])
            assert O.bits(second[0][0][1]) != O.bits(first[0][0][1])
            pick = lambda r, b: (tuple(None if x is None else x[b:b + 1] for x in r[0]), {k: v if k == "seen" else v[b:b + 1]
                                                                                          for k, v in r[1].items()}, None)
            for b in (0, 2):
                same(pick(second, b), pick(first, b), (which, forced, "beside a changed stream", b))
            for b in range(3):
                same(run(dev, which, probs[b:b + 1], sc, tr, init, lag, cuts=[9], routes=[forced]), pick(first, b), (which, forced, "alone", b))
            same(run(dev, which, probs, sc, tr, init, lag, cuts=[9], routes=[forced], optional=False), first, (which, forced, "required only"))


@pytest.mark.parametrize("C,S", SHAPES)
def test_decode_equals_the_integer_loops(C, S):
    """70 frames, 2 streams, every lag, both routes, init given and NULL: lag_path, filtered and the carry are the loops'"""
    dev = _dev()
    probs, sc, tr, init = case(2, 70, C, S)
    for lag in LAGS:
        for use_init in (init, None):
            g0, (path, filt), state = G.decode(probs, sc, tr, use_init, lag=lag, flush=True)
            for forced in (LIVE, BATCH):
                (got_path, got_filt), got_state, _ = run(dev, "decode", probs, sc, tr, use_init, lag, routes=[forced], ld=C + 2)
                assert got_path.dtype == np.int64 and (got_path == path).all(), (C, S, lag, forced, np.argwhere(got_path != path)[:4].tolist())
                assert (got_filt == filt).all()
                G.same_state(got_state, state)
                if lag == 0:
                    assert (got_path == got_filt).all()


def test_decode_against_the_existing_kernel_on_every_prefix():
    """S = 12, 40 frames, lag 5: lag_path[g] is path[g] of qt_pose_order_decode on frames [0, min(g + 5, 39)]"""
    dev = _dev()
    P = pkg()
    T, lag, S = 40, 5, 12
    probs, sc, tr, init = case(2, T, S, S)
    (path, _), _, _ = run(dev, "decode", probs, sc, tr, init, lag)
    d_probs = torch.from_numpy(np.array(probs)).to(dev)
    for g in range(T):
        w = min(g + lag, T - 1)
        decoder = P.PoseOrderDecoder(sc, tr, dev, streams=2, init=init)
        full, _ = decoder.decode(d_probs[:, :w + 1])
        assert (full[:, g].cpu().numpy() == path[:, g]).all(), g


def test_every_path_ties_on_a_zero_table():
    """trans all zero and every probability equal: every path ties, and the ties go to the lowest index at every step, so the
    revised path is state 0 throughout.  With the real probabilities a zero table forgets the other frames: psi[f + 1] is
    filtered[f] for every state, so the revised path is the filtered one"""
    dev = _dev()
    probs, sc, tr, _ = case(2, 70, 12, 12, "zero")
    for forced in (LIVE, BATCH):
        (path, filt), _, _ = run(dev, "decode", np.full_like(probs, F32(1.0 / 12)), sc, tr, None, 5, routes=[forced])
        assert (path == 0).all() and (filt == 0).all()
        (path, filt), _, _ = run(dev, "decode", probs, sc, tr, None, 5, cuts=[33], routes=[forced])
        assert (path == filt).all() and (filt != 0).any()


def test_the_live_loop_without_a_host_sync():
    """predict -> PoseTimeline.update -> push -> confidence -> FrameAnnotator.draw, 16 streams x 1 frame for 40 steps and a flush,
    under torch's sync debug mode; the joined outputs equal one push of the whole video and the loops; load_tables resets; the
    rounds counted on the lagged path are the loops' path's"""
    dev = _dev()
    P, M = pkg(), pkg("pose_order")
    C, B, T, lag = 12, 16, 40, 16
    rng = np.random.default_rng(5)
    lead = (np.arange(T)[None, :] // 2 + np.arange(B)[:, None]) % C                  # a step every two frames: rounds are made
    logits = rng.standard_normal((B, T, C)).astype(F32)
    np.put_along_axis(logits, lead[..., None], np.take_along_axis(logits, lead[..., None], 2) + F32(4.0), 2)
    d_logits = torch.from_numpy(logits).to(dev)
    frames = torch.from_numpy(rng.integers(0, 256, (B, 48, 64, 3), dtype=np.uint8)).to(dev)
    atlas = torch.from_numpy(rng.integers(0, 256, (C + 14, 8, 12), dtype=np.uint8))
    annotator = P.FrameAnnotator(atlas=(atlas, torch.full((C + 14,), 12, dtype=torch.int32)), caption_origin=(2, 2))
    timeline = P.PoseTimeline(C, dev, streams=B, window=3, min_run=2)
    sc, tr = M.cyclic_prior(range(C), stay=-40, advance=-500, skip=-2500)
    smoother = P.PoseLagSmoother(sc, tr, dev, lag, streams=B)
    lagdec = P.PoseLagDecoder(sc, tr, dev, lag, streams=B)
    counter = P.PoseOrderDecoder(sc, tr, dev, streams=B)
    annotator.draw(frames, pred=torch.zeros(B, dtype=torch.int64, device=dev))      # (the tables' upload is not the loop's)
    warm = torch.full((B, 1, C), 0.5, device=dev)
    for _ in range(lag + 1):                                                         # (nor is the first allocation of anything)
        smoother.push(warm), lagdec.push(warm)
    smoother.reset(), lagdec.reset()
    outs, shown, rows_all = [], [], []
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for f in range(T + 1):
            last = f == T
            if not last:
                probs, _, _ = P.predict(d_logits[:, f])
                _, _, _, rows = timeline.update(probs[:, None, :], smoothed=True)
                rows_all.append(rows)
            else:
                rows = rows[:, :0]
            first, lagged, cls, filt = smoother.push(rows, flush=last, by_class=True, filtered=True)
            first_d, lag_path, pfilt = lagdec.push(rows, flush=last, filtered=True)
            conf = smoother.confidence(lagged, lag_path)
            assert first == first_d == max(0, f - lag) and lagged.shape == (B, lag if last else int(f >= lag), C)
            if lagged.shape[1] == 1:
                shown.append(annotator.draw(frames, pred=lagdec.state_class[lag_path[:, 0]].long(), confidence=conf[:, 0]))
            outs.append((lagged, cls, filt, lag_path, pfilt, conf))
        video = torch.cat(rows_all, dim=1)
        smoother.reset(), lagdec.reset()
        whole = smoother.push(video, flush=True, by_class=True, filtered=True)
        whole_d = lagdec.push(video, flush=True, filtered=True)
        rounds = counter.cycles(torch.cat([o[3] for o in outs], dim=1))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert smoother.seen == lagdec.seen == T and whole[0] == 0 and whole_d[0] == 0 and len(shown) == T - lag
    joined = [torch.cat([o[i] for o in outs], dim=1) for i in range(6)]
    for got, want in zip(joined[:5], whole[1:] + whole_d[1:]):
        assert got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want)
    x = video.cpu().numpy()
    _, ref64, _ = G.smooth(x, sc, tr, None, lag=lag, flush=True, F=F64)
    _, ref32, _ = G.smooth(x, sc, tr, None, lag=lag, flush=True, F=F32)
    got = tuple(t.cpu().numpy() for t in joined[:3])
    e_k = max(float(np.abs(g.astype(F64) - w).max()) for g, w in zip(got, ref64[:3]))
    e_f = max(float(np.abs(g.astype(F64) - w).max()) for g, w in zip(ref32[:3], ref64[:3]))
    print(f"pose_lag loop: e_kernel {e_k:.3e} e_f32 {e_f:.3e}")
    assert e_k <= FACTOR * e_f + FLOOR
    _, (path, pfilt), _ = G.decode(x, sc, tr, None, lag=lag, flush=True)
    assert (joined[3].cpu().numpy() == path).all() and (joined[4].cpu().numpy() == pfilt).all()
    want_conf = np.take_along_axis(got[0], path[..., None], axis=2)[..., 0]
    assert joined[5].dtype == torch.float32 and O.bits(joined[5].cpu().numpy()) == O.bits(want_conf)
    wraps = ((path[:, :-1] == C - 1) & (path[:, 1:] == 0)).sum(axis=1)
    assert rounds.cpu().numpy().tolist() == wraps.tolist() and wraps.sum() > 0
    assert not torch.equal(shown[0], frames)
    # load_tables starts the streams anew, with the new tables
    sc2, tr2 = M.cyclic_prior(range(C), stay=-90, advance=-300)
    d_tr2 = torch.from_numpy(tr2).to(dev)
    smoother.load_tables(d_tr2), lagdec.load_tables(d_tr2)
    assert smoother.seen == 0 and lagdec.seen == 0
    fresh, fresh_d = smoother.push(video, flush=True), lagdec.push(video, flush=True)
    _, want64, _ = G.smooth(x, sc, tr2, None, lag=lag, flush=True, F=F64)
    _, want32, _ = G.smooth(x, sc, tr2, None, lag=lag, flush=True, F=F32)
    e_f = float(np.abs(want32[0].astype(F64) - want64[0]).max())
    assert fresh[0] == 0 and float(np.abs(fresh[1].cpu().numpy().astype(F64) - want64[0]).max()) <= FACTOR * e_f + FLOOR
    assert (fresh_d[1].cpu().numpy() == G.decode(x, sc, tr2, None, lag=lag, flush=True)[1][0]).all()
    assert not torch.equal(fresh[1], whole[1])
    one = P.PoseLagSmoother(sc, tr, dev, 3)
    first, flat = one.push(video[0])                                                 # [frames, C] with one stream
    assert first == 0 and flat.shape == (T - 3, C)
    for bad in (video.cpu(), video.double(), video[:1], video[:, :0], [[0.5] * C]):
        with pytest.raises(P.QtError):
            smoother.push(bad)
    with pytest.raises(P.QtError):
        smoother.confidence(fresh[1], fresh_d[1].to(torch.int32))
    with pytest.raises(P.QtError):
        smoother.confidence(fresh[1][:, :5], fresh_d[1])
