"""Fixed-lag pose-order posteriors with hold durations (include/qtcnn.h, qt_pose_duration_lag_smooth) as plain loops with a
bounded carry, built on tests/_pose_duration_posterior_ref.py: its L, pow2, tables and by_class are imported, not restated, and
every sum here is formed from the same operands in the same order as its `sweep`, so that an emitted row is, bit for bit, the row
that `loops` gives on the stream's prefix, in float64 and in the rule's mixed precision alike.  A stream's frames carry global
indices; a call covers [seen, seen + n) and emits [g0, g1) (`span`, tests/_pose_lag_ref.py's, as `split` is); the answer for
frame g is conditioned on the first F = min(g + lag, last) + 1 frames.

Between calls the history travels in a `state` dict that holds what the header's carry holds, with the two summands of a ring
entry apart (the kernel keeps the difference Bt - cum / 256, `sweep` adds a difference of cums to Bt: only the second is `loops`
to the bit):
    seen; cum int64 [B,S] = cum[seen]; bt [B,D,S] and cumr int64 [B,D,S]: Bt[f] and cum[f] at row f mod D for the last D values of
    f, rows never written zero; btl [B,lag,S]: Bt[f] of f = seen - lag + k; al [B,lag,S]: the closed Al[f] of f = seen - lag + 1 + k;
    al_open [B,S] and Z [B] of f = seen; e int64 [B,lag,S]: the emissions of frame seen - lag + k; zeros in front of the stream's
    start.
`pack_carry` turns it into the kernel's bytes (ring = bt - cumr / 256, gh = btl - cum[f] / 256 with cum[f] stepped back from
cum[seen] through e), `unpack_carry` reads a kernel's bytes as the carry's own fields.  The integers of the two agree exactly;
the levels agree as far as a kernel's f32 terms inside an L agree with numpy's, which `level_bound` states.  The probabilities
and tables of tests/test_pose_duration_lag_gpu.py (`tracks`, `tables`, `durations`) are repeated here so that NaN rows, zero rows,
ties and forbidden lengths are present.  The reference project has no such step."""
import functools

import numpy as np

import _pose_duration_posterior_ref as P
import _pose_duration_ref as Q
import _pose_order_ref as R
from _pose_lag_ref import span, split  # noqa: F401

F32, F64 = np.float32, np.float64
MAX_STREAM = 1 << 20
LEVELS = ("ring", "gh", "al", "al_open", "Z")


def fresh(B, S, D, lag):
    z = lambda *s: np.zeros(s, F64)
    zi = lambda *s: np.zeros(s, np.int64)
    return dict(seen=0, cum=zi(B, S), bt=z(B, D, S), cumr=zi(B, D, S), btl=z(B, lag, S), al=z(B, lag, S), al_open=z(B, S), Z=z(B),
                e=zi(B, lag, S))


def smooth(probs, state_class, trans, dur, init=None, dur_open=None, lag=0, flush=False, state=None, F=F64):
    """probs f32 [B, n, C] (n may be 0 with flush).  Returns (g0, (lagged [B,count,S], lagged_class [B,count,C], lagged_begin
    [B,count,S], filtered [B,n,S], evidence float64 [B,n]), state); the probabilities in float64 for F = float64 and in f32
    otherwise."""
    probs = np.asarray(probs, F32)
    B, n, C = probs.shape
    S = len(state_class)
    T, Dur, DurOpen, start = P.tables(S, trans, dur, init, dur_open)
    D = Dur.shape[1]
    out = F64 if F is F64 else F32
    if state is None:
        state = fresh(B, S, D, lag)
    seen = state["seen"]
    assert n >= 1 or flush
    assert seen + n <= MAX_STREAM
    g0, g1 = span(seen, n, lag, flush)
    end, last = seen + n, seen + n - 1
    e_new = np.stack([R.emissions(probs[b], state_class) for b in range(B)]).astype(np.int64) if n else np.zeros((B, 0, S), np.int64)

    # the rows by their frame f: what the carry holds of the past, then this call's
    Bt, Al, Alo, Z, cum, E = {}, {}, {}, {}, {}, {}
    cum[seen] = state["cum"].copy()
    for k in range(lag):
        f = seen - lag + k
        if f >= 0:
            Bt[f], E[f] = state["btl"][:, k], state["e"][:, k]
        if f + 1 >= 1:
            Al[f + 1] = state["al"][:, k]
    for f in range(seen - 1, max(seen - lag, 0) - 1, -1):
        cum[f] = cum[f + 1] - E[f]
    if seen == 0:
        Bt[0] = P.L(np.broadcast_to((start[:, None] + T)[:, None, :], (S, B, S)), F)
    else:
        for f in range(max(0, seen - D + 1), seen + 1):
            Bt[f], cum[f] = state["bt"][:, f % D], state["cumr"][:, f % D]
        Alo[seen], Z[seen] = state["al_open"], state["Z"]
    bits = lambda c: c / 256.0                                             # exact; a difference of two of them is seg

    for f in range(seen + 1, end + 1):
        E[f - 1] = e_new[:, f - 1 - seen]
        cum[f] = cum[f - 1] + E[f - 1]
        m = min(D, f)
        back = np.stack([Bt[f - d] for d in range(1, m + 1)], axis=1)      # [b][d - 1][j]
        seg = np.stack([bits(cum[f]) - bits(cum[f - d]) for d in range(1, m + 1)], axis=1)
        table = np.array(Dur.T[:m])
        if f <= D:
            table[f - 1] = DurOpen[:, f - 1]                               # f - d == 0: the stream's first segment
        Al[f] = P.L(np.moveaxis(back + table[None] + seg, 1, 0), F)
        Alo[f] = P.L(np.moveaxis(back + DurOpen.T[:m][None] + seg, 1, 0), F)    # as if the stream were cut after frame f
        Bt[f] = P.L(np.moveaxis(Al[f][:, :, None] + T[None], 1, 0), F)
        Z[f] = P.L(np.moveaxis(Alo[f], 1, 0), F)

    def window(g, Fr):
        """the backward sweep on the prefix [0, Fr) down to frame g: (occ[g] float64 [B,S], begin[g] [B,S] in F)"""
        z = Z[Fr][:, None]
        Be = {Fr: np.zeros((B, S))}
        occ = bg_next = None
        for f in range(Fr - 1, g - 1, -1):
            k = min(D, Fr - f)
            table = np.array(DurOpen.T[:k] if f == 0 else Dur.T[:k])
            if Fr - f <= D:
                table[Fr - f - 1] = DurOpen[:, Fr - f - 1]                 # f + d == Fr: the prefix's last segment
            seg = np.stack([bits(cum[f + d]) - bits(cum[f]) for d in range(1, k + 1)], axis=1)
            x = table[None] + seg + np.stack([Be[f + d] for d in range(1, k + 1)], axis=1)
            Bs = P.L(np.moveaxis(x, 1, 0), F)
            if f >= 1:
                Be[f] = P.L(np.moveaxis(T[None] + Bs[:, None, :], 2, 0), F)
            bg = P.pow2(Bt[f] + Bs - z, F)
            ep = P.pow2((Alo[Fr] if f + 1 == Fr else Al[f + 1]) + Be[f + 1] - z, F)   # endp[f + 1]
            occ = ep.astype(F64) if f == Fr - 1 else occ + ep.astype(F64) - bg_next.astype(F64)
            bg_next = bg
        return occ, bg_next

    def row(occ):
        r = np.maximum(occ, 0.0)
        Rs = np.zeros(r.shape[:-1])
        for j in range(S):                                                 # ascending j, float64
            Rs = Rs + r[..., j]
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(Rs[..., None] > 0, r / Rs[..., None], 1.0 / S).astype(out)

    lagged, begin = np.empty((B, g1 - g0, S), out), np.empty((B, g1 - g0, S), out)
    for g in range(g0, g1):
        occ, bg = window(g, min(g + lag, last) + 1)
        lagged[:, g - g0], begin[:, g - g0] = row(occ), bg
    filtered, evidence = np.empty((B, n, S), out), np.empty((B, n), F64)
    for f in range(seen + 1, end + 1):
        filtered[:, f - 1 - seen] = row(window(f - 1, f)[0])
        evidence[:, f - 1 - seen] = Z[f]

    new = fresh(B, S, D, lag)
    new.update(seen=end, cum=cum[end].copy(), bt=state["bt"].copy(), cumr=state["cumr"].copy())
    for f in range(seen if seen == 0 else seen + 1, end + 1):
        new["bt"][:, f % D], new["cumr"][:, f % D] = Bt[f], cum[f]
    for k in range(lag):
        f = end - lag + k
        if f >= 0:
            new["btl"][:, k], new["e"][:, k] = Bt[f], E[f]
        if f + 1 >= 1:
            new["al"][:, k] = Al[f + 1]
    if end > 0:
        new["al_open"], new["Z"] = np.array(Alo[end]), np.array(Z[end])
    return g0, (lagged, P.by_class(lagged, state_class, C, out), begin, filtered, evidence), new


def carry_stride(S, D, lag):
    return (8 * S + 8 * D * S + 16 * lag * S + 8 * S + 8 + 2 * lag * S + 7) // 8 * 8


def workspace_bytes(B, n, S):
    return 32 * B * n * S + 8 * B * n + (2 * B * n * S + 7) // 8 * 8


def carry_fields(state, S, D, lag):
    """the loops' state as the fields of the kernel's carry: dict(seen, cum, ring, gh, al, al_open, Z, e)"""
    seen, B = state["seen"], state["cum"].shape[0]
    gh = np.zeros((B, lag, S))
    c = state["cum"].copy()                                                # cum[f], stepping back from f = seen
    for k in range(lag - 1, -1, -1):
        if seen - lag + k >= 0:
            c = c - state["e"][:, k]
            gh[:, k] = state["btl"][:, k] - c / 256.0
    return dict(seen=seen, cum=state["cum"], ring=state["bt"] - state["cumr"] / 256.0, gh=gh, al=state["al"],
                al_open=state["al_open"], Z=state["Z"], e=state["e"])


def pack_carry(state, S, D, lag):
    """the loops' state as a kernel's carry (uint8 [B, stride]), zeros in the padding"""
    f = carry_fields(state, S, D, lag)
    B = f["cum"].shape[0]
    out = np.zeros((B, carry_stride(S, D, lag)), np.uint8)
    for b in range(B):
        body = f["cum"][b].astype(np.int64).tobytes() + b"".join(f[k][b].astype(F64).tobytes() for k in ("ring", "gh", "al", "al_open")) + \
            np.array([f["Z"][b]], F64).tobytes() + f["e"][b].astype(np.int16).tobytes()
        out[b, :len(body)] = np.frombuffer(body, np.uint8)
    return out


def unpack_carry(raw, B, S, D, lag, seen):
    """a kernel's carry (bytes) as its fields; the padding behind each stream must be zeros"""
    raw = np.frombuffer(bytes(raw), np.uint8).reshape(B, carry_stride(S, D, lag))
    lo = [0]

    def take(count, dt, shape):
        nbytes = count * np.dtype(dt).itemsize
        a = np.stack([np.frombuffer(raw[b, lo[0]:lo[0] + nbytes].tobytes(), dt) for b in range(B)]).reshape((B,) + shape)
        lo[0] += nbytes
        return a

    out = dict(seen=seen, cum=take(S, np.int64, (S,)), ring=take(D * S, F64, (D, S)), gh=take(lag * S, F64, (lag, S)),
               al=take(lag * S, F64, (lag, S)), al_open=take(S, F64, (S,)), Z=take(1, F64, ()),
               e=take(lag * S, np.int16, (lag, S)).astype(np.int64))
    assert not raw[:, lo[0]:].any(), "padding"
    return out


def level_bound(S, D, frames):
    """how far a level of a kernel's carry may lie from the mixed loops' after `frames` frames, in bits.  Both follow the same
    rule; inside an L they differ in the f32 terms: exp2f and log2f of the device and of numpy are each within 2 ulp, a sum of
    n <= max(S, D) terms in another order within n ulp of the largest partial sum, and log2 turns a relative error r of the sum
    into r / ln 2 bits; the f32 value of log2 of a sum of up to 128 terms (below 8) has an ulp of 2^-21 at most.  That is at
    most (1.45 (n + 2) 2^-24 + 2 * 2^-21) bits per L, two Ls per frame (Al from Bt, Bt from Al), and an error made at one frame
    is carried, at most undiminished, to the next: the bound is linear in the frames.  The doubles' own rounding (2^-53 of
    levels below 2^29) is far below."""
    n = max(S, D)
    return 2 * max(frames, 1) * (1.45 * (n + 2) * 2.0 ** -24 + 2.0 ** -20)


def same_carry(got, want, bound):
    """two carries as fields: the integers equal, the levels within `bound` bits"""
    assert got.keys() == want.keys()
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, k
        if k in LEVELS:
            assert np.isfinite(g).all() and float(np.abs(g - w).max(initial=0.0)) <= bound, (k, float(np.abs(g - w).max(initial=0.0)), bound)
        else:
            assert (g.astype(np.int64) == w.astype(np.int64)).all(), k


def same_state(got, want):
    """two states of the loops, bit for bit"""
    assert got.keys() == want.keys()
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype and R.bits(g) == R.bits(w), k


# ---- the inputs of the GPU tests (tests/test_pose_duration_lag_gpu.py's) --------------------------------------------------------
def chain(S, C):
    """a loose left-to-right cycle over S states, state s emitting class s mod C"""
    return R.cyclic_prior([s % C for s in range(S)], -39, -300, skip=-800, other=-3000)


def init_for(S):
    return ((np.arange(S, dtype=np.int64) * 977) % 4001 - 4000).astype(np.int32)


def durations(S, D, seed=0):
    """(dur, dur_open) int32 [S, D]: seeded scores in [-500, 0] so that many lengths compete, some lengths forbidden, equal
    neighbours; dur_open a table of its own, not the suffix maximum"""
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
