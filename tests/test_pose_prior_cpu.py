"""The pose-order learner, the parts that need no GPU: the float64 loops of tests/_pose_prior_ref.py against an enumeration of
every path, the tiled restatement and the f32 loops against them, the rule's corner statements (what the counts sum to, their
row and column sums are summed posteriors), EM on a planted chain (it loses no evidence beyond the M-step's rounding, and it
finds the chain), the M-step's corner cases, the C ABI's declaration and every host-side refusal (pointers that are never
dereferenced), the module's argument checks, the exports and the documents."""
import ctypes
import os
import re

import numpy as np
import pytest

import _pose_order_ref as O
import _pose_posterior_ref as P
import _pose_prior_ref as R
from _util import PKG, ROOT, pkg, pose_chain_header

QT_ERR_INVALID_ARG, QT_ERR_UNSUPPORTED = -1, -3
F32 = np.float32


def _case(seed, B, T, C, S, run=3):
    probs = O.make_probs(seed, B, T, C, run=run)
    sc, trans = O.cyclic_prior([s % C for s in range(S)], -30, -600, skip=-3000, other=-20000)
    return probs, sc, trans


def test_the_loops_equal_an_enumeration_of_every_path():
    """S <= 3, n <= 5, with and without init: every start state and every path, their weights summed in float64"""
    for seed, (n, C, S) in enumerate([(5, 3, 3), (4, 2, 2), (1, 3, 3), (2, 3, 3), (3, 1, 1)]):
        probs, sc, trans = _case(5 + seed, 1, n, C, S, run=2)
        probs[0, n // 2] = F32(0.2)
        for init in (None, np.array([0, -700, -90][:S])):
            counts, start, ev = R.brute_force(probs[0], sc, trans, init)
            got = R.loops64(probs, sc, trans, init)
            assert np.abs(got[0] - counts).max() <= 1e-12 and np.abs(got[1] - start).max() <= 1e-12, (n, S)
            assert abs(got[2][0] - ev) <= 1e-12 * max(1.0, abs(ev)) and got[2][1] == n
            assert abs(counts.sum() - (n - 1)) <= 1e-12 and abs(start.sum() - 1) <= 1e-12
    probs, sc, trans = _case(1, 2, 1, 3, 3)
    assert (R.loops64(probs, sc, trans)[0] == 0).all() and (R.loops32(probs, sc, trans)[0] == 0).all()   # one frame: no transition


def test_the_tiled_form_and_the_f32_loops_agree_with_the_loops():
    for seed, (B, T, C, S) in enumerate([(2, 23, 5, 6), (1, 23, 3, 3), (2, 23, 12, 12)]):
        probs, sc, trans = _case(40 + seed, B, T, C, S)
        probs[0, 5] = np.nan
        probs[-1, 11:14] = F32(0.25)
        init = -np.arange(S) * 37
        stay = np.full_like(trans, -65536)
        np.fill_diagonal(stay, 0)
        for trans_used in (trans, np.zeros_like(trans), stay):
            want = R.loops64(probs, sc, trans_used, init)
            assert abs(want[0].sum() - B * (T - 1)) <= 1e-9 and abs(want[1].sum() - B) <= 1e-9 and want[2][1] == B * T
            for tile in (1, 2, 4, 5, R.TILE):
                got = R.tiled(probs, sc, trans_used, init, tile=tile)
                for name, w, g in zip(("counts", "start_counts", "totals"), want, got):
                    scale = max(1.0, float(np.abs(w).max()))
                    assert np.abs(w - g).max() <= 1e-10 * scale, (B, T, S, tile, name, float(np.abs(w - g).max()))
                assert R.loops64(probs, sc, trans_used, init, tile=tile)[0] == pytest.approx(want[0], abs=1e-10)
            low = R.loops32(probs, sc, trans_used, init)
            assert np.abs(low[0] - want[0]).max() <= 1e-3 and np.abs(low[1] - want[1]).max() <= 1e-4
            assert abs(low[2][0] - want[2][0]) <= 1e-4 * abs(want[2][0])
            tiled32 = R.tiled(probs, sc, trans_used, init, tile=4, F=F32)
            assert np.abs(tiled32[0] - want[0]).max() <= 1e-3 and np.isfinite(tiled32[0]).all()


def test_row_and_column_sums_are_summed_posteriors():
    """sum_j xi_f[i][j] is the posterior of frame f - 1 at i, sum_i xi_f[i][j] that of frame f at j; the start counts are
    frame 0's virtual transition and have no part in counts"""
    for B, T, C, S, init in ((2, 30, 4, 6, None), (3, 17, 12, 12, -np.arange(12) * 55), (1, 2, 3, 3, None)):
        probs, sc, trans = _case(7 + T, B, T, C, S)
        probs[0, T // 2] = np.nan
        counts, start, totals = R.loops64(probs, sc, trans, init)
        post, _, _, ev, _ = P.loops64(probs, sc, trans, init)
        assert np.abs(counts.sum(axis=1) - post[:, :-1].sum(axis=(0, 1))).max() <= 1e-10
        assert np.abs(counts.sum(axis=0) - post[:, 1:].sum(axis=(0, 1))).max() <= 1e-10
        assert abs(counts.sum() - B * (T - 1)) <= 1e-10 and abs(start.sum() - B) <= 1e-10
        assert abs(totals[0] - ev.sum()) <= 1e-9 * abs(ev.sum()) and totals[1] == B * T
        if init is None:                                        # start = 0: P(start i | video) is 2^T[i][j] b-weighted, not flat
            assert np.abs(start - start.mean()).max() > 1e-6


PLANTED = (0.93, 0.06, 0.01)


def _planted(seed=11, B=4, n=1500, S=12):
    """B videos of a cycle over S steps that stays with 0.93, advances with 0.06 and skips one step with 0.01, and f32
    probability rows that point at the true step most of the time"""
    rng = np.random.default_rng(seed)
    path = np.zeros((B, n), np.int64)
    path[:, 0] = rng.integers(0, S, B)
    move = rng.choice(3, size=(B, n), p=PLANTED)
    for f in range(1, n):
        path[:, f] = (path[:, f - 1] + move[:, f]) % S
    logits = rng.standard_normal((B, n, S))
    np.put_along_axis(logits, path[..., None], np.take_along_axis(logits, path[..., None], axis=2) + 3.0, axis=2)
    probs = np.exp(logits)
    probs /= probs.sum(axis=2, keepdims=True)
    return path, probs.astype(F32)


def test_em_does_not_lose_evidence_and_finds_the_planted_chain():
    """From iteration 1 on and with pseudo_count = 0: evidence(k + 1) >= evidence(k) - frames / 256 bits.  The M-step moves
    every transition score by at most 1/512 bit from the exact maximiser, so a path of n frames moves by at most n / 512; the
    factor 2 is the margin.  And the three planted entries of every row are found within 0.05 (sampling noise at 6,000
    frames).  The reference rule only."""
    S = 12
    path, probs = _planted()
    sc, start = O.cyclic_prior(range(S), -256, -512, skip=-768, other=-3000)
    trans, init, history = R.fit([probs], sc, start, iterations=9)
    bits = [h[0] for h in history]
    frames = history[0][1]
    assert frames == 4 * 1500
    drops = [bits[k] - bits[k + 1] for k in range(1, len(bits) - 1)]
    print(f"pose_prior EM: evidence {bits[0]:.1f} -> {bits[1]:.1f} -> {bits[-1]:.1f} bits; largest drop {max(drops):.3f} of "
          f"{frames / 256:.1f} allowed")
    assert bits[1] > bits[0] + 100
    assert max(drops) <= frames / 256
    fitted = np.exp2(trans / 256.0)
    worst = max(abs(fitted[s, (s + k) % S] - PLANTED[k]) for s in range(S) for k in range(3))
    print(f"pose_prior EM: planted entries within {worst:.4f}")
    assert worst <= 0.05
    assert np.abs(fitted.sum(axis=1) - 1).max() <= S / 512
    hard, hard_start, totals = R.count_paths(path, S)           # the labelled paths give the same chain at once
    labelled, _, _, _ = R.m_step(hard, hard_start, start)
    assert max(abs(np.exp2(labelled[s, (s + k) % S] / 256.0) - PLANTED[k]) for s in range(S) for k in range(3)) <= 0.05


def test_m_step_corner_cases():
    sc, trans = O.cyclic_prior(range(4), -100, -300)             # everything else forbidden (-65536)
    counts = np.array([[6.0, 2.0, 5.0, 0.0], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 3.0, 1.0], [0.0, 0.0, 0.0, 0.0]])
    new, init, near, _ = R.m_step(counts, np.zeros(4), trans, pseudo_count=0.5)
    assert (new[trans == -65536] == -65536).all()                # a forbidden entry stays forbidden, whatever its count
    assert new[0, 0] == round(256 * np.log2(6.5 / 9.0)) and new[0, 1] == round(256 * np.log2(2.5 / 9.0))
    assert new[1].tolist() == [-65536, round(256 * np.log2(0.5)), round(256 * np.log2(0.5)), -65536]
    assert init is None and not near.any()
    new0, _, _, _ = R.m_step(counts, np.zeros(4), trans)         # pseudo_count 0
    assert new0[1].tolist() == trans[1].tolist() and new0[3].tolist() == trans[3].tolist()      # an all-zero row keeps its values
    assert new0[2].tolist() == [-65536, -65536, round(256 * np.log2(0.75)), round(256 * np.log2(0.25))]
    assert new0[0, 2] == -65536 and new0[0, 3] == -65536
    tiny = np.array([[1.0, 1e-300], [1.0, 1.0]])
    assert R.m_step(tiny, np.zeros(2), np.zeros((2, 2), int))[0].tolist() == [[0, -65536], [-256, -256]]     # clamped
    _, init, _, _ = R.m_step(counts, np.array([3.0, 1.0, 0.0, 0.0]), trans, learn_init=True)
    assert init.tolist() == [round(256 * np.log2(0.75)), -512, -65536, -65536]
    _, init, _, _ = R.m_step(counts, np.zeros(4), trans, init=np.array([0, -5, -6, -7]), learn_init=True)
    assert init.tolist() == [0, -5, -6, -7]
    c, s, t = R.count_paths(np.array([[0, 1, 1, 7, 2, -1, 3], [4, 0, 0, 0, 3, 3, 3]]), 4)
    assert c.tolist() == [[2, 1, 0, 1], [0, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 2]] and s.tolist() == [1, 0, 0, 0]
    assert t.tolist() == [0, 14]


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    declared = set(re.findall(r"\b(qt_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(os.path.join(ROOT, PKG, "libqtcnn_hip.so"))
    for symbol in ("qt_pose_prior_workspace_bytes", "qt_pose_prior_expect", "qt_pose_prior_count_paths", "qt_pose_prior_update"):
        assert symbol in declared and hasattr(lib, symbol), symbol
    Pk, M = pkg(), pkg("pose_order")
    assert Pk.PoseOrderLearner is M.PoseOrderLearner and "PoseOrderLearner" in Pk.__all__
    assert callable(Pk.PoseOrderDecoder.load_tables) and callable(Pk.PosePosterior.load_tables)
    assert int(re.search(r"constexpr int PC_TRANS_FLOOR = (-?\d+);", pose_chain_header()).group(1)) == O.TRANS_FLOOR


def _lib():
    M = pkg("pose_order")
    L = pkg("_lib").lib()
    return M, L


def _expect_bytes(B, T, S):
    tiles = -(-T // R.TILE)
    tiled = B * tiles * (S * 8 + 8 + S * S * 4 + S * 4 + S * 4) if T > R.TILE else 0
    up = lambda v: -(-v // 8) * 8
    return up(up(tiled) + B * 8 + B * tiles * S * S * 4 + B * S * 4)


def test_workspace_query():
    M, L = _lib()
    q = lambda *a: L.qt_pose_prior_workspace_bytes(ctypes.byref(M.PoseOrderDesc(*a)))
    for B, T, S in ((3, 1, 12), (3, R.TILE, 12), (1, 2, 1), (3, 2 * R.TILE + 3, 12), (1, R.TILE + 1, 64), (5, 700, 3)):
        assert q(B, T, 12, S) == _expect_bytes(B, T, S) > 0, (B, T, S)
    assert q(1, 1, 1, 1) == 16 and q(3, 1, 12, 12) == 3 * (8 + 144 * 4 + 12 * 4)
    assert q(0, 100, 12, 12) == 0 and q(1, 100, 12, 65) == 0 and q(1, 100, 0, 12) == 0 and q(2, 1 << 20, 12, 12) == 0
    assert q(1, 0, 12, 12) == 0 and q(1, 100, 65, 12) == 0 and q(1, 100, 12, 0) == 0
    assert L.qt_pose_prior_workspace_bytes(None) == 0


def _refused(L, rc, word, status=QT_ERR_INVALID_ARG):
    assert rc == status and word in L.qt_last_error(), (rc, L.qt_last_error())


def test_expect_argument_checks_need_no_device():
    """every refusal comes before the first device call: the pointers are never dereferenced"""
    M, L = _lib()
    D = lambda batch=2, frames=100, C=12, S=12: M.PoseOrderDesc(batch, frames, C, S)
    probs, sc, trans, init, counts, start, totals, ws = (0x10000000 * k for k in range(1, 9))
    good = dict(probs=probs, ld=12, sc=sc, trans=trans, init=init, counts=counts, start=start, totals=totals, ws=ws,
                ws_bytes=1 << 24)

    def call(desc, **kw):
        a = {**good, **kw}
        return L.qt_pose_prior_expect(ctypes.byref(desc), a["probs"], a["ld"], a["sc"], a["trans"], a["init"], a["counts"],
                                      a["start"], a["totals"], a["ws"], a["ws_bytes"], None)

    refused = lambda *a: _refused(L, *a)
    refused(L.qt_pose_prior_expect(None, probs, 12, sc, trans, init, counts, start, totals, ws, 1 << 24, None), b"null descriptor")
    for batch in (0, -3):
        refused(call(D(batch=batch)), b"batch")
    for frames in (0, -1):
        refused(call(D(frames=frames)), b"frames")
    for C in (0, -1, 65):
        refused(call(D(C=C), ld=70), b"num_classes")
    for S in (0, -1, 65):
        refused(call(D(S=S)), b"num_states")
    refused(call(D(), ld=11), b"ld")
    for name in ("probs", "sc", "trans", "counts", "start", "totals"):
        refused(call(D(), **{name: None}), b"null")
    refused(call(D(), start=None), b"null start_counts")
    for name, off in (("probs", 2), ("sc", 1), ("trans", 3), ("init", 2), ("counts", 4), ("start", 4), ("totals", 4), ("ws", 4)):
        refused(call(D(), **{name: good[name] + off}), b"aligned")
    need = L.qt_pose_prior_workspace_bytes(ctypes.byref(D()))
    assert need == _expect_bytes(2, 100, 12)
    refused(call(D(), ws_bytes=need - 1), b"workspace")
    refused(call(D(), ws_bytes=0), b"workspace")
    refused(call(D(), ws=None), b"workspace")
    refused(call(D(frames=R.TILE), ws=None, ws_bytes=0), b"workspace")            # the short route needs its partials too
    rows = 2 * 100
    for out, nbytes in (("counts", 144 * 8), ("start", 12 * 8), ("totals", 16), ("ws", need)):
        refused(call(D(), **{out: probs + (rows * 12 - 2) * 4}), b"overlap")
        refused(call(D(), **{out: probs - nbytes + 8}), b"overlap")
        refused(call(D(), **{out: sc + 40}), b"overlap")
        refused(call(D(), **{out: trans + (144 - 2) * 4}), b"overlap")
        refused(call(D(), **{out: init}), b"overlap")
    refused(call(D(), ld=16, counts=probs + (199 * 16 + 10) * 4), b"overlap")
    refused(call(D(), start=counts + 8), b"overlap")
    refused(call(D(), totals=start + 11 * 8), b"overlap")
    refused(call(D(), ws=totals - need + 8), b"overlap")
    refused(call(D(batch=1 << 10, frames=(1 << 10) + 1)), b"frames", QT_ERR_UNSUPPORTED)
    refused(call(D(batch=1, frames=(1 << 20) + 1)), b"frames", QT_ERR_UNSUPPORTED)


def test_count_paths_argument_checks_need_no_device():
    M, L = _lib()
    D = lambda batch=2, frames=3000, C=1, S=12: M.PoseOrderDesc(batch, frames, C, S)
    path, counts, start, totals, ws = (0x10000000 * k for k in range(1, 6))
    good = dict(path=path, counts=counts, start=start, totals=totals, ws=ws, ws_bytes=1 << 24)

    def call(desc, **kw):
        a = {**good, **kw}
        return L.qt_pose_prior_count_paths(ctypes.byref(desc), a["path"], a["counts"], a["start"], a["totals"], a["ws"],
                                           a["ws_bytes"], None)

    refused = lambda *a: _refused(L, *a)
    refused(L.qt_pose_prior_count_paths(None, path, counts, start, totals, ws, 1 << 24, None), b"null descriptor")
    refused(call(D(batch=0)), b"batch")
    refused(call(D(frames=0)), b"frames")
    for S in (0, 65):
        refused(call(D(S=S)), b"num_states")
    for name in ("path", "counts", "start", "totals"):
        refused(call(D(), **{name: None}), b"null")
    refused(call(D(), totals=None), b"null totals")
    for name in ("path", "counts", "start", "totals", "ws"):
        refused(call(D(), **{name: good[name] + 4}), b"aligned")
    need = L.qt_pose_prior_workspace_bytes(ctypes.byref(D()))
    assert need == _expect_bytes(2, 3000, 12)
    refused(call(D(), ws_bytes=need - 1), b"workspace")
    refused(call(D(), ws=None), b"workspace")
    refused(call(D(C=0), ws_bytes=2 * 3 * 144 * 4 - 1), b"workspace")             # num_classes is not used: the histograms alone
    for out, nbytes in (("counts", 144 * 8), ("start", 12 * 8), ("totals", 16), ("ws", need)):
        refused(call(D(), **{out: path + (2 * 3000 - 1) * 8}), b"overlap")
        refused(call(D(), **{out: path - nbytes + 8}), b"overlap")
    refused(call(D(), start=counts + 143 * 8), b"overlap")
    refused(call(D(), totals=start), b"overlap")
    refused(call(D(batch=1, frames=(1 << 20) + 1)), b"frames", QT_ERR_UNSUPPORTED)


def test_update_argument_checks_need_no_device():
    M, L = _lib()
    counts, start, allowed, tin, iin, tout, iout = (0x10000000 * k for k in range(1, 8))
    good = dict(S=12, counts=counts, start=start, allowed=allowed, pseudo=0.5, tin=tin, iin=iin, tout=tout, iout=iout)

    def call(**kw):
        a = {**good, **kw}
        return L.qt_pose_prior_update(a["S"], a["counts"], a["start"], a["allowed"], a["pseudo"], a["tin"], a["iin"], a["tout"],
                                      a["iout"], None)

    refused = lambda *a: _refused(L, *a)
    for S in (0, -1, 65):
        refused(call(S=S), b"num_states")
    for pseudo in (-1.0, -1e-300, float("nan"), float("inf")):
        refused(call(pseudo=pseudo), b"pseudo_count")
    for name in ("counts", "allowed", "tin", "tout"):
        refused(call(**{name: None}), b"null")
    refused(call(start=None), b"start_counts")
    for name, off in (("counts", 4), ("start", 4), ("allowed", 2), ("tin", 1), ("iin", 2), ("tout", 3), ("iout", 2)):
        refused(call(**{name: good[name] + off}), b"aligned")
    for out in ("tout", "iout"):
        refused(call(**{out: counts + 8}), b"overlap")
        refused(call(**{out: start + 11 * 8}), b"overlap")
        refused(call(**{out: allowed + 143 * 4}), b"overlap")
    refused(call(tout=tin + 4), b"overlap")                      # in place is the table itself, not a shifted one
    refused(call(tout=iin), b"overlap")
    refused(call(iout=iin + 4), b"overlap")
    refused(call(iout=tin + 8), b"overlap")
    refused(call(iout=tout + 143 * 4), b"overlap")


def test_module_argument_checks_need_no_device():
    Pk = pkg()
    sc, trans = Pk.cyclic_prior(range(4), -10, -100)
    for bad in (dict(state_class=[]), dict(state_class=list(range(65)), trans=np.zeros((65, 65), int)), dict(state_class=[0, 1, 2, 64]),
                dict(state_class=[0, -1, 2, 3]), dict(state_class=np.zeros(4)), dict(trans=trans[:3]), dict(trans=trans.astype(float)),
                dict(trans=trans - 65536), dict(trans=-trans), dict(init=[0, 0, 0]), dict(init=np.array([0, 0, 0, 1])),
                dict(init=np.zeros(4)), dict(class_names=["a", "b", "c"]), dict(pseudo_count=-0.5), dict(pseudo_count=float("nan")),
                dict(pseudo_count=float("inf")), dict(pseudo_count="1"), dict(pseudo_count=True)):
        with pytest.raises(ValueError, match="PoseOrderLearner"):
            Pk.PoseOrderLearner(**{"state_class": sc, "trans": trans, "device": "cuda:0", **bad})
    with pytest.raises(Pk.QtError, match="AMD GPU"):             # no torch fallback
        Pk.PoseOrderLearner(sc, trans, "cpu")


def test_the_documents_speak_of_the_learner():
    for doc, word in (("DESIGN.md", "Pose-order prior"), ("README.md", "PoseOrderLearner"), ("EXPERIMENTS.md", "Pose-order prior"),
                      ("INTEGRATION.md", "learner.accumulate("), ("INTEGRATION.md", "load_tables("),
                      (os.path.join("scripts", "bench_pose_prior.py"), "qt_pose_prior_expect"),
                      (os.path.join("include", "qtcnn.h"), "qt_pose_prior_update")):
        assert word in open(os.path.join(ROOT, doc)).read(), (doc, word)
    for doc in ("DESIGN.md", os.path.join(PKG, "pose_order.py")):
        text = open(os.path.join(ROOT, doc)).read()
        assert "Not built: pairwise posteriors xi" not in text, doc
        assert "ragged batches" in text and "tying rows" in text, doc
